"""Solver(compute_gradient_variance=m) on the composite plan, CPU, against the reference's recorded runs
(tests/golden/make_golden_gradvar.py): the loss log, every (N, p) matrix get_gradient_variances returned, the logged scalar,
the cadence, and the two configurations the reference raises on."""
import math

import pytest
import torch

from conftest import load_golden
from gradvar_cases import RAISE_CASES, RUN_CASES, compare_rel, make_gradvar_solver, record_matrices


@pytest.mark.parametrize("name", RUN_CASES)
def test_composite_gradient_variances_match_reference(name):
    rec = load_golden(name)
    exp = rec["expected"]
    torch.set_num_threads(1)
    model = make_gradvar_solver(rec["case"], "cpu")
    matrices = record_matrices(model)
    model.train()
    assert model.plan_name == "torch"
    assert model.N == exp["N"] and int(model.p) == exp["p"]
    assert len(model.loss_log) == len(exp["loss_log"])
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert math.isclose(got, want, rel_tol=1e-5)
    for got, want in zip(model.Y_0_log, exp["Y_0_log"]):
        assert math.isclose(got, want, rel_tol=1e-6, abs_tol=1e-9)
    assert len(matrices) == len(exp["rel_matrices"]) == len(model.grads_rel_error_log)
    for i, (got, want) in enumerate(zip(matrices, exp["rel_matrices"])):
        assert tuple(got.shape) == (exp["N"], exp["p"])
        worst, left = compare_rel(got, torch.tensor(want), rel_tol=1e-4)
        print("%s call %d: worst rel err %.2e, left out %.3f" % (name, i, worst, left))
        assert model.grads_rel_error_log[i] == float(torch.mean(got))


def test_cadence():
    rec = load_golden("gradvar_lqgc3_logvar_attached_cadence")
    s = rec["case"]["solver"]
    assert s["compute_gradient_variance"] == 2 and s["L"] == 4
    assert len(rec["expected"]["grads_rel_error_log"]) == 2       # l = 0 and l = 2
    model = make_gradvar_solver(rec["case"], "cpu", L=5)
    model.train()
    assert len(model.grads_rel_error_log) == 3 and len(model.loss_log) == 5
    off = make_gradvar_solver(rec["case"], "cpu", compute_gradient_variance=0)
    off.train()
    assert off.grads_rel_error_log == []
    assert off.loss_log == model.loss_log[:4]                     # the diagnostic does not touch the training


@pytest.mark.parametrize("name", RAISE_CASES)
def test_raising_configurations(name):
    rec = load_golden(name)
    want = rec["expected"]["raises"]
    allowed = {"RuntimeError": (RuntimeError,), "UnboundLocalError": (UnboundLocalError, NotImplementedError)}[want]
    model = make_gradvar_solver(rec["case"], "cpu")
    with pytest.raises(allowed) as info:
        model.train()
    if want == "RuntimeError":
        assert not isinstance(info.value, NotImplementedError)    # autograd's own error, not a refusal
    else:
        assert "moment" in str(info.value) and "log-variance" in str(info.value)
