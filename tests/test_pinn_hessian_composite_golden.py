"""The full-rank full-Hessian golden (tests/golden/pinn_expball_hess_d15_dense.json) on the composite torch plan, and the reasons
plan_pinn_native gives around full_hessian.  No GPU."""
import math

import pytest
import torch

from conftest import load_golden
from pinn_cases import probe_values, seed_like_reference_train
from pinn_hessian_cases import GOLDENS, build
from util_cases import psp

nat = psp.native


def test_train_pinn_composite_matches_the_dense_golden():
    rec = load_golden("pinn_expball_hess_d15_dense")
    torch.set_num_threads(1)
    case, exp = rec["case"], rec["expected"]
    prob, model = build(case)
    assert int(torch.linalg.matrix_rank(prob.B.double())) == prob.d == 15
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "torch" and "full_hessian" in model.plan_reason and "need a GPU" in model.plan_reason
    assert len(model.loss_log) == len(exp["loss_log"])
    # not bit for bit: the package's h takes (sum_i x_i)^2 where the reference sums the d x d outer product, another fp32 order
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert math.isclose(got, want, rel_tol=1e-5)
    assert model.K == exp["K"]
    for got, want in zip(model.V_L2_log, exp["V_L2_log"]):
        assert math.isclose(got, want, rel_tol=1e-5, abs_tol=0.0 if want else 1e-30)
    v = probe_values(case, exp, prob, model)
    assert torch.allclose(v, torch.tensor(exp["probe_V"]), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", GOLDENS)
def test_full_hessian_goldens_only_lack_a_gpu_here(name):
    _, model = build(load_golden(name)["case"])
    why = psp.plan_pinn_native.pinn_eligibility(model)
    assert "full_hessian" in why and "need a GPU" in why


def test_reasons_that_keep_full_hessian_and_dense_sigma_composite():
    reason = psp.plan_pinn_native.pinn_eligibility
    _, model = build(load_golden("pinn_heat_d6")["case"], full_hessian=True)        # GeneralSolver
    assert "GeneralSolver" in reason(model) and "no reference behaviour" in reason(model)
    assert model._choose_pinn_plan() is None and model.plan_name == "torch" and "GeneralSolver" in model.plan_reason
    _, model = build(load_golden("pinn_expball_hess_d4_full")["case"], full_hessian=False)
    assert "a dense sigma without full_hessian" in reason(model)
    prob, model = build(load_golden("pinn_expball_hess_d4_full")["case"])            # an h that reads z on a dense sigma
    spec = prob.general_native_spec()
    prob.general_native_spec = lambda: dict(spec, h=nat.GH_QUAD)
    assert "reads z" in reason(model)
    _, model = build(load_golden("pinn_expball_sin_d5_elliptic")["case"], full_hessian=True)   # s I: the scaled path
    assert "full_hessian" in reason(model) and "need a GPU" in reason(model)
    for name in GOLDENS:                                          # the default keeps the reference's Hessian, on any device
        _, model = build(load_golden(name)["case"], hessian="reference")
        assert "full_hessian" in reason(model) and "hessian='directions'" in reason(model) and "GPU" not in reason(model)
    with pytest.raises(ValueError, match="hessian"):
        build(load_golden("pinn_expball_hess_d4_full")["case"], hessian="fast")


def test_plan_key_carries_full_hessian(monkeypatch):
    """A plan built for one setting of full_hessian is not reused for the other."""
    ppn = psp.plan_pinn_native
    built = []

    class Plan:
        def __init__(self, solver):
            self.net, self.key = solver.V, None
            built.append(bool(solver.full_hessian))

    monkeypatch.setattr(ppn, "pinn_eligibility", lambda s: None)
    monkeypatch.setattr(ppn, "PinnNativePlan", Plan)
    monkeypatch.setattr(psp.general_solver, "_owns_parameters", lambda plan: True)
    _, model = build(load_golden("pinn_expball_sin_d5_elliptic")["case"])
    for flag in (False, False, True, True, False):
        model.full_hessian = flag
        model._choose_pinn_plan()
    assert built == [False, True, False]
    model.hessian = "reference"                                   # and neither is one built for the other setting of hessian
    model._choose_pinn_plan()
    assert len(built) == 4
