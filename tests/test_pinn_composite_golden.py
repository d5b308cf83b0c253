"""train_PINN() on the composite torch plan against the reference's fixed-seed PINN runs (tests/golden/pinn_*.json)."""
import math

import pytest
import torch

from conftest import load_golden
from pinn_cases import ALL, build, probe_values, seed_like_reference_train


@pytest.mark.parametrize("name", ALL)
def test_train_pinn_composite_matches_reference(name):
    rec = load_golden(name)
    exact = rec["torch"] == torch.__version__
    torch.set_num_threads(1)
    case, exp = rec["case"], rec["expected"]
    prob, model = build(case)
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "torch"
    assert len(model.loss_log) == len(exp["loss_log"])
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert (got == want) if exact else math.isclose(got, want, rel_tol=1e-5)
    assert model.K == exp["K"]
    assert model.K_log == exp["K_log"] == []
    assert len(model.V_L2_log) == len(exp["V_L2_log"])
    for got, want in zip(model.V_L2_log, exp["V_L2_log"]):
        assert math.isclose(got, want, rel_tol=1e-5, abs_tol=0.0 if want else 1e-30)
    for key in ("loss_log_domain", "loss_log_boundary", "V_test_L2", "V_test_abs"):
        assert len(getattr(model, key)) == len(exp[key])
        for got, want in zip(getattr(model, key), exp[key]):
            assert math.isclose(got, want, rel_tol=1e-5)
    v = probe_values(case, exp, prob, model)
    assert torch.allclose(v, torch.tensor(exp["probe_V"]), rtol=1e-5, atol=1e-7)


def test_time_dependent_h_broadcasts_like_the_reference():
    """h receives t_n as (K, 1): the parabolic exponential problem's h comes back (K, K), Allen-Cahn's (K,)."""
    rec = load_golden("pinn_expsphere_par_d3")
    prob, _ = build(rec["case"])
    K, d = 6, prob.d
    x, y, z, t = torch.rand(K, d), torch.rand(K), torch.rand(K, d), torch.rand(K, 1)
    assert tuple(prob.h(t, x, y, z).shape) == (K, K)
    prob, _ = build(load_golden("pinn_allencahn_d5")["case"])
    assert tuple(prob.h(t, torch.rand(K, prob.d), y, torch.rand(K, prob.d)).shape) == (K,)


@pytest.mark.parametrize("name", ["pinn_heat_d6", "pinn_box_d4_elliptic"])
def test_train_still_refuses_pinn_and_points_at_train_pinn(name):
    prob, model = build(load_golden(name)["case"])
    assert model.loss_method == "PINN"
    with pytest.raises(NotImplementedError, match="train_PINN"):
        model.train()


def test_train_pinn_scope():
    case = load_golden("pinn_heat_d6")["case"]
    for over, attr in ((dict(approx_method="Z"), None), (dict(solve_linear_L2_projection=True), None), ({}, "boundary")):
        prob, model = build(case, **over)
        if attr:
            prob.boundary = "triangle"
        with pytest.raises(NotImplementedError):
            model.train_PINN()


def test_train_pinn_does_not_seed():
    """It continues the generator where it stands: two different seeds before the call give two different first losses."""
    case = load_golden("pinn_heat_d6")["case"]
    first = []
    for seed in (1, 2):
        prob, model = build(case, L=1, K_test_log=None)
        torch.manual_seed(seed)
        model.train_PINN()
        first.append(model.loss_log[0])
    assert first[0] != first[1]
