"""EllipticSolver.train_PINN(full_hessian=True, hessian='directions') on the native direction-table kernels against the
reference's full-Hessian PINN goldens: the notebook's ones matrix (rank 1, one direction) and a seeded full-rank B (d = 15, two
blocks).  The project's parity contract: the loss log follows the reference's to 1e-4 relative per iteration, the probe values to the same bound."""
import warnings

import pytest
import torch

from conftest import load_golden
from pinn_cases import probe_values, seed_like_reference_train
from pinn_hessian_cases import GOLDENS, build

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def follows(model, prob, case, exp):
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    print("%s: loss rel err per iteration %s" % (case["name"], ["%.1e" % e for e in errs]))
    assert len(model.loss_log) == len(exp["loss_log"]) and max(errs) <= 1e-4, (model.loss_log, exp["loss_log"])
    assert model.K == exp["K"]
    for key in ("V_L2_log", "loss_log_domain", "loss_log_boundary", "V_test_L2"):
        got = getattr(model, key)
        assert len(got) == len(exp[key])
        for a, b in zip(got, exp[key]):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-12, (key, got, exp[key])
    v, want = probe_values(case, exp, prob, model), torch.tensor(exp["probe_V"])
    assert float((v - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


@pytest.mark.parametrize("name", GOLDENS)
def test_full_hessian_plans_native_and_follows_the_reference(name):
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    prob, model = build(case, device=dev())
    seed_like_reference_train(case, model)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                             # no composite-plan warning
        model.train_PINN()
    assert model.plan_name == "native" and model.plan_reason is None
    plan = model._pinn_plan
    assert plan.cfg.sigma_kind == 1 and plan.cfg.n_dirs == (1 if name == "pinn_expball_hess_d4_full" else 15)
    assert plan.sizes.dir_blocks == (1 if name == "pinn_expball_hess_d4_full" else 2)
    follows(model, prob, case, exp)


@pytest.mark.parametrize("name", GOLDENS)
def test_backend_native_and_backend_torch(name):
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    prob, model = build(case, device=dev(), backend="native", L=1)
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "native"
    assert abs(model.loss_log[0] - exp["loss_log"][0]) <= 1e-4 * abs(exp["loss_log"][0])
    prob, model = build(case, device=dev(), backend="torch")
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "torch" and "backend='torch'" in model.plan_reason
    follows(model, prob, case, exp)


def test_variance_loss_parts_and_device_test_log_on_the_dense_path():
    """PINN_log_variance, log_loss_parts and test_log='device' as on the scaled path: native against backend='torch' on the same
    seeds (the device test log draws its points on the device, so it is compared with itself only: finite and positive)."""
    import math
    case = load_golden("pinn_expball_hess_d15_dense")["case"]
    logs = {}
    for backend in ("native", "torch"):
        prob, model = build(case, device=dev(), backend=backend, PINN_log_variance=True, log_loss_parts=True)
        seed_like_reference_train(case, model)
        model.train_PINN()
        assert model.plan_name == backend
        logs[backend] = (model.loss_log, model.loss_log_domain, model.loss_log_boundary, model.V_L2_log)
    for got, want in zip(logs["native"], logs["torch"]):
        assert len(got) == len(want) == 3
        for a, b in zip(got, want):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-12, (logs["native"], logs["torch"])
    prob, model = build(case, device=dev(), K_test_log=16, test_log="device")
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "native" and len(model.loss_log) == 3
    for log in (model.V_test_L2, model.V_test_abs):
        assert len(log) == 3 and all(math.isfinite(v) and v > 0.0 for v in log)


def test_what_stays_composite_on_the_gpu():
    _, model = build(load_golden("pinn_heat_d6")["case"], device=dev(), full_hessian=True)      # GeneralSolver
    with pytest.warns(UserWarning, match="composite torch plan"):
        assert model._choose_pinn_plan() is None
    assert model.plan_name == "torch" and "GeneralSolver" in model.plan_reason
    _, model = build(load_golden("pinn_expball_hess_d4_full")["case"], device=dev(), full_hessian=False, L=1)
    with pytest.warns(UserWarning, match="composite torch plan"):
        model.train_PINN()
    assert model.plan_name == "torch" and "a dense sigma without full_hessian" in model.plan_reason
    _, model = build(load_golden("pinn_expball_sin_d5_elliptic")["case"], device=dev(), full_hessian=True, L=1)
    model.train_PINN()                                             # s I with full_hessian: the scaled path
    assert model.plan_name == "native" and model._pinn_plan.cfg.sigma_kind == 0
    _, model = build(load_golden("pinn_expball_hess_d15_dense")["case"], device=dev(), hessian="reference", L=1)
    with pytest.warns(UserWarning, match="composite torch plan"):  # the default: the reference's Hessian, sample by sample
        model.train_PINN()
    assert model.plan_name == "torch" and "hessian='directions'" in model.plan_reason
