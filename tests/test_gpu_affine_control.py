"""GPU parity of the linear / affine / constant control plan (csrc/aff_kernels.h behind psp_aff_*, plan_affine_native.py):
time_approx='outer' with z_n a list of Linear / Affine / Constant modules.  The bars of tests/test_gpu_dense_control.py:
D_k <= 2e-5 max(1, |D|), gradient <= 2e-4 max|g| overall and per time step against the oracle's autograd, loss / u_L2 / Y_0
logs and probes <= 1e-4 relative against the reference's own runs (tests/golden/make_golden_affine.py)."""
import math

import pytest
import torch

from affine_cases import BIG_K, DIAGONAL, GOLDEN, SWEEP, UL2_D33, assert_first_iteration, build_modules, make_affine_solver
from conftest import load_golden
from util_cases import psp

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", GOLDEN)
def test_first_iteration_D_and_gradient_match_oracle(name):
    case = load_golden(name)["case"]
    model = make_affine_solver(case, dev(), backend="native", L=1)
    assert_first_iteration(model, case)


@pytest.mark.parametrize("tag", sorted(SWEEP))
def test_shape_sweep_matches_oracle(tag):
    case = SWEEP[tag]
    model = make_affine_solver(case, dev(), backend="native", L=1)
    plan, _ = assert_first_iteration(model, case, tag=tag)
    if case["control"].get("gains") is not None:
        assert plan.G is not None
    if tag in BIG_K:
        assert plan.sizes.fwd_threads == 256 and plan.sizes.slices * 32 < plan.K_local, (plan.sizes.fwd_threads, plan.sizes.slices)
    if tag in DIAGONAL:
        assert (plan.cfg.base.drift_kind, plan.cfg.base.sigma_kind) == (psp.native.DRIFT_DIAG, psp.native.SIGMA_IDENTITY)


def test_u_l2_log_next_to_a_bucket_64_linear_reference():
    """u_l2_error_flag=True at d = 33: the LINEAR reference (N, 64, 64) next to dense A, B and the maps.  Only the log entry and the
    plan are asserted here; the values are compared with float64 at kernel level (tests/test_gpu_affine_kernels.py)."""
    model = make_affine_solver(UL2_D33, dev(), backend="native", L=1)
    model.train()
    plan = model._native_plan
    assert model.plan_name == "native" and isinstance(plan, psp.plan_affine_native.AffineNativePlan)
    assert plan.d_pad == 64 and plan.cfg.ul2_kind == psp.native.UL2_LINEAR and plan.ul2 is not None
    print("u_L2 log", model.u_L2_loss)
    assert len(model.u_L2_loss) == 1 and math.isfinite(model.u_L2_loss[0]) and model.u_L2_loss[0] > 0.0


@pytest.mark.parametrize("name", GOLDEN)
def test_logs_and_probes_match_reference_golden(name):
    rec = load_golden(name)
    model = make_affine_solver(rec["case"], dev(), backend="native")
    model.train()
    assert model.plan_name == "native"
    exp = rec["expected"]
    print(name, "loss", model.loss_log, exp["loss_log"], "u_L2", model.u_L2_loss, exp["u_L2_loss"], "Y_0", model.Y_0_log)
    assert len(model.loss_log) == len(exp["loss_log"]) and len(model.u_L2_loss) == len(exp["u_L2_loss"])
    # cross-entropy crosses zero: an absolute floor of 1e-4 max|loss_log| next to the relative bound
    floor = 1e-4 * max(abs(v) for v in exp["loss_log"]) if rec["case"]["solver"]["loss_method"] == "cross_entropy" else 0.0
    for l, (got, want) in enumerate(zip(model.loss_log, exp["loss_log"])):
        assert math.isclose(got, want, rel_tol=1e-4, abs_tol=floor), (l, model.loss_log, exp["loss_log"])
    for l, (got, want) in enumerate(zip(model.u_L2_loss, exp["u_L2_loss"])):
        assert math.isclose(got, want, rel_tol=1e-4), (l, model.u_L2_loss, exp["u_L2_loss"])
    assert len(model.Y_0_log) == len(exp["Y_0_log"])
    for got, want in zip(model.Y_0_log, exp["Y_0_log"]):
        assert math.isclose(got, want, rel_tol=1e-4, abs_tol=1e-6)
    xp = torch.tensor(exp["probe_x"]).reshape(-1, model.d).to(dev())
    for pr in exp["probes"]:
        with torch.no_grad():
            u = (-model.Z_n(xp, pr["t"])).cpu()
        want = torch.tensor(pr["minus_Z"]).reshape(u.shape)
        assert float((u - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max())), pr["t"]
    # the modules' own optimisers carry the Adam state of the run
    st = model.z_n[0].optim.state[next(iter(model.z_n[0].parameters()))]
    assert int(float(st["step"])) == len(exp["loss_log"]) and bool(torch.isfinite(st["exp_avg"]).all())


@pytest.mark.parametrize("detach", [True, False])
def test_philox_is_deterministic_and_shard_independent(detach):
    """Device noise: two runs agree bitwise in D and gradient; the upper half of the trajectories run alone
    (k_offset = K / 2) reproduces the full run's D."""
    d, K = 20, 2048
    prob = psp.LLGC(d=d, off_diag=0.05, T=0.1, seed=42, device=dev())

    def make(Kx):
        m = psp.Solver(name="affphilox", problem=prob, loss_method="log-variance", time_approx="outer", L=1, lr=0.1, seed=42,
                       delta_t=0.02, K=Kx, adaptive_forward_process=True, detach_forward=detach, u_l2_error_flag=False,
                       verbose=False, device=dev(), backend="native", noise="philox")
        m.z_n = build_modules(dict(kind="Affine", init=dict(scale=0.1, seed0=9)), d, m.N, 0.1, 42, dev())
        m.update_Phis()
        return m

    a, b = make(K), make(K)
    a.train()
    b.train()
    pa, pb = a._native_plan, b._native_plan
    assert isinstance(pa, psp.plan_affine_native.AffineNativePlan)
    assert a.loss_log == b.loss_log and math.isfinite(a.loss_log[0])
    assert torch.equal(pa.D, pb.D) and torch.equal(pa.grad, pb.grad)
    assert bool(torch.isfinite(pa.grad).all()) and float(pa.grad.abs().max()) > 0.0
    half = make(K // 2)
    ph = psp.plan_affine_native.AffineNativePlan(half, noise="philox")
    ph.cfg.base.k_offset = K // 2
    ph.cfg.base.K_global = K
    losses = torch.zeros(1, device=dev())
    ph.iteration(0, losses)
    torch.cuda.synchronize()
    assert torch.equal(ph.D, pa.D[K // 2:])


@pytest.mark.parametrize("name", ["lqgc_d10_linear_outer_logvar", "llgc_d3_constant_outer_nonadaptive"])
def test_importance_sampling_evaluation_is_native(name, monkeypatch):
    """utilities.do_importance_sampling_me with a Linear / Constant list runs psp_is_rollout (gains -M_idx(n) / rows -c_idx(n));
    against the composite sweep on the same host noise.  The evaluation grid differs from the training grid, so the step map of
    solver.py:360-362 is exercised."""
    case = load_golden(name)["case"]
    model = make_affine_solver(case, dev(), backend="native", L=2)
    model.train()
    ut = psp.utilities
    assert ut._affine_is_reason(model.problem, model) is None
    calls = []
    real = ut._is_rollout
    monkeypatch.setattr(ut, "_is_rollout", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    delta = 0.004 if "lqgc" in name else 0.01
    torch.manual_seed(11)
    got = ut.do_importance_sampling_me(model.problem, model, 400, delta_t=delta)
    assert calls == [1]
    torch.manual_seed(11)
    want = ut._is_composite(model.problem, model, 400, delta)
    print(name, got, want)
    for a, b in zip(got, want):
        assert math.isclose(a, b, rel_tol=2e-4), (got, want)


@pytest.mark.parametrize("kind", ["Linear", "Affine", "Constant"])
def test_backend_native_plans_the_affine_plan(kind):
    """backend='native' raised PlanUnsupported for these lists before the plan existed."""
    prob = psp.LQGC(d=4, off_diag=0.1, T=0.1, seed=42, delta_t=0.005, device=dev())
    model = psp.Solver(name="dispatch", problem=prob, lr=0.1, L=1, K=32, delta_t=0.01, time_approx="outer", verbose=False,
                       device=dev(), backend="native")
    model.z_n = build_modules(dict(kind=kind), 4, model.N, 0.1, 42, dev())
    model.update_Phis()
    model.train()
    assert model.plan_name == "native" and isinstance(model._native_plan, psp.plan_affine_native.AffineNativePlan)
    assert len(model.loss_log) == 1 and math.isfinite(model.loss_log[0])


def test_notebook_configurations_plan_native():
    """The six Solver configurations of `Ornstein-Uhlenbeck - quadratic costs - linear ansatz.ipynb` (K and L reduced)."""
    prob = psp.LQGC(d=10, off_diag=0.1, T=0.5, seed=42, delta_t=0.005, device=dev())
    confs = [dict(loss_method="log-variance", detach_forward=True), dict(loss_method="moment", detach_forward=True, learn_Y_0=True),
             dict(loss_method="cross_entropy", detach_forward=True), dict(loss_method="relative_entropy", detach_forward=False),
             dict(loss_method="relative_entropy", detach_forward=False, random_X_0=True),
             dict(loss_method="log-variance", detach_forward=True, random_X_0=True)]
    for kw in confs:
        model = psp.Solver(name="nb", problem=prob, lr=0.1, L=1, K=64, delta_t=0.01, time_approx="outer",
                           adaptive_forward_process=True, IS_variance_K=256, verbose=False, device=dev(), **kw)
        model.z_n = build_modules(dict(kind="Linear"), 10, model.N, 0.1, 42, dev())
        model.update_Phis()
        model.train()
        assert model.plan_name == "native", (kw, model.plan_reason)
        assert len(model.IS_rel_log) == 1 and math.isfinite(model.IS_rel_log[0])
