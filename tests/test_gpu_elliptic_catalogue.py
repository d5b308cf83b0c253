"""The h kinds of the exit-time and box problems on the GPU (PSP_GH_AFFINE_EXP, PSP_GH_SINE_SOURCE in csrc/gen_kernels.h,
csrc/genl_kernels.h and the PINN finish kernel; PSP_GH_SINNORM2 in csrc/genl_kernels.h; PSP_VTRUE_LOGQ / _SINPROD / _SINSUM /
_SINR2 in csrc/genl_eval_kernels.h):

  * the native plans against the reference's own runs on its own classes (tests/golden/cat_*.json) with the bounds of
    test_gpu_dense_sigma.py: K_log exact after asserting the recorded exit margin, loss 5e-5 relative on the first iteration
    and 1e-4 after, V_L2_log and the test log 1e-4; the PINN goldens with the 1e-4 of test_gpu_pinn.py;
  * the first-iteration gradient against the float64 statement (ref64_elliptic_catalogue.py), within 5e-4 of max|g|;
  * PSP_GH_AFFINE_EXP with (0, 0, -1/2, 0) and (0, 0, 0, 0) against PSP_GH_QUAD / PSP_GH_ZERO on QuadraticOnBox;
  * the launch shapes: K = 16 and K = 48, d = 1 and d = 2 on the padded (6, 30) instance, a deep net on the run-time-shaped
    kernels for each kind, SinNorm2 at d = 4 -- against the float64 statement;
  * the device test log's per-point v_true against the class's v_true on the dumped points."""
import math

import pytest
import torch

from conftest import load_golden
from pinn_cases import build as build_pinn, probe_values, seed_like_reference_train
from test_elliptic_catalogue import BSDE, DIFFUSION, PINN, prepare, reference64
from test_general_composite_golden import build
from util_cases import psp

pytestmark = pytest.mark.gpu
nat = psp.native
MIN_MARGIN = 1e-5
KIND = {"DoubleWell_stopping": nat.GH_AFFINE_EXP, "DoubleWell_stopping_linear": nat.GH_AFFINE_EXP,
        "DoubleWell_expectation_hitting_time": nat.GH_AFFINE_EXP, "QuadraticGradient": nat.GH_AFFINE_EXP,
        "Helmholtz": nat.GH_SINE_SOURCE, "Oscillations": nat.GH_SINE_SOURCE, "SinNorm2": nat.GH_SINNORM2}


def dev():
    return torch.device("cuda:0")


def run_native(case, **over):
    """The case on the GPU with nothing but the problem and the solver arguments set: (prob, model, plan, first gradient)."""
    prob, model = build(case, device=dev(), **over)
    prepare(case, prob)
    plan = model._choose_plan()
    assert model.plan_name == "native", model.plan_reason
    kind = case["problem"]["kind"]
    assert plan.cfg.h_kind == KIND[kind]
    assert type(plan).__name__ == ("GeneralDeepPlan" if (kind == "SinNorm2" or "net" in case) else "GeneralNativePlan")
    if "DoubleWell" in kind:
        assert plan.cfg.dwell_form == 1 and plan.cfg.domain_kind == nat.DOM_BOX_UPPER_ALL
    plan.path.fill_(float("nan"))
    seen = []
    step = plan.iteration

    def iteration(l):
        out = step(l)
        seen.append(plan.grad.detach().cpu().clone())
        return out
    plan.iteration = iteration
    model.train()
    assert model._gen_plan is plan
    return prob, model, plan, seen[0]


def check_first_iteration(name, K=None, arch=None):
    case, ref = reference64(name, K, arch)
    assert ref["margins"]["exit"] >= MIN_MARGIN, ref["margins"]
    prob, model, plan, g = run_native(case)
    g64 = ref["grad"]
    eg = float((g.double() - g64).abs().max()) / float(g64.abs().max())
    el = abs(model.loss_log[0] - ref["loss"]) / abs(ref["loss"])
    print("%s K=%s arch=%s: %s, K_log %s, loss rel err %.1e, gradient err %.1e of max|g|"
          % (name, case["solver"]["K"], arch, type(plan).__name__, model.K_log, el, eg))
    assert model.K_log == [ref["K_count"]]
    assert el <= 5e-5, (model.loss_log, ref["loss"])
    assert eg <= 5e-4, eg
    return plan


# ---- the reference's goldens -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", DIFFUSION + BSDE)
def test_loss_log_matches_reference_golden(name):
    """The bounds of test_gpu_dense_sigma.py, unchanged.  Measured on an MI355X over the ten cases: K_log exact, loss within 4.6e-7
    relative of the reference in every iteration (each case prints its figures)."""
    rec = load_golden(name)
    exp = rec["expected"]
    assert exp["min_exit_margin"] >= MIN_MARGIN
    prob, model, plan, _ = run_native(rec["case"])
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    print("%s: K_log %s, loss rel err per iteration vs the reference %s" % (name, model.K_log, ["%.1e" % e for e in errs]))
    assert model.K_log == exp["K_log"]
    assert len(model.loss_log) == len(exp["loss_log"])
    for l, (got, want) in enumerate(zip(model.loss_log, exp["loss_log"])):
        assert math.isclose(got, want, rel_tol=5e-5 if l == 0 else 1e-4), (l, model.loss_log, exp["loss_log"])
    assert len(model.V_L2_log) == len(exp["V_L2_log"])
    for got, want in zip(model.V_L2_log, exp["V_L2_log"]):
        assert math.isclose(got, want, rel_tol=1e-4, abs_tol=1e-9), (model.V_L2_log, exp["V_L2_log"])
    assert len(model.V_test_L2) == len(exp["V_test_L2"]) == len(exp["loss_log"])
    for got, want in zip(model.V_test_L2 + model.V_test_abs, exp["V_test_L2"] + exp["V_test_abs"]):
        assert math.isclose(got, want, rel_tol=1e-4), (model.V_test_L2, exp["V_test_L2"])
    xp = torch.tensor(exp["probe_x"]).reshape(-1, prob.d).to(dev())
    with torch.no_grad():
        v = model.V(xp).squeeze().cpu()
    want = torch.tensor(exp["probe_V"])
    assert float((v - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


@pytest.mark.parametrize("name", PINN)
def test_train_pinn_matches_reference_golden(name):
    rec = load_golden(name)
    case, exp = rec["case"], rec["expected"]
    prob, model = build_pinn(case, device=dev())
    prepare(case, prob)
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "native", model.plan_reason
    assert model._pinn_plan.cfg.h_kind == KIND[case["problem"]["kind"]]
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    print("%s: loss rel err per iteration %s" % (name, ["%.1e" % e for e in errs]))
    assert len(model.loss_log) == len(exp["loss_log"]) and max(errs) <= 1e-4, (model.loss_log, exp["loss_log"])
    for a, b in zip(model.V_L2_log, exp["V_L2_log"]):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-12, (model.V_L2_log, exp["V_L2_log"])
    v, want = probe_values(case, exp, prob, model), torch.tensor(exp["probe_V"])
    assert float((v - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


@pytest.mark.parametrize("name", DIFFUSION + BSDE)
def test_first_iteration_gradient_matches_float64(name):
    check_first_iteration(name)


# ---- launch shapes ---------------------------------------------------------------------------------------------------------

SHAPES = [("cat_oscillations_diffusion", 16, None), ("cat_oscillations_diffusion", 48, None),        # d = 1 on (6, 30)
          ("cat_helmholtz_diffusion", 16, None), ("cat_helmholtz_diffusion", 48, None),              # d = 2 on (6, 30)
          ("cat_dwstop_diffusion", 48, None), ("cat_quadgrad_diffusion", 16, None),
          ("cat_helmholtz_diffusion", 48, (10, 10, 10)), ("cat_oscillations_diffusion", 16, (10, 10, 10)),
          ("cat_quadgrad_diffusion", 48, (10, 10, 10)), ("cat_dwhit_diffusion", 16, (10, 10, 10)),
          ("cat_sinnorm2_lin_d4_diffusion", 16, None), ("cat_sinnorm2_nl_d4_diffusion", 48, None)]


@pytest.mark.parametrize("name,K,arch", SHAPES, ids=["%s-K%d-%s" % (n[4:-10], K, "deep" if a else "default") for n, K, a in SHAPES])
def test_launch_shapes_match_float64(name, K, arch):
    plan = check_first_iteration(name, K, arch)
    if type(plan).__name__ == "GeneralNativePlan":
        assert (plan.d_pad, plan.H_pad) == (6, 30)


# ---- the new kind on the parameters of the old ones ------------------------------------------------------------------------

@pytest.mark.parametrize("arch", [None, (10, 10, 10)], ids=["templated", "deep"])
@pytest.mark.parametrize("quad", [True, False], ids=["quad", "zero"])
def test_affine_exp_reproduces_quad_and_zero(quad, arch):
    """PSP_GH_AFFINE_EXP with (0, 0, -1/2, 0) / (0, 0, 0, 0) against PSP_GH_QUAD / PSP_GH_ZERO on QuadraticOnBox, adaptive forward
    process: the tangent coefficient (-2 p2) dt against dt, and -(p2 S) against S / 2.  Observed on an MI355X: 0 (bit-identical
    Y_N, V_N, X_N and gradient) in all four cases; the bound is the issue's 1e-6."""
    case = dict(name="box", family="elliptic", numpy_seed=9,
                problem=dict(kind="QuadraticOnBox", kwargs=dict(d=2, X_l=-1.0, X_r=1.0, parabolic=False, quad_h=quad, scale=1.2)),
                solver=dict(seed=42, delta_t=0.01, N=12, lr=0.001, L=1, K=48, K_boundary=10, loss_method="diffusion",
                            adaptive_forward_process=True, alpha=[1.0, 0.5]))
    if arch is not None:
        case["net"] = dict(kind="densenet", arch=list(arch), seed=7)
    out = []
    for affine in (False, True):
        prob, model = build(case, device=dev())
        if affine:
            spec = dict(prob.general_native_spec(), h=nat.GH_AFFINE_EXP, h_par=(0.0, 0.0, -0.5 if quad else 0.0, 0.0))
            prob.general_native_spec = lambda spec=spec: spec
        plan = model._choose_plan()
        assert model.plan_name == "native", model.plan_reason
        assert plan.cfg.h_kind == (nat.GH_AFFINE_EXP if affine else (nat.GH_QUAD if quad else nat.GH_ZERO))
        model.train()
        out.append((model.K_log, [plan.YN.clone(), plan.VN.clone(), plan.XN.clone(), plan.grad.clone()]))
    (k0, a), (k1, b) = out
    assert k0 == k1 and k0[0] > 0
    worst = 0.0
    for u, v in zip(a, b):
        assert bool(torch.isfinite(u).all()) and float(u.abs().max()) > 0
        worst = max(worst, float((u - v).abs().max()) / float(u.abs().max()))
    print("AFFINE_EXP against %s (%s): largest relative difference %.1e" % ("QUAD" if quad else "ZERO", arch or "templated", worst))
    assert worst <= 1e-6


# ---- device test log -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,kw", [("QuadraticGradient", dict(d=3)), ("Helmholtz", dict(d=2)), ("Oscillations", dict(d=1)),
                                     ("SinNorm2", dict(d=4))])
def test_device_test_log_v_true_matches_the_class(kind, kw):
    from path_space_pde_solver_amd.utilities import compute_test_error_native
    prob = getattr(psp, kind)(device=dev(), **kw)
    model = psp.EllipticSolver(problem=prob, name="t", verbose=False, device=dev(), seed=3)
    K = 1000
    l2, mae, mre, pts = compute_test_error_native(model, prob, K, "elliptic", seed=11, iteration=1, return_points=True)
    x = pts["x"]
    assert tuple(x.shape) == (K, prob.d) and bool(pts["keep"].all())
    want = prob.v_true(x).float()
    err = float((pts["v_true"] - want).abs().max()) / float(want.abs().max())
    print("%s: per-point v_true against the class, relative to max|v_true|: %.1e" % (kind, err))
    assert err <= 1e-6
    with torch.no_grad():
        e = want - model.V(x).squeeze()
    assert math.isclose(l2, float((e.double() ** 2).mean()), rel_tol=1e-4) and math.isclose(mae, float(e.double().abs().mean()), rel_tol=1e-4)
    if kind in ("Helmholtz", "Oscillations"):                        # the sampler fills the box the class names
        assert float(x.min()) >= prob.X_l and float(x.max()) <= prob.X_r and float(x.max() - x.min()) > 0.9 * (prob.X_r - prob.X_l)


# ---- the parabolic linear problem --------------------------------------------------------------------------------------------

def test_parabolic_linear_sphere_problem_plans_native_once_boundary_type_is_set():
    prob = psp.ExponentialOnSphereParabolic(d=4, T=0.3, alpha=0.5, device=dev())
    prob.boundary_type = "Dirichlet"
    model = psp.GeneralSolver(problem=prob, name="t", verbose=False, device=dev(), seed=42, delta_t=0.01, N=20, L=2, K=48,
                              K_boundary=10)
    model.train()
    assert model.plan_name == "native", model.plan_reason
    assert model._gen_plan.cfg.h_kind == nat.GH_EXPBALL_LIN and list(model._gen_plan.cfg.h_par) == [0.5, 4.0, 1.0, 0.0]
    _, twin = None, psp.GeneralSolver(problem=psp.ExponentialOnSphereParabolic(d=4, T=0.3, alpha=0.5, device="cpu"), name="t",
                                      verbose=False, device="cpu", seed=42, delta_t=0.01, N=20, L=2, K=48, K_boundary=10)
    twin.problem.boundary_type = "Dirichlet"
    twin.train()
    assert twin.plan_name == "torch" and model.K_log == twin.K_log
    for got, want in zip(model.loss_log, twin.loss_log):
        assert math.isclose(got, want, rel_tol=1e-4), (model.loss_log, twin.loss_log)
