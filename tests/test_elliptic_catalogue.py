"""The exit-time and box-domain problems (DoubleWell_stopping, DoubleWell_stopping_linear, DoubleWell_expectation_hitting_time,
QuadraticGradient, Helmholtz, Oscillations, SinNorm2, ExponentialOnSphereParabolic, Committor_DoubleWell) without a GPU:

  * the composite torch plan against the reference's own runs on its own classes (tests/golden/cat_*.json, made by
    make_golden_elliptic_catalogue.py) within the bounds of test_general_composite_golden.py / test_pinn_composite_golden.py;
  * every general_native_spec() / native_vtrue_spec() against the class's own h / v_true in float64 on random points, through
    the float64 statement of the kinds in ref64_elliptic_catalogue.py;
  * what psp_gen_query / psp_genl_query / psp_pinn_query accept and refuse of PSP_GH_AFFINE_EXP / _SINE_SOURCE / _SINNORM2;
  * the plan reasons of what stays on the composite plan."""
import copy
import ctypes as C
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from pinn_cases import build as build_pinn, probe_values, seed_like_reference_train
from test_general_composite_golden import build
from util_cases import psp
import ref64_elliptic_catalogue as r64c
import ref64_general as r64

nat = psp.native
KEYS = ["dwstop", "dwstoplin", "dwhit", "quadgrad", "helmholtz", "oscillations"]
DIFFUSION = ["cat_%s_diffusion" % k for k in KEYS] + ["cat_sinnorm2_lin_d4_diffusion", "cat_sinnorm2_nl_d4_diffusion"]
BSDE = ["cat_helmholtz_bsde", "cat_oscillations_bsde"]
PINN = ["cat_%s_pinn" % k for k in KEYS]


def prepare(case, prob):
    """What the notebooks call on the problem before training (compute_reference_solution)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # (the hitting-time table takes log(0) for its unused control, as the reference)
        for call, kw in case["problem"].get("calls", []):
            getattr(prob, call)(**kw)
    return prob


# ---- the composite plan against the reference ------------------------------------------------------------------------

@pytest.mark.parametrize("name", DIFFUSION + BSDE)
def test_composite_matches_reference(name):
    rec = load_golden(name)
    exact = rec["torch"] == torch.__version__
    torch.set_num_threads(1)
    prob, model = build(rec["case"])
    prepare(rec["case"], prob)
    model.train()
    assert model.plan_name == "torch"
    exp = rec["expected"]
    assert exp["min_exit_margin"] >= 1e-5
    assert model.K_log == exp["K_log"]
    assert len(model.loss_log) == len(exp["loss_log"])
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert (got == want) if exact else math.isclose(got, want, rel_tol=1e-5)
    for got, want in zip(model.V_L2_log, exp["V_L2_log"]):
        assert math.isclose(got, want, rel_tol=1e-5)
    assert len(exp["V_test_L2"]) == len(exp["loss_log"]) == len(model.V_test_L2)      # K_test_log after every update
    for got, want in zip(model.V_test_L2 + model.V_test_abs, exp["V_test_L2"] + exp["V_test_abs"]):
        assert math.isclose(got, want, rel_tol=1e-5)
    xp = torch.tensor(exp["probe_x"]).reshape(-1, prob.d)
    with torch.no_grad():
        v = model.V(xp).squeeze()
    assert torch.allclose(v, torch.tensor(exp["probe_V"]), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", PINN)
def test_train_pinn_composite_matches_reference(name):
    rec = load_golden(name)
    exact = rec["torch"] == torch.__version__
    torch.set_num_threads(1)
    case, exp = rec["case"], rec["expected"]
    prob, model = build_pinn(case)
    prepare(case, prob)
    seed_like_reference_train(case, model)
    model.train_PINN()
    assert model.plan_name == "torch"
    assert len(model.loss_log) == len(exp["loss_log"]) and model.K == exp["K"]
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert (got == want) if exact else math.isclose(got, want, rel_tol=1e-5)
    for got, want in zip(model.V_L2_log, exp["V_L2_log"]):
        assert math.isclose(got, want, rel_tol=1e-5)
    v = probe_values(case, exp, prob, model)
    assert torch.allclose(v, torch.tensor(exp["probe_V"]), rtol=1e-5, atol=1e-7)


@functools.lru_cache(maxsize=None)
def reference64(name, K=None, arch=None):
    """(case, float64 first iteration) of a golden's case, optionally at another batch size / with a deep net; computed once."""
    case = copy.deepcopy(load_golden(name)["case"])
    case["solver"]["L"] = 1
    case["solver"].pop("K_test_log", None)
    if K is not None:
        case["solver"]["K"] = K
    if arch is not None:
        case["net"] = dict(kind="densenet", arch=list(arch), seed=7)
    prob, model = build(case, device="cpu", backend="torch")
    prepare(case, prob)
    ref = r64c.iteration(case, prob, r64.net64(model.V), r64c.draws(model))
    return case, ref



@pytest.mark.parametrize("name", DIFFUSION + BSDE)
def test_float64_statement_follows_the_reference_first_iteration(name):
    """The float64 iteration the GPU tests judge the gradient by, against the reference's fp32 run: the same K_log and the first
    loss within 1e-5 (fp32 rounding of the reference's own arithmetic)."""
    exp = load_golden(name)["expected"]
    case, ref = reference64(name)
    assert ref["K_count"] == exp["K_log"][0]
    assert ref["margins"]["exit"] >= 1e-5
    assert math.isclose(ref["loss"], exp["loss_log"][0], rel_tol=1e-5), (ref["loss"], exp["loss_log"][0])
    assert float(ref["grad"].abs().max()) > 0 and bool(torch.isfinite(ref["grad"]).all())


# ---- the specs against the classes' own formulas, float64 ---------------------------------------------------------------

def _problems():
    out = {}
    for cls in ("DoubleWell_stopping", "DoubleWell_stopping_linear", "DoubleWell_expectation_hitting_time"):
        out[cls] = getattr(psp, cls)(d=1, beta=1.5, device="cpu")
    out["QuadraticGradient"] = psp.QuadraticGradient(d=3, device="cpu")
    out["Helmholtz"] = psp.Helmholtz(d=2, device="cpu")
    out["Helmholtz_k"] = psp.Helmholtz(d=2, device="cpu")
    out["Helmholtz_k"].a_1, out["Helmholtz_k"].a_2, out["Helmholtz_k"].k = 2.0, 3.0, 1.7
    out["Oscillations"] = psp.Oscillations(d=1, device="cpu")
    out["Oscillations_a"] = psp.Oscillations(d=1, device="cpu")
    out["Oscillations_a"].a = 9
    out["SinNorm2_lin"] = psp.SinNorm2(d=4, linear=True, alpha=0.7, device="cpu")
    out["SinNorm2_nl"] = psp.SinNorm2(d=4, linear=False, alpha=1.3, device="cpu")
    return out


PROBLEMS = _problems()


@pytest.mark.parametrize("key", list(PROBLEMS))
def test_native_spec_states_the_class_h(key):
    prob = PROBLEMS[key]
    g = torch.Generator().manual_seed(5)
    K, d = 200, prob.d
    x = (torch.rand(K, d, generator=g, dtype=torch.float64) * 2 - 1)
    y = torch.randn(K, generator=g, dtype=torch.float64)
    z = torch.randn(K, d, generator=g, dtype=torch.float64)
    want = prob.h(x, y, z).to(torch.float64)
    got = r64c.h64(prob.general_native_spec())(None, x, y, z)
    assert got.shape == want.shape == (K,)
    scale = float(want.abs().max()) + 1.0
    assert float((got - want).abs().max()) <= 1e-12 * scale, (key, float((got - want).abs().max()), scale)


def test_exit_double_wells_describe_their_drift_and_domain():
    for cls in ("DoubleWell_stopping", "DoubleWell_stopping_linear", "DoubleWell_expectation_hitting_time"):
        prob = PROBLEMS[cls]
        spec = prob.general_native_spec()
        assert spec["drift"][0] == nat.DRIFT_DOUBLE_WELL and spec["dwell_form"] == 1
        x = torch.linspace(-2, 1, 50, dtype=torch.float64).reshape(-1, 1)
        assert torch.allclose(r64c.coeffs64(prob)["drift"](x), prob.b(x), rtol=1e-14, atol=0)
        assert spec["sigma_scale"] == float(prob.B[0, 0]) == (2.0 if "hitting" in cls else 1.0)
        assert (prob.boundary, prob.one_boundary, prob.X_l, prob.X_r) == ("square", True, -2.0, 1.0)


def test_parabolic_linear_sphere_problem_is_expball_lin_with_e_1():
    prob = psp.ExponentialOnSphereParabolic(d=3, T=0.5, alpha=0.7, device="cpu")
    assert not hasattr(prob, "boundary_type")                        # as the reference class: the notebook sets it
    spec = prob.general_native_spec()
    assert spec["h"] == nat.GH_EXPBALL_LIN
    al, d, e, tau = spec["h_par"]
    assert (al, d, e, tau) == (0.7, 3.0, 1.0, 0.0)
    g = torch.Generator().manual_seed(1)
    x, y = torch.rand(50, 3, generator=g, dtype=torch.float64) - 0.5, torch.randn(50, generator=g, dtype=torch.float64)
    want = prob.h(0.1, x, y, None)
    got = -2 * al * y * (2 * al * (x ** 2).sum(1) + d) - e * y
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-14)
    t = torch.rand(50, generator=g, dtype=torch.float64)
    vt = prob.native_vtrue_spec()
    assert vt["kind"] == nat.VTRUE_EXP
    assert torch.allclose(torch.exp(vt["par"][0] * (x ** 2).sum(1) + vt["par"][1] * t), prob.v_true(x, t), rtol=1e-13)


@pytest.mark.parametrize("key", ["QuadraticGradient", "Helmholtz", "Helmholtz_k", "Oscillations", "Oscillations_a", "SinNorm2_lin"])
def test_native_vtrue_spec_states_the_class_v_true(key):
    prob = PROBLEMS[key]
    g = torch.Generator().manual_seed(6)
    x = torch.rand(300, prob.d, generator=g, dtype=torch.float64) * 2 - 1
    want = prob.v_true(x).to(torch.float64)
    got = r64c.vtrue64(prob.native_vtrue_spec())(x)
    assert float((got - want).abs().max()) <= 1e-12 * (float(want.abs().max()) + 1.0)


def test_tabulated_v_true_keeps_the_reference_index_arithmetic():
    x = torch.tensor([[-2.5], [-2.0], [-1.0], [0.0], [0.975], [0.99], [1.5], [3.0]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for cls, hi, table in (("DoubleWell_stopping", 298, lambda p: -np.log(p.psi)), ("DoubleWell_stopping_linear", 298, lambda p: p.psi),
                               ("DoubleWell_expectation_hitting_time", 300, lambda p: p.psi)):
            prob = getattr(psp, cls)(device="cpu")
            prob.compute_reference_solution()
            assert prob.psi.shape == (400,) and prob.u.shape == (399,)
            i = np.clip(np.floor((x.squeeze().numpy() + np.float32(2)) / np.float32(0.01)).astype(np.int64), 0, hi)
            v = prob.v_true(x)
            assert tuple(v.shape) == (1, 8) and v.dtype == torch.float64
            assert np.array_equal(v.numpy()[0], table(prob)[i])
            assert int(i[-1]) == hi and int(i[0]) == 0
    # the pinned rows of the hitting-time table: psi = 0 on index_r .. 1.1 index_r (up to the solve's rounding)
    assert np.allclose(prob.psi[300:330], 0.0, atol=1e-12) and prob.psi[150] > 0.1


def test_committor_double_well_is_a_class_without_a_native_spec():
    prob = psp.Committor_DoubleWell(device="cpu")
    assert not hasattr(prob, "general_native_spec") and not hasattr(prob, "native_vtrue_spec")
    x, t = torch.zeros(4, 1), torch.zeros(4)
    assert torch.equal(prob.sigma(x, t), prob.B) and float(prob.B[0, 0]) == pytest.approx(math.sqrt(2.0))
    assert torch.equal(prob.h(x, t, torch.zeros(4), None), torch.zeros(4)) and torch.equal(prob.g(x, t), torch.ones(4))
    assert (prob.X_l, prob.X_r, prob.boundary_type) == (-2.0, 0.0, "Dirichlet")


# ---- validation (no GPU: the queries read no device memory) ---------------------------------------------------------------

def gen_cfg(h_kind, h_par, d=6, d_real=2):
    c = nat.GenConfig()
    c.d, c.H, c.K_local, c.N, c.dt, c.sqrt_dt, c.T, c.sigma_scale = d, 30, 64, 10, 0.01, 0.1, float("inf"), 1.0
    c.h_kind, c.d_real, c.store_path = h_kind, d_real, 1
    for i, v in enumerate(h_par):
        c.h_par[i] = v
    return c


def genl_cfg(h_kind, h_par, d=2, dense=False):
    c = nat.GenlConfig()
    c.base = gen_cfg(h_kind, h_par, d=d, d_real=d)
    c.n_hidden, c.widths[0], c.widths[1], c.widths[2] = 3, 10, 10, 10
    keep = None
    if dense:
        keep = torch.eye(d)
        c.sigma_kind, c.sigma = nat.GENL_SIGMA_DENSE, nat.ptr(keep)
    return c, keep


def pinn_cfg(h_kind, h_par, d=2, dense=False, has_time=0):
    c = nat.PinnConfig()
    c.d, c.K, c.has_time, c.n_hidden, c.h_kind, c.sigma_scale = d, 32, has_time, 2, h_kind, 1.0
    c.widths[0], c.widths[1] = 12, 12
    for i, v in enumerate(h_par):
        c.h_par[i] = v
    keep = None
    if dense:
        keep = torch.eye(d)
        c.sigma_kind, c.n_dirs, c.dirs = nat.GENL_SIGMA_DENSE, d, nat.ptr(keep)
    return c, keep


def test_gen_query_takes_the_scaled_identity_kinds_only():
    lib = nat.load()
    sz = nat.GenSizes()
    for kind, par in ((nat.GH_AFFINE_EXP, (1, 0, -0.5, 0)), (nat.GH_AFFINE_EXP, (0, 0, 0.5, -2)),
                      (nat.GH_SINE_SOURCE, (0, 3.1, 12.5, 1)), (nat.GH_SINE_SOURCE, (1, 6.2, 15.7, 0.1))):
        assert lib.psp_gen_query(C.byref(gen_cfg(kind, par)), C.byref(sz)) == 0, nat.last_error()
    for kind in (nat.GH_SINNORM2, nat.GH_EXPBALL_SIN_FULL):
        assert lib.psp_gen_query(C.byref(gen_cfg(kind, (1, 4, 1, 0))), C.byref(sz)) != 0      # (they read sum_i x_i: psp_genl_* only)
        assert "enum" in nat.last_error()
    assert lib.psp_gen_query(C.byref(gen_cfg(10, (0, 0, 0, 0))), C.byref(sz)) != 0 and "enum" in nat.last_error()
    assert lib.psp_gen_query(C.byref(gen_cfg(nat.GH_SINE_SOURCE, (2, 1, 1, 1))), C.byref(sz)) != 0 and "sub-mode" in nat.last_error()
    # Helmholtz reads x_0 and x_1: one real coordinate on the padded instance is refused, Oscillations is not
    assert lib.psp_gen_query(C.byref(gen_cfg(nat.GH_SINE_SOURCE, (0, 1, 1, 1), d_real=1)), C.byref(sz)) != 0 and "x_1" in nat.last_error()
    assert lib.psp_gen_query(C.byref(gen_cfg(nat.GH_SINE_SOURCE, (1, 1, 1, 1), d_real=1)), C.byref(sz)) == 0
    # the double-well drift in both roundings
    kappa = torch.ones(6)
    for form in (0, 1):
        c = gen_cfg(nat.GH_AFFINE_EXP, (1, 0, 0, 0), d_real=1)
        c.drift_kind, c.drift, c.dwell_form = nat.DRIFT_DOUBLE_WELL, nat.ptr(kappa), form
        c.domain_kind, c.dom_a, c.dom_b = nat.DOM_BOX_UPPER_ALL, -2.0, 1.0
        assert lib.psp_gen_query(C.byref(c), C.byref(sz)) == 0, nat.last_error()


def test_genl_query_accepts_and_refuses():
    lib = nat.load()
    sz = nat.GenlSizes()
    for kind, par in ((nat.GH_AFFINE_EXP, (0, 0, 0.5, -2)), (nat.GH_SINE_SOURCE, (0, 3.1, 12.5, 1)), (nat.GH_SINNORM2, (1, 2, 1, 0))):
        c, _ = genl_cfg(kind, par)
        assert lib.psp_genl_query(C.byref(c), C.byref(sz)) == 0, nat.last_error()
    plain = int(sz.table_bytes)                                       # SINNORM2 with s I: the dense path with the tables of s I
    c, keep = genl_cfg(nat.GH_SINNORM2, (1, 2, 0, 0), dense=True)
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) == 0 and int(sz.table_bytes) == plain
    c, _ = genl_cfg(nat.GH_ZERO, (0, 0, 0, 0))
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) == 0 and int(sz.table_bytes) < plain
    for kind, par in ((nat.GH_AFFINE_EXP, (0, 0, 0.5, -2)), (nat.GH_SINE_SOURCE, (1, 6.2, 15.7, 0.1))):
        c, keep = genl_cfg(kind, par, dense=True)
        assert lib.psp_genl_query(C.byref(c), C.byref(sz)) != 0 and "sigma = s I" in nat.last_error()
    c, _ = genl_cfg(nat.GH_SINE_SOURCE, (0, 1, 1, 1), d=1)
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) != 0 and "x_1" in nat.last_error()
    c, _ = genl_cfg(10, (0, 0, 0, 0))
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) != 0 and "enum" in nat.last_error()
    # a running cost and the adjoint sweep stay with PSP_GH_QUAD
    q = nat.GenlCoeffs()
    q.struct_bytes, q.runcost_kind = C.sizeof(nat.GenlCoeffs), nat.RUNCOST_DIAG_QUAD
    p = torch.ones(2)
    q.runcost = nat.ptr(p)
    for kind in (nat.GH_AFFINE_EXP, nat.GH_SINE_SOURCE, nat.GH_SINNORM2):
        c, _ = genl_cfg(kind, (1, 1, 1, 0))
        assert lib.psp_genl_query_lq(C.byref(c), C.byref(q), C.byref(sz)) != 0
        assert "PSP_GH_QUAD" in nat.last_error()


def test_pinn_query_accepts_and_refuses():
    lib = nat.load()
    sz = nat.PinnSizes()
    for kind, par in ((nat.GH_AFFINE_EXP, (1, 0, -0.5, 0)), (nat.GH_AFFINE_EXP, (0, 0, 0.5, -2)),
                      (nat.GH_SINE_SOURCE, (0, 3.1, 12.5, 1)), (nat.GH_SINE_SOURCE, (1, 6.2, 15.7, 0.1))):
        c, _ = pinn_cfg(kind, par)                                   # (h_par[3] is no time term for these kinds)
        assert lib.psp_pinn_query(C.byref(c), C.byref(sz)) == 0, nat.last_error()
    c, _ = pinn_cfg(nat.GH_SINNORM2, (1, 2, 1, 0))
    assert lib.psp_pinn_query(C.byref(c), C.byref(sz)) != 0 and "SINNORM2" in nat.last_error()
    c, keep = pinn_cfg(nat.GH_AFFINE_EXP, (0, 0, 0.5, -2), dense=True)      # reads z
    assert lib.psp_pinn_query(C.byref(c), C.byref(sz)) != 0 and "reads z" in nat.last_error()
    c, keep = pinn_cfg(nat.GH_AFFINE_EXP, (0, -1, 0, 0), dense=True)        # does not
    assert lib.psp_pinn_query(C.byref(c), C.byref(sz)) == 0, nat.last_error()
    c, _ = pinn_cfg(nat.GH_SINE_SOURCE, (0, 1, 1, 1), d=1)
    assert lib.psp_pinn_query(C.byref(c), C.byref(sz)) != 0 and "x_1" in nat.last_error()
    pairs = C.c_int64()
    for kind, par in ((nat.GH_AFFINE_EXP, (1, 0, -0.5, 0)), (nat.GH_SINE_SOURCE, (1, 6.2, 15.7, 0.1))):
        c, _ = pinn_cfg(kind, par, has_time=1)
        assert lib.psp_pinn_pairs_query(C.byref(c), C.byref(sz), C.byref(pairs)) != 0 and "psp_pinn_pairs" in nat.last_error()


def test_eval_query_takes_the_new_closed_forms():
    from path_space_pde_solver_amd import device_test_log as dtl
    net = dict(dims=[2, 16, 16, 1], act="relu2", linear=False)
    for key in ("QuadraticGradient", "Helmholtz", "Oscillations", "SinNorm2_lin"):
        prob = PROBLEMS[key]
        assert dtl.eval_reason(prob) is None
        cfg = dtl.eval_config(dict(net, dims=[prob.d, 16, 16, 1]), prob, 100, "elliptic")
        assert dtl.eval_query(cfg)[0] is not None, dtl.eval_query(cfg)[1]
    cfg = dtl.eval_config(dict(net, dims=[1, 16, 16, 1]), PROBLEMS["Oscillations"], 100, "elliptic")
    cfg.vtrue_kind = nat.VTRUE_SINPROD
    assert dtl.eval_query(cfg)[0] is None and "x_1" in dtl.eval_query(cfg)[1]
    cfg.vtrue_kind = nat.VTRUE_SINR2 + 1
    assert dtl.eval_query(cfg)[0] is None
    assert "table" in dtl.eval_reason(PROBLEMS["DoubleWell_stopping"])


# ---- what stays on the composite plan says why ---------------------------------------------------------------------------

def test_plan_reasons():
    from path_space_pde_solver_amd.plan_pinn_native import pinn_eligibility, h_reads_t
    for key in ("Helmholtz", "Oscillations", "QuadraticGradient"):     # h_par[3] is no time term for the new kinds
        assert not h_reads_t(PROBLEMS[key].general_native_spec())
    model = psp.EllipticSolver(problem=PROBLEMS["SinNorm2_lin"], name="t", verbose=False, device="cpu", loss_method="PINN")
    assert "dense sigma without full_hessian" in pinn_eligibility(model)
    model = psp.EllipticSolver(problem=PROBLEMS["SinNorm2_lin"], name="t", verbose=False, device="cpu", loss_method="PINN",
                               full_hessian=True, hessian="directions")
    assert "SINNORM2" in pinn_eligibility(model)
    model = psp.EllipticSolver(problem=PROBLEMS["Helmholtz"], name="t", verbose=False, device="cpu")
    model._choose_plan()
    assert model.plan_name == "torch" and "GPU" in model.plan_reason
    model = psp.EllipticSolver(problem=PROBLEMS["Helmholtz"], name="t", verbose=False, device="cpu", loss_method="PINN")
    assert "GPU" in pinn_eligibility(model)


def test_helmholtz_in_one_dimension_is_outside_the_kernels(monkeypatch):
    from path_space_pde_solver_amd import plan_general_native as pgn
    prob = psp.Helmholtz(d=1, device="cpu")
    model = psp.EllipticSolver(problem=prob, name="t", verbose=False, device="cpu")
    monkeypatch.setattr(model, "device", torch.device("cuda"))       # (the device test comes first; nothing is launched)
    assert "x_0 and x_1" in pgn.native_eligibility(model)
