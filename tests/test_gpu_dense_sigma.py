"""GPU parity of the dense constant sigma in the run-time-shaped value-net kernels (csrc/genl_kernels.h: genl_fwd_kernel<NW,
true>, the tables of B and B^T): the full-Hessian elliptic problem against the reference's goldens, and dense -- non-symmetric --
matrices on QuadraticOnBox against the oracle's autograd, which multiplies by problem.sigma(X) with torch.mm and so is a valid
oracle for any constant B.  The backward kernel is the one of sigma = s I: the gradient tests here are what proves that the
stored tangent direction B u^ is all it needs.

Bounds as for this kernel family (test_gpu_general_deep.py, test_gpu_genl_fuzz.py): loss <= 5e-5 relative on the first
iteration and <= 1e-4 after, first-iteration gradient <= 5e-4 max|g|, K_log exact.

Exit margin: the GPU forms X_n by fp32 MFMA products (k-ordered fmaf chains) where the CPU calls torch.mm, so X_n differs in
its last bits, and an exit test decides K_log.  Every case therefore first asserts that the CPU run never tested a point
closer than 1e-5 to the boundary (about a hundred fp32 ulps at 1; sphere: | |X_n| - 1 | over n >= 1, boxes: the distance of
every proposal coordinate to the faces) -- the goldens record that margin, the oracle cases measure it in the oracle run the
test does anyway -- and then demands K_log exactly.  The seeds were chosen on the CPU such that the oracle alone satisfies it."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_general_composite_golden import build as build_pkg
from test_gpu_genl_fuzz import check_against_oracle, expected_geometry, geometries, run_native
from util_cases import orc, psp

MIN_MARGIN = 1e-5
GOLDENS = ["expball_hess_d20_elliptic_diffusion", "expball_hess_d5_elliptic_bsde", "expball_hess_d4_elliptic_neumann"]
HESS = "ExponentialOnBallNonlinearSinHessian"


def dev():
    return torch.device("cuda:0")


def random_B(d, seed, scale=1.0):
    """Non-symmetric, entries O(scale / sqrt d): |B xi| = O(scale) per coordinate, as for scale I."""
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(d, d, generator=g) / math.sqrt(d)


# ---- the oracle with a dense B, and the exit margin of its run --------------------------------------------------------

def oracle_problem(case):
    kind, kw = case["problem"]["kind"], dict(case["problem"]["kwargs"])
    if kind == HESS:
        d, al = kw["d"], kw.get("alpha", 1.0)
        base = orc.make_problem("ExponentialOnBallNonlinearSin", **kw)
        B = math.sqrt(2.0 / d) * torch.ones(d, d)

        def h(x, y, z):
            return -2 * al * y * (2 * al * torch.sum(x, 1) ** 2 + d) + torch.sin(torch.exp(2 * al * torch.sum(x ** 2, 1)) - y ** 2)
        return dataclasses.replace(base, kind=kind, B=B, sigma=lambda x: B, h=h)
    B = kw.pop("B", None)
    base = orc.make_problem(kind, **kw)
    if B is None:
        return base
    B = torch.as_tensor(B, dtype=torch.float32)
    return dataclasses.replace(base, B=B, sigma=lambda x: B)


class ExitMargin:
    """Wraps the oracle's exit test: the smallest distance to the boundary of anything it decided on."""

    def __init__(self, monkeypatch):
        self.margin, self.n = float("inf"), 0
        test, sample = orc.exit_test, orc.sample_boundary

        def exit_test(problem, X, X_prop, elliptic):
            ex = problem.extra
            with torch.no_grad():
                if ex["boundary"] == "sphere":
                    if self.n >= 1:              # (X_0 is the same array on both sides)
                        r = torch.sqrt(torch.sum(X.double() ** 2, 1))
                        self.margin = min(self.margin, float(torch.min(torch.abs(r - ex["boundary_distance"]))))
                elif ex["boundary"] == "square":
                    dist = torch.abs(X_prop.double() - ex["X_r"])
                    if not ex["one_boundary"]:
                        dist = torch.minimum(dist, torch.abs(X_prop.double() - ex["X_l"]))
                    self.margin = min(self.margin, float(dist.min()))
            self.n += 1
            return test(problem, X, X_prop, elliptic)

        def sample_boundary(problem, Kb):        # once per iteration, before its time loop
            self.n = 0
            return sample(problem, Kb)
        monkeypatch.setattr(orc, "exit_test", exit_test)
        monkeypatch.setattr(orc, "sample_boundary", sample_boundary)


def oracle_run(case, monkeypatch, L=None):
    """util_cases.general_oracle_run for a problem with a dense B; out['min_exit_margin'] from the run itself."""
    rec = ExitMargin(monkeypatch)
    if "numpy_seed" in case:
        np.random.seed(case["numpy_seed"])
    prob = oracle_problem(case)
    s = case["solver"]
    common = dict(K=s["K"], N=s["N"], delta_t=s["delta_t"], lr=s["lr"], L=s["L"] if L is None else L, seed=s["seed"],
                  K_boundary=s["K_boundary"], loss_method=s["loss_method"],
                  adaptive_forward_process=s.get("adaptive_forward_process", False), K_test_log=s.get("K_test_log"))
    net = case.get("net")
    if case["family"] == "elliptic":
        cfg = orc.EllipticConfig(alpha=tuple(s.get("alpha", (1.0, 1.0))), boundary_type=s.get("boundary_type", "Dirichlet"), **common)
        out = orc.elliptic_train(prob, cfg, V=orc.elliptic_build(prob, cfg, net=net), trace=True)
    else:
        cfg = orc.GeneralConfig(alpha=tuple(s["alpha"]), **common)
        out = orc.general_train(prob, cfg, V=orc.general_build(prob, cfg, net=net), trace=True)
    out["min_exit_margin"] = rec.margin
    return out


def box_case(name, d, B, parabolic, quad_h, adaptive, one_boundary=False, K=40, N=12, loss="diffusion", arch=(30, 30), seed=42,
             L=2, dt=0.01):
    kw = dict(d=d, X_l=-1.0, X_r=0.8 if one_boundary else 1.0, one_boundary=one_boundary, parabolic=parabolic, quad_h=quad_h, B=B)
    if parabolic:
        kw["T"] = 1.5 * N * dt
    solver = dict(seed=seed, delta_t=dt, N=N, lr=0.001, L=L, K=K, K_boundary=10, loss_method=loss,
                  adaptive_forward_process=adaptive, alpha=[1.0, 0.5, 1.0] if parabolic else [1.0, 0.5])
    return dict(name=name, family="general_bounded" if parabolic else "elliptic", problem=dict(kind="QuadraticOnBox", kwargs=kw),
                solver=solver, net=dict(kind="densenet", arch=list(arch), seed=7), numpy_seed=9)


def hess_case(name, d, adaptive, K=40, N=12, loss="diffusion", arch=(30, 30), seed=42, L=2, dt=None, alpha=0.3, neumann=False):
    """(B xi has the norm sqrt(2 d) |N(0, 1)|: the default step keeps a move at 0.2 of the ball's radius, as the notebook's)"""
    dt = 0.02 / d if dt is None else dt
    kw = dict(d=d, alpha=alpha)
    solver = dict(seed=seed, delta_t=dt, N=N, lr=0.001, L=L, K=K, K_boundary=10, loss_method=loss,
                  adaptive_forward_process=adaptive, alpha=[1.0, 0.5])
    if neumann:
        kw["boundary_type"] = solver["boundary_type"] = "Neumann"
    return dict(name=name, family="elliptic", problem=dict(kind=HESS, kwargs=kw), solver=solver,
                net=dict(kind="densenet", arch=list(arch), seed=7))


def _d_in(case):
    return case["problem"]["kwargs"]["d"] + (0 if case["family"] == "elliptic" else 1)


def run_geometries(case, monkeypatch, nws=None):
    """The case under every PSP_GENL_NW setting its net admits, each against one oracle run; asserts the geometry that ran."""
    ref = oracle_run(case, monkeypatch)
    print("%s: oracle exit margin %.2e, K_log %s" % (case["name"], ref["min_exit_margin"], ref["K_log"]))
    assert ref["min_exit_margin"] >= MIN_MARGIN, ref["min_exit_margin"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    d_in, arch = _d_in(case), case["net"]["arch"]
    ran = []
    for nw in (nws or geometries(d_in, arch)):
        model, plan, seen = run_native(case, nw=nw, monkeypatch=monkeypatch)       # (fills the path store with NaN first)
        assert plan.gcfg.sigma_kind == psp.native.GENL_SIGMA_DENSE
        fwd, bwd = expected_geometry(d_in, arch, plan.K_local, nw, cus)
        assert int(plan.sizes.waves_per_tile) == fwd, (case["name"], nw, int(plan.sizes.waves_per_tile), fwd)
        err = check_against_oracle(case, model, seen, ref, what="PSP_GENL_NW=%s" % nw)
        losses = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, ref["loss_log"])]
        print("%s NW=%s: fwd<%d, dense> + %s, loss rel err %s, gradient rel err %.1e"
              % (case["name"], nw, fwd, bwd, ["%.1e" % e for e in losses], err))
        ran.append(fwd)
    return ran


# ---- the notebook's problem against the reference ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_loss_log_matches_reference_golden(name):
    rec = load_golden(name)
    exp = rec["expected"]
    assert exp["min_exit_margin"] >= MIN_MARGIN
    prob, model = build_pkg(rec["case"], device=dev(), backend="native")
    plan = model._choose_plan()
    assert model.plan_name == "native" and type(plan).__name__ == "GeneralDeepPlan"
    assert plan.gcfg.sigma_kind == psp.native.GENL_SIGMA_DENSE and plan.cfg.h_kind == psp.native.GH_EXPBALL_SIN_FULL
    plan.path.fill_(float("nan"))
    model.train()
    assert model._gen_plan is plan
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, exp["loss_log"])]
    print("%s: K_log %s, loss rel err per iteration vs the reference %s" % (name, model.K_log, ["%.1e" % e for e in errs]))
    assert model.K_log == exp["K_log"]
    assert len(model.loss_log) == len(exp["loss_log"])
    for l, (got, want) in enumerate(zip(model.loss_log, exp["loss_log"])):
        assert math.isclose(got, want, rel_tol=5e-5 if l == 0 else 1e-4), (l, model.loss_log, exp["loss_log"])
    assert len(model.V_L2_log) == len(exp["V_L2_log"])
    for got, want in zip(model.V_L2_log, exp["V_L2_log"]):
        assert math.isclose(got, want, rel_tol=1e-4, abs_tol=1e-9), (model.V_L2_log, exp["V_L2_log"])
    assert len(model.V_test_L2) == len(exp["V_test_L2"])                   # K_test_log: compute_test_error after every update
    for got, want in zip(model.V_test_L2, exp["V_test_L2"]):
        assert math.isclose(got, want, rel_tol=1e-4), (model.V_test_L2, exp["V_test_L2"])
    xp = torch.tensor(exp["probe_x"]).reshape(-1, prob.d).to(dev())
    with torch.no_grad():
        v = model.V(xp).squeeze().cpu()
    want = torch.tensor(exp["probe_V"])
    assert float((v - want).abs().max()) <= 1e-4 * max(1e-2, float(want.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_first_iteration_gradient_matches_oracle(name, monkeypatch):
    """The unchanged backward kernel on the stored direction U = act B u^."""
    case = load_golden(name)["case"]
    ref = oracle_run(case, monkeypatch, L=1)
    assert ref["min_exit_margin"] >= MIN_MARGIN
    model, plan, seen = run_native(case, L=1)
    err = check_against_oracle(case, model, seen, ref)
    print("%s: gradient rel err %.2e" % (name, err))


# ---- non-symmetric B: B against B^T, the B Z term of the quadratic h, B c ---------------------------------------------

NONSYM = [box_case("box_ell_quad_adapt", 6, random_B(6, 11), parabolic=False, quad_h=True, adaptive=True),
          box_case("box_ell_zero_plain", 6, random_B(6, 12), parabolic=False, quad_h=False, adaptive=False),
          box_case("box_ell_quad_plain_upper", 5, random_B(5, 13), parabolic=False, quad_h=True, adaptive=False, one_boundary=True),
          box_case("box_par_quad_adapt", 6, random_B(6, 14), parabolic=True, quad_h=True, adaptive=True, loss="BSDE"),
          box_case("box_par_zero_adapt_upper", 4, random_B(4, 15), parabolic=True, quad_h=False, adaptive=True, one_boundary=True),
          box_case("box_par_quad_plain", 7, random_B(7, 16), parabolic=True, quad_h=True, adaptive=False)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", NONSYM, ids=[c["name"] for c in NONSYM])
def test_nonsymmetric_matrix_matches_oracle(case, monkeypatch):
    B = case["problem"]["kwargs"]["B"]
    assert not torch.allclose(B, B.t(), atol=1e-2)
    run_geometries(case, monkeypatch)


# ---- d on both sides of the 16-block edges up to the family's limit, ragged K, every geometry -------------------------

# (a box in many dimensions: some coordinate of a uniform sample always sits near a face, so the matrices and steps shrink
#  with d -- a coordinate moves by scale sqrt(dt) per step -- until about half of the K N steps are active)
SWEEP = [hess_case("hess_d1", 1, adaptive=False, K=33, dt=0.01, alpha=0.5),
         box_case("box_d3", 3, random_B(3, 21), parabolic=True, quad_h=True, adaptive=True, K=17),
         hess_case("hess_d16", 16, adaptive=True, K=33, loss="BSDE", N=150),
         box_case("box_d17", 17, random_B(17, 22, 0.5), parabolic=False, quad_h=True, adaptive=True, K=21, arch=(50, 50, 50, 50),
                  dt=1e-3),
         hess_case("hess_d20_neumann", 20, adaptive=False, K=37, arch=(50, 50, 50, 50), neumann=True),
         box_case("box_d48", 48, random_B(48, 23, 0.5), parabolic=False, quad_h=False, adaptive=True, K=19, one_boundary=True,
                  dt=2e-4),
         hess_case("hess_d100", 100, adaptive=True, K=23, arch=(110, 110, 50)),
         box_case("box_d111_par", 111, random_B(111, 24, 0.3), parabolic=True, quad_h=True, adaptive=True, K=18, N=6, arch=(64, 33),
                  dt=1e-4),
         box_case("box_d111_ell", 111, random_B(111, 25, 0.3), parabolic=False, quad_h=True, adaptive=False, K=35, N=6, arch=(20,),
                  dt=1e-4)]


def test_sweep_covers_the_block_edges_and_geometries():
    """What the sweep reaches, without a GPU."""
    assert {c["problem"]["kwargs"]["d"] for c in SWEEP} == {1, 3, 16, 17, 20, 48, 100, 111}
    assert max(_d_in(c) for c in SWEEP) == 112
    assert all(c["solver"]["K"] % 16 for c in SWEEP)
    geo = set()
    for c in SWEEP:
        for nw in geometries(_d_in(c), c["net"]["arch"]):
            geo.add(expected_geometry(_d_in(c), c["net"]["arch"], c["solver"]["K"], nw, 256)[0])
    assert geo == {1, 4, 8}


@pytest.mark.gpu
@pytest.mark.parametrize("case", SWEEP, ids=[c["name"] for c in SWEEP])
def test_dimension_sweep_matches_oracle_under_every_geometry(case, monkeypatch):
    ran = run_geometries(case, monkeypatch)                  # (asserts per run that the geometry asked for is the one that ran)
    assert len(ran) == len(geometries(_d_in(case), case["net"]["arch"])) and set(ran) <= {1, 4, 8}


# ---- s I passed as a dense matrix ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("arch", [[30, 30, 30], [110, 110, 50]])
def test_scaled_identity_as_a_dense_matrix_agrees_with_the_identity_path(arch):
    """Summation order only: the products with s I add exact zeros."""
    s, d = 1.25, 20
    out = {}
    for dense in (False, True):
        kw = dict(d=d, X_l=-1.0, X_r=1.0, parabolic=False, quad_h=True)
        kw.update(dict(B=s * torch.eye(d)) if dense else dict(scale=s))
        case = dict(name="si", family="elliptic", problem=dict(kind="QuadraticOnBox", kwargs=kw), numpy_seed=9,
                    solver=dict(seed=42, delta_t=0.01, N=15, lr=0.001, L=2, K=150, K_boundary=10, loss_method="diffusion",
                                adaptive_forward_process=True, alpha=[1.0, 0.5]), net=dict(kind="densenet", arch=arch, seed=7))
        model, plan, seen = run_native(case)
        assert plan.gcfg.sigma_kind == (1 if dense else 0)
        out[dense] = (model.K_log, model.loss_log, seen[0][0])
    (k0, l0, g0), (k1, l1, g1) = out[False], out[True]
    print("s I dense against scaled identity: loss rel diff %s" % ["%.1e" % (abs(a - b) / abs(a)) for a, b in zip(l0, l1)])
    assert k0 == k1
    for a, b in zip(l0, l1):
        assert math.isclose(a, b, rel_tol=2e-6), (l0, l1)
    assert float((g0 - g1).abs().max()) <= 2e-5 * float(g0.abs().max())


# ---- device noise ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_philox_noise_is_finite_and_deterministic():
    case = load_golden("expball_hess_d20_elliptic_diffusion")["case"]
    runs = []
    for _ in range(2):
        prob, model = build_pkg(case, device=dev(), backend="native", L=2, noise="philox", K=1000, K_test_log=None)
        model.train()
        plan = model._gen_plan
        assert type(plan).__name__ == "GeneralDeepPlan" and plan.gcfg.sigma_kind == 1
        runs.append((model.loss_log, model.K_log, plan.YN.clone(), plan.VN.clone(), plan.XN.clone(), plan.grad.clone()))
    a, b = runs
    assert all(math.isfinite(v) for v in a[0]) and bool(torch.isfinite(a[5]).all()) and float(a[5].abs().max()) > 0
    assert 0 < a[1][0] < 1000 * case["solver"]["N"]                              # trajectories moved, and some left the ball
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)


# ---- validation ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_dense_kind_without_a_matrix_is_refused():
    nat = psp.native
    lib = nat.load()
    c = nat.GenlConfig()
    c.base.d, c.base.K_local, c.base.N = 20, 200, 20
    c.n_hidden, c.widths[0], c.widths[1] = 2, 30, 30
    sz = nat.GenlSizes()
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) == 0
    plain = int(sz.table_bytes)
    c.sigma_kind = nat.GENL_SIGMA_DENSE
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) != 0 and "sigma matrix missing" in nat.last_error()
    rc = lib.psp_genl_rollout_fwd(C.byref(c), None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None)
    assert rc != 0 and "sigma matrix missing" in nat.last_error()
    B = torch.eye(20, device=dev())
    c.sigma = nat.ptr(B)
    c.base.h_kind = nat.GH_EXPBALL_SIN_FULL
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) == 0
    assert int(sz.table_bytes) == plain + 2 * 2 * 2 * 256 * 4                    # B and B^T: DB0 x DB0 blocks of 256 floats
    c.sigma_kind = 2
    assert lib.psp_genl_query(C.byref(c), C.byref(sz)) != 0 and "enum" in nat.last_error()
