"""Solver(approx_method='value_function') on LLGC with off-diagonal entries and on LQGC: the linear-quadratic instances of the
run-time-shaped value-net kernels (csrc/genl_kernels.h genl_fwd_kernel<NW, true, true>: Z = B grad_x V, the drift product
(dt A) X, the running cost at the moved state; plan_value_native.py, psp_genl_rollout_fwd_lq) against the CPU oracle
(oracle/pathspace_oracle.py hjb_train(approx_method='value_function'), generic in problem.b / sigma / h and pinned bit for bit on the
reference's own lqgc_d3_value_function run).  The backward kernel is the one of sigma = s I: the gradient tests are what proves that
the stored tangent direction B^T u is all it needs.

Bounds as for this kernel family (test_gpu_value_function.py, test_gpu_dense_sigma.py): first-iteration loss <= 5e-5 relative,
first-iteration gradient <= 5e-4 max|g| (output bias excluded), whole loss log <= 1e-4 relative."""
import copy
import ctypes as C
import functools
import math

import pytest
import torch

from test_gpu_genl_fuzz import _dwell, run_native
from util_cases import make_oracle, make_pkg_solver, orc, psp

pytestmark = pytest.mark.gpu
nat = psp.native

VF = dict(approx_method="value_function", time_approx="inner", u_l2_error_flag=False, early_stopping_time=None, seed=42, L=3,
          lr=0.005)
CASES = {
    # non-symmetric A and B: B against B^T, A against A^T; ragged K (three tiles, eight live rows in the last)
    "llgc_d8_off": dict(
        problem=dict(kind="LLGC", kwargs=dict(d=8, off_diag=0.1, T=0.4, seed=42)),
        solver=dict(VF, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, delta_t=0.02, K=40)),
    # c = 0; the time input in the second 16-feature block (DB0 = 2)
    "llgc_d17_off_nonadaptive_moment": dict(
        problem=dict(kind="LLGC", kwargs=dict(d=17, off_diag=0.1, T=0.3, seed=42)),
        solver=dict(VF, loss_method="moment", adaptive_forward_process=False, detach_forward=False, delta_t=0.02, K=40)),
    # the running cost at X_{n+1}, dense A and B together
    "lqgc_d5": dict(
        problem=dict(kind="LQGC", kwargs=dict(d=5, off_diag=0.1, T=0.5, seed=42, delta_t=0.05)),
        solver=dict(VF, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, delta_t=0.05, K=40)),
    # the state fills block 0 exactly, the time alone in block 1; three layers
    "lqgc_d16_arch3": dict(
        problem=dict(kind="LQGC", kwargs=dict(d=16, off_diag=0.05, T=0.3, seed=42, delta_t=0.05)),
        solver=dict(VF, loss_method="log-variance", adaptive_forward_process=True, detach_forward=True, delta_t=0.05, K=40),
        net=dict(kind="value_densenet", arch=[20, 16, 12], seed=7)),
    # sigma = I and a diagonal drift routed through the dense path because of the running cost; D0 = 16 exactly
    "lqgc_d15_diag": dict(
        problem=dict(kind="LQGC", kwargs=dict(d=15, off_diag=0.0, T=0.3, seed=42, delta_t=0.05)),
        solver=dict(VF, loss_method="moment", adaptive_forward_process=True, detach_forward=True, delta_t=0.05, K=24)),
}
for _name, _case in CASES.items():
    _case.update(name=_name, family="solver")
NAMES = list(CASES)


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def oracle(name):
    """One oracle run per case (L = 3, traced), shared by the tests and left unchanged."""
    torch.set_num_threads(4)
    oprob, ocfg, omodels = make_oracle(CASES[name])
    ref = orc.hjb_train(oprob, ocfg, step_models=omodels, trace=True)
    g = torch.cat([g.reshape(-1) for g in ref["traces"][0]["grads"]])
    return tuple(ref["loss_log"]), g


def native_run(name, **over):
    model = make_pkg_solver(copy.deepcopy(CASES[name]), dev(), backend="native", **over)
    model.train()
    assert model.plan_name == "native", (model.plan_name, getattr(model, "plan_reason", None))
    plan = model._native_plan
    assert isinstance(plan, psp.plan_value_native.ValueNativePlan) and plan.deep is not None
    assert plan.coeffs is not None and plan.coeffs.z_kind == nat.GENL_Z_SIGMA
    return model, plan


@pytest.mark.parametrize("name", NAMES)
def test_first_iteration_loss_and_gradient_match_the_oracle(name):
    model, plan = native_run(name, L=1)
    loss_ref, g_ref = oracle(name)
    g = plan.grad.cpu()
    assert g.shape == g_ref.shape
    # (the output bias is excluded: neither loss term depends on a constant offset of the value net)
    err = float((g - g_ref)[:-1].abs().max()) / float(g_ref.abs().max())
    print("%s: gradient rel err %.1e, loss %.6e vs %.6e (rel %.1e)"
          % (name, err, model.loss_log[0], loss_ref[0], abs(model.loss_log[0] - loss_ref[0]) / abs(loss_ref[0])))
    assert math.isclose(model.loss_log[0], loss_ref[0], rel_tol=5e-5), (model.loss_log, loss_ref)
    assert err <= 5e-4, err


@pytest.mark.parametrize("name", NAMES)
def test_loss_log_matches_the_oracle(name):
    model, plan = native_run(name)
    loss_ref, _ = oracle(name)
    errs = [abs(a - b) / abs(b) for a, b in zip(model.loss_log, loss_ref)]
    print("%s: loss rel err per iteration vs the oracle %s" % (name, ["%.1e" % e for e in errs]))
    assert len(model.loss_log) == len(loss_ref) == 3
    for a, b in zip(model.loss_log, loss_ref):
        assert math.isclose(a, b, rel_tol=1e-4), (model.loss_log, loss_ref)


def test_cases_take_the_paths_they_are_meant_to():
    """Without a run: which coefficients each case hands to the kernel."""
    kinds = {}
    for name, case in CASES.items():
        pb = getattr(psp, case["problem"]["kind"])(device="cpu", **case["problem"]["kwargs"])
        spec = pb.native_spec()
        kinds[name] = (spec["sigma"][0], spec["drift"][0], spec["runcost"][0])
        assert psp.plan_value_native.needs_lq(spec)
    dense = (nat.SIGMA_DENSE, nat.DRIFT_DENSE)
    assert kinds["llgc_d8_off"] == dense + (nat.RUNCOST_ZERO,) == kinds["llgc_d17_off_nonadaptive_moment"]
    assert kinds["lqgc_d5"] == dense + (nat.RUNCOST_DIAG_QUAD,) == kinds["lqgc_d16_arch3"]
    assert kinds["lqgc_d15_diag"] == (nat.SIGMA_IDENTITY, nat.DRIFT_DIAG, nat.RUNCOST_DIAG_QUAD)


# ---- the entry point itself ---------------------------------------------------------------------------------------------

def raw_forward(plan, gcfg, coeffs, x0, t0, xi, lq=True):
    """One psp_genl_rollout_fwd[_lq] call on buffers of its own; returns VN, YN, XN, the path store and the coefficients a^."""
    lib, d = plan.lib, int(gcfg.base.d)
    K, f32 = int(gcfg.base.K_local), torch.float32
    sz = nat.GenlSizes()
    ref = C.byref(coeffs) if coeffs is not None else None
    nat.check(lib.psp_genl_query_lq(C.byref(gcfg), ref, C.byref(sz)), "psp_genl_query_lq")
    tables = torch.zeros(sz.table_bytes // 4, dtype=f32, device=dev())
    path = torch.zeros(sz.path_bytes // 4, dtype=f32, device=dev())
    ahat = torch.zeros((sz.ahat_bytes + 3) // 4, dtype=f32, device=dev())
    VN, YN, tN = (torch.zeros(K, dtype=f32, device=dev()) for _ in range(3))
    XN = torch.zeros(K, d, dtype=f32, device=dev())
    kcount = torch.zeros(1, dtype=torch.int64, device=dev())
    st = nat.stream_ptr(dev())
    tail = (nat.ptr(plan.flat), nat.ptr(x0), nat.ptr(t0), nat.ptr(xi), 42, 0, nat.ptr(tables), nat.ptr(path), nat.ptr(ahat),
            nat.ptr(VN), nat.ptr(YN), nat.ptr(XN), nat.ptr(tN), nat.ptr(kcount), st)
    if lq:
        nat.check(lib.psp_genl_rollout_fwd_lq(C.byref(gcfg), ref, *tail), "psp_genl_rollout_fwd_lq")
    else:
        nat.check(lib.psp_genl_rollout_fwd(C.byref(gcfg), *tail), "psp_genl_rollout_fwd")
    torch.cuda.synchronize()
    return dict(VN=VN, YN=YN, XN=XN, path=path, ahat=ahat, kcount=kcount)


def supplied_inputs(gcfg, seed, scale=0.5):
    d, K, N = int(gcfg.base.d), int(gcfg.base.K_local), int(gcfg.base.N)
    g = torch.Generator().manual_seed(seed)
    x0 = (scale * torch.randn(K, d, generator=g)).to(dev())
    xi = torch.randn(N, K, d, generator=g).to(dev()).contiguous()
    return x0, torch.zeros(K, device=dev()), xi


def config_copy(gcfg):
    c = nat.GenlConfig()
    C.memmove(C.byref(c), C.byref(gcfg), C.sizeof(nat.GenlConfig))
    c.base.noise_mode = nat.NOISE_SUPPLIED
    return c


def test_null_coefficients_are_a_no_op():
    """A NULL struct, an all-zero one and one that asks for nothing dispatch to the kernel instance of psp_genl_rollout_fwd."""
    model, plan, seen = run_native(_dwell(5, [12, 10], K=40, N=6))
    gcfg = config_copy(plan.gcfg)
    x0, t0, xi = supplied_inputs(gcfg, 5)
    want = raw_forward(plan, gcfg, None, x0, t0, xi, lq=False)
    assert bool(torch.isfinite(want["YN"]).all()) and float(want["XN"].abs().max()) > 0 and int(want["kcount"]) > 0
    for coeffs in (None, nat.GenlCoeffs(), nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs))):
        got = raw_forward(plan, gcfg, coeffs, x0, t0, xi)
        for key in ("VN", "YN", "XN", "path", "ahat", "kcount"):
            assert torch.equal(got[key], want[key]), key


def test_dense_drift_product_agrees_with_the_diagonal_drift():
    """GeneralSolver's orientation (Z = B^T grad_x V) with the drift as a matrix diag(a), against the diagonal drift kind of the
    plain kernels on the same inputs: the A product, which no Solver plan reaches in this orientation.  The two differ by the
    fp32 summation order the dense-sigma tests accept (products with s I and diag(a) add exact zeros): 1e-5 on O(1) states."""
    d = 20
    model, plan, seen = run_native(_dwell(d, [30, 30, 30], K=24, N=6))
    gcfg = config_copy(plan.gcfg)
    assert gcfg.base.h_kind == nat.GH_QUAD and gcfg.sigma_kind == nat.GENL_SIGMA_SCALED
    x0, t0, xi = supplied_inputs(gcfg, 6)
    g = torch.Generator().manual_seed(7)
    a = (-(0.5 + torch.rand(d, generator=g))).to(dev())
    gcfg.base.drift_kind, gcfg.base.drift = nat.DRIFT_DIAG, a.data_ptr()
    want = raw_forward(plan, gcfg, None, x0, t0, xi, lq=False)
    A = torch.diag(a).contiguous()
    gcfg.base.drift_kind, gcfg.base.drift = nat.DRIFT_ZERO, None
    q = nat.GenlCoeffs(struct_bytes=C.sizeof(nat.GenlCoeffs), z_kind=nat.GENL_Z_SIGMA_T, drift_matrix=A.data_ptr())
    got = raw_forward(plan, gcfg, q, x0, t0, xi)
    none = raw_forward(plan, gcfg, None, x0, t0, xi)                 # no drift at all: the product matters at this scale
    ex, ey = float((got["XN"] - want["XN"]).abs().max()), float((got["YN"] - want["YN"]).abs().max())
    print("dense drift against diagonal drift: |dXN| %.1e, |dYN| %.1e; states up to %.2f, drift moved them by %.1e"
          % (ex, ey, float(want["XN"].abs().max()), float((none["XN"] - want["XN"]).abs().max())))
    assert float((none["XN"] - want["XN"]).abs().max()) > 1e-3
    assert 0.1 < float(want["XN"].abs().max()) < 10 and int(got["kcount"]) == int(want["kcount"]) > 0
    assert ex <= 1e-5 and ey <= 1e-5
    assert float((got["VN"] - want["VN"]).abs().max()) <= 1e-5


def test_philox_noise_is_finite_and_deterministic():
    runs = []
    for _ in range(2):
        model, plan = native_run("llgc_d8_off", noise="philox", K=4096, L=2)
        runs.append((model.loss_log, plan.grad.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert len(runs[0][0]) == 2 and all(math.isfinite(v) for v in runs[0][0]) and bool(torch.isfinite(runs[0][1]).all())
    assert float(runs[0][1].abs().max()) > 0
