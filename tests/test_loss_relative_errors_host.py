"""utilities.loss_relative_errors and psp_loss_stats_*: host logic, no GPU -- argument validation, the plan reasons, the refusals,
the chunk rounding, the float64 host statistics against numpy, and the ABI's argument checks (no launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref64_loss_relerr as r64
from util_cases import psp

U = psp.utilities
nat = psp.native


def llgc(d=3, **kw):
    return psp.LLGC(d=d, off_diag=0.1, T=1, seed=7, device="cpu", **kw)


def dense(d=3):
    return psp.DenseNet(d_in=d + 1, d_out=d, lr=0.05)


def test_arguments_are_validated():
    p, net = llgc(), dense()
    with pytest.raises(ValueError, match="backend"):
        U.loss_relative_errors(p, net, 16, delta_t=0.125, backend="hip")
    with pytest.raises(ValueError, match="noise"):
        U.loss_relative_errors(p, net, 16, delta_t=0.125, noise="sobol")
    with pytest.raises(ValueError, match="K must be positive"):
        U.loss_relative_errors(p, net, 0, delta_t=0.125)
    with pytest.raises(ValueError, match="no time step"):
        U.loss_relative_errors(p, net, 16, delta_t=2.0)
    with pytest.raises(ValueError, match="seed"):
        U.loss_relative_errors(p, net, 16, delta_t=0.125, noise="philox", seed=None)
    with pytest.raises(ValueError, match="chunk must be positive"):
        U.loss_relative_errors(p, net, 16, delta_t=0.125, chunk=0)
    with pytest.raises(TypeError, match="control"):
        U.loss_relative_errors(p, 3.0, 16, delta_t=0.125)
    with pytest.raises(ValueError, match="one net per time step"):
        U.loss_relative_errors(p, [psp.DenseNet(3, 3, lr=0.05) for _ in range(5)], 16, delta_t=0.125)


def test_plan_reasons_on_the_composite_plan():
    p, net = llgc(), dense()
    kw = dict(delta_t=0.125, noise="reference", seed=3)
    out = U.loss_relative_errors(p, net, 16, **kw)
    assert out["plan"] == "torch" and "GPU" in out["plan_reason"] and "cpu" in out["plan_reason"]
    assert out["K"] == 16 and out["N"] == 8
    user = torch.nn.Sequential(torch.nn.Linear(4, 3))
    out = U.loss_relative_errors(p, user, 16, **kw)
    assert out["plan"] == "torch" and "user net" in out["plan_reason"]
    q = psp.LLGC_general_f(d=3, off_diag=0.1, T=1, seed=7, device="cpu")
    out = U.loss_relative_errors(q, net, 16, **kw)
    assert out["plan"] == "torch" and ("native_spec" in out["plan_reason"] or "native catalogue" in out["plan_reason"])
    out = U.loss_relative_errors(p, net, 16, backend="torch", **kw)
    assert out["plan_reason"] == "backend='torch' requested"


def test_backend_native_raises_where_the_kernels_do_not_reach():
    p = llgc()
    with pytest.raises(NotImplementedError, match="native loss_relative_errors unavailable"):
        U.loss_relative_errors(p, dense(), 16, delta_t=0.125, backend="native", device="cpu")
    with pytest.raises(NotImplementedError, match="user net"):
        U.loss_relative_errors(p, torch.nn.Linear(4, 3), 16, delta_t=0.125, backend="native")


def test_refusals_are_made_before_any_work():
    p = llgc()

    def never(*a):
        raise AssertionError("the control was evaluated")
    with pytest.raises(ValueError, match=r"return_samples.*2\*\*24"):
        U.loss_relative_errors(p, never, U.LRE_MAX_SAMPLES + 1, return_samples=True)
    K = U.LRE_REFERENCE_NOISE_LIMIT // (200 * 3) + 1
    with pytest.raises(ValueError, match=r"noise='reference'.*2\*\*28"):
        U.loss_relative_errors(p, never, K, noise="reference")


def test_chunk_rounding():
    assert U.LRE_TILE == 16
    assert U.lre_chunk(1000, None, 1 << 20) == 1008                  # at most K, in whole tiles
    assert U.lre_chunk(1000, 1, 1 << 20) == 16
    assert U.lre_chunk(1000, 16, 1 << 20) == 16
    assert U.lre_chunk(1000, 17, 1 << 20) == 32
    assert U.lre_chunk(1000, 333, 1 << 20) == 336
    assert U.lre_chunk(5 * 10 ** 7, None, 1 << 20) == 1 << 20
    assert U.lre_chunk(5, None, 1 << 16) == 16
    assert U._lre_chunks(1000, 336) == [(0, 336), (336, 336), (672, 328)]
    with pytest.raises(ValueError):
        U.lre_chunk(10, -4, 16)
    out = U.loss_relative_errors(llgc(), dense(), 100, delta_t=0.125, noise="reference", seed=1, chunk=33)
    assert out["chunk"] == 48 and out["K"] == 100


def test_chunking_keeps_each_trajectory_on_its_own_draws():
    """Chunked and unchunked composite runs see the same draws per trajectory.  torch's fp32 matrix products may order their sums
    by batch size, so the samples agree to fp32 rounding, not bit for bit: 8 steps of O(1) values at 6e-8 each -> 2e-6."""
    p, net = llgc(), dense()
    kw = dict(delta_t=0.125, noise="reference", seed=11, return_samples=True)
    one = U.loss_relative_errors(p, net, 100, **kw)
    many = U.loss_relative_errors(p, net, 100, chunk=16, **kw)
    for key in ("Y", "D"):
        assert float((one[key] - many[key]).abs().max()) <= 2e-6 * max(1.0, float(one[key].abs().max()))
    for key in U.LRE_KEYS:
        assert many[key] == pytest.approx(one[key], rel=1e-4)


@pytest.mark.parametrize("control", ["dense_inner", "mlp", "dense_outer", "solver"])
@pytest.mark.parametrize("adaptive", [False, True])
def test_host_statistics_are_the_float64_statistics_of_the_samples(control, adaptive):
    """Every control kind on the composite plan: the returned statistics against numpy float64 on the returned fp32 samples, in
    chunks of 16, under the bound of the kernel tests (1e-10 of the mean absolute centred term)."""
    d, K = 3, 100
    p = llgc(d)
    if control == "dense_inner":
        ctl = dense(d)
    elif control == "mlp":
        ctl = psp.MySequential(d + 1, d, lr=0.05, seed=5)
    elif control == "dense_outer":
        ctl = [psp.DenseNet(d, d, lr=0.05, seed=40 + n) for n in range(8)]
    else:
        ctl = psp.Solver("lre", p, lr=1e-3, L=1, K=16, delta_t=0.125, time_approx="inner", u_l2_error_flag=False, verbose=False,
                         seed=3, device="cpu", backend="torch")
    out = U.loss_relative_errors(p, ctl, K, delta_t=0.125, adaptive_forward_process=adaptive, noise="reference", seed=2, chunk=16,
                                 return_samples=True)
    ref, count, scale = r64.numpy_statistics(out["Y"].numpy(), out["D"].numpy())
    assert out["cross_entropy_detach_selection"][3] == count
    r64.assert_statistics(out, ref, scale, tag=control)


def test_one_sample_has_nan_variances():
    out = U.loss_relative_errors(llgc(), dense(), 1, delta_t=0.125, noise="reference", seed=2)
    for key in U.LRE_KEYS:
        assert np.isnan(out[key][1]) and np.isnan(out[key][2]), key
    assert np.isfinite(out["terminal"][0]) and np.isnan(out["log_variance"][0])


# ---- the C ABI: sizes and argument checks, no launch ---------------------------------------------------------------------------
def test_loss_stats_abi_checks_its_arguments_without_a_launch():
    if not nat.is_built():
        import __graft_entry__
        __graft_entry__.build()
    lib = nat.load()
    nbytes = lib.psp_loss_stats_state_bytes()
    assert nbytes > 0 and nbytes % 8 == 0
    assert nbytes == 8 * (56 + 512 * (7 + 14))                       # header, then the two per-workgroup partial tables
    y, d = (C.c_float * 4)(), (C.c_float * 4)()
    state, out = (C.c_double * (nbytes // 8))(), (C.c_double * 20)()
    assert lib.psp_loss_stats_accumulate(None, d, 4, state, None) == -1 and "null" in nat.last_error()
    assert lib.psp_loss_stats_accumulate(y, None, 4, state, None) == -1
    assert lib.psp_loss_stats_accumulate(y, d, 4, None, None) == -1
    assert lib.psp_loss_stats_accumulate(y, d, -1, state, None) == -1 and "negative" in nat.last_error()
    assert lib.psp_loss_stats_accumulate(y, d, 0, state, None) == 0  # nothing to add: no launch either
    assert lib.psp_loss_stats_finish(None, out, None) == -1 and "null" in nat.last_error()
    assert lib.psp_loss_stats_finish(state, None, None) == -1


def test_the_statistics_unit_is_built_from_its_own_headers():
    """build.py compiles csrc/lstat_instance.hip as its own unit; what it depends on is read from its #include lines."""
    import importlib.util
    import os
    pkg = os.path.dirname(os.path.abspath(psp.utilities.__file__))
    spec = importlib.util.spec_from_file_location("psp_build_for_lstat", os.path.join(pkg, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    deps = {os.path.relpath(p, pkg).replace(os.sep, "/") for p in build.unit_deps(os.path.join(pkg, "csrc", "lstat_instance.hip"))}
    assert deps == {"csrc/lstat_instance.hip", "csrc/lstat_kernels.h", "csrc/launch.h"}     # no MFMA machinery, no C header
    api = {os.path.relpath(p, pkg).replace(os.sep, "/") for p in build.unit_deps(os.path.join(pkg, "csrc", "api_common.hip"))}   # psp_loss_stats_*
    assert "csrc/lstat_kernels.h" in api
    assert "lstat_instance.hip" in open(os.path.join(pkg, "build.py")).read()
