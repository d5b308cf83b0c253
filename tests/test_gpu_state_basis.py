"""The sigma-basis rollout on the GPU (plan_native.py: state_basis; csrc/hjb_kernels.h: hjb_fwd_kernel FAST_ = 3; csrc/
hjb_basis_kernels.h): every case runs with the basis on (state_basis='sigma') and off ('x') against the CPU oracle on the Philox
stream the kernels used, at the bounds tests/test_gpu_parity.py sets for the same quantities.

Shapes: d in {7, 32, 33, 40, 100} x H in {16, 64} x K in {40 (ragged tile), 48}, N = 6; a non-symmetric B = I + off_diag randn with
cond_2(B) between 2 and 4 (off_diag per d below), a non-zero X_0 (so that x~0 = B^-1 x0 is exercised), both matrix modes.

Resident against path_chunks=2 (test d): D is bit-identical; the gradient of a K-chunked run is summed in another order than the
resident run's in either basis, so bit equality cannot hold there and is not claimed: both chunk modes are run and held to the
bound tests/test_gpu_chunked.py sets for each (1e-6 of max |grad| for 'recompute', 5e-6 for 'two_gradient').
"""
import functools
import math

import pytest
import torch

from util_cases import orc, psp

pytestmark = pytest.mark.gpu
nat = psp.native

# ---- the bounds of tests/test_gpu_parity.py (check_first_iteration / check_loss_log), by name ---------------------------------
D_TOL = 2e-5            # per-trajectory D: |diff| <= D_TOL * max(1, max |D|)
GRAD_TOL = 2e-4         # flat gradient: max |diff| <= GRAD_TOL * max |grad|
LOSS_LOG_TOL = 1e-4     # loss per iteration, relative
CHUNK_GRAD_TOL_TWO_GRADIENT, CHUNK_GRAD_TOL_RECOMPUTE, CHUNK_LOSS_TOL = 5e-6, 1e-6, 1e-6   # tests/test_gpu_chunked.py: a K-chunked
#                         run against the resident one, gradient of max |grad| per chunk mode, loss relative
BIG = 7.0e4             # tests/test_gpu_range_guard.py: beyond the largest finite f16


def first_loss_tol(D_ref, loss_ref):
    """test_gpu_parity.check_first_iteration: the reference's own fp32 mean(D^2) - mean(D)^2 error follows the conditioning"""
    cond = float((D_ref.double() ** 2).mean()) / max(abs(loss_ref), 1e-30)
    return min(1e-4, max(2e-5, 4 * 6e-8 * cond))


OFF = {7: 0.2, 32: 0.06, 33: 0.06, 40: 0.05, 100: 0.03, 20: 0.3}       # cond_2(B): 2.63, 2.36, 2.48, 2.34, 2.29 (and 41: the guard)
T_, DT = 0.065, 0.01                                                   # N = 6
SHAPES = [(d, H, K) for d in (7, 32, 33, 40, 100) for H in (16, 64) for K in (40, 48)]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def x0_of(d, big=False):
    x0 = 0.5 * torch.cos(torch.arange(d, dtype=torch.float32))
    if big:
        x0[min(3, d - 1)] = BIG
    return x0


def run(d, H, K, mode, basis, L=1, scale=1.0, big=False, loss="log-variance", **over):
    prob = psp.LLGC(d=d, off_diag=OFF[d], T=T_, seed=42, device=dev())
    kw = dict(lr=1e-3, L=L, K=K, delta_t=DT, loss_method=loss, time_approx="inner", adaptive_forward_process=True, detach_forward=True,
              u_l2_error_flag=False, verbose=False, seed=42, device=dev(), backend="native", noise="philox", widths=(H, H),
              mlp_dtype=mode, state_basis=basis)
    kw.update(over)
    model = psp.Solver("basis", prob, **kw)
    model.X_0 = x0_of(d, big).to(dev())
    with torch.no_grad():
        for p in model.z_n.parameters():
            p.mul_(scale)
    model.train()
    assert model.plan_name == "native" and model.N == 6
    plan = model._native_plan
    if basis != "auto":
        assert plan.state_basis == basis, (plan.state_basis, plan.state_basis_reason)
    assert plan.state_basis in model.plan_reason
    torch.cuda.synchronize()
    return model, plan


@functools.lru_cache(maxsize=None)
def oracle(d, H, K, L=1, scale=1.0, big=False, loss="log-variance"):
    """The CPU oracle on the ORIGINAL problem with the kernels' Philox stream (computed once per case, never modified)."""
    N = 6
    noise = []
    for l in range(L):
        xi = torch.empty(N + 1, K, d, device=dev())
        nat.check(nat.load().psp_philox_normal_fill(nat.ptr(xi), N, K, d, 0, 42, l, None), "fill")
        torch.cuda.synchronize()
        noise.append(xi.cpu().permute(1, 2, 0).contiguous())
    oprob = orc.make_problem("LLGC", d=d, off_diag=OFF[d], T=T_, seed=42)
    oprob.X_0 = x0_of(d, big)
    ocfg = orc.HJBConfig(K=K, delta_t=DT, lr=1e-3, L=L, seed=42, loss_method=loss, adaptive_forward_process=True, detach_forward=True)
    z = orc.TanhMLP(d + 1, d, 1e-3, seed=123, widths=(H, H))
    with torch.no_grad():
        for p in z.parameters():
            p.mul_(scale)
    _, y0, N_ = orc.hjb_build(oprob, ocfg)
    assert N_ == N
    ref = orc.hjb_train(oprob, ocfg, step_models=(z, y0, N), noise=noise, trace=True)
    grads = [torch.cat([g.reshape(-1) for g in tr["grads"]]) for tr in ref["traces"]]
    params = torch.cat([p.detach().reshape(-1) for p in z.parameters()])
    return dict(loss_log=ref["loss_log"], D=[tr["D"] for tr in ref["traces"]], grads=grads, params=params)


def check_iteration0(model, plan, ref, tag):
    D, D_ref = plan.D.cpu(), ref["D"][0]
    g, g_ref = plan.grad.cpu(), ref["grads"][0]
    eD = float((D - D_ref).abs().max()) / max(1.0, float(D_ref.abs().max()))
    eg = float((g - g_ref).abs().max()) / float(g_ref.abs().max())
    tol = first_loss_tol(D_ref, ref["loss_log"][0])
    el = abs(model.loss_log[0] - ref["loss_log"][0]) / abs(ref["loss_log"][0])
    print("%s: D %.3g (<= %.3g)  grad %.3g (<= %.3g)  loss %.3g (<= %.3g)" % (tag, eD, D_TOL, eg, GRAD_TOL, el, tol))
    assert eD <= D_TOL, (tag, eD)
    assert g.shape == g_ref.shape and eg <= GRAD_TOL, (tag, eg)
    assert el <= tol, (tag, model.loss_log[0], ref["loss_log"][0])


@pytest.fixture
def tile_per_wave(monkeypatch):
    """fp32 mode at these K would take the small-K forwards (test g covers them); pin hjb_fwd_kernel, as the range-guard tests do"""
    monkeypatch.setenv("PSP_FWD_VARIANT", "1")
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)


# ---- a. parity with the oracle, basis on and off ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("d,H,K", SHAPES)
def test_iteration0_matches_the_oracle_in_both_bases(d, H, K, mode, tile_per_wave):
    ref = oracle(d, H, K)
    for basis in ("x", "sigma"):
        model, plan = run(d, H, K, mode, basis)
        assert plan.matrix_mode == mode and plan.cfg.sigma_kind == (nat.SIGMA_IDENTITY if basis == "sigma" else nat.SIGMA_DENSE)
        check_iteration0(model, plan, ref, "d=%d H=%d K=%d %s %s" % (d, H, K, mode, basis))


# ---- b. the W1x block of the gradient -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("d,H,K", [(33, 16, 40), (100, 64, 48)])
def test_w1x_gradient_block_is_back_in_the_x_basis(d, H, K, mode, tile_per_wave):
    """dW1x = dW~1x B^T (psp_hjb_basis_grad): the x columns of W1's gradient against the oracle's, relative to THAT block's largest
    entry (the whole-gradient bound of test a is dominated by the output layer).  Weights x 30 so that the control is O(1) and every
    block carries signal.  With cond_2(B) > 2 a missing transform is an O(1) relative error of the block."""
    ref = oracle(d, H, K, 1, 30.0)
    blk_ref = ref["grads"][0][:H * (d + 1)].view(H, d + 1)
    for basis in ("x", "sigma"):
        model, plan = run(d, H, K, mode, basis, scale=30.0)
        blk = plan.grad.cpu()[:H * (d + 1)].view(H, d + 1)
        ex = float((blk[:, 1:] - blk_ref[:, 1:]).abs().max()) / float(blk_ref[:, 1:].abs().max())
        et = float((blk[:, 0] - blk_ref[:, 0]).abs().max()) / float(blk_ref[:, 0].abs().max())
        print("d=%d H=%d %s %s: W1x block %.3g, time column %.3g (<= %.3g)" % (d, H, mode, basis, ex, et, GRAD_TOL))
        assert float(blk_ref[:, 1:].abs().max()) > 0
        assert ex <= GRAD_TOL and et <= GRAD_TOL, (basis, ex, et)
        check_iteration0(model, plan, ref, "weights x 30 d=%d %s %s" % (d, mode, basis))


# ---- c. three training iterations with Adam -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
@pytest.mark.parametrize("d,H,K", [(33, 16, 40), (100, 64, 48)])
def test_three_adam_iterations(d, H, K, mode, tile_per_wave):
    ref = oracle(d, H, K, 3, 30.0)
    res = {}
    for basis in ("x", "sigma"):
        model, plan = run(d, H, K, mode, basis, L=3, scale=30.0, use_graph=False)
        for l, (got, want) in enumerate(zip(model.loss_log, ref["loss_log"])):
            assert math.isclose(got, want, rel_tol=LOSS_LOG_TOL), (basis, l, model.loss_log, ref["loss_log"])
        res[basis] = plan.flat.cpu().clone()
    ep = float((res["sigma"] - res["x"]).abs().max()) / float(res["x"].abs().max())
    eo = float((res["sigma"] - ref["params"]).abs().max()) / float(ref["params"].abs().max())
    print("d=%d %s: parameters after three steps, sigma vs x %.3g, sigma vs oracle %.3g (<= %.3g)" % (d, mode, ep, eo, GRAD_TOL))
    assert ep <= GRAD_TOL, ep


# ---- d. bit equality with the basis on ----------------------------------------------------------------------------------------
def big_K():
    """just past the 'more than two tiles per CU' rule, ragged: store_path 4 and the K-chunked passes exist from here on"""
    return 16 * (2 * torch.cuda.get_device_properties(dev()).multi_processor_count + 3) + 8


def test_bit_equality_store_path_chunks_and_repeats(monkeypatch):
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    d, H, K = 33, 16, big_K()
    a, pa = run(d, H, K, "f16x3", "sigma", L=2, path_noise="store")
    b, pb = run(d, H, K, "f16x3", "sigma", L=2)
    assert pa.cfg.store_path == 1 and pb.cfg.store_path == 4 and pb.regen_xi
    assert a.loss_log == b.loss_log and torch.equal(pa.D, pb.D) and torch.equal(pa.grad, pb.grad) and torch.equal(pa.flat, pb.flat)
    # 'auto' picks the same basis at this size
    c, pc = run(d, H, K, "auto", "auto", L=2)
    assert pc.state_basis == "sigma" and pc.matrix_mode == "f16x3"
    assert c.loss_log == b.loss_log and torch.equal(pc.grad, pb.grad)
    # three repeated launches of the same iteration: every segment of the gradient
    Hd = H * (d + 1)
    segs = [0, Hd, Hd + H, Hd + H + H * H, Hd + 2 * H + H * H, Hd + 2 * H + H * H + d * H, pb.P]
    runs = [run(d, H, K, "f16x3", "sigma", L=1)[1] for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r.D, runs[0].D)
        for lo, hi in zip(segs[:-1], segs[1:]):
            assert torch.equal(r.grad[lo:hi], runs[0].grad[lo:hi]), (lo, hi)
    assert float(runs[0].grad[:Hd].abs().max()) > 0
    # resident against two chunks, both chunk modes: D bit for bit; the gradient at the bound tests/test_gpu_chunked.py sets for
    # the mode (the chunks' partial gradients are summed in another order than the resident run's, in either basis)
    for mode, tol in (("two_gradient", CHUNK_GRAD_TOL_TWO_GRADIENT), ("recompute", CHUNK_GRAD_TOL_RECOMPUTE)):
        e, pe = run(d, H, K, "f16x3", "sigma", L=1, path_chunks=2, chunk_mode=mode)
        assert pe.n_chunks == 2 and pe.chunk_mode == mode and pe.state_basis == "sigma"
        assert torch.equal(pe.D, runs[0].D)
        assert math.isclose(e.loss_log[0], b.loss_log[0], rel_tol=CHUNK_LOSS_TOL)
        err = float((pe.grad - runs[0].grad).abs().max()) / float(runs[0].grad.abs().max())
        print("chunked (%s) vs resident gradient: %.3g (<= %.3g)" % (mode, err, tol))
        assert err <= tol, (mode, err)
    e, pe = run(d, H, K, "f16x3", "sigma", L=1, path_chunks=2)
    assert pe.chunk_mode == "two_gradient"                # what 'auto' picks for a detached log-variance run


# ---- e. range guard -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,K", [(100, 64, 48), (33, 16, 40)])
def test_range_fallback_runs_in_the_same_basis(d, H, K, tile_per_wave):
    """One state component at 7e4 (tests/test_gpu_range_guard.py): x~0 = B^-1 x0 leaves the f16 range too, the guarded split kernels
    hand the iteration to the fp32-MFMA twins -- which take the SAME transformed problem from the plan's config -- and the result
    is the fp32 plan's bit for bit and the oracle's at the usual bounds (moment loss, as there).  Measured: d = 100 gradient error
    1.8e-4 of max |grad| in the sigma basis against 9e-8 in the x basis (bound 2e-4) -- an fp32 X~ resolves X = B X~ to
    eps ||B|| max |X~| in every component, and here one component is 7e4 next to O(1) ones; d = 33: 2e-7 against 8e-7."""
    ref = oracle(d, H, K, 1, 1.0, True, "moment")
    for basis in ("x", "sigma"):
        got, pg = run(d, H, K, "f16x3", basis, big=True, loss="moment")
        f32, pf = run(d, H, K, "fp32", basis, big=True, loss="moment")
        assert pg.range_flag is not None and pg.range_fallbacks() == 1 and got.range_fallback_iterations == 1
        assert got.loss_log == f32.loss_log and torch.equal(pg.grad, pf.grad) and torch.equal(pg.D, pf.D)
        assert float(pg.x0_vec.abs().max()) > 65504.0
        el = abs(got.loss_log[0] - ref["loss_log"][0]) / abs(ref["loss_log"][0])
        eg = float((pg.grad.cpu() - ref["grads"][0]).abs().max()) / float(ref["grads"][0].abs().max())
        print("range fallback d=%d %s: loss %.3g (<= %.3g)  grad %.3g (<= %.3g)" % (d, basis, el, LOSS_LOG_TOL, eg, GRAD_TOL))
        assert el <= LOSS_LOG_TOL and eg <= GRAD_TOL, (basis, el, eg)
        raw, pr = run(d, H, K, "f16x3", basis, big=True, loss="moment", range_guard=False)
        assert not math.isfinite(raw.loss_log[0])            # the test means something: the split kernels cannot hold this state


# ---- f. the conditioning guard ------------------------------------------------------------------------------------------------
def test_ill_conditioned_sigma_runs_exactly_as_with_the_basis_forced_off(monkeypatch):
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    d, H, K = 20, 16, big_K()
    a, pa = run(d, H, K, "auto", "auto", L=2)
    assert pa.state_basis == "x" and "cond_2" in pa.state_basis_reason, pa.state_basis_reason
    monkeypatch.setenv("PSP_STATE_BASIS", "0")
    prob = psp.LLGC(d=d, off_diag=OFF[d], T=T_, seed=42, device=dev())
    b = psp.Solver("basis", prob, lr=1e-3, L=2, K=K, delta_t=DT, loss_method="log-variance", time_approx="inner",
                   adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42, device=dev(),
                   backend="native", noise="philox", widths=(H, H))
    b.X_0 = x0_of(d).to(dev())
    b.train()
    pb = b._native_plan
    assert pb.state_basis == "x" and pb.state_basis_reason == "PSP_STATE_BASIS=0"
    assert a.loss_log == b.loss_log and torch.equal(pa.D, pb.D) and torch.equal(pa.grad, pb.grad) and torch.equal(pa.flat, pb.flat)
    # ... and the environment switch wins over an eligible problem too
    c = psp.Solver("basis", psp.LLGC(d=33, off_diag=OFF[33], T=T_, seed=42, device=dev()), lr=1e-3, L=1, K=K, delta_t=DT,
                   loss_method="log-variance", time_approx="inner", adaptive_forward_process=True, detach_forward=True,
                   u_l2_error_flag=False, verbose=False, seed=42, device=dev(), backend="native", noise="philox", widths=(H, H))
    c.train()
    assert c._native_plan.state_basis == "x" and c._native_plan.cfg.sigma_kind == nat.SIGMA_DENSE


def test_sigma_on_an_ineligible_plan_raises(monkeypatch):
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    prob = psp.LLGC(d=20, off_diag=OFF[20], T=T_, seed=42, device=dev())
    model = psp.Solver("basis", prob, lr=1e-3, L=1, K=48, delta_t=DT, loss_method="log-variance", time_approx="inner",
                       adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42, device=dev(),
                       backend="native", noise="philox", widths=(16, 16), state_basis="sigma")
    with pytest.raises(ValueError):
        model.train()
    model.backend = "auto"                                # ... and no quiet composite plan under backend='auto' either
    with pytest.raises(ValueError):
        model.train()


# ---- consumers the basis leaves alone ---------------------------------------------------------------------------------------
def test_u_l2_log_and_final_state_come_out_in_the_x_basis(tile_per_wave):
    """u_L2 against an x-independent reference control is accumulated from Z inside the forward (the general instance with identity
    sigma at run time); forward_only(want_XN) maps X~_N back with B.  Bounds: the u_L2 log's 1e-4 relative of
    tests/test_gpu_parity.check_loss_log; X_N at the D bound (D = Y - alpha . X_N is that bound's own quantity)."""
    d, H, K = 33, 16, 40
    res = {}
    for basis in ("x", "sigma"):
        model, plan = run(d, H, K, "f16x3", basis, L=2, use_graph=False, u_l2_error_flag=True)
        D, XN = plan.forward_only(0, want_XN=True)
        torch.cuda.synchronize()
        res[basis] = (list(model.u_L2_loss), XN.cpu().clone(), D.cpu().clone())
    assert len(res["x"][0]) == 2 and all(v > 0 for v in res["x"][0])
    for a, b in zip(res["sigma"][0], res["x"][0]):
        assert math.isclose(a, b, rel_tol=LOSS_LOG_TOL), (res["sigma"][0], res["x"][0])
    eX = float((res["sigma"][1] - res["x"][1]).abs().max()) / max(1.0, float(res["x"][1].abs().max()))
    eD = float((res["sigma"][2] - res["x"][2]).abs().max()) / max(1.0, float(res["x"][2].abs().max()))
    print("X_N sigma vs x %.3g, D %.3g (<= %.3g)" % (eX, eD, D_TOL))
    assert eX <= D_TOL and eD <= D_TOL


# ---- g. the small-K forwards and the hipGraph body ----------------------------------------------------------------------------
@pytest.mark.parametrize("K,variant", [(16, "2"), (4, None)])
def test_small_K_routes_with_the_basis_on(K, variant, monkeypatch):
    """K = 16 on the feature-split forward (hjbs_fwd_kernel, forced), K = 4 on the quad forward (hjbq_fwd_kernel, the default at this
    size): both branch on sigma_kind at run time; three iterations, the second and third replayed from the captured hipGraph,
    whose body carries the two transform launches."""
    monkeypatch.delenv("PSP_STATE_BASIS", raising=False)
    if variant is None:
        monkeypatch.delenv("PSP_FWD_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PSP_FWD_VARIANT", variant)
    d, H = 33, 16
    ref1 = oracle(d, H, K, 1, 30.0)
    model, plan = run(d, H, K, "fp32", "sigma", L=1, scale=30.0)
    check_iteration0(model, plan, ref1, "small K=%d" % K)
    ref = oracle(d, H, K, 3, 30.0)
    model, plan = run(d, H, K, "fp32", "sigma", L=3, scale=30.0)
    assert plan.graph_active
    for l, (got, want) in enumerate(zip(model.loss_log, ref["loss_log"])):
        assert math.isclose(got, want, rel_tol=LOSS_LOG_TOL), (l, model.loss_log, ref["loss_log"])
    x, px = run(d, H, K, "fp32", "x", L=3, scale=30.0)
    ep = float((plan.flat - px.flat).abs().max()) / float(px.flat.abs().max())
    print("small K=%d: parameters after three steps (graph), sigma vs x %.3g (<= %.3g)" % (K, ep, GRAD_TOL))
    assert ep <= GRAD_TOL, ep
