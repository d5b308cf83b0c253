"""The per-coordinate and radial coefficient kinds of the DenseNet-control kernels (csrc/hjbd_kernels.h: PSP_DRIFT_WELL_DIAG,
PSP_DRIFT_RADIAL_WELL, PSP_TERM_QUAD_LINEAR, PSP_TERM_RADIAL_QUAD) on the GPU, through the plan and the C ABI, against the float64
statement of tests/ref64_wells.py on the noise the kernels used.

Per case of tests/wells_cases.py (first iteration, both matrix modes): per-trajectory D, X_N and Y_N, the loss, and EACH of the nine
gradient blocks of EACH per-step net; the padded coordinates of X_N are exactly zero (they must stay out of r^2).  Bounds: those of
tests/test_gpu_dense_block_gradients.py, imported from there.  Then: the three wells on Solver(name, problem) with nothing else set
are native and follow the reference's fixed-seed runs (tests/golden/wells_*.json) to 1e-4; the u_L2 log of DoubleWell_OU and
DoubleWell_multidim_3 per trajectory; do_importance_sampling_me on a trained OU model; what the C ABI answers to the kinds.

Measured on an MI355X (the test prints every figure): D <= 3.9e-7, X_N <= 1.5e-7, Y <= 2.9e-7 of max(1, max |.|) (bound 2e-5); every
gradient block <= 2.3e-6 of its own maximum (bound 2e-4); u_L2 per trajectory <= 1.2e-7 with no trajectory near a cell edge; r in
[1.00, 4.59] over the radial cases.  No radial case came near a bound, so none was widened.  The whole file runs in about 6 s.
"""
import ctypes as C
import glob
import math
import os

import pytest
import torch

import block_cases as bc
import dense_block_cases as dc
import ref64_wells as rw
import wells_cases as wc
from conftest import load_golden
from test_gpu_dense_block_gradients import BLOCK_TOL, D_TOL, dev, philox_noise
from util_cases import assert_dense_blocks, make_pkg_solver, psp

pytestmark = pytest.mark.gpu
nat = psp.native
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NATIVE_GOLDENS = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLDEN, "wells_*.json"))
                        if "llgc_general_f" not in p)


def run_case(c, mode=None):
    prob = wc.problem(c, dev())
    model = psp.Solver(name="wells", problem=prob, verbose=False, device=dev(), backend="native", noise=c["noise"],
                       mlp_dtype=mode or c["mode"], loss_method=c["loss"], adaptive_forward_process=c["adaptive"],
                       detach_forward=c["detach"], L=1, lr=0.0, seed=42, delta_t=wc.DT, K=c["K"], u_l2_error_flag=False)
    model.z_n = wc.nets(c, dev())                       # lr = 0: the Adam step leaves the parameters where the forward found them
    model.update_Phis()
    model.train()
    assert model.plan_name == "native" and model.N == c["N"], (model.plan_name, model.plan_reason)
    torch.cuda.synchronize()
    return model, model._native_plan


def forward_again(c, model, plan, noise):
    """psp_dnet_rollout_fwd once more on the plan's own config and (unchanged) parameters, with X_N and Y_N written out."""
    K, Dp, N = c["K"], plan.d_pad, c["N"]
    xi = None
    if c["noise"] == "reference":
        xi = torch.nn.functional.pad(noise.permute(2, 0, 1), (0, Dp - c["d"])).contiguous().to(dev())
    D = torch.empty(K, device=dev())
    XN = torch.full((K, Dp), float("nan"), device=dev())
    Y = torch.empty(K, device=dev())
    nat.check(plan.lib.psp_dnet_rollout_fwd(C.byref(plan.cfg), nat.ptr(plan.flat), nat.ptr(plan.x0_vec), 0, None, nat.ptr(xi),
                                            int(model.seed), 0, None, nat.ptr(plan.PX), nat.ptr(plan.PXI), nat.ptr(D), None,
                                            nat.ptr(XN), nat.ptr(Y), nat.ptr(plan.fwd_partial), nat.ptr(plan.tables),
                                            nat.stream_ptr(dev())), "psp_dnet_rollout_fwd")
    torch.cuda.synchronize()
    return D.cpu(), XN.cpu(), Y.cpu()


@pytest.mark.parametrize("c", wc.CASES, ids=wc.IDS)
def test_first_iteration_matches_the_float64_reference(c):
    if c["refused"]:
        # the C ABI answers -3 to this combination (csrc/hjbd_kernels.h dnet_adj_x3_has_radial): asserted in place of the run; the
        # plan's default matrix mode then runs the same case on the fp32 kernels, which is what is compared below
        with pytest.raises(nat.NativeCallError, match=r"\(-3\).*radial drift"):
            run_case(c)
        model, plan = run_case(c, mode="auto")
        assert plan.matrix_mode == "fp32"
    else:
        model, plan = run_case(c)
        assert plan.matrix_mode == c["mode"]
    assert (plan.d_pad, plan.H_pad) == c["expect"] and plan.kernel_bwd
    assert plan.attached == (c["adaptive"] and not c["detach"]) and plan.relent == (c["loss"] == "relative_entropy")
    assert plan.cfg.base.drift_kind in (nat.DRIFT_WELL_DIAG, nat.DRIFT_RADIAL_WELL)
    if plan.matrix_mode == "f16x3":
        assert plan.range_fallbacks() == 0
    draw = philox_noise if c["noise"] == "philox" else dc.host_noise
    noise = draw(int(model.seed), c["K"], c["d"], c["N"])
    ref = wc.reference(c, lambda: noise, stream="device")
    D, D_ref = plan.D.double().cpu(), ref["D"]
    assert bool(torch.isfinite(D).all())
    eD = float((D - D_ref).abs().max()) / max(1.0, float(D_ref.abs().max()))
    tol_l = bc.first_loss_tol(bc.loss_values(c["loss"], D_ref), ref["loss"])
    el = abs(model.loss_log[0] - ref["loss"]) / abs(ref["loss"])
    D2, XN, Y = forward_again(c, model, plan, noise)
    assert torch.equal(D2, plan.D.cpu())                                  # the same launch on the same numbers
    assert torch.equal(XN[:, c["d"]:], torch.zeros(c["K"], plan.d_pad - c["d"]))      # padding stays zero (and out of r^2)
    eX = float((XN[:, :c["d"]].double() - ref["XN"]).abs().max()) / max(1.0, float(ref["XN"].abs().max()))
    eY = float((Y.double() - ref["Y"]).abs().max()) / max(1.0, float(ref["Y"].abs().max()))
    print("%s: D %.2e  X_N %.2e  Y %.2e (<= %.1e)  loss %.2e (<= %.1e)  r in [%.2f, %.2f]"
          % (c["id"], eD, eX, eY, D_TOL, el, tol_l, float(ref["r"].min()), float(ref["r"].max())))
    g = plan.grad.cpu()
    assert g.shape == ref["grad"].shape and bool(torch.isfinite(g).all())
    assert_dense_blocks(g, ref["grad"], c["d"], c["H"], c["N"], False, BLOCK_TOL, tag=c["id"])
    assert eD <= D_TOL and eX <= D_TOL and eY <= D_TOL, (eD, eX, eY)
    assert el <= tol_l, (model.loss_log[0], ref["loss"])


@pytest.mark.parametrize("name", NATIVE_GOLDENS)
def test_default_solver_is_native_and_follows_the_reference(name):
    rec = load_golden(name)
    model = make_pkg_solver(rec["case"], dev())                           # Solver(name, problem) and the case's flags, nothing else
    model.train()
    assert model.plan_name == "native", model.plan_reason
    exp = rec["expected"]
    assert len(model.loss_log) == len(exp["loss_log"])
    for got, want in zip(model.loss_log, exp["loss_log"]):
        assert math.isclose(got, want, rel_tol=1e-4), (model.loss_log, exp["loss_log"])
    if any(v != 0 for v in exp["u_L2_loss"]):
        assert len(model.u_L2_loss) == len(exp["u_L2_loss"])
        for got, want in zip(model.u_L2_loss, exp["u_L2_loss"]):
            assert math.isclose(got, want, rel_tol=1e-4), (model.u_L2_loss, exp["u_L2_loss"])


@pytest.mark.parametrize("cls,d,kw,call", [("DoubleWell_OU", 3, dict(alpha=0.5, kappa=1.0), "compute_reference_solution_x_1"),
                                           ("DoubleWell_OU", 20, dict(alpha=0.5, kappa=1.0), "compute_reference_solution_x_1"),
                                           ("DoubleWell_multidim_3", 5, dict(eta=0.5, kappa=1.0), "compute_reference_solution")])
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_u_l2_per_trajectory(cls, d, kw, call, mode):
    """plan.ul2 against sum_n |-Z_n - u*(X_{n+1}, t_n)|^2 dt in float64, u* read from the same tables with the kernel's cell
    arithmetic (tests/test_double_wells_host.py holds those tables to problem.u_true).  A trajectory whose table coordinate lies within
    1e-4 dx of a cell edge at some step may read the neighbouring cell in fp32 and is exempt -- at most K // 8 of them, as in
    tests/test_gpu_solver_ul2.py; the others are held to D_TOL max(1, max ul2)."""
    c = wc._c("u", cls, d, 30, 37, 4, None, "att", mode, **kw)
    c["scale"] = 0.8
    T = (c["N"] + 0.5) * wc.DT
    prob = getattr(psp, cls)(d=d, T=T, device=dev(), **kw)
    getattr(prob, call)(nx=300)
    model = psp.Solver(name="wells-ul2", problem=prob, verbose=False, device=dev(), backend="native", mlp_dtype=mode, L=1, lr=0.0,
                       seed=42, delta_t=wc.DT, K=c["K"])
    model.z_n = wc.nets(c, dev())
    model.update_Phis()
    model.train()
    assert model.plan_name == "native" and model._native_plan.ul2 is not None
    torch.cuda.synchronize()
    plan = model._native_plan
    cpu = getattr(psp, cls)(d=d, T=T, device="cpu", **kw)
    getattr(cpu, call)(nx=300)
    out = rw.iteration(cpu.native_spec(), cpu.X_0, c["N"], wc.DT, wc.nets(c, "cpu"), dc.host_noise(42, c["K"], d, c["N"]))
    table = psp.plan_common.ul2_reference(cpu, c["N"], model.delta_t_np, plan.d_pad, c["K"], 0)
    want = rw.ul2_per_trajectory(table, out, wc.DT)
    got = plan.ul2.double().cpu()
    ncoord = 1 if cls == "DoubleWell_OU" else d
    pos = (torch.clamp(out["X"][1:, :, :ncoord], -table["xb"], table["xhi"]) + table["xb"]) / table["dx"]
    near = ((pos - torch.round(pos)).abs() < 1e-4).any(2).any(0)
    err = (got - want).abs() / max(1.0, float(want.abs().max()))
    print("%s d=%d %s: ul2 %.2e (<= %.1e), %d of %d trajectories near a cell edge" % (cls, d, mode, float(err[~near].max()), D_TOL,
                                                                                     int(near.sum()), c["K"]))
    assert int(near.sum()) <= c["K"] // 8                                 # (as tests/test_gpu_solver_ul2.py; measured: none)
    assert float(err[~near].max()) <= D_TOL
    assert math.isclose(model.u_L2_loss[0], float(got.sum()) / c["K"], rel_tol=1e-6)


def test_importance_sampling_on_a_trained_ou_model_is_native():
    """do_importance_sampling_me on DenseNet controls trained on DoubleWell_OU runs psp_dnet_rollout_fwd (utilities._is_dense_native)
    and agrees with the composite evaluation on the same draws within the existing IS test's bounds (tests/test_composite_golden.py:
    mean 1e-5, variance and relative error 1e-4)."""
    rec = load_golden("wells_ou_d3_detached")
    model = make_pkg_solver(rec["case"], dev(), u_l2_error_flag=False)
    model.train()
    assert model.plan_name == "native"
    ut = psp.utilities
    assert ut._native_reason(model.problem, model, "approx", False) is not None and ut._dense_reason(model.problem, model) is None
    torch.manual_seed(7)
    m, v, r = psp.do_importance_sampling_me(model.problem, model, 300, delta_t=0.05)
    torch.manual_seed(7)
    mc, vc, rc = ut._is_composite(model.problem, model, 300, 0.05)
    assert math.isclose(m, mc, rel_tol=1e-5) and math.isclose(v, vc, rel_tol=1e-4) and math.isclose(r, rc, rel_tol=1e-4), (m, mc, v, vc)


def test_c_abi_answers():
    """psp_dnet_query takes the four kinds (and checks coord_split); the other families keep answering -1 to them."""
    lib = nat.load()
    cfg, sizes = nat.DnetConfig(), nat.DnetSizes()
    b = cfg.base
    b.d, b.H, b.K_local, b.N, b.K_global = 32, 32, 37, 4, 37
    b.dt, b.sqrt_dt = 0.05, 0.05 ** 0.5
    cfg.d_real, cfg.H_real, cfg.per_step = 20, 30, 1
    for dk, tk in ((nat.DRIFT_WELL_DIAG, nat.TERM_QUAD_LINEAR), (nat.DRIFT_RADIAL_WELL, nat.TERM_RADIAL_QUAD),
                   (nat.DRIFT_WELL_DIAG, nat.TERM_SHIFTED_QUAD), (nat.DRIFT_DOUBLE_WELL, nat.TERM_RADIAL_QUAD)):
        b.drift_kind, b.term_kind, b.coord_split = dk, tk, 5
        for mode in (nat.MLP_FP32, nat.MLP_F16X3):
            b.mlp_dtype = mode
            assert lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)) == 0, nat.last_error()
    b.drift_kind, b.term_kind = nat.DRIFT_WELL_DIAG, nat.TERM_QUAD_LINEAR
    for bad in (-1, 21):
        b.coord_split = bad
        assert lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)) == -1
    b.coord_split = 20
    assert lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)) == 0
    # the two kernels that do not carry the kinds (they would gain scratch: csrc/hjbd_kernels.h dnet_adj_x3_has_kinds) answer -3
    b.d, b.H, cfg.d_real, cfg.H_real, b.drift_kind, b.term_kind = 128, 64, 120, 60, nat.DRIFT_RADIAL_WELL, nat.TERM_RADIAL_QUAD
    for mode, store, want in ((nat.MLP_F16X3, 2, -3), (nat.MLP_F16X3, 3, -3), (nat.MLP_F16X3, 1, 0), (nat.MLP_FP32, 2, 0)):
        b.mlp_dtype, b.store_path = mode, store
        assert lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)) == want, (mode, store, nat.last_error())
    # ... and the split-product sweep of (16, 32) does not carry the radial drift (occupancy); the per-coordinate kind stays
    b.d, b.H, cfg.d_real, cfg.H_real = 16, 32, 4, 30
    for dk, tk, mode, store, want in ((nat.DRIFT_RADIAL_WELL, nat.TERM_RADIAL_QUAD, nat.MLP_F16X3, 2, -3),
                                      (nat.DRIFT_RADIAL_WELL, nat.TERM_RADIAL_QUAD, nat.MLP_F16X3, 1, 0),
                                      (nat.DRIFT_RADIAL_WELL, nat.TERM_RADIAL_QUAD, nat.MLP_FP32, 2, 0),
                                      (nat.DRIFT_WELL_DIAG, nat.TERM_QUAD_LINEAR, nat.MLP_F16X3, 2, 0),
                                      (nat.DRIFT_DOUBLE_WELL, nat.TERM_RADIAL_QUAD, nat.MLP_F16X3, 2, 0)):
        b.drift_kind, b.term_kind, b.mlp_dtype, b.store_path, b.coord_split = dk, tk, mode, store, 1
        assert lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)) == want, (dk, tk, mode, store, nat.last_error())
    b.d, b.H, cfg.d_real, cfg.H_real, b.mlp_dtype, b.store_path = 32, 32, 20, 30, nat.MLP_FP32, 0
    for dk, tk in ((4, 0), (7, 0), (10, 0), (0, 3), (0, 10)):               # unknown kinds stay unknown
        b.drift_kind, b.term_kind = dk, tk
        assert lib.psp_dnet_query(C.byref(cfg), C.byref(sizes)) == -1
    h, hs = nat.HjbConfig(), nat.HjbSizes()
    h.d, h.H, h.K_local, h.N, h.K_global = 32, 32, 37, 4, 37
    for dk, tk in ((nat.DRIFT_WELL_DIAG, 0), (nat.DRIFT_RADIAL_WELL, 0), (0, nat.TERM_QUAD_LINEAR), (0, nat.TERM_RADIAL_QUAD)):
        h.drift_kind, h.term_kind = dk, tk
        assert lib.psp_hjb_query(C.byref(h), C.byref(hs)) == -1
