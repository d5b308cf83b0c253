"""Per-block gradient tests of the DenseNet-control kernels (csrc/hjbd_kernels.h, plan_dense_native.py) against the float64 reference,
in a regime where every block of every parameter set carries signal.

The whole-gradient criterion of tests/test_gpu_dense_control.py (max |g - g_ref| <= 2e-4 max |g_ref|) is set by b3 alone at the
DenseNets' initial state: zero biases and X_0 = 0 make every block of the step-0 set but b3 exactly zero, and the W2[h1] rows of the
later sets are 3e-5 .. 5e-4 of the maximum (tests/test_ref64_dense.py plants five errors that criterion accepts).  Here the weight
matrices are scaled, the biases drawn N(0, 0.1) and X_0 moved off zero (tests/dense_block_cases.py; the regime is asserted on the CPU),
the first iteration is compared with tests/ref64.py::iteration_dense on the noise the kernels used -- the host stream, or the Philox
stream materialised by psp_philox_normal_fill with the real d (the counters do not see d: tests/test_ref64_dense.py) -- and EACH of
the 9 ('outer') or 12 ('inner') blocks of EACH parameter set is held to 2e-4 of its own maximum, in both matrix modes.
D: 2e-5 max(1, max |D|); loss: the conditioning rule of tests/test_gpu_parity.py.

Routes (asserted on the plan: instance, matrix mode, kernel / GEMM backward, attached, relent, store_path, generic weights, slices):
one-launch backward on (16, 32), (32, 32), (32, 64), (64, 64), (112, 32), (128, 32), two column passes on (112, 64) and (128, 64),
the GEMM formulation on (256, 32), (256, 64) and under PSP_DENSE_BWD=gemm; the fp32 and the split-product forward, the SPEC forward
(Philox, LLGC, 'outer') detached and attached, Philox off SPEC; split-product and fp32 outer products; hjbd_adj_kernel in both
modes with dense and element-wise drift Jacobians, running cost, relative entropy, cross entropy (explicit wT); variance (generic
weights); the non-adaptive image; K = 9001 over several slices and rounds; N = 1.

Measured on an MI355X: D within 7.2e-7, loss within 1.4e-6, and the worst block error per route (bound 2e-4; the test prints them;
route = instance / forward / backward, "adj" = hjbd_adj_kernel + the fp32 outer products, "-2pass" = two column passes):
  16x32/fp32/bwd-fp32 5.4e-7 (b1)      16x32/f16x3/bwd-x3 5.2e-7 (W3x)      16x32/fp32/adj-fp32 5.5e-7 (W2h1)    16x32/f16x3/adj-x3 4.8e-7 (W3x)
  16x32/fp32/gemm 5.4e-7 (b1)          32x32/fp32/bwd-fp32 2.1e-6 (b1)      32x32/f16x3/bwd-x3 1.3e-6 (W2h1)     32x32/f16x3/adj-x3 6.0e-7 (W2h1)
  32x32/spec/bwd-x3 4.7e-7 (W2x)       32x64/fp32/bwd-fp32 4.2e-7 (W3h2)    32x64/f16x3/bwd-x3 4.0e-7 (W3t)      32x64/fp32/adj-fp32 4.0e-7 (W3h2)
  32x64/f16x3/adj-x3 2.1e-7 (W3h1)     32x64/fp32/gemm 5.3e-7 (W1t)         64x64/fp32/bwd-fp32 1.2e-6 (W2h1)    64x64/f16x3/bwd-x3 5.6e-7 (W2x)
  64x64/fp32/adj-fp32 1.3e-6 (W2h1)    64x64/f16x3/adj-x3 7.0e-7 (b2)       112x32/fp32/bwd-fp32 1.3e-6 (W2h1)   112x32/f16x3/bwd-x3 8.4e-7 (W2x)
  112x32/f16x3/bwd-fp32 2.0e-6 (b2)    112x32/fp32/adj-fp32 2.3e-6 (b1)     112x32/f16x3/adj-x3 1.2e-6 (b1)      112x32/spec/bwd-x3 6.1e-7 (W2x)
  112x32/spec/adj-x3 5.9e-7 (W2h1)     112x32/fp32/adj-fp32-relent 9.1e-7 (W3x)                                  112x32/f16x3/adj-x3-relent 1.1e-6 (W3x)
  112x64/fp32/bwd-fp32-2pass 1.1e-6 (W2x)   112x64/f16x3/bwd-x3-2pass 7.4e-7 (W2h1)   112x64/fp32/adj-fp32-2pass 1.3e-6 (W2h1)   112x64/f16x3/adj-x3-2pass 9.6e-7 (b1)
  128x64/f16x3/bwd-x3-2pass 7.9e-7 (W1x)    128x64/fp32/adj-fp32-2pass 1.8e-6 (b1)    128x32/fp32/adj-fp32 1.8e-6 (W2t)     128x32/f16x3/adj-x3 1.9e-6 (W2t)
  128x32/f16x3/bwd-fp32 7.8e-7 (W2h1)  256x32/fp32/gemm 1.4e-6 (W1x)        256x32/f16x3/gemm 7.5e-7 (W1t)       256x64/fp32/gemm 1.7e-6 (W2x)
  256x64/f16x3/gemm 7.5e-7 (W3x)
i.e. every route is at the fp32-against-float64 floor (the fp32 oracle itself: up to 3.8e-6, tests/test_ref64_dense.py); no block of
any route comes within a factor 80 of the bound, and the whole file runs in 6 s.
"""
import ctypes as C

import pytest
import torch

import block_cases as bc
import dense_block_cases as dc
from util_cases import assert_dense_blocks, dense_block_names, flat_params, make_pkg_problem, psp

pytestmark = pytest.mark.gpu
nat = psp.native

D_TOL = 2e-5                # per-trajectory D: |diff| <= D_TOL * max(1, max |D|)
BLOCK_TOL = 2e-4            # each gradient block of each set, of that block's own maximum
SWITCHES = ("PSP_DENSE_BWD",)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def philox_noise(seed, K, d, N):
    """The stream the Philox routes draw from, materialised by the library with the real d (tests/test_ref64_dense.py)."""
    xi = torch.empty(N + 1, K, d, device=dev())
    nat.check(nat.load().psp_philox_normal_fill(nat.ptr(xi), N, K, d, 0, seed, 0, None), "fill")
    torch.cuda.synchronize()
    return xi.cpu().permute(1, 2, 0).contiguous()


def run_case(c, monkeypatch):
    """The first iteration of the case on the GPU: (model, plan)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)                                          # read by the plan at construction
    case = dc.golden_style(c)
    oprob, _, onets = dc.scaled_oracle(c)
    prob = make_pkg_problem(case["problem"], dev())
    prob.X_0 = dc.x0_of(c, prob.X_0).to(dev())                            # before the solver is built: it copies X_0
    model = psp.Solver(name=case["name"], problem=prob, verbose=False, device=dev(), backend="native", noise=c["noise"],
                       mlp_dtype=c["mode"], **case["solver"])
    nets = [psp.DenseNet(d_in=d_in, d_out=c["d"], lr=case["solver"]["lr"], arch=[c["H"], c["H"]], seed=seed).to(dev())
            for d_in, seed in dc.net_specs(c)]
    dc.prepare_nets(c, nets)
    model.z_n = nets if c["tmode"] == "outer" else nets[0]
    model.update_Phis()
    assert torch.equal(model.X_0.cpu(), oprob.X_0)
    assert torch.equal(torch.cat([flat_params(n) for n in nets]), torch.cat([flat_params(n) for n in onets]))   # the same numbers on both sides
    model.train()
    assert model.plan_name == "native" and model.N == c["N"], (model.plan_name, model.N)
    torch.cuda.synchronize()
    return model, model._native_plan


def assert_route(c, plan):
    assert isinstance(plan, psp.plan_dense_native.DenseNativePlan)
    assert (plan.d_pad, plan.H_pad) == c["expect"], (plan.d_pad, plan.H_pad)
    assert plan.matrix_mode == c["mode"] and plan.kernel_bwd == (c["bwd"] != "gemm")
    attached, relent = c["adaptive"] and not c["detach"], c["loss"] == "relative_entropy"
    assert plan.attached == attached and plan.relent == relent
    assert plan.cfg.base.store_path == (3 if relent else (2 if attached else 1)), plan.cfg.base.store_path
    assert plan.generic_loss == (c["loss"] in ("variance", "cross_entropy"))
    assert plan.outer == (c["tmode"] == "outer") and plan.B == (c["N"] if plan.outer else 1)
    if c["mode"] == "f16x3":
        assert plan.range_fallbacks() == 0                                # in range: the split kernels did the work
    if c["slices_gt1"]:
        # several slices per step, and more (step, 16-trajectory tile) items than four per backward workgroup: several rounds each
        sizes = nat.DnetSizes()
        nat.check(plan.lib.psp_dnet_query(C.byref(plan.cfg), C.byref(sizes)), "psp_dnet_query")
        assert plan.slices == int(sizes.slices) and plan.slices > 1, plan.slices
        assert c["N"] * ((c["K"] + 15) // 16) > 4 * int(sizes.bwd_workgroups), (c["N"], c["K"], int(sizes.bwd_workgroups))


WORST = {}                   # route -> (largest block error, block, set, case id): printed by the last case of the module
WORST_DL = [0.0, 0.0]        # largest D and loss errors


@pytest.mark.parametrize("c", dc.CASES, ids=[c["id"] for c in dc.CASES])
def test_first_iteration_blocks_match_the_float64_reference(c, monkeypatch):
    model, plan = run_case(c, monkeypatch)
    assert_route(c, plan)
    draw = philox_noise if c["noise"] == "philox" else dc.host_noise
    ref = dc.reference(c, lambda: draw(int(model.seed), c["K"], c["d"], c["N"]), stream="device")
    D, D_ref = plan.D.double().cpu(), ref["D"]
    assert D.shape == D_ref.shape and bool(torch.isfinite(D).all())
    eD = float((D - D_ref).abs().max()) / max(1.0, float(D_ref.abs().max()))
    tol_l = bc.first_loss_tol(bc.loss_values(c["loss"], D_ref), ref["loss"])
    el = abs(model.loss_log[0] - ref["loss"]) / abs(ref["loss"])
    print("%s [%s]: D %.2e (<= %.1e)  loss %.2e (<= %.1e)" % (c["id"], c["route"], eD, D_TOL, el, tol_l))
    g = plan.grad.cpu()
    assert g.shape == ref["grad"].shape and bool(torch.isfinite(g).all())
    inner = c["tmode"] == "inner"
    WORST_DL[0], WORST_DL[1] = max(WORST_DL[0], eD), max(WORST_DL[1], el)
    try:
        errs = assert_dense_blocks(g, ref["grad"], c["d"], c["H"], len(ref["sets"]), inner, BLOCK_TOL, tag=c["id"])
        worst, s, n = max((e, s, n) for s, es in enumerate(errs) for e, n in zip(es, dense_block_names(inner)))
        if worst > WORST.get(c["route"], (-1.0,))[0]:
            WORST[c["route"]] = (worst, n, s, c["id"])
        assert eD <= D_TOL, eD
        assert el <= tol_l, (model.loss_log[0], ref["loss"])
    finally:
        if c is dc.CASES[-1]:
            for route, (e, blk, s, cid) in sorted(WORST.items()):
                print("worst block per route: %-32s %.2e (%s of set %d) %s" % (route, e, blk, s, cid))
            print("worst D %.2e  worst loss %.2e" % tuple(WORST_DL))
