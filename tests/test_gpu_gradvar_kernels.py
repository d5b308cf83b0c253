"""psp_dnet_rollout_bwd_sq (hjbd_bwd_kernel<.., SQ>: the second moment of the per-trajectory gradients) through the C ABI against
the float64 reference tests/ref64_gradvar.py, with psp_dnet_rollout_bwd on the same images and weights as a control.

The images come from ONE forward of a net in the regime of tests/dense_block_cases.py (non-adaptive forward process: the stored
image is dY_k / dZ_n / sqrt(dt) itself; the nets' Adam has lr = 0 so that the parameters the kernels read are the ones the images
were made with -- asserted bit for bit), the weights w are random with mixed signs.  Compared, per step:
    S[w] = sum_k w_k G_k          (psp_dnet_rollout_bwd, the control)
    Q[w] = sum_k w_k^2 G_k o G_k  (psp_dnet_rollout_bwd_sq)
slices summed and gathered to the real parameters; EACH of the 9 blocks of EACH set within 2e-4 of that block's own maximum
(the project's BLOCK_TOL).  tests/test_ref64_gradvar.py asserts on the CPU that every block carries signal in this regime.

Shapes: (12, 16, K 37, N 4) ragged last tile, padded d and H on (16, 32); (20, 40, K 80, N 3) two slices on (32, 64); (70, 40, K 48,
N 3) the two column passes of (112, 64); (20, 30, K 9001, N 4) several slices of more than four tiles, i.e. more than one round;
N = 1 on the first shape.

Measured on an MI355X (worst block of any set, bound 2e-4; the test prints every block):
  shape (instance)                 S[w]      Q[w]
  d12-H16-K37-N4   (16x32)         6.29e-07  7.68e-07
  d20-H40-K80-N3   (32x64)         6.78e-07  7.59e-07
  d70-H40-K48-N3   (112x64)        7.28e-07  1.92e-06
  d20-H30-K9001-N4 (32x32)         8.43e-07  6.98e-07
  d12-H16-K37-N1   (16x32)         3.97e-07  4.25e-07
i.e. the squared products sit at the same fp32-against-float64 floor as the first moment; the file runs in 5 s.
"""
import ctypes as C

import pytest
import torch

import dense_block_cases as dc
import gradvar_cases as gc
import ref64_gradvar as r64
from util_cases import assert_dense_blocks, psp

pytestmark = pytest.mark.gpu
nat = psp.native
BLOCK_TOL = 2e-4


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape", gc.KERNEL_SHAPES, ids=["d%d-H%d-K%d-N%d" % s[:4] for s in gc.KERNEL_SHAPES])
def test_squared_outer_products_match_float64(shape):
    d, H, K, N, expect = shape
    c = gc.block_case(d, H, K, N, expect, loss="moment", adaptive=False)
    model, plan, oprob, ocfg, onets = gc.forward_once(c, dev())
    sizes = nat.DnetSizes()
    nat.check(plan.lib.psp_dnet_query(C.byref(plan.cfg), C.byref(sizes)), "psp_dnet_query")
    slices, PP = int(sizes.slices), int(sizes.padded_params)
    assert plan.partial.shape == (N * slices, PP)
    ntile = (K + 15) // 16
    if K > 1000:
        assert slices > 1 and ntile > 4 * slices, (slices, ntile)           # more than four tiles per slice: several rounds
        assert N * ntile > 4 * int(sizes.bwd_workgroups)
    if shape == gc.KERNEL_SHAPES[1]:
        assert slices >= 2, slices
    w = torch.randn(K, generator=torch.Generator().manual_seed(11))
    assert bool((w > 0).any()) and bool((w < 0).any())
    wpad = torch.zeros(16 * ntile, dtype=torch.float32, device=dev())
    wpad[:K] = w.to(dev())
    gidx = plan._gather_index()
    st = nat.stream_ptr(dev())
    out = {}
    for name in ("psp_dnet_rollout_bwd", "psp_dnet_rollout_bwd_sq"):
        partial = torch.zeros(N * slices, PP, dtype=torch.float32, device=dev())
        nat.check(getattr(plan.lib, name)(C.byref(plan.cfg), nat.ptr(plan.flat), nat.ptr(plan.images), nat.ptr(wpad), nat.ptr(partial),
                                          st), name)
        torch.cuda.synchronize()
        out[name] = partial.double().view(N, slices, PP).sum(1).index_select(1, gidx).cpu()
        assert bool(torch.isfinite(out[name]).all())
    ref = r64.moments(oprob, ocfg, onets, dc.host_noise(int(model.seed), K, d, N), weights=[w])
    tag = "d%d-H%d-K%d-N%d" % (d, H, K, N)
    eS = assert_dense_blocks(out["psp_dnet_rollout_bwd"].reshape(-1), ref["S"][0].reshape(-1), d, H, N, False, BLOCK_TOL, tag=tag + " S[w]")
    assert bool((out["psp_dnet_rollout_bwd_sq"] >= 0).all())
    eQ = assert_dense_blocks(out["psp_dnet_rollout_bwd_sq"].reshape(-1), ref["Q"][0].reshape(-1), d, H, N, False, BLOCK_TOL, tag=tag + " Q[w]")
    print("worst block %s (%dx%d): S[w] %.2e  Q[w] %.2e (<= %.1e)" % (tag, expect[0], expect[1], max(map(max, eS)), max(map(max, eQ)), BLOCK_TOL))


def test_entry_point_checks():
    """The arguments and checks of psp_dnet_rollout_bwd: null buffers, and an instance the hand-written backward does not cover."""
    d, H, K, N, expect = gc.KERNEL_SHAPES[0]
    c = gc.block_case(d, H, K, N, expect)
    _, plan, *_ = gc.forward_once(c, dev())
    lib = plan.lib
    assert lib.psp_dnet_rollout_bwd_sq(C.byref(plan.cfg), nat.ptr(plan.flat), nat.ptr(plan.images), None, nat.ptr(plan.partial),
                                       nat.stream_ptr(dev())) == -1
    cfg = nat.DnetConfig()
    C.memmove(C.byref(cfg), C.byref(plan.cfg), C.sizeof(cfg))
    cfg.base.d, cfg.base.H = 256, 32                                  # covered by the forward, not by the backward (kPasses = 0)
    assert lib.psp_dnet_rollout_bwd_sq(C.byref(cfg), nat.ptr(plan.flat), nat.ptr(plan.images), nat.ptr(plan.wpad),
                                       nat.ptr(plan.partial), nat.stream_ptr(dev())) == -3
