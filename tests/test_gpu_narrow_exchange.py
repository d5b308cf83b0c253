"""The exchange image of the narrow split-product backward (csrc/hjbx_kernels.h): the producers store their split panels by sample
rows in 8-byte chunks, the consumers read them back with the transposing LDS read, a partial last feature tile of G is kept
compact (RT = ceil((d mod 16) / 4) values per lane) and the accumulator rows come back permuted.  hjb_bwd3_kernel against its fp32
twin hjb_bwd2_kernel on the SAME path store through the C ABI (psp_hjb_rollout_bwd with caller-supplied trajectory weights), for
every tail shape of the compiled instances -- RT = 1 (d = 100: the LDS-bound case; d = 20: behind a full tile; d = 2: two real
features), RT = 2 (d = 8), RT = 3 (d = 10, tail only), no tail (16, 16), a zero-padded problem on (48, 32) -- with the increments
in the store (store_path 1) and regenerated (store_path 4: the other instance of the kernel).  K is ragged (16 m + 5) and gives
every workgroup at least three rounds (tests/block_cases.py case_K: more than two tiles per CU); N x tiles is no multiple of four,
so the last round has absent blocks.  Element by element within the bound tests/test_gpu_wide_backward_x3.py holds the same
comparison to, and three runs of the split kernel bit-equal."""
import pytest
import torch

from test_gpu_range_guard import _bwd, nat
from util_cases import assert_blocks, flat_params, psp

pytestmark = pytest.mark.gpu

N_STEPS = 7
# (d, H, instance the plan must choose)
SHAPES = [(100, 64, (100, 64)), (20, 30, (20, 30)), (10, 30, (10, 30)), (8, 30, (8, 30)), (2, 30, (2, 30)), (16, 16, (16, 16)),
          (40, 20, (48, 32))]


def ragged_K(cus):
    """16 m + 5 with m + 1 tiles, m >= 2 cus + 1 (block_cases.case_K), and 7 (m + 1) no multiple of four."""
    m = 2 * cus + 1
    while (m + 1) % 4 == 0:
        m += 1
    return 16 * m + 5


@pytest.mark.parametrize("store_path", [1, 4])
@pytest.mark.parametrize("d,H,inst", SHAPES, ids=["d%d-H%d" % s[:2] for s in SHAPES])
def test_split_backward_equals_fp32_twin_on_the_same_store(d, H, inst, store_path):
    dev = torch.device("cuda:0")
    K, N = ragged_K(torch.cuda.get_device_properties(dev).multi_processor_count), N_STEPS
    prob = psp.LLGC(d=d, off_diag=0.1 / d ** 0.5, T=(N + 0.5) * 0.01, seed=42, device=dev)
    m = psp.Solver("nx", prob, lr=1e-3, L=1, K=K, delta_t=0.01, loss_method="log-variance", time_approx="inner",
                   adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42,
                   device=dev, backend="native", noise="philox", widths=(H, H), mlp_dtype="f16x3",
                   path_noise="store" if store_path == 1 else "auto")
    params0 = flat_params(m.z_n)                                          # (train() takes an Adam step; the store is of THESE)
    m.train()                                                             # one forward fills the path store
    plan = m._native_plan
    assert m.N == N and plan.matrix_mode == "f16x3" and plan.family == 1
    assert (plan.d_pad, plan.H_pad) == inst and plan.cfg.store_path == store_path
    params0 = plan.pad.scatter_params(params0.to(dev), plan.pad.new_padded_params())      # the kernels' (padded) layout
    g = torch.Generator(device="cpu").manual_seed(11)
    w = (torch.randn(K, generator=g) * (2.0 / K)).to(dev)
    g3, rows3 = _bwd(plan, m, params0, w, nat.MLP_F16X3)
    g2, rows2 = _bwd(plan, m, params0, w, nat.MLP_FP32)
    nblk = N * ((K + 15) // 16)
    assert K % 16 == 5 and nblk % 4 != 0 and rows3.shape[0] * 4 * 3 <= nblk, "ragged K, absent blocks, three rounds per workgroup"
    scale = float(g2.abs().max())
    err = float((g3 - g2).abs().max())
    print("d=%d H=%d store_path=%d workgroups=%d: max |g3 - g2| = %.3e of max |g2| = %.3e" % (d, H, store_path, rows3.shape[0], err / scale, scale))
    assert scale > 0 and torch.isfinite(g3).all() and not torch.equal(g3, g2)
    assert err <= 2e-5 * scale                                            # every element, of the gradient's scale
    assert_blocks(g3, g2, plan.d_pad, plan.H_pad, 2e-5, tag="x3 vs fp32 d=%d H=%d" % (d, H))      # ... and of its block's
    for _ in range(2):
        g3b, rows3b = _bwd(plan, m, params0, w, nat.MLP_F16X3)
        assert torch.equal(g3b, g3) and torch.equal(rows3b, rows3)
