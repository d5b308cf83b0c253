"""The producers of the role-specialised backward kernels walk their sample blocks with psp::BlockCursor (csrc/block_index.h):
(tile, step) of round it + 1 is that of round it plus a constant pair and one carry, no division in the round loop
(tests/test_block_index_host.py holds the cursor itself to the division form, on the host).  Here the kernels that use it:
hjb_bwd3_kernel against its fp32 twin hjb_bwd2_kernel on the SAME path store through the C ABI (psp_hjb_rollout_bwd with
caller-supplied trajectory weights), at the bound of tests/test_gpu_narrow_exchange.py, with the increments read from the store
(store_path 1) and regenerated from the Philox counters (store_path 4: the other instance of the kernel, and the only reader of the
cursor's step as a COUNTER) -- the two bit-identical, which a wrong tile, step or k_offset of any block breaks.

Shapes at d = 100, H = 64, the smallest at which the recurrence can go wrong (figures for a 256-workgroup grid: stride 1024
blocks per round; the test reads the grid of each launch from the library's size query and works out rounds and carries from it):
  K = 590, N = 60     ntile16 = 37, last tile partial, 2220 blocks; 1024 = 27 * 37 + 25: the carry fires on some rounds only
  K = 48, N = 700     ntile16 = 3: stride >> ntile16, r = 1
  K = 17600, N = 3    ntile16 = 1100 > stride: q = 0; 3300 blocks are no multiple of 1024: the last round has absent blocks
  K = 16, N = 2       two blocks, one round, two idle producers from round 0 on
  K = 592, N = 60 in two chunks (304 + 288): the backward of the second chunk, k_offset = 304
The store is written once per case with the increments in it (store_path 1, which a launch this small gets by default); the same
store then serves both backward instances: under store_path 4 the kernel ignores the stored increments and regenerates them."""
import ctypes as C
import functools

import pytest
import torch

from util_cases import assert_blocks, flat_params, psp

pytestmark = pytest.mark.gpu
nat = psp.native

D, H = 100, 64
# name: (K, N, delta_t, chunks)
CASES = {
    "K590-N60": (590, 60, 0.01, None),
    "K48-N700": (48, 700, 0.001, None),
    "K17600-N3": (17600, 3, 0.01, None),
    "K16-N2": (16, 2, 0.01, None),
    "K592-N60-chunk2": (592, 60, 0.01, 2),
}


def _bwd(plan, model, base_cfg, params, w, mlp, store_path):
    """psp_hjb_rollout_bwd over the plan's path store under `base_cfg` (a weights config: its K_local and k_offset say which
    trajectories the store holds) with the matrix mode and the noise source chosen here."""
    dev = torch.device("cuda:0")
    cfg = nat.HjbConfig.from_buffer_copy(base_cfg)
    cfg.loss_kind, cfg.mlp_dtype, cfg.range_flag, cfg.store_path = nat.LOSS_WEIGHTS, mlp, None, store_path
    sizes = nat.query(cfg)
    grad = torch.zeros(plan.pad.Pp, dtype=torch.float32, device=dev)
    part = torch.zeros(sizes.grad_partial_bytes // 4, dtype=torch.float32, device=dev)
    nat.check(nat.load().psp_hjb_rollout_bwd(C.byref(cfg), nat.ptr(params), None, int(model.seed), 0, nat.ptr(plan.path),
                                              nat.ptr(w), nat.ptr(plan.sums), nat.ptr(part), nat.ptr(grad),
                                              nat.stream_ptr(dev)), "psp_hjb_rollout_bwd")
    torch.cuda.synchronize()
    return grad, int(sizes.bwd_workgroups)


def _walk(grid, ntile16, N):
    """(most rounds of a workgroup, valid round-to-round steps with a carry, without) of a launch, by the division form."""
    nblk = N * ntile16
    nround = (nblk + 3) // 4
    stride = 4 * grid
    carry = plain = 0
    for b in range(nblk - stride if nblk > stride else 0):             # every block whose slot has a next block in the store
        if b % ntile16 + stride % ntile16 >= ntile16:
            carry += 1
        else:
            plain += 1
    return (nround + grid - 1) // grid, carry, plain


@functools.lru_cache(maxsize=None)
def _case(name):
    K, N, dt, chunks = CASES[name]
    dev = torch.device("cuda:0")
    prob = psp.LLGC(d=D, off_diag=0.1 / D ** 0.5, T=(N + 0.5) * dt, seed=42, device=dev)
    extra = dict(path_chunks=chunks, chunk_mode="two_gradient") if chunks else {}
    m = psp.Solver("bi", prob, lr=1e-3, L=1, K=K, delta_t=dt, loss_method="log-variance", time_approx="inner",
                   adaptive_forward_process=True, detach_forward=True, u_l2_error_flag=False, verbose=False, seed=42,
                   device=dev, backend="native", noise="philox", widths=(H, H), mlp_dtype="f16x3", path_noise="store", **extra)
    params0 = flat_params(m.z_n)                                          # (train() takes an Adam step; the store is of THESE)
    m.train()                                                             # one forward (per chunk) fills the path store
    plan = m._native_plan
    assert m.N == N and plan.matrix_mode == "f16x3" and plan.family == 1 and (plan.d_pad, plan.H_pad) == (D, H)
    assert plan.cfg.store_path == 1
    if chunks:
        assert plan.n_chunks == chunks
        off, Kc, _, _, base = plan.chunks[-1]                             # the store holds the LAST chunk's paths
        assert off > 0 and base.k_offset == off and base.K_local == Kc
    else:
        base, Kc = plan.cfg, K
        assert base.K_local == K and base.k_offset == 0
    params0 = plan.pad.scatter_params(params0.to(dev), plan.pad.new_padded_params())      # the kernels' (padded) layout
    g = torch.Generator(device="cpu").manual_seed(11)
    w = (torch.randn(Kc, generator=g) * (2.0 / Kc)).to(dev)
    g2, grid2 = _bwd(plan, m, base, params0, w, nat.MLP_FP32, 1)          # the reference: computed once, shared, left alone
    g3 = {sp: _bwd(plan, m, base, params0, w, nat.MLP_F16X3, sp) for sp in (1, 4)}
    g2r, _ = _bwd(plan, m, base, params0, w, nat.MLP_FP32, 4)             # the twin's own regenerating path
    grid3 = g3[1][1]
    assert g3[4][1] == grid3
    ntile16 = (Kc + 15) // 16
    return dict(g2=g2, g2r=g2r, g3={sp: g3[sp][0] for sp in (1, 4)}, grid=grid3, grid2=grid2, ntile16=ntile16, N=N,
                walk=_walk(grid3, ntile16, N), plan=plan)


@pytest.mark.parametrize("store_path", [1, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_split_backward_equals_fp32_twin_on_the_same_store(name, store_path):
    r = _case(name)
    g3, g2 = r["g3"][store_path], r["g2"]
    scale = float(g2.abs().max())
    err = float((g3 - g2).abs().max())
    print("%s store_path=%d workgroups=%d ntile16=%d rounds<=%d carries=%d plain=%d: max |g3 - g2| = %.3e of max |g2| = %.3e"
          % ((name, store_path, r["grid"], r["ntile16"]) + r["walk"] + (err / scale, scale)))
    assert scale > 0 and torch.isfinite(g3).all() and not torch.equal(g3, g2)
    assert err <= 2e-5 * scale                                            # every element, of the gradient's scale
    assert_blocks(g3, g2, D, H, 2e-5, tag="x3 vs fp32 %s" % name)         # ... and of its block's


@pytest.mark.parametrize("name", list(CASES))
def test_stored_and_regenerated_increments_give_the_same_bits(name):
    r = _case(name)
    assert torch.equal(r["g3"][1], r["g3"][4])                            # hjb_bwd3_kernel<.., false> and <.., true>
    assert torch.equal(r["g2"], r["g2r"])                                 # hjb_bwd2_kernel, store_path read at run time


def test_cases_reach_three_rounds_and_a_carry():
    walks = {name: _case(name)["walk"] for name in CASES}
    print(walks)
    assert any(R >= 3 for R, _, _ in walks.values()), walks
    assert any(carry > 0 and plain > 0 for _, carry, plain in walks.values()), walks
