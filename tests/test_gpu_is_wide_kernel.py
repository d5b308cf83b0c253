"""GPU: isw_rollout_kernel (csrc/hjbew_kernels.h) behind psp_isw_rollout, per trajectory, through direct C-ABI calls on the cases
of tests/is_wide_cases.py: every (block bucket, control kind) instance, every drift x sigma pair.  logw and XN are pre-filled
with NaN, the table scratch too.

(a) float64 differential on supplied noise, every case: E_w and E_x of ref64_is.errors against rollout64, bound
    is_kernel_cases.bounds(E32_w, E32_x) = 8 x the float32 recursion's own error + 5e-7, computed from the reference side only
    (the rule of tests/test_gpu_is_kernel.py).  GRID cases leave out the `near` trajectories (<= 10 %, asserted in
    tests/test_ref64_is_wide.py).
(b) X_N bit-equal to rollout32 for every case without a dense drift, a dense sigma or a LINEAR control; every trajectory, no
    `near` exclusion.  (logw is not compared bit for bit: the sums over features are reduced across lanes.)
(c) d = 16 and 48 on the same supplied noise: psp_isw_rollout and psp_is_rollout both meet (a), X_N bit-equal between them on
    the op-by-op cases.
(d) Philox mode against supplied mode on psp_philox_normal_fill's stream at k_offset = 12345, a seed with a high word, iter = 9,
    K = 257, d = 65 and d = 256: bit-identical.
(e) sharding: K_global = 300 as one call and as (0, 130) + (130, 170), Philox mode: bit-identical per trajectory; the GRID case's
    last trajectory (local index 169 of the second call) against rollout64.
(f) buffer edges: 64 sentinel elements / rows around logw and XN stay untouched at K = 1, 17, 257, no entry stays NaN,
    XN_out = NULL and a repeated call give the same bits.

Measured on an MI355X (gfx950): maxima of (a) per (d, control kind), E_w / E_x.  E_x equals the float32 recursion's own E32_x in
every printed digit, the dense cases included; E_w lies between 0.32 x and 1.13 x E32_w (mostly below: the lane-wise partial
sums are shorter than one sequential sum), so the bounds 8 x E32 + 5e-7 are met with a factor 7 to spare.
           NONE                 TABLE                LINEAR               GRID
    16    5.14e-07 / 7.94e-08  -                    -                    5.74e-07 / 1.77e-07
    48    -                    1.12e-07 / 1.08e-07  2.77e-07 / 1.76e-07  -
    65    5.82e-07 / 1.23e-07  5.91e-08 / 7.34e-08  2.04e-07 / 1.40e-07  1.48e-07 / 1.58e-07
    80    1.23e-07 / 1.74e-07  7.11e-07 / 1.59e-07  -                    1.94e-07 / 1.20e-07
    100   -                    -                    1.57e-06 / 1.40e-07  1.88e-07 / 1.78e-07
    130   2.31e-06 / 1.13e-07  1.47e-07 / 1.91e-07  1.57e-07 / 9.51e-08  1.58e-06 / 1.81e-07
    200   1.99e-06 / 2.07e-07  -                    2.58e-07 / 2.33e-07  2.42e-07 / 1.19e-07
    256   -                    2.89e-07 / 1.00e-07  5.88e-07 / 1.97e-07  -
E32_w of the same cells, for comparison (E32_x = E_x):
    16    4.56e-07             -                    -                    5.56e-07
    48    -                    2.28e-07             3.93e-07             -
    65    1.30e-06             1.33e-07             3.38e-07             2.96e-07
    80    1.52e-07             1.13e-06             -                    3.39e-07
    100   -                    -                    1.66e-06             4.72e-07
    130   2.68e-06             2.86e-07             2.47e-07             2.47e-06
    200   2.85e-06             -                    4.04e-07             7.55e-07
    256   -                    8.60e-07             7.92e-07             -
(b) compared 1891 trajectories of 11 cases bit for bit (XN): none differs.  (c): the narrow kernel has E32's digits, the wide one
the figures above; XN is bit-equal between them on w16_none, w16_grid and w48_table.  (d) at k_offset = 12345: 1.38e-07 / 1.29e-07
(d = 65, GRID), 9.80e-07 / 2.65e-07 (d = 256, LINEAR).  (e): 1.52e-07 / 1.37e-07 (GRID), 1.36e-06 / 1.28e-07 (LINEAR); the GRID
case's last trajectory: kernel -98.4462433, float64 -98.4462408, float64 with the unshifted cell -98.0411368.
`near` trajectories of the GRID cases: w65_grid_row_oob 11 / 257, w80_grid_x0_low 1 / 37, w100_grid_x0_high 9 / 257, w130_grid
12 / 257, w200_grid 9 / 257, w16_grid 4 / 257.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import is_kernel_cases as ikc
import is_wide_cases as wc
import ref64_is as r64
from util_cases import psp

pytestmark = pytest.mark.gpu
nat = psp.native
SENTINEL = 7.25
PAD = 64


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rollout(desc, noise_mode=None, xi=None, seed=0, it=0, want_XN=True, pad=0, narrow=False):
    """One psp_isw_rollout call (narrow: psp_is_rollout): (logw, XN or None) as numpy fp32, the `pad` sentinel elements / rows at
    each end included."""
    cfg, keep = ikc.device_config(desc, dev(), noise_mode)
    K, d = desc["K_local"], desc["d"]
    logw = torch.full((K + 2 * pad,), float("nan"), device=dev())
    XN = torch.full((K + 2 * pad, d), float("nan"), device=dev()) if want_XN else None
    for t in ((logw, XN) if pad else ()):
        if t is not None:
            t[:pad] = SENTINEL
            t[K + pad:] = SENTINEL
    lib = nat.load()
    if narrow:
        nat.check(lib.psp_is_rollout(C.byref(cfg), nat.ptr(xi), seed, it, nat.ptr(logw, pad),
                                     nat.ptr(XN, pad * d) if want_XN else None, nat.stream_ptr(dev())), "psp_is_rollout")
    else:
        s, why = wc.sizes(cfg)
        assert why is None, why
        assert s.table_bytes == wc.table_bytes(desc)
        tables = torch.full((s.table_bytes // 4 + PAD,), float("nan"), device=dev())
        tables[s.table_bytes // 4:] = SENTINEL
        nat.check(lib.psp_isw_rollout(C.byref(cfg), nat.ptr(xi), seed, it, nat.ptr(tables), nat.ptr(logw, pad),
                                      nat.ptr(XN, pad * d) if want_XN else None, nat.stream_ptr(dev())), "psp_isw_rollout")
        torch.cuda.synchronize()
        assert bool(torch.all(tables[s.table_bytes // 4:] == SENTINEL)), "the table kernel wrote past table_bytes"
    torch.cuda.synchronize()
    return logw.cpu().numpy(), (XN.cpu().numpy() if want_XN else None)


def supplied(desc, **kw):
    xi = torch.from_numpy(desc["noise"]).to(dev())
    return rollout(desc, nat.NOISE_SUPPLIED, xi, **kw)


def philox_fill(N, K, d, k_offset):
    xi = torch.full((N + 1, K, d), float("nan"), device=dev())
    nat.check(nat.load().psp_philox_normal_fill(nat.ptr(xi), N, K, d, k_offset, ikc.PHILOX_SEED, ikc.PHILOX_ITER, None),
              "psp_philox_normal_fill")
    torch.cuda.synchronize()
    return xi.cpu().numpy()


_GPU = {}


def gpu_result(c):
    """The kernel's (logw, XN) of a case on its host noise, computed once for (a), (b), (c) and (f)."""
    if c["id"] not in _GPU:
        _GPU[c["id"]] = supplied(wc.reference(c)[0])
    return _GPU[c["id"]]


def check_against_float64(tag, ref, logw, XN):
    desc, logw64, XN64, keep, ew32, ex32 = ref[:6]
    assert np.all(np.isfinite(logw)) and np.all(np.isfinite(XN)), tag
    ew, ex = r64.errors(logw, XN, logw64, XN64, keep)
    bw, bx = ikc.bounds(ew32, ex32)
    print("%s: E_w %.2e (E32 %.2e, <= %.2e)  E_x %.2e (E32 %.2e, <= %.2e)  near %d / %d"
          % (tag, ew, ew32, bw, ex, ex32, bx, keep.size - keep.sum(), keep.size))
    assert ew <= bw and ex <= bx, (tag, ew, bw, ex, bx)
    return ew, ex


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", wc.IDS)
def test_float64_differential(cid):
    c = wc.BY_ID[cid]
    ref = wc.reference(c)
    logw, XN = gpu_result(c)
    kl = r64.last_local(ref[0])
    assert kl == c["K"] - 1 and ref[3][kl]                               # the last global trajectory always counts
    check_against_float64("%s %s" % (wc.route(c), cid), ref, logw, XN)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in wc.CASES if wc.bit_exact(c)])
def test_final_state_bit_equal_to_the_float32_recursion(cid):
    c = wc.BY_ID[cid]
    XN32 = wc.reference(c)[7]
    XN = gpu_result(c)[1]
    bad = np.flatnonzero(np.any(XN != XN32, axis=1))
    print("%s %s: %d trajectories compared bit for bit; differing XN: %d" % (wc.route(c), cid, c["K"], bad.size))
    assert np.array_equal(XN, XN32), (cid, bad[:8], np.abs(XN - XN32).max())


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", wc.NARROW_IDS)
def test_wide_and_narrow_kernel_on_the_same_noise(cid):
    c = wc.BY_ID[cid]
    ref = wc.reference(c)
    lw_w, XN_w = gpu_result(c)
    lw_n, XN_n = supplied(ref[0], narrow=True)
    check_against_float64("%s %s wide" % (wc.route(c), cid), ref, lw_w, XN_w)
    check_against_float64("%s %s narrow" % (wc.route(c), cid), ref, lw_n, XN_n)
    if wc.bit_exact(c):
        assert np.array_equal(XN_w, XN_n), (cid, np.flatnonzero(np.any(XN_w != XN_n, axis=1))[:8])


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", wc.PHILOX_IDS)
def test_philox_mode_matches_supplied_mode_at_an_offset(cid):
    c = wc.BY_ID[cid]
    K, off = 257, ikc.PHILOX_OFFSET
    assert off == 12345 and ikc.PHILOX_SEED >> 32 != 0 and ikc.PHILOX_ITER == 9
    xi = philox_fill(c["N"], K, c["d"], off)
    desc = wc.describe(c, K=K, K_global=off + K, k_offset=off, noise=xi)
    lw_s, XN_s = supplied(desc)
    lw_p, XN_p = rollout(desc, nat.NOISE_PHILOX, None, ikc.PHILOX_SEED, ikc.PHILOX_ITER)
    assert np.all(np.isfinite(lw_p)) and np.all(np.isfinite(XN_p))
    assert np.array_equal(lw_s, lw_p) and np.array_equal(XN_s, XN_p), (cid, np.flatnonzero(lw_s != lw_p)[:8])
    check_against_float64("%s %s k_offset %d" % (wc.route(c), cid, off), ikc.evaluate(desc), lw_s, XN_s)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", wc.SHARD_IDS)
def test_two_shards_reproduce_one_call(cid):
    c = wc.BY_ID[cid]
    K, K0 = ikc.SHARD_K, ikc.SHARD_SPLIT
    assert (K, K0) == (300, 130)
    zeros = lambda k: np.zeros((c["N"] + 1, k, c["d"]), np.float32)     # (Philox mode reads no supplied noise)
    run = lambda desc: rollout(desc, nat.NOISE_PHILOX, None, ikc.PHILOX_SEED, ikc.PHILOX_ITER)
    lw, XN = run(wc.describe(c, K=K, K_global=K, k_offset=0, noise=zeros(K)))
    lw0, XN0 = run(wc.describe(c, K=K0, K_global=K, k_offset=0, noise=zeros(K0)))
    lw1, XN1 = run(wc.describe(c, K=K - K0, K_global=K, k_offset=K0, noise=zeros(K - K0)))
    assert np.all(np.isfinite(lw)) and np.all(np.isfinite(XN))
    assert np.array_equal(np.concatenate([lw0, lw1]), lw), np.flatnonzero(np.concatenate([lw0, lw1]) != lw)[:8]
    assert np.array_equal(np.concatenate([XN0, XN1]), XN)
    # against float64 on the materialised stream; in the split run the last-trajectory rule fires in the second call alone
    desc = wc.describe(c, K=K, K_global=K, k_offset=0, noise=philox_fill(c["N"], K, c["d"], 0))
    ref = ikc.evaluate(desc)
    check_against_float64("%s %s sharded" % (wc.route(c), cid), ref, np.concatenate([lw0, lw1]), np.concatenate([XN0, XN1]))
    if c["ctrl"] == nat.ISC_GRID:
        logw64, keep = ref[1], ref[3]
        kl = K - K0 - 1
        assert kl == 169 and keep[K - 1]
        unshifted = r64.rollout64(dict(desc, K_global=K + 1))[0][K - 1]
        bw = ikc.bounds(ref[4], ref[5])[0] * max(1.0, abs(logw64[K - 1]))
        print("last trajectory: kernel %.7f  float64 %.7f  float64 with the unshifted cell %.7f" % (lw1[kl], logw64[K - 1], unshifted))
        assert abs(unshifted - logw64[K - 1]) > 100 * bw                  # (random tables: an O(1) change of the control)
        assert abs(lw1[kl] - logw64[K - 1]) <= bw


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", wc.EDGE_IDS)
def test_buffer_edges(cid):
    c = wc.BY_ID[cid]
    desc = wc.reference(c)[0]
    K = c["K"]
    lw, XN = supplied(desc, pad=PAD)
    for t in (lw, XN):
        assert np.all(t[:PAD] == SENTINEL) and np.all(t[K + PAD:] == SENTINEL), cid
        assert np.all(np.isfinite(t[PAD:K + PAD])), cid
    lw_only, none = supplied(desc, want_XN=False, pad=PAD)
    assert none is None and np.array_equal(lw_only, lw)
    again = supplied(desc, pad=PAD)
    assert np.array_equal(again[0], lw) and np.array_equal(again[1], XN)
    first = gpu_result(c)
    assert np.array_equal(first[0], lw[PAD:K + PAD]) and np.array_equal(first[1], XN[PAD:K + PAD])
