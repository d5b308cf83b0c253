"""GPU: hjbe_rollout_kernel (csrc/hjbe_kernels.h) behind psp_is_rollout, per trajectory, through direct C-ABI calls on the cases
of tests/is_kernel_cases.py: every (d bucket, control kind) instance, both ends of every bucket, every drift x sigma pair.
logw and XN are pre-filled with NaN.

(a) float64 differential on supplied noise, every case: |logw - logw64| / max(1, |logw64|) per trajectory and
    |XN - XN64| / max(1, max |XN64|) against tests/ref64_is.rollout64, bound 8 x E32 + 5e-7 with E32 the error of the numpy
    float32 recursion (rollout32) against the same reference -- computed from the reference side only.  GRID cases leave out the
    `near` trajectories (a lookup within 1e-4 cells of an edge; <= 10 %, asserted in tests/test_ref64_is.py).
(b) bit equality with rollout32 where the kernel header promises op-by-op rounding: drift ZERO / DIAG / DOUBLE_WELL, sigma
    IDENTITY / SCALED_IDENTITY, control NONE / TABLE / GRID; every trajectory, no `near` exclusion.
(c) Philox mode against supplied mode on psp_philox_normal_fill's stream at k_offset = 12345, a seed with a high word, iter = 9,
    K = 257, d at both ends of every bucket: bit-identical; the supplied run also meets (a)'s bound there, with the GRID kind's
    last trajectory at k_offset + K_local = K_global.
(d) sharding: K_global = 300 as one call and as (0, 130) + (130, 170), Philox mode: bit-identical per trajectory; the GRID case's
    last trajectory (local index 169 of the second call) against rollout64.
(e) buffer edges: 64 sentinel elements / rows around logw and XN stay untouched at K = 1, 37, 257, no entry stays NaN,
    XN_out = NULL and a repeated call give the same bits.

Measured on an MI355X (gfx950): maxima of (a) per instance (bucket / control kind), E_w / E_x.  In every case, the dense ones
included, they equal the float32 recursion's own E32_w / E32_x in every printed digit, so one column serves both; the bounds are
8 x these + 5e-7.
             NONE                 TABLE                LINEAR               GRID
    1    2.37e-07 / 1.20e-07  1.62e-08 / 6.76e-08  3.82e-07 / 1.80e-07  2.93e-07 / 1.65e-07
    4    3.44e-07 / 1.26e-07  2.96e-07 / 9.73e-08  4.84e-07 / 1.87e-07  3.67e-07 / 1.49e-07
    16   5.64e-07 / 1.40e-07  2.08e-07 / 1.27e-07  1.79e-07 / 1.23e-07  5.85e-07 / 1.43e-07
    32   2.73e-07 / 1.48e-07  2.68e-07 / 1.57e-07  2.63e-07 / 1.82e-07  9.76e-07 / 1.47e-07
    64   1.56e-06 / 1.36e-07  1.62e-07 / 1.45e-07  1.54e-06 / 2.04e-07  3.49e-07 / 1.65e-07
(c) at k_offset = 12345: between 2.17e-07 / 1.07e-07 and 1.55e-06 / 1.91e-07, again E32's digits; the fill against its float64
definition 5.96e-07.  (d): 3.09e-07 / 1.91e-07 (GRID), 2.83e-07 / 1.69e-07 (LINEAR); the GRID case's last trajectory: kernel
-13.3464746, float64 -13.3464743, float64 with the unshifted cell -13.5622849.
(b) compared 2639 trajectories of 14 cases bit for bit (logw and XN): none differs.
`near` trajectories of the GRID cases: b1_grid 1 / 300, b4_grid_d4 0 / 256, b4_grid_d2_x0_low 0 / 300, b16_grid_d16_row_oob
1 / 257, b16_grid_d5_x0_high 0 / 130, b32_grid_d17 2 / 257, b32_grid_d32 1 / 37, b64_grid_d64 4 / 257, b64_grid_d33 4 / 256.
Two one-line wrong-answer mutants of the kernel, built outside the tree: reading noise slice n for step n fails 50 of this
module's 53 tests (and tests/test_gpu_is_estimators.py); `last` without k_offset fails (c) on b1_grid and (d) on b4_grid_d4 and
nothing else in the suite's importance-sampling tests.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import is_kernel_cases as kc
import oracle.philox_oracle as po
import ref64_is as r64
from util_cases import psp

pytestmark = pytest.mark.gpu
nat = psp.native
SENTINEL = 7.25
PAD = 64


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rollout(desc, noise_mode=None, xi=None, seed=0, it=0, want_XN=True, pad=0):
    """One psp_is_rollout call: (logw, XN or None) as numpy fp32, the `pad` sentinel elements / rows at each end included."""
    cfg, keep = kc.device_config(desc, dev(), noise_mode)
    K, d = desc["K_local"], desc["d"]
    logw = torch.full((K + 2 * pad,), float("nan"), device=dev())
    XN = torch.full((K + 2 * pad, d), float("nan"), device=dev()) if want_XN else None
    for t in ((logw, XN) if pad else ()):
        if t is not None:
            t[:pad] = SENTINEL
            t[K + pad:] = SENTINEL
    nat.check(nat.load().psp_is_rollout(C.byref(cfg), nat.ptr(xi), seed, it, nat.ptr(logw, pad),
                                        nat.ptr(XN, pad * d) if want_XN else None, nat.stream_ptr(dev())), "psp_is_rollout")
    torch.cuda.synchronize()
    return logw.cpu().numpy(), (XN.cpu().numpy() if want_XN else None)


def supplied(desc, **kw):
    xi = torch.from_numpy(desc["noise"]).to(dev())
    return rollout(desc, nat.NOISE_SUPPLIED, xi, **kw)


def philox_fill(N, K, d, k_offset):
    xi = torch.full((N + 1, K, d), float("nan"), device=dev())
    nat.check(nat.load().psp_philox_normal_fill(nat.ptr(xi), N, K, d, k_offset, kc.PHILOX_SEED, kc.PHILOX_ITER, None),
              "psp_philox_normal_fill")
    torch.cuda.synchronize()
    return xi.cpu().numpy()


_GPU = {}


def gpu_result(c):
    """The kernel's (logw, XN) of a case on its host noise, computed once for (a) and (b)."""
    if c["id"] not in _GPU:
        _GPU[c["id"]] = supplied(kc.reference(c)[0])
    return _GPU[c["id"]]


def check_against_float64(tag, ref, logw, XN):
    desc, logw64, XN64, keep, ew32, ex32 = ref[:6]
    assert np.all(np.isfinite(logw)) and np.all(np.isfinite(XN)), tag
    ew, ex = r64.errors(logw, XN, logw64, XN64, keep)
    bw, bx = kc.bounds(ew32, ex32)
    print("%s: E_w %.2e (E32 %.2e, <= %.2e)  E_x %.2e (E32 %.2e, <= %.2e)  near %d / %d"
          % (tag, ew, ew32, bw, ex, ex32, bx, keep.size - keep.sum(), keep.size))
    assert ew <= bw and ex <= bx, (tag, ew, bw, ex, bx)
    return ew, ex


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", kc.IDS)
def test_float64_differential(cid):
    c = kc.BY_ID[cid]
    ref = kc.reference(c)
    logw, XN = gpu_result(c)
    kl = r64.last_local(ref[0])
    assert kl == c["K"] - 1 and ref[3][kl]                               # the last global trajectory always counts
    check_against_float64("%s %s" % (kc.route(c), cid), ref, logw, XN)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in kc.CASES if kc.bit_exact(c)])
def test_bit_equality_with_the_float32_recursion(cid):
    c = kc.BY_ID[cid]
    logw32, XN32 = kc.reference(c)[6:8]
    logw, XN = gpu_result(c)
    bad_w, bad_x = np.flatnonzero(logw != logw32), np.flatnonzero(np.any(XN != XN32, axis=1))
    print("%s %s: %d trajectories compared bit for bit; differing: logw %d, XN %d" % (kc.route(c), cid, c["K"], bad_w.size, bad_x.size))
    assert np.array_equal(XN, XN32), (cid, bad_x[:8], np.abs(XN - XN32).max())
    assert np.array_equal(logw, logw32), (cid, bad_w[:8], np.abs(logw - logw32).max())


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def test_philox_fill_matches_its_definition_at_an_offset():
    N, K, d = 3, 33, 5
    got = philox_fill(N, K, d, kc.PHILOX_OFFSET).astype(np.float64)
    want = po.normal_stream(N, K, d, k_offset=kc.PHILOX_OFFSET, seed=kc.PHILOX_SEED, iteration=kc.PHILOX_ITER)
    assert np.all(got[0] == 0.0)
    err = np.abs(got - want).max()
    print("d = 5, k_offset = %d: max |device - float64 definition| = %.2e" % (kc.PHILOX_OFFSET, err))
    assert err <= 2e-5, err                                             # (tests/test_philox_oracle.py's tolerance)


@pytest.mark.parametrize("cid", kc.PHILOX_IDS)
def test_philox_mode_matches_supplied_mode_at_an_offset(cid):
    c = kc.BY_ID[cid]
    K, off = 257, kc.PHILOX_OFFSET
    assert kc.PHILOX_SEED >> 32 != 0
    xi = philox_fill(c["N"], K, c["d"], off)
    desc = kc.describe(c, K=K, K_global=off + K, k_offset=off, noise=xi)
    lw_s, XN_s = supplied(desc)
    lw_p, XN_p = rollout(desc, nat.NOISE_PHILOX, None, kc.PHILOX_SEED, kc.PHILOX_ITER)
    assert np.array_equal(lw_s, lw_p) and np.array_equal(XN_s, XN_p), (cid, np.flatnonzero(lw_s != lw_p)[:8])
    check_against_float64("%s %s k_offset %d" % (kc.route(c), cid, off), kc.evaluate(desc), lw_s, XN_s)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", kc.SHARD_IDS)
def test_two_shards_reproduce_one_call(cid):
    c = kc.BY_ID[cid]
    K, K0 = kc.SHARD_K, kc.SHARD_SPLIT
    zeros = lambda k: np.zeros((c["N"] + 1, k, c["d"]), np.float32)     # (Philox mode reads no supplied noise)
    run = lambda desc: rollout(desc, nat.NOISE_PHILOX, None, kc.PHILOX_SEED, kc.PHILOX_ITER)
    lw, XN = run(kc.describe(c, K=K, K_global=K, k_offset=0, noise=zeros(K)))
    lw0, XN0 = run(kc.describe(c, K=K0, K_global=K, k_offset=0, noise=zeros(K0)))
    lw1, XN1 = run(kc.describe(c, K=K - K0, K_global=K, k_offset=K0, noise=zeros(K - K0)))
    assert np.all(np.isfinite(lw)) and np.all(np.isfinite(XN))
    assert np.array_equal(np.concatenate([lw0, lw1]), lw), np.flatnonzero(np.concatenate([lw0, lw1]) != lw)[:8]
    assert np.array_equal(np.concatenate([XN0, XN1]), XN)
    # against float64 on the materialised stream; in the split run the last-trajectory rule fires in the second call alone
    desc = kc.describe(c, K=K, K_global=K, k_offset=0, noise=philox_fill(c["N"], K, c["d"], 0))
    ref = kc.evaluate(desc)
    check_against_float64("%s %s sharded" % (kc.route(c), cid), ref, np.concatenate([lw0, lw1]), np.concatenate([XN0, XN1]))
    if c["ctrl"] == nat.ISC_GRID:
        logw64, keep = ref[1], ref[3]
        kl = K - K0 - 1
        assert kl == 169 and keep[K - 1]
        unshifted = r64.rollout64(dict(desc, K_global=K + 1))[0][K - 1]
        bw = kc.bounds(ref[4], ref[5])[0] * max(1.0, abs(logw64[K - 1]))
        print("last trajectory: kernel %.7f  float64 %.7f  float64 with the unshifted cell %.7f" % (lw1[kl], logw64[K - 1], unshifted))
        assert abs(unshifted - logw64[K - 1]) > 100 * bw                  # (random tables: an O(1) change of the control)
        assert abs(lw1[kl] - logw64[K - 1]) <= bw


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", kc.EDGE_IDS)
def test_buffer_edges(cid):
    c = kc.BY_ID[cid]
    desc = kc.reference(c)[0]
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
