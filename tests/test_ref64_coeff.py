"""What makes tests/test_gpu_coeff_vectors.py meaningful, checked on the CPU with the float64 reference alone, for every distinct
reference of tests/coeff_cases.py:

  a. every varied vector is injective (minimum gap between any two entries >= 1e-3 of its range), has no period of 4, 16 or 64,
     and no two vectors share a phase;
  b. the case is still in the regime the block tests were built for: tanh nets median |h1|, |h2| in [0.15, 0.85]
     (tests/test_ref64.py), DenseNets every block >= 1e-2 of its set's maximum, every set >= 0.1 of the global one, 0.2 .. 0.8 of
     the hidden units active with a mean relu(z) >= 0.1 (tests/test_ref64_dense.py); max |D| < 100 (DenseNets: <= 50, as there);
  c. PLANTED ERRORS: the reference recomputed with one vector as a mis-indexed read would see it -- entries 1 and 2 exchanged, the
     in-block permutation i -> 4 (i & 3) + (i >> 2), entry 0 for every coordinate -- moves D by at least 10 x D_TOL max(1, max |D|)
     and, in attached cases, at least one gradient block by at least 10 x BLOCK_TOL of that block's maximum: D_TOL and BLOCK_TOL are
     the GPU test's bounds.  A condition on the INPUTS: a case that falls short gets a wider range or more steps, never a lower
     factor.  (On K = 16 trajectories of the case's noise, which keeps the file under a minute.)
  d. the bounds are reachable: ref64.iteration(..., dtype=torch.float32), the stand-in of a correct fp32 kernel, is within D_TOL / 10
     and BLOCK_TOL / 10 of float64 on every tanh case.

Measured (the tests print every figure): the smallest planted-error factors are 13 x D_TOL (kappa, entries 1 and 2 exchanged, d = 200
and 250) and, attached, 16 x BLOCK_TOL (P, entries 1 and 2 exchanged, d = 200); the fp32 stand-in is within 1.8e-7 (D) and 3.1e-6 (worst
block) of float64.
"""
import math

import pytest
import torch

import coeff_cases as cc
from oracle import philox_oracle
from test_gpu_block_gradients import BLOCK_TOL, D_TOL          # (its tests are marked gpu; the module itself imports without one)
from util_cases import (BLOCK_NAMES, block_errors, dense_block_errors, dense_block_names, dense_grad_blocks, grad_blocks)

FACTOR = 10.0
K_PLANTED = 16
DISTINCT = cc.distinct(cc.CASES)
IDS = [c["id"] for c in DISTINCT]


def cpu_noise(c, K):
    """The stream the case's kernels draw from: the host generator, or the numpy restatement of the device Philox stream (real d)."""
    if c["noise"] == "philox":
        return torch.from_numpy(philox_oracle.normal_stream(c["N"], K, c["d"], 0, 42, 0)).float().permute(1, 2, 0).contiguous()
    return cc.bc.host_noise(42, K, c["d"], c["N"])


def ref(c, **kw):
    return cc.reference(c, c["K"], lambda: cpu_noise(c, c["K"]), **kw)


def worst_block(c, g, r):
    """(largest block error, its name) of gradient g against the reference result r."""
    if c["family"] == "tanh":
        return max(zip(block_errors(g, r["grad"], c["d"], c["H"]), BLOCK_NAMES))
    inner = c["tmode"] == "inner"
    errs = dense_block_errors(g, r["grad"], c["d"], c["H"], len(r["sets"]), inner)
    return max((e, "%s[%d]" % (n, s)) for s, es in enumerate(errs) for e, n in zip(es, dense_block_names(inner)))


def test_vectors_are_injective_and_aperiodic():
    phases = [v[2] for v in cc.RANGES.values()] + [cc.X0_RANGES["LLGC"][2]]
    assert len(set(phases)) == len(phases) and {r[2] for r in cc.X0_RANGES.values()} == {cc.X0_RANGES["LLGC"][2]}
    seen = set()
    for c in cc.CASES:
        if (c["cset"], c["d"]) in seen:
            continue
        seen.add((c["cset"], c["d"]))
        vs = cc.vectors(c["cset"], c["d"])
        assert set(vs) == set(cc.SETS[c["cset"]][1])
        for name, v in vs.items():
            assert v.dtype == torch.float32 and v.shape == (c["d"],)
            lo, hi, _ = cc.X0_RANGES[c["kind"]] if name == "X_0" else cc.RANGES[name]      # (alpha: the range before the sign flips)
            s = torch.sort(v.double()).values
            gap = float((s[1:] - s[:-1]).min()) / (hi - lo)
            per = min(float((v[p:] - v[:-p]).abs().min()) for p in (4, 16, 64) if p < c["d"]) / (hi - lo)
            print("%s d=%d %s: min gap %.2e of the range, nearest periodic image %.2e" % (c["cset"], c["d"], name, gap, per))
            assert gap >= 1e-3 and per >= 1e-3, (c["cset"], c["d"], name, gap, per)
            for which in cc.PLANTED:                                     # ... so that every planted error changes the vector
                assert not torch.equal(cc.plant(v, which), v)
    assert {c["d"] for c in cc.CASES} >= {20, 65, 100, 120, 200, 250, 320, 500}


@pytest.mark.parametrize("c", DISTINCT, ids=IDS)
def test_case_is_in_the_regime(c):
    r = ref(c)
    Dmax = float(r["D"].abs().max())
    assert r["N"] == c["N"] and math.isfinite(Dmax)
    if c["family"] == "tanh":
        m1, m2 = float(r["h1"].abs().median()), float(r["h2"].abs().median())
        bm = [float(b.abs().max()) for b in grad_blocks(r["grad"], c["d"], c["H"])]
        print("%s: median |h1| %.2f |h2| %.2f  max |D| %.3g  smallest block %s at %.3g of the largest" %
              (c["id"], m1, m2, Dmax, BLOCK_NAMES[bm.index(min(bm))], min(bm) / max(bm)))
        assert 0.15 <= m1 <= 0.85 and 0.15 <= m2 <= 0.85, (m1, m2)
        assert Dmax < 100.0, Dmax
        return
    inner = c["tmode"] == "inner"
    names = dense_block_names(inner)
    gmax = float(r["grad"].abs().max())
    low = []
    for s, bl in enumerate(dense_grad_blocks(r["grad"], c["d"], c["H"], len(r["sets"]), inner)):
        m = [float(b.abs().max()) for b in bl]
        low.append((min(m) / max(m), names[m.index(min(m))], max(m) / gmax, s))
    a1, a2 = r["z1"] > 0, r["z2"] > 0
    s1, s2 = float(a1.double().mean()), float(a2.double().mean())
    m1, m2 = float(r["z1"][a1].mean()), float(r["z2"][a2].mean())
    print("%s: max |D| %.3g  active %.2f %.2f  mean relu %.2f %.2f  smallest block %.2e (%s of set %d)  smallest set %.2f" %
          (c["id"], Dmax, s1, s2, m1, m2, min(low)[0], min(low)[1], min(low)[3], min(x[2] for x in low)))
    assert all(x[0] >= 1e-2 for x in low), low
    assert all(x[2] >= 0.1 for x in low), low
    assert Dmax <= 50.0, Dmax
    assert 0.2 <= s1 <= 0.8 and 0.2 <= s2 <= 0.8, (s1, s2)
    assert m1 >= 0.1 and m2 >= 0.1, (m1, m2)


@pytest.mark.parametrize("c", DISTINCT, ids=IDS)
def test_planted_misreads_are_far_outside_the_gpu_bounds(c):
    small = dict(c, K=K_PLANTED)
    base = ref(small)
    scale = max(1.0, float(base["D"].abs().max()))
    attached = not c["detach"]
    short = []
    for name in cc.SETS[c["cset"]][1]:
        for which in cc.PLANTED:
            p = ref(small, planted=(name, which))
            fD = float((p["D"] - base["D"]).abs().max()) / scale / D_TOL
            fB, blk = worst_block(c, p["grad"], base)
            fB /= BLOCK_TOL
            print("%s %-5s %-6s: D moves by %8.0f x D_TOL, worst block (%s) by %8.0f x BLOCK_TOL" % (c["id"], name, which, fD, blk, fB))
            if not fD >= FACTOR or (attached and not fB >= FACTOR):
                short.append((name, which, fD, fB))
    assert not short, (c["id"], short)


TANH = [c for c in DISTINCT if c["family"] == "tanh"]


@pytest.mark.parametrize("c", TANH, ids=[c["id"] for c in TANH])
def test_fp32_stand_in_is_ten_times_inside_the_gpu_bounds(c):
    r64, r32 = ref(c), ref(c, dtype=torch.float32)
    eD = float((r32["D"].double() - r64["D"]).abs().max()) / max(1.0, float(r64["D"].abs().max()))
    eB, blk = worst_block(c, r32["grad"], r64)
    print("%s: fp32 stand-in D %.2e (<= %.1e)  worst block %.2e (%s, <= %.1e)" % (c["id"], eD, D_TOL / 10, eB, blk, BLOCK_TOL / 10))
    assert eD <= D_TOL / 10, eD
    assert eB <= BLOCK_TOL / 10, (eB, blk)
