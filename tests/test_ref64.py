"""tests/ref64.py (the float64 reference of one Solver iteration) and the block-wise gradient comparison of tests/util_cases.py,
checked on the CPU:

  a. ref64 against the fp32 oracle on the same fp32 problem data, net and noise: every one of the seven gradient blocks to 1e-5 of
     that block's own maximum, D to 2e-5 max(1, |D|), at weight scales 1 and 30 (measured: at most 2e-6 per block on LLGC / LQGC,
     3e-6 on the double well -- the bound leaves x 3 .. x 5 for other CPU math libraries);
  b. the block-wise helper rejects three planted errors which the whole-gradient criterion of the GPU suites
     (max |g - g_ref| <= 2e-4 max |g_ref|) accepts at the default weights -- the gap tests/test_gpu_block_gradients.py closes;
  c. every case of tests/block_cases.py is in the nonlinear regime: median |h1| and median |h2| in [0.15, 0.85] at the middle step,
     max |D| finite and below 200, the smallest of the seven block maxima above 2e-2 of the largest.
"""
import math

import pytest
import torch

import block_cases as bc
import ref64
from oracle import philox_oracle
from util_cases import BLOCK_NAMES, assert_blocks, block_errors, grad_blocks, make_oracle, orc

BLOCK_TOL = 1e-5            # ref64 against the fp32 oracle, per block
D_TOL = 2e-5
FLAT_TOL = 2e-4             # the whole-gradient criterion of tests/test_gpu_parity.py and its siblings


def _case(kind, d, H, K, detach, loss="log-variance", N=4, dt=0.05):
    c = dict(kind=kind, d=d, H=H, N=N, dt=dt, detach=detach, loss=loss)
    return bc.golden_style(c, K)


# (kind, d, H, K, detached, loss)
ORACLE_SHAPES = [
    ("LLGC", 12, 16, 50, True, "log-variance"),
    ("LQGC", 20, 40, 72, False, "log-variance"),
    ("LLGC", 100, 64, 48, False, "log-variance"),
    ("LQGC", 33, 17, 33, False, "variance"),
    ("LLGC", 17, 33, 17, False, "relative_entropy"),
    ("DoubleWell_multidim", 30, 64, 50, False, "log-variance"),
    ("LLGC", 20, 40, 40, True, "moment"),
    ("LQGC", 12, 16, 33, False, "cross_entropy"),
]


def both(kind, d, H, K, detach, loss, scale, weights=None):
    """(ref64 result, fp32 oracle trace) on the same data; ref64 first: hjb_train ends with an Adam step on the net."""
    case = _case(kind, d, H, K, detach, loss)
    oprob, ocfg, omodels = make_oracle(case, L=1)
    with torch.no_grad():
        for p in omodels[0].parameters():
            p.mul_(scale)
    xi = bc.host_noise(42, K, d, omodels[2])
    r64 = ref64.iteration(oprob, ocfg, omodels[0], xi, weights=weights)
    keep = orc.hjb_loss
    if weights is not None:
        orc.hjb_loss = lambda kind_, D, Y, gX, **kw: (weights * D).sum()
    try:
        ref = orc.hjb_train(oprob, ocfg, step_models=omodels, noise=[xi], trace=True)
    finally:
        orc.hjb_loss = keep
    return r64, ref["traces"][0], ref["loss_log"][0]


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("kind,d,H,K,detach,loss", ORACLE_SHAPES)
def test_ref64_matches_the_fp32_oracle_per_block(kind, d, H, K, detach, loss, scale):
    r64, tr, loss32 = both(kind, d, H, K, detach, loss, scale)
    assert r64["N"] == 4 and r64["h1"].shape == (K, H) and r64["h2"].shape == (K, H)
    D32 = -tr["Zsum_g"] if loss == "relative_entropy" else tr["D"]
    assert bool(torch.isfinite(r64["D"]).all()) and bool(torch.isfinite(D32).all())
    eD = float((r64["D"] - D32.double()).abs().max()) / max(1.0, float(r64["D"].abs().max()))
    g32 = torch.cat([g.reshape(-1) for g in tr["grads"]])
    print("%s d=%d H=%d x%g: D %.2e (<= %.1e)  loss %.9g / %.9g" % (kind, d, H, scale, eD, D_TOL, r64["loss"], loss32))
    assert eD <= D_TOL, eD
    assert_blocks(g32, r64["grad"], d, H, BLOCK_TOL, tag="fp32 oracle vs ref64 %s d=%d x%g" % (kind, d, scale))
    assert [tuple(b.shape) for b in r64["blocks"]] == [tuple(g.shape) for g in tr["grads"]]
    # the loss: the fp32 value of mean(D^2) - mean(D)^2 follows the conditioning (tests/test_gpu_parity.check_first_iteration)
    assert math.isclose(loss32, r64["loss"], rel_tol=bc.first_loss_tol(bc.loss_values(loss, r64["D"]), r64["loss"])), (loss32, r64["loss"])


def test_ref64_weighted_loss_matches_the_oracle_with_the_same_weights():
    """loss = sum_k w_k D_k, as tests/test_gpu_range_guard._oracle_weighted_gradient forms it."""
    K = 40
    w = torch.randn(K, generator=torch.Generator().manual_seed(7)) * (2.0 / K)
    r64, tr, loss32 = both("LLGC", 20, 40, K, True, "log-variance", 30.0, weights=w)
    assert math.isclose(r64["loss"], float((w.double() * r64["D"]).sum()), rel_tol=1e-12)
    assert_blocks(torch.cat([g.reshape(-1) for g in tr["grads"]]), r64["grad"], 20, 40, BLOCK_TOL, tag="weighted")


def flat_accepts(g, g_ref):
    return float((g - g_ref).abs().max()) <= FLAT_TOL * float(g_ref.abs().max())


def test_block_comparison_rejects_what_the_flat_criterion_accepts():
    """Default weights, LLGC d = 12, H = 16, detached: the time column zeroed, W2's block off by 2 %, two rows of W1's x columns
    swapped.  Each is an O(1) .. 2e-2 error of its block and passes max |g - g_ref| <= 2e-4 max |g_ref|."""
    d, H, K = 12, 16, 50
    r64, tr, _ = both("LLGC", d, H, K, True, "log-variance", 1.0)
    g_ref = r64["grad"]
    assert max(block_errors(g_ref, g_ref, d, H)) == 0.0
    assert_blocks(g_ref.float(), g_ref, d, H, 2e-4, tag="fp32 rounding of the reference")          # ... and what is right passes
    nW1 = H * (d + 1)

    def planted(which):
        g = g_ref.clone()
        W1 = g[:nW1].view(H, d + 1)
        if which == "time column zeroed":
            W1[:, 0] = 0.0
        elif which == "W2 x 1.02":
            g[nW1 + H:nW1 + H + H * H] *= 1.02
        else:
            # the first pair of rows whose swap the flat criterion cannot see but which moves the block by more than 10 %
            gmax, bmax = float(g_ref.abs().max()), float(W1[:, 1:].abs().max())
            pairs = [(i, j) for i in range(H) for j in range(i + 1, H)
                     if 0.1 * bmax < float((W1[i, 1:] - W1[j, 1:]).abs().max()) <= 0.5 * FLAT_TOL * gmax]
            i, j = pairs[0]
            W1[[i, j], 1:] = W1[[j, i], 1:]
        return g

    for which, block in (("time column zeroed", "W1t"), ("W2 x 1.02", "W2"), ("W1 x rows swapped", "W1x")):
        g = planted(which)
        errs = dict(zip(BLOCK_NAMES, block_errors(g, g_ref, d, H)))
        flat = float((g - g_ref).abs().max()) / float(g_ref.abs().max())
        print("%s: flat %.2e (<= %.1e passes), block %s %.2e" % (which, flat, FLAT_TOL, block, errs[block]))
        assert flat_accepts(g, g_ref), (which, flat)
        assert errs[block] > 2e-4 and all(e == 0.0 for n, e in errs.items() if n != block), (which, errs)
        with pytest.raises(AssertionError):
            assert_blocks(g, g_ref, d, H, 2e-4, tag=which)


def test_block_floor_keeps_a_zero_block_in_the_comparison():
    """A block that is zero in the reference is held to 1e-4 of the whole gradient's maximum, not skipped and not divided by."""
    d, H = 3, 2
    n = (d + 1) * H + H + H * H + H + d * H + d
    g_ref = torch.zeros(n, dtype=torch.float64)
    g_ref[-1] = 1.0                                               # b3 only
    g = g_ref.clone()
    g[0] = 3e-8                                                   # time column: 3e-8 / (1e-4 * 1) = 3e-4
    errs = block_errors(g, g_ref, d, H)
    assert math.isclose(errs[0], 3e-4, rel_tol=1e-9) and all(e == 0.0 for e in errs[1:])
    assert [b.numel() for b in grad_blocks(g, d, H)] == [H, d * H, H, H * H, H, d * H, d]
    with pytest.raises(AssertionError):
        assert_blocks(g, g_ref, d, H, 2e-4)


def cpu_noise(c, K):
    """The stream the case's kernels draw from: the host generator, or the numpy restatement of the device Philox stream."""
    if c["noise"] == "philox":
        return torch.from_numpy(philox_oracle.normal_stream(c["N"], K, c["d"], 0, 42, 0)).float().permute(1, 2, 0).contiguous()
    return bc.host_noise(42, K, c["d"], c["N"])


@pytest.mark.parametrize("c", bc.CASES, ids=[c["id"] for c in bc.CASES])
def test_gpu_cases_are_in_the_nonlinear_regime(c):
    K = bc.case_K(c)
    r = bc.reference(c, K, lambda: cpu_noise(c, K))
    assert r["N"] == c["N"]
    m1, m2 = float(r["h1"].abs().median()), float(r["h2"].abs().median())
    Dmax = float(r["D"].abs().max())
    bm = [float(b.abs().max()) for b in grad_blocks(r["grad"], c["d"], c["H"])]
    print("%s: median |h1| %.2f |h2| %.2f  max |D| %.3g  smallest block %s at %.3g of the largest" %
          (c["id"], m1, m2, Dmax, BLOCK_NAMES[bm.index(min(bm))], min(bm) / max(bm)))
    assert 0.15 <= m1 <= 0.85 and 0.15 <= m2 <= 0.85, (m1, m2)
    assert math.isfinite(Dmax) and Dmax < 200.0, Dmax
    assert min(bm) > 2e-2 * max(bm), bm
