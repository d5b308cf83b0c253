"""psp_loss_stats_accumulate / psp_loss_stats_finish (csrc/lstat_kernels.h) alone, on the GPU, against numpy float64 on the same
fp32 inputs (ref64_loss_relerr.numpy_statistics: every formula of the table written out).

Bound for every output: |got - ref| <= 1e-10 s, s the mean absolute value of the terms that were summed in the centred form
(|v - mean v|^2 for a variance, |D - mean D|^4 for the fourth moment): a sequential double sum of n terms is wrong by at most
n 2^-53 sum|terms| = 1.1e-11 s at n = 1e5, a double exp adds a few ulp; 1e-10 leaves a factor of about 9.  A split run and a
single run may differ by rounding only (the same bound against the reference, twice it between them); two identical runs agree
bit for bit."""
import numpy as np
import pytest
import torch

import ref64_loss_relerr as r64
from util_cases import psp

nat = psp.native
pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 1000, 100003)


def splits(n):
    """n as one call, two calls and three calls, cut at unaligned points (1000 = 613 + 387)."""
    out = [(n,)]
    if n >= 2:
        a = max(1, (n * 613) // 1000)
        out.append((a, n - a))
    if n >= 3:
        a, b = max(1, (n * 307) // 1000), max(1, (n * 331) // 1000)
        out.append((a, b, n - a - b))
    return out


def inputs(kind, n):
    rng = np.random.default_rng(20240 + n)
    if kind == "normal":                                  # (i) Y, D ~ N(0, 1)
        Y, D = rng.standard_normal(n), rng.standard_normal(n)
    elif kind == "offset":                                # (ii) D = 1000 + N(0, 1): fp32 sums or sums without a pivot lose M4 here
        Y, D = rng.standard_normal(n), 1000.0 + rng.standard_normal(n)
    else:                                                 # (iii) |Y exp(-g + Y)| on either side of 100, about half each
        D = 4.0 + 0.1 * rng.standard_normal(n)            # v = Y exp(D) up to rounding: exp(4) = 54.6, so |Y| around 1.83 decides
        Y = np.where(rng.random(n) < 0.5, 1.0, 3.0) + 0.2 * rng.random(n)
        Y *= np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return Y.astype(np.float32), D.astype(np.float32)


def device_statistics(Y32, D32, parts):
    """The state after accumulate calls of the sizes `parts`, finished: ({key: (mean, variance, relative error)}, selected count,
    count, the 20 raw doubles)."""
    lib, dev = nat.load(), torch.device("cuda:0")
    Y, D = torch.from_numpy(Y32).to(dev), torch.from_numpy(D32).to(dev)
    state = torch.zeros(lib.psp_loss_stats_state_bytes() // 8, dtype=torch.float64, device=dev)
    out = torch.full((20,), -7.0, dtype=torch.float64, device=dev)
    k = 0
    for n in parts:
        nat.check(lib.psp_loss_stats_accumulate(nat.ptr(Y, k), nat.ptr(D, k), n, nat.ptr(state), nat.stream_ptr(dev)), "accumulate")
        k += n
    assert k == Y32.size
    nat.check(lib.psp_loss_stats_finish(nat.ptr(state), nat.ptr(out), nat.stream_ptr(dev)), "finish")
    raw = out.cpu().numpy()
    return {key: tuple(raw[3 * i:3 * i + 3]) for i, key in enumerate(r64.KEYS)}, int(raw[18]), int(raw[19]), raw


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["normal", "offset", "selection"])
def test_statistics_match_float64_numpy(kind, n):
    Y, D = inputs(kind, n)
    ref, count, scale = r64.numpy_statistics(Y, D)
    if kind == "selection":                               # the margin that makes `count` exact: nothing within 1e-6 of 100
        v = np.abs(Y.astype(np.float64) * np.exp(-(Y.astype(np.float64) - D.astype(np.float64)) + Y.astype(np.float64)))
        assert np.abs(v - 100.0).min() > 1e-6
        if n >= 63:
            assert 0.3 * n < count < 0.7 * n
    first = None
    for parts in splits(n):
        got, got_count, got_n, raw = device_statistics(Y, D, parts)
        assert got_n == n and got_count == count, (parts, got_n, got_count, count)
        worst = r64.assert_statistics(got, ref, scale, tag="%s n=%d %s" % (kind, n, parts), other=first)
        print("%s n=%d parts=%s worst error / s = %.2e (bound 1e-10)" % (kind, n, parts, worst))
        if first is None:
            first = got
            again = device_statistics(Y, D, parts)[3]
            assert raw.tobytes() == again.tobytes()        # equal calls, equal bits
    if n == 1:                                            # (iv) torch.var of one sample is NaN
        assert all(np.isnan(first[key][1]) for key in r64.KEYS if key != "cross_entropy_detach_selection" or count == 1)
    if n == 2 and kind == "normal":                       # ... and of two it is finite
        assert count == 2 and all(np.isfinite(first[key][1]) for key in r64.KEYS)
    if kind != "selection":                               # what reads D alone is finite in every set from two samples on
        assert n == 1 or (np.isfinite(first["log_variance"][1]) and np.isfinite(first["moment"][1]))


def test_split_runs_repeat_bit_for_bit():
    Y, D = inputs("offset", 1000)
    a = device_statistics(Y, D, (613, 387))[3]
    b = device_statistics(Y, D, (613, 387))[3]
    assert a.tobytes() == b.tobytes()


def test_non_finite_samples_are_not_filtered():
    """exp overflows for one trajectory: what it enters is NaN or inf, as the notebook's fp32 reductions would be; the selection
    leaves it out (|v| < 100 is false for it) and stays finite, and so does everything that reads D alone."""
    Y, D = inputs("normal", 1000)
    Y[17], D[17] = 800.0, 0.0                            # exp(-g + Y) = exp(0) but exp(-g) = exp(-800) = 0; then the other way round
    Y[18], D[18] = -800.0, 0.0                           # exp(-g) = exp(800) = inf
    got, count, n, _ = device_statistics(Y, D, (1000,))
    ref, ref_count, _ = r64.numpy_statistics(Y, D)
    assert n == 1000 and count == ref_count
    assert np.isinf(got["terminal"][0]) and np.isnan(got["terminal"][1])
    assert np.isinf(got["cross_entropy"][0]) and np.isnan(got["cross_entropy"][1])
    assert np.isfinite(got["cross_entropy_detach_selection"][1]) and np.isfinite(got["log_variance"][1])
    assert np.isfinite(got["moment"][1])
