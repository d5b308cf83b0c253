"""The arithmetic of the one-accumulator split product (csrc/hjb_kernels.h: split_tab, gemm_Tx ONE), modelled in numpy next to the
two-chain form of tests/test_split_product.py: A = 2^6 a = Ah + Al, B = 2^5 b = Bh + Bl with UNSCALED f16 residuals, and
Ah Bh + Ah Bl + Al Bh = 2048 a b in one fp32 sum.  At the magnitudes of the narrow forward the product is as accurate as the
two-chain one; where the scaled lo parts fall below the f16 normal range it degrades to an absolute error, which is what the choice
of the two powers is about; beyond the scaled range hi and lo are +inf and -inf and the sum is NaN (the range guard's signal)."""
import numpy as np
import pytest

from test_split_product import product_errors

LG_A, LG_B = 6, 5


def split_scaled(a, lg):
    s = a * np.float32(2.0 ** lg)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def one_accumulator_error(scale_w, scale_x, k=100, seed=0):
    rng = np.random.default_rng(seed)                 # (the operands of product_errors: same seed, same draws)
    W = (rng.standard_normal((k, k)) * scale_w).astype(np.float32)
    X = (rng.standard_normal((k, 4096)) * scale_x).astype(np.float32)
    ref = W.astype(np.float64) @ X.astype(np.float64)
    (wh, wl), (xh, xl) = split_scaled(W, LG_A), split_scaled(X, LG_B)
    up = lambda a: a.astype(np.float32)   # noqa: E731
    acc = (up(wh) @ up(xh) + up(wh) @ up(xl) + up(wl) @ up(xh)) * np.float32(1.0 / 2048)
    return np.abs(acc - ref).mean() / np.abs(ref).mean()


@pytest.mark.parametrize("scale_w,scale_x", [(0.1, 1.0), (0.01, 0.1), (1.0, 3.0), (0.1, 0.3)])
def test_one_accumulator_product_is_fp32_grade(scale_w, scale_x):
    e32, e3, _ = product_errors(scale_w, scale_x)
    e1 = one_accumulator_error(scale_w, scale_x)
    assert e1 <= 1.3 * e32 and e1 <= 1.5 * e3, (e32, e3, e1)


def test_operand_keeps_22_bits_where_its_scaled_lo_part_is_normal():
    rng = np.random.default_rng(1)
    for mag, lg in ((0.1, LG_A), (0.01, LG_A), (0.1, LG_B), (3.0, LG_B), (1000.0, LG_B)):
        x = (rng.uniform(0.5, 1.0, 10000) * mag * rng.choice([-1.0, 1.0], 10000)).astype(np.float32)
        hi, lo = split_scaled(x, lg)
        back = (hi.astype(np.float64) + lo.astype(np.float64)) / 2.0 ** lg
        assert np.max(np.abs(back - x) / np.abs(x)) <= 2.0 ** -21


def test_beyond_the_scaled_range_hi_and_lo_cancel_to_nan():
    for x, lg in ((3000.0, LG_B), (2100.0, LG_B), (1100.0, LG_A)):      # finite f16 numbers unscaled: the SCALED hi part overflows
        hi, lo = split_scaled(np.array([x], dtype=np.float32), lg)
        assert np.isposinf(hi[0]) and np.isneginf(lo[0])
        with np.errstate(invalid="ignore"):
            assert np.isnan(np.float32(hi[0]) * np.float32(1.0) + np.float32(1.0) * np.float32(lo[0]))
    hi, lo = split_scaled(np.array([1023.0], dtype=np.float32), LG_B)      # half the input threshold: finite
    assert np.isfinite(hi[0]) and np.isfinite(lo[0])
