"""CPU: the float64 model of the backward pass's split-fp16 arithmetic (tests/backward_f16x3_model.py) - the scale rule and the
three-product split - against plain float64.  The bound: every output element within 4 * 2^-24 * (|A| . |B|) of float64, the
element-wise fp32-rounding scale of the product (the model reaches a ratio of 1.8 at worst, at K = 25)."""
import numpy as np
import pytest

import backward_f16x3_model as X

U32 = 2.0 ** -24
KS = (25, 1600, 6272)              # a 5x5 tap block, layer 2's and layer 1's reduction


def operands(K, seed, M=24, N=40, spread=False):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    if spread:                   # magnitudes over 2^-24 .. 1 inside one operand
        a *= np.exp2(-rng.integers(0, 25, size=a.shape)).astype(np.float32)
    return a, b


def ratio(got, a, b):
    ref = a.astype(np.float64) @ b.astype(np.float64)
    bound = U32 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64))
    return float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("K", KS)
def test_every_element_within_fp32_rounding_of_float64(K):
    a, b = operands(K, K)
    r = ratio(X.matmul(a, b), a, b)
    print("K", K, "ratio", r)
    assert r < 4


@pytest.mark.parametrize("K", KS)
def test_magnitudes_spread_over_24_binades_inside_one_operand(K):
    """An element 2^-24 of the operand's largest is converted with the operand's scale: it keeps fewer bits of its own, but its
    error is that much smaller against the result.  Relative max error below 4 roundings of fp32 (torch's own fp32 GEMM on such
    inputs: 1.9e-7 .. 4.2e-7)."""
    a, b = operands(K, K + 1, spread=True)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    err = float(np.abs(X.matmul(a, b) - ref).max() / np.abs(ref).max())
    print("K", K, "relative max error", err)
    assert err < 4 * U32


@pytest.mark.parametrize("K", KS)
def test_small_batch_slice_needs_and_gets_its_own_scale(K):
    a, b0 = operands(K, 7 * K)
    b = np.stack([b0, b0[::-1] * np.float32(2.0 ** -20), b0 * np.float32(0.5)])
    got = X.batched_matmul(a, b, per_slice_b=True)
    for z in range(3):
        assert ratio(got[z], a, b[z]) < 4, z
    # one scale for the whole batch loses the small slice: the reason for the per-slice rule
    coarse = X.batched_matmul(a, b, per_slice_b=False)
    assert ratio(coarse[1], a, b[1]) > 4 > ratio(coarse[0], a, b[0])


def test_scale_rule():
    assert X.scale_exponent(1.0) == 14 and X.scale_exponent(1.9999) == 14 and X.scale_exponent(2.0) == 13
    assert X.scale_exponent(2.0 ** -20) == 34 and X.scale_exponent(3.0e38) == 14 - 127
    assert X.scale_exponent(0.0) == 0 and X.scale_exponent(-0.0) == 0
    assert X.scale_exponent(np.inf) == 0 and X.scale_exponent(np.nan) == 0
    assert X.scale_exponent(1e-45) == 126 and X.scale_exponent(2.0 ** -126) == 126 and X.scale_exponent(2.0 ** -112) == 126
    assert X.scale_exponent(2.0 ** -111) == 125
    assert X.exponents(np.array([[1.0, -3.0], [0.0, 0.25]], dtype=np.float32), True) == [13, 16]
    assert np.isnan(X.absmax(np.array([1.0, np.nan, 5.0], dtype=np.float32)))          # a NaN is above every number


@pytest.mark.parametrize("scale", [2.0 ** -100, 2.0 ** -20, 1.0, 2.0 ** 20, 2.0 ** 110])
def test_no_scaled_operand_leaves_the_fp16_range(scale):
    a0, _ = operands(1600, 3, spread=True)
    a = a0 * np.float32(scale)
    hi, lo, xs = X.split(a, X.exponents(a, False))
    assert 2.0 ** 14 <= float(np.abs(xs).max()) < 2.0 ** 15
    assert float(np.abs(hi).max()) <= 2.0 ** 15 < X.FP16_MAX and np.isfinite(lo).all()
    for s, e in zip(a[:3], X.exponents(a[:3], True)):
        assert 2.0 ** 14 <= float(np.abs(X.split(s, e)[2]).max()) < 2.0 ** 15
    tiny = a0 * np.float32(2.0 ** -126)            # below 2^-112 the scale stops at 2^126: lower in the range, never out of it
    assert 0 < float(np.abs(X.split(tiny, X.exponents(tiny, False))[2]).max()) < 2.0 ** 15


def test_zero_operand_gives_exact_zeros():
    a, b = operands(25, 1)
    assert not X.matmul(np.zeros_like(a), b).any() and not X.matmul(a, np.zeros_like(b)).any()
    got = X.batched_matmul(a, np.stack([b, np.zeros_like(b)]))
    assert not got[1].any() and ratio(got[0], a, b) < 4


def test_non_finite_value_reaches_what_depends_on_it():
    a, b = operands(25, 2)
    a[3, 7] = np.nan
    got = X.matmul(a, b)
    assert not np.isfinite(got[3]).any()
    bad = np.stack([b, b])
    bad[1, 0, 5] = np.inf
    got = X.batched_matmul(operands(25, 2)[0], bad)
    assert np.isfinite(got[0]).all() and not np.isfinite(got[1][:, 5]).any()
