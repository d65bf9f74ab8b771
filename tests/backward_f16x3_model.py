"""CPU model of the split-fp16 ("f16x3") arithmetic of the backward GEMMs (os2d_amd/csrc_train/train_gemm.hip), test
infrastructure only.

Scale rule.  An operand's scale is 2^e with e from the fp32 bit pattern of its largest magnitude: e = 141 - biased exponent puts
that magnitude into [2^14, 2^15), one binade below the end of the fp16 range (at most 126: the largest scale a float holds; a
subnormal maximum).  A zero maximum and a non-finite one (pattern >= 0x7f800000) give e = 0.  An operand the GEMM reduces over as
a whole has one e, a batched operand one per slice of the batch index.

Product.  x 2^e is rounded to fp16 hi and fp16 lo = rn16(x 2^e - hi); a product of two operands is hi*hi + hi*lo + lo*hi (the
MFMA multiplies fp16 values exactly and accumulates in fp32; float64 here), multiplied by 2^-(ea+eb)."""
import numpy as np

FP16_MAX = 65504.0


def scale_exponent(max_abs):
    """e of the scale rule from the largest magnitude (a float32 value, NaN / Inf allowed)."""
    bits = int(np.array(abs(np.float32(max_abs)), dtype=np.float32).view(np.uint32))
    if bits == 0 or bits >= 0x7F800000:
        return 0
    return min(141 - (bits >> 23), 126)


def absmax(x):
    """Largest |x| the way the maxima pass orders it: by bit pattern, so a NaN is above every number."""
    a = np.abs(np.asarray(x, dtype=np.float32)).reshape(-1)
    return a.view(np.uint32).max().view(np.float32) if a.size else np.float32(0)


def exponents(x, per_slice):
    """One exponent for the whole tensor, or one per slice of axis 0."""
    x = np.asarray(x, dtype=np.float32)
    return [scale_exponent(absmax(s)) for s in x] if per_slice else scale_exponent(absmax(x))


def split(x, e):
    """float32 array, exponent -> (hi, lo) float64 arrays holding fp16 values, and the scaled fp32 array."""
    with np.errstate(over="ignore", invalid="ignore"):
        xs = (np.asarray(x, dtype=np.float32) * np.float32(2.0 ** e)).astype(np.float32)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), xs


def matmul(a, b, ea=None, eb=None):
    """a [M,K] @ b [K,N] in the f16x3 arithmetic (float64 accumulation); ea / eb default to the whole-operand rule."""
    ea = exponents(a, False) if ea is None else ea
    eb = exponents(b, False) if eb is None else eb
    ah, al, _ = split(a, ea)
    bh, bl, _ = split(b, eb)
    with np.errstate(invalid="ignore"):
        return (al @ bh + ah @ bl + ah @ bh) * 2.0 ** -ea * 2.0 ** -eb


def batched_matmul(a, b, per_slice_b=True):
    """a [M,K] (one scale) against b [Z,K,N] (one scale per slice z, or one for all): [Z,M,N]."""
    ea = exponents(a, False)
    ebs = exponents(b, True) if per_slice_b else [exponents(b, False)] * len(b)
    return np.stack([matmul(a, bz, ea, ez) for bz, ez in zip(b, ebs)])
