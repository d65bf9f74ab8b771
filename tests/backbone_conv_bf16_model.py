"""Model of libos2d_backbone_conv_bf16.so (include/os2d_backbone_conv_bf16.h): the split of an fp32 value into three bf16 values bit for
bit in numpy, the packed weights as the library lays them out, and the derived bound of os2d_backbone_conv1x1_bf16x3 against the
float64 quantities of tests/backbone_conv_model.py (y64, S = sum |w x|, v64, d64), which are those of the fp32 entry point: the two
compute the same function of the same fp32 operands."""
import numpy as np
import torch

import backbone_conv_model as C
import backbone_model as B

PARTS = 3
U24 = 2.0 ** -24
TOP = 0x7F7F8000          # bit patterns from here on round to bf16's infinity (or are Inf / NaN)
INF = 0x7F800000


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def widen(b):
    """bf16 bit patterns (uint16) as the fp32 of the same value"""
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def rne(x):
    """round to nearest even of fp32 to bf16 on the bit pattern, as torch's conversion does (NaN and overflow are the caller's)"""
    u = bits(x).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def split(x):
    """fp32 array -> (b0, b1, b2) uint16 arrays of bf16 bit patterns, by the rules of bf16x3_split.h"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = bits(x)
    mag = u & 0x7FFFFFFF
    nonfinite, nan = mag >= INF, mag > INF
    with np.errstate(invalid="ignore", over="ignore"):
        b0 = np.where(mag >= TOP, (u >> 16).astype(np.uint16), rne(x))
        r1 = np.where(nonfinite, np.float32(0), x - widen(b0)).astype(np.float32)
        b1 = rne(r1)
        r2 = (r1 - widen(b1)).astype(np.float32)
        b2 = rne(r2)
    b0 = np.where(nan, np.uint16(0x7FC0), b0).astype(np.uint16)
    return b0, np.where(nonfinite, 0, b1).astype(np.uint16), np.where(nonfinite, 0, b2).astype(np.uint16)


def split_x(x):
    """The split of an activation (bf16x3_split_x): a non-finite value stands in the last part alone"""
    b0, b1, b2 = split(x)
    nonfinite = (bits(x) & 0x7FFFFFFF) >= INF
    return np.where(nonfinite, 0, b0).astype(np.uint16), b1, np.where(nonfinite, b0, b2).astype(np.uint16)


def padded_k(cin, tile_k):
    return (cin + tile_k - 1) // tile_k * tile_k


def pack(w, tile_k):
    """w [Cout, Cin] fp32 -> uint16 [3, Kp / 8, Cout, 8]: the layout of os2d_backbone_conv_bf16_pack_weights, zeros for k >= Cin"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, cin = w.shape
    kp = padded_k(cin, tile_k)
    padded = np.zeros((cout, kp), dtype=np.float32)
    padded[:, :cin] = w
    parts = np.stack(split(padded))                                        # [3, Cout, Kp]
    return np.ascontiguousarray(parts.reshape(PARTS, cout, kp // 8, 8).transpose(0, 2, 1, 3))


def nnz(x, w, stride=1):
    """[N, Cout, Ho, Wo]: the number of k whose product w[co][k] * x[n][k][pixel] is not zero"""
    xs = (x.double()[:, :, ::stride, ::stride] != 0).double()
    return torch.einsum("ok,nkhw->nohw", (w.double().reshape(w.shape[0], -1) != 0).double(), xs)


def bound(x, w, s, S, v64, d64=None, folds_of_r=0, stride=1):
    """The derived bound of os2d_backbone_conv1x1_bf16x3 against the float64 model, WITHOUT the slack and the floor (``within`` adds them):

        (2^-23 + 6 nnz 2^-24) S |s|  +  2^-23 |v64|  (+ 2^-23 |d64|  (+ 2^-23 |d64|))

    2^-23 S: the three products left out, at most (2^-23 + 2^-32) |w x| per k (|x1 w2| + |x2 w1| + |x2 w2| <= (2 * 2^-24 + 2^-32) |w x|), the
    2^-32 absorbed by the slack.  6 nnz 2^-24 S: the accumulator is a sum of 6 exact product terms per k with a non-zero product; summed in
    fp32 in ANY order, every partial sum is at most S in magnitude and is rounded once, and there are fewer than 6 nnz additions.  The
    rest is the epilogue's, as in backbone_conv_model.bound."""
    n = nnz(x, w, stride)
    b = (B.U23 + 6 * n * U24) * S * s.double().abs().view(1, -1, 1, 1) + B.U23 * v64.abs()
    if d64 is not None:
        b = b + (1 + folds_of_r) * B.U23 * d64.abs()
    return b


def floor(w, tile_k):
    """What parts that fall below bf16's normal range can lose: at most 2^-126 per part product of unit weight, six of them per k < Kp"""
    w = w.reshape(w.shape[0], -1)
    return padded_k(w.shape[1], tile_k) * 6 * 2.0 ** -126 * float(w.abs().max())


def within(y, y64, bound, floor=0.0):
    """NaN exactly where the model has it, elsewhere |y - y64| <= slack * bound + floor"""
    y = y.detach().cpu().double()
    nan = torch.isnan(y64)
    if not torch.equal(torch.isnan(y), nan):
        return False
    err = torch.where(nan, torch.zeros_like(y), (y - y64).abs())
    return bool((err <= B.SLACK * torch.where(nan, torch.zeros_like(bound), bound) + floor).all())


conv1x1 = C.conv1x1          # the float64 quantities are those of the fp32 entry point
