"""Plain float64 references of the small forward entry points of libos2d_hip.so (include/os2d_hip.h) that the head tests reach
only through ``Os2dHead.forward``: class map preparation, the split class operand, the image norms, the TransformNet input
normalisation, the alignment epilogue and the box decode with its clamp.  TEST INFRASTRUCTURE ONLY.

Nothing is restated here that the oracle (oracle/head_oracle.py, oracle/decode_oracle.py) or tests/backward_model.py already
states: the models call their functions on float64 copies of the float32 inputs and bring the result into the layout of the C
ABI.  Every input is float32, drawn from fixed seeds on the host; tests/test_forward_model.py checks the models and the case
tables on the CPU, tests/test_forward_stages_gpu.py compares the kernels with them.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import backward_model as M
from oracle import decode_oracle as D
from oracle import head_oracle as O

T, K = M.T, M.K
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------- class maps
def class_prepare_model(raws, normalize):
    """os2d_class_prepare / os2d_class_prepare_batch: raw class maps [1,C,h_b,w_b] -> (q15 [B,C,15,15], qp [B,C,256]) in float64:
    the bilinear resize of the oracle, L2-normalised over the channels (eps 1e-5) unless ``normalize`` is off, and the same
    values as the x-major correlation operand."""
    maps = [r.to(F64) for r in raws]
    q15 = O.prepare_class_maps(maps) if normalize else O.resize_class_maps(maps)
    return q15, M.class_operand(q15)


# (h, w) of the class maps: a single cell, single rows and columns, the template size itself, strong down- and up-sampling
CLASS_SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (15, 15), (14, 16), (7, 31), (33, 40), (64, 3)]
CLASS_CHANNELS = (1, 31, 33, 67)        # around the 32-channel block of the batch kernel
CLASS_CHANNELS_SINGLE = CLASS_CHANNELS + (257,)      # the single-class kernel's 256-thread channel loop wraps at 257
ZERO_SIZE = (5, 6)
ZERO_AT = 4                             # the all-zero map sits in the middle of the ragged batch
BATCH_SIZES = CLASS_SIZES[:ZERO_AT] + [ZERO_SIZE] + CLASS_SIZES[ZERO_AT:]


@functools.lru_cache(maxsize=None)
def class_raws(C):
    """The ragged batch for C channels: all nine sizes and an all-zero map at ZERO_AT.  1 + 0.2 randn keeps every cell's vector
    away from zero (x / (|x| + 1e-5) is ill-conditioned there - tests/test_head_gpu.py::test_odd_shapes_match_oracle - and for
    C = 1 the vector is one number): tests/test_forward_model.py asserts the per-cell norms."""
    g = torch.Generator().manual_seed(5000 + C)
    raws = [1.0 + 0.2 * torch.randn(1, C, h, w, generator=g) for h, w in BATCH_SIZES]
    raws[ZERO_AT] = torch.zeros(1, C, *ZERO_SIZE)
    return raws


def resize_rounding_bound(raw):
    """What fp32 arithmetic can move a value of the RESIZED-ONLY map (normalize == 0) of raw [1,C,h,w] by, absolute; u = 2^-24.

    The kernels compute the sampling position as the reference does (F.affine_grid + F.grid_sample in fp32): xu = fma(step, j, -1)
    with step = fl(2/14) is within 2u of the exact coordinate, (xu + 1) adds a rounding of at most 2u, the halving is exact and
    the product with (w - 1) one more rounding: the position ix is within 3u (w - 1) of the float64 model's, 4u (w - 1) with a
    rounding to spare (the same along y).  The fraction ix - floor(ix) is exact.  A position error d moves a bilinear value by
    at most d times the largest difference of two neighbouring cells, Dx along x and Dy along y.  The interpolation itself -
    four products of three factors, the roundings of (1 - a), three additions - adds at most 8u of the largest |value|.
        bound = 4u ((w - 1) Dx + (h - 1) Dy) + 8u |raw|_max
    The normalised maps need none of this: their values are <= 1 and the project's bound of 1e-6 holds for them as it is."""
    h, w = raw.shape[2:]
    r = raw.to(F64)
    dx = float((r[..., 1:] - r[..., :-1]).abs().max()) if w > 1 else 0.0
    dy = float((r[:, :, 1:] - r[:, :, :-1]).abs().max()) if h > 1 else 0.0
    return 4 * M.U32 * ((w - 1) * dx + (h - 1) * dy) + 8 * M.U32 * float(r.abs().max())


@functools.lru_cache(maxsize=None)
def class_case(C, normalize):
    """(raws, q15, qp) of the ragged batch, the model computed once."""
    raws = class_raws(C)
    q15, qp = class_prepare_model(raws, normalize)
    return raws, q15, qp


# ---------------------------------------------------------------------------------------------------------- split class operand
SPLIT_EXP = 12                          # os2d_class_split scales by 2^12
SPLIT_CHANNELS = (1, 7, 8, 9, 33, 256)
SPLIT_B = 3
TINY = 2.0 ** -14 / 4096                # below it value * 2^12 is an fp16 subnormal


def split_groups(C):
    """8-channel groups of the split operand: ceil(C/8) padded to a multiple of 4."""
    return -(-(-(-C // 8)) // 4) * 4


def class_split_model(qp, C):
    """os2d_class_split on qp [B,C,256]: in the layout [B, G, 256, 8] of one half (the buffer is [B, G, hi|lo, 256, 8] halves,
    unit (g, m) = channels 8g .. 8g+7 of row m)
      hi    the expected hi halves as int16 bit patterns: np.float16(np.float32(v) * 4096), bit-exact
      v     the float64 value (hi + lo) * 2^-12 must reconstruct (0 at the pads)
      zero  bool mask of the lanes that must be exactly zero in BOTH halves: channels >= C (the rest of a half-filled group
            and the pad groups) and rows 225..255."""
    B = qp.shape[0]
    G = split_groups(C)
    full = np.zeros((B, G * 8, 256), dtype=np.float32)
    full[:, :C] = qp.detach().to(torch.float32).numpy()
    hi = (full * np.float32(2.0 ** SPLIT_EXP)).astype(np.float16)

    def units(a):
        return np.ascontiguousarray(a.reshape(B, G, 8, 256).transpose(0, 1, 3, 2))

    zero = np.zeros((B, G * 8, 256), dtype=bool)
    zero[:, C:] = True
    zero[:, :, K:] = True
    return (torch.from_numpy(units(hi).view(np.int16)), torch.from_numpy(units(full.astype(np.float64))),
            torch.from_numpy(units(zero)))


@functools.lru_cache(maxsize=None)
def split_input(C):
    """qp [3,C,256] float32: the model's operand of three class maps rounded to float32, with a few values below TINY (fp16
    subnormals after the scaling, of both signs) and a few exact zeros planted in the 225 rows."""
    g = torch.Generator().manual_seed(6000 + C)
    raws = [1.0 + 0.2 * torch.randn(1, C, h, w, generator=g) for h, w in ((15, 15), (7, 31), (2, 2))]
    qp = class_prepare_model(raws, 1)[1].to(torch.float32)
    tiny = [0.9 * TINY, -0.3 * TINY, TINY / 64, 2.0 ** -40, -(2.0 ** -26) * 1.37, 2.0 ** -27]
    for k, val in enumerate(tiny):
        qp[k % SPLIT_B, (5 * k) % C, (37 * k + 3) % K] = val
    for k in range(4):
        qp[k % SPLIT_B, (3 * k) % C, (53 * k + 11) % K] = 0.0
    return qp


# ---------------------------------------------------------------------------------------------------------- norms
SUMSQ_SHAPES = [(1, 1, 1, 1), (2, 7, 3, 5), (3, 130, 4, 4), (1, 257, 1, 17), (2, 1024, 2, 2)]     # (A, C, H, W)


def sumsq_model(fm):
    """os2d_fm_sumsq: fm [A,C,H,W] -> [A,H*W] = sum over the channels of fm^2."""
    return fm.to(F64).pow(2).sum(1).reshape(fm.size(0), -1)


CORR_NORM_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 17, 19)]       # (NB, H, W); 17x19 = 323 positions: two blocks of 256


def corr_normalize_model(corr):
    """os2d_corr_normalize / _f16x3: corr [NB,225,H,W] -> relu, then L2 over the 225 channels with eps 1e-6 (head.py:650)."""
    return O.l2_normalize_channels(F.relu(corr.to(F64)), 1e-6)


def corr_norm_dead(shape):
    """The location (nb, h, w) of a CORR_NORM_SHAPES case whose 225 values are all negative: 0 / (0 + 1e-6) = 0."""
    NB, H, W = shape
    return NB - 1, H // 2, W - 1


@functools.lru_cache(maxsize=None)
def corr_norm_input(shape):
    NB, H, W = shape
    corr = torch.randn(NB, K, H, W, generator=torch.Generator().manual_seed(7000 + H * W))
    nb, h, w = corr_norm_dead(shape)
    corr[nb, :, h, w] = -corr[nb, :, h, w].abs() - 0.01
    return corr


# ---------------------------------------------------------------------------------------------------------- alignment epilogue
CORNER_POINTS = ((0, 0), (0, T - 1), (T - 1, 0), (T - 1, T - 1))      # template (row, col) of corner k = 2*row_bit + col_bit


def decode_forward_model(corr, params, inverse, stride, rec_field):
    """os2d_sample_decode: corr [NB,225,H,W], params [NB,P,H,W] -> (loc [NB,4,H,W], cls [NB,1,H,W], corners [NB,8,H,W], aux) in
    float64: backward_model.decode_forward, plus the image-level positions of the four template corners, x then y."""
    NB, _, H, W = corr.shape
    with torch.no_grad():
        loc, cls, aux = M.decode_forward(corr.to(F64), params.to(F64), inverse, stride, rec_field)
    g = aux["g_img"].reshape(NB, H, W, T, T, 2)
    corners = torch.stack([g[:, :, :, i, j, a] for i, j in CORNER_POINTS for a in (0, 1)], dim=1)
    return loc, cls, corners, aux


def theta_rounding_bound(aux, NB, H, W, stride, rec_field):
    """[NB,2,H,W]: what fp32 rounding of theta can move a corner coordinate by (x: row 0 of theta, y: row 1), as
    backward_model.fragility derives delta_c: 16 * 2^-24 * (half_box * (|t0| + |t1| + |t2|) + stride * centre)."""
    theta = aux["theta"].detach().abs().reshape(NB, H, W, 2, 3)
    half_box = 0.5 * (stride * (T - 1) + rec_field)
    centre = torch.stack([(torch.arange(W, dtype=F64) + 0.5).view(1, W).expand(H, W),
                          (torch.arange(H, dtype=F64) + 0.5).view(H, 1).expand(H, W)], dim=0)        # [2,H,W]
    return 16 * M.U32 * (half_box * theta.sum(-1).permute(0, 3, 1, 2) + stride * centre.unsqueeze(0))


# ---------------------------------------------------------------------------------------------------------- box clamp
XFORM_CLIP = D.XFORM_CLIP
CLAMP_LEVEL = (3, 4)                    # (H, W) at stride 16
CLAMP_IMAGE = (64, 48)                  # (w, h)
_AT = np.float32(5.0 * XFORM_CLIP)
ULP_BELOW = float(np.nextafter(_AT, np.float32(0)))
ULP_ABOVE = float(np.nextafter(_AT, np.float32(np.inf)))
INF = float("inf")
# A loc[2] / loc[3] value and the side of the clamp it is MEANT to sit on ("ulp": the pair one fp32 ulp either side of
# 5 * log(1000/16), where clamped and unclamped results differ by a rounding).  -12.5 .. -8 are ordinary sizes here: the anchor
# is 240 px wide on a 64 x 48 image, exp(-12.5 / 5) * 240 = 19.7 px.
CLAMP_VALUES = {"below": (ULP_BELOW, "ulp"), "above": (ULP_ABOVE, "ulp"), "25": (25.0, "clamped"), "1e4": (1e4, "clamped"),
                "+inf": (INF, "clamped"), "-1e4": (-1e4, "unclamped"), "-inf": (-INF, "unclamped"), "2": (2.0, "unclamped"),
                "0.5": (0.5, "unclamped"), "-8": (-8.0, "unclamped"), "-10": (-10.0, "unclamped"),
                "-12.5": (-12.5, "unclamped"), "-14": (-14.0, "unclamped")}
# (loc[0], loc[1], loc[2], loc[3], what the reference does with the box).  loc[0] = 400 moves the centre 9600 px to the right:
# a box CLAMPED to exp(log(1000/16)) * 240 = 15000 px then starts at 2100 px and clipping leaves zero area, while the same
# box without the clamp (exp(5) * 240 = 35619 px and more) would reach back over the image and survive.
CLAMP_TABLE = [
    # class 0
    (0.0, 0.0, "below", "below", "kept"),
    (0.0, 0.0, "above", "above", "kept"),
    (0.0, 0.0, "25", "-12.5", "kept"),
    (0.0, 0.0, "-12.5", "1e4", "kept"),
    (0.0, 0.0, "+inf", "+inf", "kept"),
    (0.0, 0.0, "-1e4", "-12.5", "empty"),           # exp(-2000) = 0: zero width
    (0.0, 0.0, "-12.5", "-inf", "empty"),           # zero height
    (400.0, 0.0, "25", "-12.5", "empty"),           # clamped, wholly to the right
    (0.0, 400.0, "-12.5", "1e4", "empty"),          # clamped, wholly below
    (400.0, 0.0, "below", "-10", "empty"),
    (400.0, 0.0, "above", "-10", "empty"),
    (-50.0, 0.0, "-12.5", "-12.5", "empty"),        # an ordinary box 1200 px to the left
    # class 1
    (0.0, 0.0, "-12.5", "-12.5", "kept"),
    (0.3, -0.2, "-10", "-14", "kept"),
    (0.0, 0.0, "-14", "-10", "kept"),
    (-0.4, 0.1, "-12.5", "-8", "kept"),
    (0.0, 0.0, "-12.5", "-12.5", "kept"),
    (0.0, 0.0, "-10", "-10", "kept"),
    (0.0, 50.0, "-12.5", "-12.5", "empty"),         # an ordinary box 1200 px below
    (400.0, 400.0, "+inf", "+inf", "empty"),
    (0.0, 0.0, "-inf", "-inf", "empty"),
    (0.0, 0.0, "2", "0.5", "kept"),
    (0.2, 0.3, "-12.5", "-12.5", "kept"),
    (0.0, 0.0, "-12.5", "-12.5", "kept"),
]
CLAMP_B = 2
CLAMP_EMPTY = [k for k, row in enumerate(CLAMP_TABLE) if row[4] == "empty"]       # candidate = class * 12 + location
assert len(CLAMP_EMPTY) == 10


def clamp_inputs():
    """loc [2,4,12] and cls [2,12] (24 distinct scores) of the box-clamp table."""
    H, W = CLAMP_LEVEL
    loc = torch.zeros(CLAMP_B, 4, H * W)
    for k, (l0, l1, wk, hk, _) in enumerate(CLAMP_TABLE):
        loc[k // (H * W), :, k % (H * W)] = torch.tensor([l0, l1, CLAMP_VALUES[wk][0], CLAMP_VALUES[hk][0]])
    n = CLAMP_B * H * W
    cls = ((torch.arange(n) * 7) % n).float().view(CLAMP_B, H * W) / n - 0.5
    return loc, cls


def decode_boxes_model(loc, H, W, img_w, img_h, stride=16, rec_field=16):
    """os2d_decode_boxes: decode_oracle.decode_level evaluated in float64 on the float32 inputs."""
    return D.decode_level(loc.to(F64), H, W, img_w, img_h, stride, rec_field)


def clamp_distance(value):
    """loc / 5 - log(1000/16) in float64."""
    return value / O.LOC_WEIGHTS[2] - math.log(1000.0 / 16)
