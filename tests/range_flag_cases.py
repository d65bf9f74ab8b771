"""Case builders for the RANGE FLAG of the split-fp16 stage kernels (Os2dRangeFlag, os2d_amd/csrc/os2d_common.h): inputs for
os2d_transform_conv_f16x3 (layers 1 and 2) and for the four inverse-transform entry points that put chosen cells just below, on,
or just above the fp16 range - or make a pre-activation non-finite - together with what each case must do to the status word.
Test infrastructure, CPU only: tests/test_range_flag_model.py holds every case to its own statement with a float64 model of the
stage, tests/test_range_flag_stages_gpu.py runs the kernels on them.

The kernels test the STORED value  relu(acc * 2^-weight_exp + bias) * 2^out_exp  against 65504 (and the pre-activation against
NaN), for the cells they store.  A case is
  raises   the status word must become OS2D_STATUS_F16_RANGE (True) or stay what it was (False)
  fixed    for a raising case: the same inputs with the offending value made finite (the case's twin) - every cell of ``clean``
           must have the same bits in both calls
  clean    boolean mask over the outputs [NB, Cout, H, W]: the cells the offending value cannot reach

Convolutions.  BatchNorm is the identity in any arithmetic (gamma 1, beta 0, mean 0, var 1 with eps = 0, which the packing entry
point takes as an argument), weight_exp = in_exp = 0, out_exp[o] = o % 3:
  at_max / next_above   zero weights, bias[o] = 65504 * 2^-out_exp[o]: every stored value is EXACTLY 65504 (no raise); one channel
                        at the next float32 above (raise).  A bias is per channel: the offending "cell" is a whole channel.
  cell_hi / cell_lo     centre-tap-only filter w[o][o] = 2^(1 - out_exp[o]): stored(o, cell) = 2 * x(o, cell) exactly; the chosen
                        cell of pair 1 holds x = 32752 (1 + MARGIN) (hi: raise) or 32752 (1 - MARGIN) (lo: the twin), every other
                        cell a multiple of 2^-4 of at most 32752 (1 - MARGIN).  All of these are exact as fp16 hi + lo.
  nan_pre               a NaN input under bias -1: the pre-activation is NaN and fmaxf(NaN, 0) = 0 stores a clean 0 (raise)
  pos_inf / neg_inf     bias[o] = +Inf (raise) / -Inf (the ReLU gives 0, as the reference's: no raise).  (An infinite INPUT would
                        make the other taps' products 0 * Inf = NaN: the bias is the one way to an infinite pre-activation.)
  pad_cell              an input PAD cell of pair 1 holds 32752 (1 + MARGIN): the kernel computes 65504 (1 + MARGIN) for the
                        output pad cell, does not store it (valid == false) and must not raise.
  Pad ROWS at or above CoutStore cannot be reached through os2d_transform_conv_f16x3: both layers store as many rows as they
  compute (128 = 128, 64 = 64).

Inverse transforms.  Every (pair, tile, channel) spectrum is that of a scaled delta image (built in float64 with torch.fft.rfft2
and rounded to complex64, as tests/test_dft_gpu.py builds spectra): amplitude LOW 2^-out_exp[o] at the first cell the tile stores,
except ONE spectrum of pair 1: over / under (amplitude (1 +- MARGIN) at the chosen map cell), nan_pre (one NaN bin, bias -1),
pos_inf / neg_inf (bias), overhang (the over-range amplitude in a window cell the kernel does not store: the halo of a tiled
transform, the rows below an untiled map - ``inside == false``).  The BatchNorm fold plays no part here (the entry points take
the folded bias), so there is no exact-threshold case: the transform's rounding error stands between the spectrum and the cell.
"""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import train_forward_f16x3_model as SHB

F64 = torch.float64
FP16_MAX = 65504.0
STATUS_F16_RANGE = 1                 # OS2D_STATUS_F16_RANGE


@functools.lru_cache(maxsize=None)
def margin():
    """The relative distance of the single-cell cases from 65504, from the pins of tests/test_forward_matrix_gpu.py: the power of
    two at or below 200 times the largest relative error pinned for the split-fp16 layers with all three product terms (the
    two-term form rounds the WEIGHTS to fp16; the weights of these cases are powers of two)."""
    import test_forward_matrix_gpu as G
    worst = max(G.PIN["conv1_f16x3"], G.PIN["conv2_f16x3"])
    return 2.0 ** math.floor(math.log2(200.0 * worst))


def next_above(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


# =================================================================================================== convolutions
LAYERS = {1: (225, 128, 7), 2: (128, 64, 5)}          # cin, cout, kernel
CONV_NB = 2
CONV_GROUPS = [(1, 3, (9, 14)), (1, 3, (17, 13)), (1, 2, (9, 14)), (1, 2, (17, 13)), (2, 3, (9, 14)), (2, 3, (17, 13)), (2, 3, (1, 317)), (2, 3, (2, 317))]

ConvCase = collections.namedtuple("ConvCase", "name layer terms shape x w b bn eps exps nan_at pad_at raises fixed clean")


def conv_positions(layer, H, W):
    """{label: (h, w)} - first and last data cell, the last column of a row, and the cells either side of where the work tiles cut.
    Linear maps: tiles of NT plane cells counted from the first data cell.  NB = 2 runs the 128-cell shape, so the ``tile128``
    cells are seams of the kernel that runs; the ``tile256`` cells are where the 256-cell shape would cut (it needs 384
    work-groups and is NOT run by these cases: there they are ordinary cells).  Column strips of the 5x5 kernel beyond 316
    columns, which always run the 256-cell shape over the strip plane of pitch SP: the strip seam, the wave boundary at
    strip-plane index 128 (``wave``), and - where a strip has more than 256 cells (2 x 317) - the tile seam at index 256."""
    Ws = W + 3
    pos = collections.OrderedDict()
    pos["first"] = (0, 0)
    pos["last"] = (H - 1, W - 1)
    pos["row_end"] = (min(1, H - 1), W - 1) if H > 1 else (0, W - 2)
    if W > 316:
        assert layer == 2
        NS = (Ws + 255) // 256
        SW = (Ws + NS - 1) // NS
        SP = SW + 4
        pos["strip_seam_l"], pos["strip_seam_r"] = (0, SW - 1), (0, SW)
        for s in range(NS):                       # strip-plane index n' = h * SP + j is map cell (h, s * SW - 2 + j)
            for label, n in (("wave", 128), ("tile_seam", 256)):
                h, j = divmod(n, SP)
                c = s * SW - 2 + j
                if h < H and 2 < j < SP - 2 and 0 < c < W:
                    pos["strip{}_{}_l".format(s, label)], pos["strip{}_{}_r".format(s, label)] = (h, c - 1), (h, c)
        return pos

    def data_before(r):
        while r % Ws >= W:
            r -= 1
        return divmod(r, Ws)

    def data_after(r):
        while r % Ws >= W:
            r += 1
        return divmod(r, Ws)
    for NT in (128, 256):
        for k in range(1, (H * Ws + NT - 1) // NT):
            pos["tile{}_seam{}_l".format(NT, k)] = data_before(NT * k - 1)
            pos["tile{}_seam{}_r".format(NT, k)] = data_after(NT * k)
    return pos


def _identity_bn(cout):
    return tuple(np.full(cout, v, dtype=np.float32) for v in (1.0, 0.0, 0.0, 1.0))       # gamma, beta, mean, var


def _conv_exps(layer):
    cin, cout, _ = LAYERS[layer]
    return (np.zeros(cout, dtype=np.int32), np.zeros(cin, dtype=np.int32), (np.arange(cout) % 3).astype(np.int32))


def _background(layer, H, W, seed):
    """[NB, Cin, H, W] float32: multiples of 2^-4 in [0, 32752 (1 - MARGIN)] - exact as fp16 hi + lo, and so are their doubles."""
    cin = LAYERS[layer][0]
    g = np.random.RandomState(seed)
    top = math.floor(32752.0 * (1.0 - margin()) * 16.0)
    return (g.randint(0, top + 1, size=(CONV_NB, cin, H, W)).astype(np.float64) / 16.0).astype(np.float32)


def _mk(name, layer, terms, shape, x, w, b, nan_at=None, pad_at=None, raises=False, fixed=None, clean=None):
    cout = LAYERS[layer][1]
    return ConvCase(name, layer, terms, shape, x, w, b, _identity_bn(cout), 0.0, _conv_exps(layer), nan_at, pad_at, raises, fixed, clean)


@functools.lru_cache(maxsize=None)
def conv_cases(layer, terms, shape):
    """The list of ConvCase of one (layer, terms, shape) group."""
    H, W = shape
    cin, cout, ks = LAYERS[layer]
    m = margin()
    oexp = _conv_exps(layer)[2]
    hi_x, lo_x = np.float32(32752.0 * (1.0 + m)), np.float32(32752.0 * (1.0 - m))
    cases = []
    allc = np.ones((CONV_NB, cout, H, W), dtype=bool)

    # ---- exact threshold: zero weights, the bias alone
    w0 = np.zeros((cout, cin, ks, ks), dtype=np.float32)
    x0 = _background(layer, H, W, 100 * layer + H)
    b_max = np.ldexp(np.float32(FP16_MAX), -oexp).astype(np.float32)
    at_max = _mk("at_max", layer, terms, shape, x0, w0, b_max)
    cases.append(at_max)
    for o in (0, cout - 1):
        b = b_max.copy()
        b[o] = np.ldexp(np.float32(next_above(FP16_MAX)), -int(oexp[o]))
        clean = allc.copy()
        clean[:, o] = False
        cases.append(_mk("next_above_o{}".format(o), layer, terms, shape, x0, w0, b, raises=True, fixed=at_max, clean=clean))

    # ---- single cells: centre tap only, out channel o copies input channel o times 2^(1 - out_exp[o])
    wc = np.zeros((cout, cin, ks, ks), dtype=np.float32)
    for o in range(cout):
        wc[o, o, ks // 2, ks // 2] = np.ldexp(np.float32(1.0), 1 - int(oexp[o]))
    bz = np.zeros(cout, dtype=np.float32)
    xb = _background(layer, H, W, 200 * layer + W)
    for i, (label, (h, wcol)) in enumerate(conv_positions(layer, H, W).items()):
        o = (0, cout - 1, 3, 4, 8, cout // 2 - 1, cout // 2)[i % 7]           # either side of the 4- / 8- / 32-row runs of a lane
        xl, xh = xb.copy(), xb.copy()
        xl[1, o, h, wcol], xh[1, o, h, wcol] = lo_x, hi_x
        twin = _mk("cell_lo_{}".format(label), layer, terms, shape, xl, wc, bz)
        clean = allc.copy()
        clean[1, o, h, wcol] = False
        cases += [twin, _mk("cell_hi_{}".format(label), layer, terms, shape, xh, wc, bz, raises=True, fixed=twin, clean=clean)]

    # ---- non-finite pre-activations
    h, wcol = H // 2, W // 2
    bneg = np.full(cout, -1.0, dtype=np.float32)
    finite = _mk("nan_pre_fixed", layer, terms, shape, xb, wc, bneg)
    R = ks // 2
    clean = allc.copy()
    clean[1, :, max(h - R, 0):h + R + 1, max(wcol - R, 0):wcol + R + 1] = False       # 0 * NaN = NaN: every tap, every output channel
    cases.append(_mk("nan_pre", layer, terms, shape, xb, wc, bneg, nan_at=(1, 5, h, wcol), raises=True, fixed=finite, clean=clean))
    plain = _mk("inf_fixed", layer, terms, shape, xb, wc, bz)
    for o in (2, cout - 1):
        clean = allc.copy()
        clean[:, o] = False
        bp_, bn_ = bz.copy(), bz.copy()
        bp_[o], bn_[o] = np.inf, -np.inf
        cases.append(_mk("pos_inf_o{}".format(o), layer, terms, shape, xb, wc, bp_, raises=True, fixed=plain, clean=clean))
        cases.append(_mk("neg_inf_o{}".format(o), layer, terms, shape, xb, wc, bn_))

    # ---- a cell the kernel computes and does not store: the pad cell behind row 0 (linear tiles and strips alike)
    cases.append(_mk("pad_cell", layer, terms, shape, xb, wc, bz, pad_at=(1, cout - 1, 0, W, float(hi_x))))
    return cases


def conv_shb_input(case):
    """The split-half blocked input of the case as bytes (uint8 tensor): SHB.pack of x at in_exp, then the NaN / pad-cell edit."""
    H, W = case.shape
    halves = SHB.pack(case.x, case.exps[1])
    if case.nan_at is not None:
        nb, c, h, w = case.nan_at
        halves[nb, c // 8, 0, SHB.base(W) + h * SHB.ws(W) + w, c % 8] = np.float16(np.nan)
    if case.pad_at is not None:
        nb, c, h, w, v = case.pad_at
        assert w >= W
        hi, lo = SHB.split(np.float32(v))
        halves[nb, c // 8, 0, SHB.base(W) + h * SHB.ws(W) + w, c % 8] = hi
        halves[nb, c // 8, 1, SHB.base(W) + h * SHB.ws(W) + w, c % 8] = lo
    return torch.from_numpy(halves.view(np.uint8).reshape(-1).copy())


def conv_stored_model(case, with_pads=False):
    """float64: what the layer stores, [NB, Cout, H, W] = relu(BatchNorm(conv(x))) * 2^out_exp (and the pre-activation), from the
    values the SHB input holds (hi + lo, exactly).  with_pads: over the H x (W + 3) cells of the data rows, the pad columns of the
    input taken from the buffer (what the kernel COMPUTES there before it writes zeros)."""
    H, W = case.shape
    cin, cout, ks = LAYERS[case.layer]
    halves = conv_shb_input(case).numpy().view(np.float16).reshape(CONV_NB, SHB.groups(cin), 2, SHB.plane(H, W), 8).astype(np.float64)
    vals = (halves[:, :, 0] + halves[:, :, 1]).transpose(0, 1, 3, 2).reshape(CONV_NB, -1, SHB.plane(H, W))[:, :cin]
    vals = vals * np.exp2(-case.exps[1].astype(np.float64)).reshape(1, -1, 1)
    Ws, base = SHB.ws(W), SHB.base(W)
    # the data rows with their pad columns as an image of Ws columns.  (The kernel's taps run over the FLAT plane index, so a tap
    # left of column 0 reads the pad cells of the row above: with centre-tap-only or zero filters and the non-finite value at
    # least R columns inside the map, those products are 0 * finite = 0 either way.)
    x = torch.from_numpy(vals[:, :, base:base + H * Ws].reshape(CONV_NB, cin, H, Ws).copy())
    if case.nan_at is not None:
        assert ks // 2 <= case.nan_at[3] < W - ks // 2
    gamma, beta, mean, var = [torch.from_numpy(t.astype(np.float64)) for t in case.bn]
    acc = F.conv2d(x, torch.from_numpy(case.w.astype(np.float64)), None, padding=ks // 2)
    acc = acc * torch.exp2(-torch.from_numpy(case.exps[0].astype(np.float64))).view(1, -1, 1, 1)      # weight_exp = 0: the packed weights ARE w
    y = acc + torch.from_numpy(case.b.astype(np.float64)).view(1, -1, 1, 1)
    pre = (y - mean.view(1, -1, 1, 1)) * (gamma / torch.sqrt(var + case.eps)).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    stored = torch.relu(pre) * torch.exp2(torch.from_numpy(case.exps[2].astype(np.float64))).view(1, -1, 1, 1)
    if with_pads:
        return pre, stored
    return pre[..., :W], stored[..., :W]


def conv_fold_f32(case):
    """The fold of os2d_pack_conv_f16x3 in float32, operation for operation (prep.hip): (folded bias, 2^-weight_exp, 2^out_exp),
    and the value the kernel stores for a ZERO accumulator: fmaxf(0 * 2^-wexp + bias, 0) * 2^out_exp."""
    gamma, beta, mean, var = case.bn
    with np.errstate(invalid="ignore", over="ignore"):
        s = (gamma / np.sqrt((var + np.float32(case.eps)).astype(np.float32)).astype(np.float32)).astype(np.float32)
        bias = (((case.b - mean).astype(np.float32) * s).astype(np.float32) + beta).astype(np.float32)
        unscale = np.ldexp(np.float32(1.0), -case.exps[0]).astype(np.float32)
        oscale = np.ldexp(np.float32(1.0), case.exps[2]).astype(np.float32)
        pre = (np.float32(0.0) * unscale + bias).astype(np.float32)
        stored = (np.where(pre > 0, pre, np.float32(0.0)).astype(np.float32) * oscale).astype(np.float32)
    return bias, unscale, oscale, stored


# =================================================================================================== inverse transforms
ENTRIES = ("fft_rows", "fft_quads", "dft", "dft_planes")
TRANSFORM_SHAPES = [(9, 14), (5, 212)]
T_NB, T_COUT = 2, 128

Plan = collections.namedtuple("Plan", "P Q nbins TY TX TH TW u_fastest")
TCase = collections.namedtuple("TCase", "name entry shape plan special nan_bin bias raises fixed clean")
# special: (pair, tile, channel, window row, window column, amplitude before the channel scale) of the ONE changed spectrum


def t_out_exp():
    return (np.arange(T_COUT) % 3).astype(np.int32)


def plan_windows(plan, H, W):
    """Per tile (row-major): (y0, x0, oy, ox, th, tw) - the tile stores map cells [y0, y0 + th) x [x0, x0 + tw), found at window
    cell (oy + i, ox + j) of its inverse transform."""
    oy, ox = (3 if plan.TY > 1 else 0), (3 if plan.TX > 1 else 0)
    return [(ty * plan.TH, tx * plan.TW, oy, ox, min(plan.TH, H - ty * plan.TH), min(plan.TW, W - tx * plan.TW))
            for ty in range(plan.TY) for tx in range(plan.TX)]


def transform_positions(plan, H, W):
    """{label: (h, w)} map cells: first, last, the last column of a row, both sides of every transform-tile seam, the first cell
    of the (partial) last tile."""
    pos = collections.OrderedDict([("first", (0, 0)), ("last", (H - 1, W - 1)), ("row_end", (min(1, H - 1), W - 1))])
    for tx in range(1, plan.TX):
        pos["tile_x{}_l".format(tx)], pos["tile_x{}_r".format(tx)] = (H // 2, tx * plan.TW - 1), (H // 2, tx * plan.TW)
    for ty in range(1, plan.TY):
        pos["tile_y{}_l".format(ty)], pos["tile_y{}_r".format(ty)] = (ty * plan.TH - 1, W // 2), (ty * plan.TH, W // 2)
    if plan.TX * plan.TY > 1:
        pos["last_tile_first"] = ((plan.TY - 1) * plan.TH, (plan.TX - 1) * plan.TW)
    return pos


def locate(plan, H, W, h, w):
    """(tile, window row, window column) of map cell (h, w)."""
    for t, (y0, x0, oy, ox, th, tw) in enumerate(plan_windows(plan, H, W)):
        if y0 <= h < y0 + th and x0 <= w < x0 + tw:
            return t, h - y0 + oy, w - x0 + ox
    raise AssertionError((h, w))


def transform_cases(entry, shape, plan):
    H, W = shape
    m = margin()
    T = plan.TY * plan.TX
    allc = np.ones((T_NB, T_COUT, H, W), dtype=bool)
    zero = np.zeros(T_COUT, dtype=np.float32)
    cases = []

    def mk(name, special, nan_bin=None, bias=zero, raises=False, fixed=None, clean=None):
        return TCase(name, entry, shape, plan, special, nan_bin, bias, raises, fixed, clean)

    def not_image(o):
        c = allc.copy()
        c[1, o] = False
        return c
    base = mk("all_low", None)
    cases.append(base)
    for i, (label, (h, w)) in enumerate(transform_positions(plan, H, W).items()):
        o = (0, T_COUT - 1, 3, 4, 8, 63, 64)[i % 7]            # either side of the 4- / 8-image iterations of the kernels
        t, hw_, ww_ = locate(plan, H, W, h, w)
        twin = mk("under_{}".format(label), (1, t, o, hw_, ww_, FP16_MAX * (1.0 - m)))
        cases += [twin, mk("over_{}".format(label), (1, t, o, hw_, ww_, FP16_MAX * (1.0 + m)), raises=True, fixed=twin, clean=not_image(o))]
    # non-finite pre-activations
    o = 21
    bneg = zero.copy()
    bneg[o] = -1.0
    fin = mk("nan_pre_fixed", None, bias=bneg)
    cases.append(mk("nan_pre", None, nan_bin=(1, T - 1, o, 5), bias=bneg, raises=True, fixed=fin, clean=not_image(o)))
    for o in (2, T_COUT - 1):
        bp_, bn_ = zero.copy(), zero.copy()
        bp_[o], bn_[o] = np.inf, -np.inf
        clean = allc.copy()
        clean[:, o] = False
        cases += [mk("pos_inf_o{}".format(o), None, bias=bp_, raises=True, fixed=base, clean=clean), mk("neg_inf_o{}".format(o), None, bias=bn_)]
    # a window cell the kernel does not store: the halo corner of the last tile / the row below an untiled map
    if T > 1:
        cases.append(mk("overhang", (1, T - 1, 7, 0, 0, FP16_MAX * (1.0 + m))))
    else:
        assert plan.P > H
        cases.append(mk("overhang", (1, 0, 7, H, W - 1, FP16_MAX * (1.0 + m))))
    return cases


def _delta_spectrum(plan, hwin, wwin):
    """rfft2 of the unit delta at window cell (hwin, wwin) of the P x Q grid, float64 -> complex128 [P, Q/2 + 1]."""
    img = torch.zeros(plan.P, plan.Q, dtype=F64)
    img[hwin, wwin] = 1.0
    return torch.fft.rfft2(img)


def transform_spectra(case):
    """Y as complex64 [NB, T, Cout, P, V] (u, v order; the GPU test lays it out for the entry point)."""
    H, W = case.shape
    plan = case.plan
    T, V = plan.TY * plan.TX, plan.Q // 2 + 1
    low = FP16_MAX * (1.0 - margin())
    amp = torch.exp2(-torch.from_numpy(t_out_exp().astype(np.float64)))
    Y = torch.zeros(T_NB, T, T_COUT, plan.P, V, dtype=torch.complex128)
    for t, (y0, x0, oy, ox, th, tw) in enumerate(plan_windows(plan, H, W)):
        Y[:, t] = (low * amp).view(1, -1, 1, 1) * _delta_spectrum(plan, oy, ox).view(1, 1, plan.P, V)
    if case.special is not None:
        nb, t, o, hwin, wwin, a = case.special
        Y[nb, t, o] = a * float(amp[o]) * _delta_spectrum(plan, hwin, wwin)
    Y = Y.to(torch.complex64)
    if case.nan_bin is not None:
        nb, t, o, b = case.nan_bin
        Y[nb, t, o].view(-1)[b] = complex(float("nan"), 0.0)
    return Y


def transform_stored_model(case):
    """float64: (pre-activation, stored value) [NB, Cout, H, W] and the largest |stored| over the window cells the kernel does NOT
    store - the inverse transform of the complex64 spectra, + bias, ReLU, channel scale."""
    H, W = case.shape
    plan = case.plan
    Y = transform_spectra(case).to(torch.complex128)
    win = torch.fft.irfft2(Y, s=(plan.P, plan.Q))                   # [NB, T, Cout, P, Q]
    bias = torch.from_numpy(case.bias.astype(np.float64)).view(1, -1, 1, 1)
    scale = torch.exp2(torch.from_numpy(t_out_exp().astype(np.float64))).view(1, -1, 1, 1)
    pre = torch.zeros(T_NB, T_COUT, H, W, dtype=F64)
    outside = 0.0
    for t, (y0, x0, oy, ox, th, tw) in enumerate(plan_windows(plan, H, W)):
        pre[:, :, y0:y0 + th, x0:x0 + tw] = win[:, t, :, oy:oy + th, ox:ox + tw] + bias
        rest = (torch.relu(win[:, t] + bias) * scale).clone()
        rest[:, :, oy:oy + th, ox:ox + tw] = 0.0
        outside = max(outside, float(torch.nan_to_num(rest, nan=0.0, posinf=0.0).abs().max()))      # (a bias of +Inf is everywhere)
    return pre, torch.relu(pre) * scale, outside
