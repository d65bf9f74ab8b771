"""GPU: the entry points of libos2d_backbone_conv_bf16.so alone through their C ABI against the model (tests/backbone_conv_bf16_model.py).

pack_weights is compared with the numpy split exactly.  The GEMM's outputs are pre-filled with NaN and stand inside a NaN frame that must
survive; the model gets the same fp32 operands.  The bound is derived, not measured (backbone_conv_bf16_model.bound, slack 1.01):
    (2^-23 + 6 nnz 2^-24) S |s|    the three products left out and the fp32 accumulation of six product terms per non-zero k, in any order
  + 2^-23 |v64| (+ 2^-23 |d64| (+ 2^-23 |d64|))     the epilogue, as for the fp32 entry point
  + Kp * 6 * 2^-126 * max |w|      parts below bf16's normal range
It is loose for dense columns and sharp for sparse ones - with one non-zero k it is about 2^-21.4 S, and a kernel that drops or misplaces
one of the six products misses it by 2^-16 - so the sparse cases carry the weight.  Inputs are normal draws of unit scale."""
import numpy as np
import pytest
import torch

import backbone_conv_bf16_model as M
import backbone_conv_model as C
from os2d_amd import _backbone_conv_bf16_lib as L
from os2d_amd import _backbone_conv_lib as L32
from os2d_amd._native import STREAM
from test_backbone_conv_stages_gpu import FORMS, draw
from test_backbone_stages_gpu import fold_draw, frame_intact, framed, gen, shifted

pytestmark = pytest.mark.gpu

NAN = float("nan")
TM, TN, TK = L.TILE_M, L.TILE_N, L.TILE_K
COUTS = [1, L.SMALL_TILE_M - 1, L.SMALL_TILE_M, L.SMALL_TILE_M + 1, TM - 1, TM, TM + 1, 2 * TM + 1]
CINS = [1, 7, 8, 9, 15, 16, 17, TK - 1, TK, TK + 1, 2 * TK + 1]
HWS = [1, 3, 4, 5, TN - 1, TN, TN + 1, L.SMALL_TILE_N - 1, L.SMALL_TILE_N, L.SMALL_TILE_N + 1]
SENTINEL = 0x5A5A


def packed(w, device):
    """-> (whole, wp): the packed weights of w [Cout, Cin] (a CPU tensor) made on the device, inside a frame of sentinels"""
    cout, cin = w.shape
    n = L.packed_elems(cout, cin)
    whole = torch.full((8 + n + 8,), SENTINEL, dtype=torch.int16, device=device)
    wp = whole[8:8 + n]
    assert wp.data_ptr() % 16 == 0
    L.call("os2d_backbone_conv_bf16_pack_weights", w.contiguous().to(device), wp, cout, cin, STREAM)
    return whole, wp


def run(ops, stride, relu, device, shifts=(0, 0, 0), fp32=False):
    """One call on device copies of the operands (x, y, r start `shifts` floats behind a 16-byte boundary) -> (whole, y, xd, rd);
    fp32: the fp32 entry point of libos2d_backbone_conv.so instead."""
    x, w, s, t, r, sr, tr = ops
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    to = lambda v: v.to(device) if v is not None else None
    xd, rd = shifted(x, device, shifts[0]), (shifted(r, device, shifts[2]) if r is not None else None)
    whole, y = framed((N, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1), device, shifts[1])
    if fp32:
        L32.call("os2d_backbone_conv1x1", xd, to(w), to(s), to(t), rd, to(sr), to(tr), y, N, Cin, Cout, H, W, stride, int(relu), STREAM)
    else:
        L.call("os2d_backbone_conv1x1_bf16x3", xd, packed(w, device)[1], to(s), to(t), rd, to(sr), to(tr), y, N, Cin, Cout, H, W, stride, int(relu), STREAM)
    torch.cuda.synchronize()
    return whole, y, xd, rd


def model(ops, stride, relu):
    """-> (y64, bound, floor, the float64 quantities) of one call"""
    x, w, s, t, r, sr, tr = ops
    y64, S, v64, d64 = C.conv1x1(x, w, s, t, r, sr, tr, stride=stride, relu=relu)
    b = M.bound(x, w, s, S, v64, d64 if r is not None else None, folds_of_r=int(sr is not None), stride=stride)
    return y64, b, M.floor(w, TK), (S, v64, d64)


def check(ops, stride, relu, device, shifts=(0, 0, 0), what=None, expected=None):
    x, r = ops[0], ops[4]
    y64, bound, floor, _ = expected if expected is not None else model(ops, stride, relu)
    whole, y, xd, rd = run(ops, stride, relu, device, shifts)
    assert tuple(y.shape) == tuple(y64.shape)
    assert M.within(y, y64, bound, floor), what
    assert frame_intact(whole, y) and torch.equal(xd.cpu(), x) and (r is None or torch.equal(rd.cpu(), r)), what
    return y


@pytest.mark.parametrize("Cout,Cin", [(1, 1), (5, TK - 1), (5, TK), (3, TK + 1), (TM + 2, 3 * TK + 5)])
def test_pack_weights_equals_the_numpy_split(Cout, Cin, device):
    """Exactly, k >= Cin as zeros, nothing written outside; among the values powers of two, values at the top of the range, +-0, +-Inf, NaN
    and subnormals."""
    w = torch.randn(Cout, Cin, generator=gen(Cout + Cin))
    flat = w.view(-1)
    special = torch.tensor(np.array([0x7F7FFFFF, 0xFF7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0, 0x80000000, 0x3F800000, 0x00012345,
                                     0x807FFFFF, 0x3F808000, 0x3F818000], dtype=np.uint32).view(np.float32))
    flat[:min(len(flat), len(special))] = special[:len(flat)]
    whole, wp = packed(w, device)
    torch.cuda.synchronize()
    want = M.pack(w.numpy(), TK)
    got = wp.cpu().numpy().view(np.uint16).reshape(want.shape)
    assert np.array_equal(got, want)
    assert not got.transpose(0, 2, 1, 3).reshape(3, Cout, -1)[:, :, Cin:].any()                      # the padding is zeros
    assert bool((whole[:8] == SENTINEL).all()) and bool((whole[-8:] == SENTINEL).all())


@pytest.mark.parametrize("Cin", [TK, TK + 8, 2 * TK, 1, 9])
def test_sparse_columns(Cin, device):
    """One-hot and two-hot k per output with full 24-bit significands, at the first, a middle and the last real k (with Cin = TK + 8 the last
    one before the padding): nnz is 1 or 2 and the bound sharp.  Every product but the named ones is 0 * x."""
    ks = sorted({0, Cin // 2, Cin - 1})
    hots = [(k,) for k in ks] + [(a, b) for a in ks for b in ks if a < b]
    for Cout_pad, HW in ((0, 7), (TM - len(hots) + 1, TN + 3)):           # the small tile shape and the large one
        Cout = len(hots) + Cout_pad
        g = gen(Cin + Cout)
        x = torch.randn(2, Cin, HW, 1, generator=g)
        w = torch.zeros(Cout, Cin)
        for co in range(Cout):
            for k in hots[co % len(hots)]:
                w[co, k] = float(torch.randn(1, generator=g)) * 2.0 ** (co % 5)
        s, t = torch.ones(Cout), torch.zeros(Cout)                         # the accumulator itself
        ops = (x, w, s, t, None, None, None)
        y64, bound, floor, (S, _, _) = model(ops, 1, 0)
        assert float(M.nnz(x, w).max()) <= 2 and bool((bound <= 2.0 ** -20 * S * (1 + 1e-9)).all())        # (2^-23 + 12 * 2^-24) S + 2^-23 |v|, |v| <= S
        check(ops, 1, 0, device, what=(Cin, Cout), expected=(y64, bound, floor, None))
        fs, ft = fold_draw(Cout, g)                                        # and through a fold with a residual
        r = torch.randn(2, Cout, HW, 1, generator=g)
        check((x, w, fs, ft, r, None, None), 1, 1, device, what=(Cin, Cout, "fold"))


@pytest.mark.parametrize("Cout", COUTS)
def test_tile_edges(Cout, device):
    """Every Cin and HW at the edges of the tile and of the k-step; batch, epilogue form and relu rotate through the cases."""
    k = 0
    for Cin in CINS:
        for HW in HWS:
            N, form, relu = 1 + k % 2, FORMS[k % 3], (k // 3) % 2
            k += 1
            g = gen(100000 * Cout + 1000 * Cin + 2 * HW + N)
            check(draw(N, Cin, Cout, HW, 1, 1, form, g), 1, relu, device, what=(Cin, HW, N, form, relu))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_epilogue_forms(form, relu, device):
    for Cout, Cin, HW in ((3, 5, 9), (TM + 1, TK + 1, TN + 4)):
        y = check(draw(2, Cin, Cout, HW, 1, 1, form, gen(7 + relu)), 1, relu, device, what=(Cout, form, relu))
        assert bool((y < 0).any()) != bool(relu)               # the ReLU ran exactly when asked for


@pytest.mark.parametrize("HW", [TN + 4, TN + 5])
def test_every_position_inside_a_16_byte_unit(HW, device):
    """x, y and r each at every offset of 0 ... 3 floats behind a 16-byte boundary: with HW even the offset of x decides between the 8-byte
    path and the element-wise one, with HW odd every call is element-wise."""
    ops = draw(2, TK + 1, TM + 1, HW, 1, 1, "residual_fold", gen(HW))
    first, expected = None, model(ops, 1, 1)
    for sx in range(4):
        for sy in range(4):
            for sr in range(4):
                y = check(ops, 1, 1, device, shifts=(sx, sy, sr), what=(sx, sy, sr), expected=expected).clone()
                first = y if first is None else first
                assert torch.equal(y, first), (sx, sy, sr)          # and the path taken does not change a bit


@pytest.mark.parametrize("Cout", [5, TM + 1])
def test_stride_2(Cout, device):
    for H in range(1, 9):
        for W in range(1, 9):
            form = FORMS[(H + W) % 3]
            check(draw(2, TK + 1, Cout, H, W, 2, form, gen(100 * H + W + Cout)), 2, (H * W) % 2, device, shifts=(W % 4, H % 4, 0), what=(H, W, form))


@pytest.mark.parametrize("Cout", [1, TM + 1])
def test_more_tiles_than_work_groups(Cout, device):
    """Cin = 1 and enough pixels that the tiles outnumber OS2D_BACKBONE_CONV_BF16_MAX_GROUPS in either tile shape: every work-group strides."""
    tn, mt = (L.SMALL_TILE_N, 1) if Cout <= L.SMALL_TILE_M else (TN, 2)
    HW = (L.MAX_GROUPS // mt + 1) * tn + 1
    assert mt * ((HW + tn - 1) // tn) > L.MAX_GROUPS
    check(draw(1, 1, Cout, HW, 1, 1, "residual", gen(11)), 1, 1, device, shifts=(1, 3, 2))


def test_resnet_layer_shapes(device):
    """Every distinct 1x1 convolution of ResNet50-C4, read from the module, with the epilogue of its place in the block, at 2 x 5 x 7 pixels."""
    layers = C.resnet_c4_layers()
    assert len(layers) == 12
    for role, Cin, Cout, stride in layers:
        form, relu = {"conv1": ("fold", 1), "conv3": ("residual", 1), "downsample": ("fold", 0)}[role]
        check(draw(2, Cin, Cout, 5, 7, stride, form, gen(Cin + Cout)), stride, relu, device, what=(role, Cin, Cout, stride))


def test_placement_independence(device):
    """An output's bits depend on its own input column alone: not on the batch, the position, the tile shape's fill, the load path, or the
    call."""
    Cin, Cout = 2 * TK + 1, TM + 1
    ops = draw(2, Cin, Cout, TN + 2, 1, 1, "residual_fold", gen(21))
    x, w, s, t, r, sr, tr = ops
    _, both, _, _ = run(ops, 1, 1, device)
    _, again, _, _ = run(ops, 1, 1, device)
    assert torch.equal(both, again)                                                     # a second call
    _, other_path, _, _ = run(ops, 1, 1, device, shifts=(1, 0, 0))
    assert torch.equal(both, other_path)                                                # x off the 8-byte boundary: element by element
    _, alone, _, _ = run((x[1:].contiguous(), w, s, t, r[1:].contiguous(), sr, tr), 1, 1, device)
    assert torch.equal(both[1:], alone)                                                 # image 1 of 2 against the same image alone
    lead = (x[:, :, :5].contiguous(), w, s, t, r[:, :, :5].contiguous(), sr, tr)
    _, short, _, _ = run(lead, 1, 1, device)
    assert torch.equal(both[:, :, :5], short)                                           # columns 0 ... 4 of HW = TN + 2 against HW = 5 (odd)
    m = L.SMALL_TILE_M
    few = (x[:, :, :5].contiguous(), w[:m].contiguous(), s[:m], t[:m], r[:, :m, :5].contiguous(), sr[:m], tr[:m])
    _, small, _, _ = run(few, 1, 1, device)
    assert torch.equal(both[:, :m, :5], small)                                          # and against the other tile shape
    assert not bool(torch.isnan(both).any())


def test_nan_and_inf_poison_their_own_column(device):
    """NaN and Inf * 0 make their column NaN, Inf * w is +-Inf, a finite value at the top of the range stays finite arithmetic; every other
    column has the bits of the clean call."""
    Cin, Cout, HW = TK + 3, TM + 1, TN + 2
    x, w, s, t, r, sr, tr = draw(2, Cin, Cout, HW, 1, 1, "residual", gen(22))
    w[5, TK + 1] = 0.0
    clean = x.clone()
    x[0, 2, 7] = NAN
    x[1, TK + 1, HW - 1] = float("inf")          # in the partial k-step, in the last column: Inf * 0 in row 5
    x[1, 3, 11] = -float("inf")                  # no zero weight meets it: +-Inf everywhere
    y64 = C.conv1x1(x, w, s, t, r, relu=False)[0]
    poisoned = torch.zeros(2, Cout, HW, 1, dtype=torch.bool)
    poisoned[0, :, 7] = True
    poisoned[1, :, HW - 1] = True
    poisoned[1, :, 11] = True
    _, y, _, _ = run((x, w, s, t, r, sr, tr), 1, 0, device)
    got = y.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(y64)) and int(torch.isnan(got).sum()) == Cout + 1 and bool(torch.isnan(got[1, 5, HW - 1]))
    assert torch.equal(torch.isfinite(got), ~poisoned)
    assert torch.equal(got[1, :, 11].double(), y64[1, :, 11]) and bool(torch.isinf(got[1, :, 11]).all())          # the signs of the infinities
    _, yc, _, _ = run((clean, w, s, t, r, sr, tr), 1, 0, device)
    assert torch.equal(torch.where(poisoned, torch.zeros_like(got), got), torch.where(poisoned, torch.zeros_like(got), yc.cpu()))
    # a value between bf16's largest finite number and FLT_MAX: exact parts, a finite result where fp32 has one
    big = torch.zeros(1, TK, 4, 1)
    big[0, 1, 2] = 3.4e38
    wb = torch.zeros(2, TK)
    wb[0, 1], wb[1, 1] = 0.5, -0.25
    _, yb, _, _ = run((big, wb, torch.ones(2), torch.zeros(2), None, None, None), 1, 0, device)
    want = torch.zeros(1, 2, 4, 1)
    want[0, 0, 2], want[0, 1, 2] = 0.5 * big[0, 1, 2], -0.25 * big[0, 1, 2]
    assert torch.equal(yb.cpu(), want)


def test_against_the_fp32_entry_point(device):
    """The same operands through os2d_backbone_conv1x1: the two outputs differ by at most the sum of both bounds, and the ratio of their errors
    against float64 is printed per case.  Measured: 0.60 - 1.28 over the 12 layers, 1.55 for Cin = 1 - not at or
    below 1 everywhere, so the new entry point is held to its own derived bound and not to the fp32 entry point's Cin 2^-24 S |s|."""
    cases = [(2, Cin, Cout, 5, 7, stride, {"conv1": "fold", "conv3": "residual", "downsample": "fold"}[role], int(role != "downsample"))
             for role, Cin, Cout, stride in C.resnet_c4_layers()]
    cases += [(1, 7, 3, 9, 1, 1, "residual_fold", 1), (2, TK + 1, TM + 1, TN + 3, 1, 1, "residual_fold", 0), (1, 1, 1, 5, 1, 1, "fold", 0)]
    ratios = []
    for N, Cin, Cout, H, W, stride, form, relu in cases:
        ops = draw(N, Cin, Cout, H, W, stride, form, gen(Cin + 3 * Cout + H))
        x, w, s, t, r, sr, tr = ops
        y64, bound, floor, (S, v64, d64) = model(ops, stride, relu)
        bound32 = C.bound(Cin, S, s, v64, d64 if r is not None else None, folds_of_r=int(sr is not None))
        _, ours, _, _ = run(ops, stride, relu, device)
        _, theirs, _, _ = run(ops, stride, relu, device, fp32=True)
        assert M.within(ours, y64, bound, floor) and M.within(theirs, y64, bound32)
        assert M.within(ours, theirs.cpu().double(), bound + bound32, floor), (Cin, Cout)
        e_ours, e_theirs = float((ours.cpu().double() - y64).abs().max()), float((theirs.cpu().double() - y64).abs().max())
        rms = lambda e: float((e.cpu().double() - y64).pow(2).mean().sqrt())
        ratios.append(e_ours / e_theirs if e_theirs > 0 else float(e_ours > 0))
        print("Cin {:5d} Cout {:5d} stride {} {:13s}: max error bf16x3 {:.3g} fp32 {:.3g} ratio {:.3f}; rms ratio {:.3f}".format(
            Cin, Cout, stride, form, e_ours, e_theirs, ratios[-1], rms(ours) / rms(theirs) if rms(theirs) > 0 else float(rms(ours) > 0)))
    print("largest ratio of the maximal errors: {:.3f}".format(max(ratios)))
