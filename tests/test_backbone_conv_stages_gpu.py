"""GPU: os2d_backbone_conv1x1 alone through its C ABI against its float64 model (tests/backbone_conv_model.py).

Every output is pre-filled with NaN and stands inside a NaN frame that must survive; the model gets the same fp32 operands.  The bound
is derived, not measured (backbone_conv_model.bound, slack 1.01 for the float64 model's own rounding):
    Cin * 2^-24 * S * |s|     the accumulator, a chain of Cin fmaf whose partial sums are at most S = sum |w x| in magnitude, through the fold
  + 2^-23 |v64|               the fold's rounding and, with a residual, its share of the add's
  + 2^-23 |d64|               with a residual: its share of the add's rounding
  + 2^-23 |d64|               when the residual has a fold of its own: that fold's rounding
Inputs are normal draws of unit scale: no result comes near the subnormal range, where a relative bound would not hold.

The cases stand one below, at and one above each tile size of the kernel (read from the binding), for both of its tile shapes.  The
contract has three epilogue forms - the fold alone, with a residual, with a residual that has a fold of its own - and each runs with
relu 0 and 1."""
import ctypes

import pytest
import torch

import backbone_conv_model as C
from os2d_amd import _backbone_conv_lib as L
from test_backbone_stages_gpu import fold_draw, frame_intact, framed, gen, shifted, within

pytestmark = pytest.mark.gpu

NAN = float("nan")
M, N_, K = L.TILE_M, L.TILE_N, L.TILE_K
COUTS = [1, L.SMALL_TILE_M - 1, L.SMALL_TILE_M, L.SMALL_TILE_M + 1, M - 1, M, M + 1, 2 * M + 1]
CINS = [1, 2, 3, K - 1, K, K + 1, 4 * K + 1]
HWS = [1, 3, 4, 5, N_ - 1, N_, N_ + 1, L.SMALL_TILE_N - 1, L.SMALL_TILE_N, L.SMALL_TILE_N + 1]
FORMS = ["fold", "residual", "residual_fold"]


def draw(N, Cin, Cout, H, W, stride, form, g):
    """The operands of one call on the CPU: x, w, (s, t), r, (sr, tr)"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, w = torch.randn(N, Cin, H, W, generator=g), torch.randn(Cout, Cin, generator=g)
    s, t = fold_draw(Cout, g)
    r = torch.randn(N, Cout, Ho, Wo, generator=g) if form != "fold" else None
    sr, tr = fold_draw(Cout, g) if form == "residual_fold" else (None, None)
    return x, w, s, t, r, sr, tr


def run(ops, stride, relu, device, shifts=(0, 0, 0)):
    """One call on device copies of the operands (x, y, r start `shifts` floats behind a 16-byte boundary) -> (whole, y, xd, rd)"""
    x, w, s, t, r, sr, tr = ops
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    to = lambda v: v.to(device) if v is not None else None
    xd, rd = shifted(x, device, shifts[0]), (shifted(r, device, shifts[2]) if r is not None else None)
    whole, y = framed((N, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1), device, shifts[1])
    from os2d_amd._native import STREAM
    L.call("os2d_backbone_conv1x1", xd, to(w), to(s), to(t), rd, to(sr), to(tr), y, N, Cin, Cout, H, W, stride, int(relu), STREAM)
    torch.cuda.synchronize()
    return whole, y, xd, rd


def model(ops, stride, relu):
    """-> (y64, bound) of one call"""
    x, w, s, t, r, sr, tr = ops
    y64, S, v64, d64 = C.conv1x1(x, w, s, t, r, sr, tr, stride=stride, relu=relu)
    return y64, C.bound(x.shape[1], S, s, v64, d64 if r is not None else None, folds_of_r=int(sr is not None))


def check(ops, stride, relu, device, shifts=(0, 0, 0), what=None, expected=None):
    x, r = ops[0], ops[4]
    y64, bound = expected if expected is not None else model(ops, stride, relu)
    whole, y, xd, rd = run(ops, stride, relu, device, shifts)
    assert tuple(y.shape) == tuple(y64.shape)
    assert within(y, y64, bound), what
    assert frame_intact(whole, y) and torch.equal(xd.cpu(), x) and (r is None or torch.equal(rd.cpu(), r)), what
    return y


@pytest.mark.parametrize("Cout", COUTS)
def test_tile_edges(Cout, device):
    """Every Cin and HW at the edges of the tile, batch 1 and 2; the epilogue form and relu rotate through the cases."""
    k = 0
    for Cin in CINS:
        for HW in HWS:
            for N in (1, 2):
                form, relu = FORMS[k % 3], (k // 3) % 2
                k += 1
                g = gen(100000 * Cout + 1000 * Cin + 2 * HW + N)
                check(draw(N, Cin, Cout, HW, 1, 1, form, g), 1, relu, device, what=(Cin, HW, N, form, relu))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_epilogue_forms(form, relu, device):
    for Cout, Cin, HW in ((3, 5, 9), (M + 1, K + 1, N_ + 4)):
        y = check(draw(2, Cin, Cout, HW, 1, 1, form, gen(7 + relu)), 1, relu, device, what=(Cout, form, relu))
        assert bool((y < 0).any()) != bool(relu)               # the ReLU ran exactly when asked for


@pytest.mark.parametrize("HW", [N_ + 4, N_ + 5])
def test_every_position_inside_a_16_byte_unit(HW, device):
    """x, y and r each at every offset of 0 ... 3 floats behind a 16-byte boundary: with HW a multiple of 4 the offset of x decides between
    the 16-byte path and the element-wise one, with HW odd every row starts somewhere else anyway."""
    ops = draw(2, K + 1, M + 1, HW, 1, 1, "residual_fold", gen(HW))
    first, expected = None, model(ops, 1, 1)
    for sx in range(4):
        for sy in range(4):
            for sr in range(4):
                y = check(ops, 1, 1, device, shifts=(sx, sy, sr), what=(sx, sy, sr), expected=expected).clone()
                first = y if first is None else first
                assert torch.equal(y, first), (sx, sy, sr)          # and the path taken does not change a bit


@pytest.mark.parametrize("Cout", [5, M + 1])
def test_stride_2(Cout, device):
    sizes = [1, 2, 3, 4, 5, 7, 8]
    for H in sizes:
        for W in sizes:
            form = FORMS[(H + W) % 3]
            check(draw(2, K + 1, Cout, H, W, 2, form, gen(100 * H + W + Cout)), 2, (H * W) % 2, device, shifts=(W % 4, H % 4, 0), what=(H, W, form))


@pytest.mark.parametrize("Cout", [1, M + 1])
def test_more_tiles_than_work_groups(Cout, device):
    """Cin = 1 and enough pixels that the tiles outnumber OS2D_BACKBONE_CONV_MAX_GROUPS in either tile shape: every work-group strides."""
    tn, mt = (L.SMALL_TILE_N, 1) if Cout <= L.SMALL_TILE_M else (N_, 2)
    HW = (L.MAX_GROUPS // mt + 1) * tn + 1
    assert mt * ((HW + tn - 1) // tn) > L.MAX_GROUPS
    check(draw(1, 1, Cout, HW, 1, 1, "residual", gen(11)), 1, 1, device, shifts=(1, 3, 2))


def test_resnet_layer_shapes(device):
    """Every distinct 1x1 convolution of ResNet50-C4 with the epilogue of its place in the block, at 2 x 5 x 7 pixels."""
    for role, Cin, Cout, stride in C.resnet_c4_layers():
        form, relu = {"conv1": ("fold", 1), "conv3": ("residual", 1), "downsample": ("fold", 0)}[role]
        check(draw(2, Cin, Cout, 5, 7, stride, form, gen(Cin + Cout)), stride, relu, device, what=(role, Cin, Cout, stride))


def test_placement_independence(device):
    """An output's bits depend on its own input column alone: not on the batch, the position, the tile shape's fill, or the call."""
    Cin, Cout = 4 * K + 1, M + 1
    ops = draw(2, Cin, Cout, N_ + 1, 1, 1, "residual_fold", gen(21))
    x, w, s, t, r, sr, tr = ops
    _, both, _, _ = run(ops, 1, 1, device)
    _, again, _, _ = run(ops, 1, 1, device)
    assert torch.equal(both, again)                                                     # a second call
    _, alone, _, _ = run((x[1:].contiguous(), w, s, t, r[1:].contiguous(), sr, tr), 1, 1, device)
    assert torch.equal(both[1:], alone)                                                 # image 1 of 2 against the same image alone
    lead = (x[:, :, :5].contiguous(), w, s, t, r[:, :, :5].contiguous(), sr, tr)
    _, short, _, _ = run(lead, 1, 1, device)
    assert torch.equal(both[:, :, :5], short)                                           # columns 0 ... 4 of HW = N + 1 against HW = 5
    few = (x[:, :, :5].contiguous(), w[:L.SMALL_TILE_M], s[:L.SMALL_TILE_M], t[:L.SMALL_TILE_M], r[:, :L.SMALL_TILE_M, :5].contiguous(),
           sr[:L.SMALL_TILE_M], tr[:L.SMALL_TILE_M])
    _, small, _, _ = run(few, 1, 1, device)
    assert torch.equal(both[:, :L.SMALL_TILE_M, :5], small)                             # and against the other tile shape
    assert not bool(torch.isnan(both).any())


def test_nan_and_inf_times_zero_poison_their_own_column(device):
    Cin, Cout, HW = K + 3, M + 1, N_ + 1
    x, w, s, t, r, sr, tr = draw(2, Cin, Cout, HW, 1, 1, "residual", gen(22))
    clean = (x.clone(), w.clone(), s, t, r, sr, tr)
    x[0, 2, 7] = NAN
    x[1, K + 1, HW - 1] = float("inf")          # in the partial k-step, in the last column
    w[5, K + 1] = 0.0
    y64 = C.conv1x1(x, w, s, t, r, relu=False)[0]
    want = torch.zeros(2, Cout, HW, 1, dtype=torch.bool)
    want[0, :, 7] = True
    want[1, :, HW - 1] = True                   # Inf * 0 in row 5, +-Inf in the other rows (no ReLU here: it would turn -Inf into 0)
    _, y, _, _ = run((x, w, s, t, r, sr, tr), 1, 0, device)
    got = y.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(y64)) and int(torch.isnan(got).sum()) == Cout + 1 and bool(torch.isnan(got[1, 5, HW - 1]))
    assert torch.equal(torch.isfinite(got), ~want)
    # every other column has the bits of the clean call
    wc = clean[1].clone()
    wc[5, K + 1] = 0.0
    _, yc, _, _ = run((clean[0], wc, s, t, r, sr, tr), 1, 0, device)
    assert torch.equal(torch.where(want, torch.zeros_like(got), got), torch.where(want, torch.zeros_like(got), yc.cpu()))


def test_refused_calls_launch_nothing_and_leave_the_outputs(device):
    lib = L.load()
    N, Cin, Cout, H, W = 1, 4, 8, 6, 6
    x, w, r = torch.randn(N, Cin, H, W, device=device), torch.randn(Cout, Cin, device=device), torch.randn(N, Cout, H, W, device=device)
    s, t = torch.ones(Cout, device=device), torch.zeros(Cout, device=device)
    whole, y = framed((N, Cout, H, W), device)
    p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
    before = (x.clone(), w.clone(), r.clone())
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    cases = [
        (p(x), p(w), p(s), p(t), None, None, None, p(y), 0, Cin, Cout, H, W, 1, 1),
        (p(x), None, p(s), p(t), None, None, None, p(y), N, Cin, Cout, H, W, 1, 1),
        (p(x), p(w), p(s), p(t), None, p(s), p(t), p(y), N, Cin, Cout, H, W, 1, 1),
        (p(x), p(w), p(s), p(t), p(r), p(s), None, p(y), N, Cin, Cout, H, W, 1, 1),
        (p(x), p(w), p(s), p(t), None, None, None, ctypes.c_void_p(y.data_ptr() + 2), N, Cin, Cout, H, W, 1, 1),
        (p(x), p(w), p(s), p(t), None, None, None, p(y), N, Cin, Cout, H, W, 3, 1),
        (p(x), p(w), p(s), p(t), None, None, None, p(y), N, Cin, Cout, H, W, 1, 2),
        (p(x), p(w), p(s), p(t), None, None, None, p(y), 1 << 12, 1 << 19, Cout, 1, 1, 1, 1),
        (p(x), p(w), p(s), p(t), None, None, None, p(x), N, Cin, Cout, H, W, 1, 1),
        (p(x), p(w), p(s), p(t), None, None, None, p(w), N, Cin, Cout, 1, 1, 1, 1),
        (p(x), p(w), p(s), p(t), p(r), None, None, p(r), N, Cin, Cout, H, W, 1, 1),
    ]
    for args in cases:
        assert lib.os2d_backbone_conv1x1(*(list(args) + [stream])) == -1, args
        assert lib.os2d_backbone_conv_last_error().decode().startswith("conv1x1:")
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole).all()) and torch.equal(x, before[0]) and torch.equal(w, before[1]) and torch.equal(r, before[2])
    with pytest.raises(RuntimeError, match="conv1x1: stride is 1 or 2"):
        L.call("os2d_backbone_conv1x1", x, w, s, t, None, None, None, y, N, Cin, Cout, H, W, 0, 1, None)
