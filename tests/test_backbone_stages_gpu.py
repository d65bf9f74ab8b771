"""GPU: every entry point of libos2d_backbone.so alone through its C ABI against its float64 model (tests/backbone_model.py).

Outputs are pre-filled with NaN and stand inside a NaN frame that must survive; the model gets the same fp32 s and t.  The
bounds are derived, not measured (slack 1.01 for the float64 model's own rounding):
  bn_relu           one fmaf: half an ulp of the result,                       |y - y64| <= 2^-23 |y64|
  bn_add_relu       two fmaf (2^-24 |v|, 2^-24 |d|) and one add (2^-24 |v + d| <= 2^-24 (|v| + |d|)):  <= 2^-23 (|v64| + |d64|)
  bn_relu_maxpool   the maximum of correctly rounded values, rounding being monotonic: the bn_relu bound at the window's largest |v64|
Inputs are normal draws of unit scale: no result comes near the subnormal range, where a relative bound would not hold."""
import ctypes

import pytest
import torch

import backbone_model as B

pytestmark = pytest.mark.gpu

FRAME = 8          # NaN elements on either side of every output
NAN = float("nan")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def fold_draw(c, g):
    """s of either sign in 0.5 ... 1.5, t of unit scale"""
    s = (0.5 + torch.rand(c, generator=g)) * (1 - 2 * (torch.rand(c, generator=g) < 0.3).float())
    return s, torch.randn(c, generator=g)


def framed(shape, device, shift=0):
    """A NaN-filled output of `shape` whose first element stands `shift` floats behind a 16-byte boundary, inside a NaN frame."""
    n = 1
    for d in shape:
        n *= d
    whole = torch.full((FRAME + shift + n + FRAME,), NAN, device=device)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[FRAME + shift:FRAME + shift + n].view(shape)


def shifted(t, device, shift):
    """A device copy of t whose first element stands `shift` floats behind a 16-byte boundary."""
    whole = torch.empty(t.numel() + shift, device=device)
    view = whole[shift:].view(t.shape)
    view.copy_(t)
    return view


def frame_intact(whole, view):
    n = view.numel()
    at = (view.data_ptr() - whole.data_ptr()) // 4
    return bool(torch.isnan(whole[:at]).all()) and bool(torch.isnan(whole[at + n:]).all())


def call(name, *args):
    from os2d_amd import _backbone_lib
    from os2d_amd._native import STREAM
    _backbone_lib.call("os2d_backbone_" + name, *(list(args) + [STREAM]))
    torch.cuda.synchronize()


def within(y, y64, bound):
    """NaN exactly where the model has it, elsewhere within the bound (with the slack of the model's own arithmetic)."""
    y = y.detach().cpu().double()
    nan = torch.isnan(y64)
    if not torch.equal(torch.isnan(y), nan):
        return False
    err = torch.where(nan, torch.zeros_like(y), (y - y64).abs())
    return bool((err <= B.SLACK * torch.where(nan, torch.zeros_like(bound), bound)).all())


POINTWISE_HW = [1, 3, 4, 5, 1023, 1024, 1025, 70 * 94]


@pytest.mark.parametrize("C", [1, 3, 64])
@pytest.mark.parametrize("HW", POINTWISE_HW)
def test_bn_relu(C, HW, device):
    for N in (1, 2):
        g = gen(1000 * C + HW + N)
        x, (s, t) = torch.randn(N, C, HW, 1, generator=g), fold_draw(C, g)
        y64, _ = B.bn_relu(x, s, t)
        sd, td = s.to(device), t.to(device)
        # out of place at every position of x and y inside a 16-byte unit that differs in kind: same (vector units with a
        # head and a tail), different (element by element); then in place
        for shift_x, shift_y in ((0, 0), (1, 1), (3, 3), (0, 1), (2, 0)):
            xd = shifted(x, device, shift_x)
            whole, y = framed(x.shape, device, shift_y)
            call("bn_relu", xd, sd, td, y, N, C, HW)
            assert within(y, y64, B.U23 * y64.abs()), (N, shift_x, shift_y)
            assert frame_intact(whole, y) and torch.equal(xd.cpu(), x)
        for shift in (0, 1):
            xd = shifted(x, device, shift)
            call("bn_relu", xd, sd, td, xd, N, C, HW)
            assert within(xd, y64, B.U23 * y64.abs()), (N, "in place", shift)


@pytest.mark.parametrize("with_sr", [False, True])
@pytest.mark.parametrize("C", [1, 3, 64])
@pytest.mark.parametrize("HW", POINTWISE_HW)
def test_bn_add_relu(C, HW, with_sr, device):
    for N in (1, 2):
        g = gen(2000 * C + HW + N + 7 * with_sr)
        x, r = torch.randn(N, C, HW, 1, generator=g), torch.randn(N, C, HW, 1, generator=g)
        (s, t), (sr, tr) = fold_draw(C, g), fold_draw(C, g)
        if not with_sr:
            sr = tr = None
        y64, v64, d64 = B.bn_add_relu(x, s, t, r, sr, tr)
        bound = B.U23 * (v64.abs() + d64.abs())
        sd, td = s.to(device), t.to(device)
        srd, trd = (sr.to(device), tr.to(device)) if with_sr else (None, None)
        for shift_x, shift_r, shift_y in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (1, 0, 1), (0, 0, 3)):
            xd, rd = shifted(x, device, shift_x), shifted(r, device, shift_r)
            whole, y = framed(x.shape, device, shift_y)
            call("bn_add_relu", xd, sd, td, rd, srd, trd, y, N, C, HW)
            assert within(y, y64, bound), (N, shift_x, shift_r, shift_y)
            assert frame_intact(whole, y) and torch.equal(xd.cpu(), x) and torch.equal(rd.cpu(), r)
        for shift_x, shift_r in ((0, 0), (3, 3), (1, 2)):
            xd, rd = shifted(x, device, shift_x), shifted(r, device, shift_r)
            call("bn_add_relu", xd, sd, td, rd, srd, trd, xd, N, C, HW)
            assert within(xd, y64, bound), (N, "in place", shift_x, shift_r)
            assert torch.equal(rd.cpu(), r)


def test_pointwise_more_tiles_than_work_groups(device):
    """Short rows, many of them: the tiles outnumber OS2D_BACKBONE_MAX_GROUPS and every work-group strides."""
    from os2d_amd import _backbone_lib
    N, C, HW = 4, 1024 * 9, 35              # 16 lanes per row, 16 rows per work-group: 2304 row groups, more than the cap
    assert (N * C + 15) // 16 > _backbone_lib.MAX_GROUPS
    g = gen(5)
    x, r, (s, t) = torch.randn(N, C, HW, 1, generator=g), torch.randn(N, C, HW, 1, generator=g), fold_draw(C, g)
    y64, v64, d64 = B.bn_add_relu(x, s, t, r)
    whole, y = framed(x.shape, device, 1)
    call("bn_add_relu", x.to(device), s.to(device), t.to(device), r.to(device), None, None, y, N, C, HW)
    assert within(y, y64, B.U23 * (v64.abs() + d64.abs())) and frame_intact(whole, y)
    xd = x.to(device)
    call("bn_relu", xd, s.to(device), t.to(device), xd, N, C, HW)
    assert within(xd, B.bn_relu(x, s, t)[0], B.U23 * v64.abs())


def test_pointwise_nan_passes_through(device):
    N, C, HW = 2, 3, 1025
    g = gen(6)
    x, r, (s, t), (sr, tr) = torch.randn(N, C, HW, 1, generator=g), torch.randn(N, C, HW, 1, generator=g), fold_draw(C, g), fold_draw(C, g)
    x[1, 2, 1024] = NAN         # the scalar tail
    x[1, 0, 17] = NAN           # a vector unit
    r[1, 1, 0] = NAN
    dev = lambda *ts: [v.to(device) for v in ts]
    y64, _ = B.bn_relu(x, s, t)
    assert int(torch.isnan(y64).sum()) == 2 and not torch.isnan(y64[0]).any()
    _, y = framed(x.shape, device)
    call("bn_relu", *dev(x, s, t), y, N, C, HW)
    assert within(y, y64, B.U23 * y64.abs()) and not torch.isnan(y[0]).any()
    y64, v64, d64 = B.bn_add_relu(x, s, t, r, sr, tr)
    assert int(torch.isnan(y64).sum()) == 3 and not torch.isnan(y64[0]).any()
    _, y = framed(x.shape, device)
    call("bn_add_relu", *dev(x, s, t, r, sr, tr), y, N, C, HW)
    assert within(y, y64, torch.nan_to_num(B.U23 * (v64.abs() + d64.abs()))) and not torch.isnan(y[0]).any()


# (1,1) ... (31,45); around the kernel's 4 outputs per lane (Wp = 3, 4, 5) and its 256 lanes per tile (Hp * ceil(Wp / 4) = 255, 256, 514);
# a level of the class images
POOL_SIZES = [(1, 1), (2, 3), (7, 8), (17, 33), (31, 45), (509, 5), (511, 7), (513, 9), (64, 96)]


@pytest.mark.parametrize("H,W", POOL_SIZES)
def test_bn_relu_maxpool(H, W, device):
    N, C = 2, 3 if H > 100 else 5
    g = gen(31 * H + W)
    x, (s, t) = torch.randn(N, C, H, W, generator=g), fold_draw(C, g)
    y64, vmax = B.bn_relu_maxpool(x, s, t)
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(y64.shape) == (N, C, Hp, Wp)
    for shift_x, shift_y in ((0, 0), (1, 3)):
        xd = shifted(x, device, shift_x)
        whole, y = framed(y64.shape, device, shift_y)
        call("bn_relu_maxpool", xd, s.to(device), t.to(device), y, N, C, H, W)
        assert within(y, y64, B.U23 * vmax), (shift_x, shift_y)
        assert frame_intact(whole, y) and torch.equal(xd.cpu(), x)


def test_bn_relu_maxpool_64_channels_more_tiles_than_work_groups(device):
    from os2d_amd import _backbone_lib
    N, C, H, W = 36, 64, 17, 33
    assert N * C > _backbone_lib.MAX_GROUPS
    g = gen(8)
    x, (s, t) = torch.randn(N, C, H, W, generator=g), fold_draw(C, g)
    y64, vmax = B.bn_relu_maxpool(x, s, t)
    whole, y = framed(y64.shape, device)
    call("bn_relu_maxpool", x.to(device), s.to(device), t.to(device), y, N, C, H, W)
    assert within(y, y64, B.U23 * vmax) and frame_intact(whole, y)


def test_bn_relu_maxpool_special_values(device):
    """== and the NaN mask against the model: an all-negative window is 0, one NaN reaches exactly the windows that hold it."""
    N, C, H, W = 2, 3, 17, 33
    g = gen(9)
    x = torch.randn(N, C, H, W, generator=g)
    s, t = torch.tensor([1.0, -1.0, 2.0]), torch.zeros(C)             # exact arithmetic: the comparison is ==
    x[:, 0, :6, :8] = -x[:, 0, :6, :8].abs() - 1                      # windows of negative values only (channel 0: s = 1)
    x[1, 2, 9, 17] = NAN                                              # an odd row and column: 2 x 2 windows; another image stays clean
    x[1, 1, 16, 32] = NAN                                             # the last (even) row and column: one window
    y64, _ = B.bn_relu_maxpool(x, s, t)
    assert bool((y64[:, 0, :2, :3] == 0).all()) and int(torch.isnan(y64).sum()) == 4 + 1 and not torch.isnan(y64[0]).any()
    _, y = framed(y64.shape, device)
    call("bn_relu_maxpool", x.to(device), s.to(device), t.to(device), y, N, C, H, W)
    got = y.cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(y64)) and not torch.isnan(got[0]).any()
    assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(y64, nan=-1.0))
    assert bool((got[:, 0, :2, :3] == 0).all())


def test_refused_calls_launch_nothing_and_leave_the_outputs(device):
    from os2d_amd import _backbone_lib
    lib = _backbone_lib.load()
    N, C, H, W = 1, 4, 6, 6
    x = torch.randn(N, C, H, W, device=device)
    r = torch.randn(N, C, H, W, device=device)
    s, t = torch.ones(C, device=device), torch.zeros(C, device=device)
    whole, y = framed((N, 64, H, W), device)
    p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
    before = (x.clone(), r.clone())
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    cases = [
        ("bn_relu", (p(x), p(s), p(t), p(y), 0, C, H * W)),
        ("bn_relu", (p(x), None, p(t), p(y), N, C, H * W)),
        ("bn_relu", (p(x), p(s), p(t), ctypes.c_void_p(x.data_ptr() + 8), N, C, H * W)),
        ("bn_relu", (p(x), p(s), p(t), p(y), 1 << 16, 1 << 15, 1)),
        ("bn_add_relu", (p(x), p(s), p(t), p(r), p(s), None, p(y), N, C, H * W)),
        ("bn_add_relu", (p(x), p(s), p(t), p(r), None, None, p(r), N, C, H * W)),
        ("bn_add_relu", (p(x), p(s), p(t), p(r), None, None, p(y), N, -C, H * W)),
        ("bn_add_relu", (p(x), p(s), p(t), p(r), None, None, ctypes.c_void_p(y.data_ptr() + 2), N, C, H * W)),
        ("bn_relu_maxpool", (p(x), p(s), p(t), p(x), N, C, H, W)),
        ("bn_relu_maxpool", (p(x), p(s), p(t), p(y), N, C, H, 0)),
    ]
    for name, args in cases:
        assert getattr(lib, "os2d_backbone_" + name)(*(list(args) + [stream])) == -1, (name, args)
        assert lib.os2d_backbone_last_error().decode().startswith(name + ":")
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole).all()) and torch.equal(x, before[0]) and torch.equal(r, before[1])
    with pytest.raises(RuntimeError, match="bn_relu: bad shape"):
        _backbone_lib.call("os2d_backbone_bn_relu", x, s, t, y, 0, C, H * W, None)
