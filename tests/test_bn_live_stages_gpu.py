"""GPU: the batch-statistics BatchNorm entry points of libos2d_train.so (include/os2d_train.h), each on its own, called through
os2d_amd/_train_lib.py with tensors built on the host, against the float64 model of the same stage (tests/bn_live_model.py).

Written outputs start as NaN, workspaces as NaN, and the pad cells of every input are exact zeros (the header's precondition).
Errors are relative max errors per output tensor, |got - ref|_max / |ref|_max, against the float64 model - never against another
run of the kernel.  Every figure is printed (STAGE ...) before it is asserted.
"""
import ctypes
import functools

import pytest
import torch

import backward_model as M
import bn_live_model as L

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24
SHAPES = [(1, 2), (2, 2), (9, 13), (70, 2), (2, 209), (38, 38)]
NBS = [1, 3]
CHANNELS = {1: 128, 2: 64}

# Pins: 3x the largest relative max error measured on the MI355X over the cases of this file (measured value in the comment; the
# table is in DESIGN.md section 16).
PIN = {
    "conv_f32": 1.3e-5,         # measured 4.3e-6 (layer 1, 1x38x38: 11025 fp32 products per output; layer 2: 2.1e-6)
    "conv_f16x3": 9.0e-6,       # measured 3.0e-6 (layer 1, 3x9x13; the fp32 figure of the same case: 4.2e-6; layer 2: 1.5e-6)
    "apply": 2.8e-7,            # measured 9.4e-8
    "backward_dy": 4.0e-7,      # measured 1.3e-7 over the cases with n >= 8 values per channel
    "backward_dgamma": 3.4e-6,  # measured 1.14e-6 at n = 2 (xhat = +-1: the two addends of a channel nearly cancel)
    "backward_dbeta": 1.7e-7,   # measured 5.5e-8
}
# The statistics: fp64 centred accumulation, then one fp32 rounding of each output
STATS_BOUND = 4 * U32
# With n < 8 values per channel the normalised values are close to +-1 whatever z is, and dy = gamma invstd (g - mean(g) - xhat
# mean(g xhat)) is what is left of O(|g|) terms that cancel (for n = 2 down to eps / var of them): the rounding of those terms,
# 2^-24 |gamma invstd g| each, is then compared with that scale instead of the cancelled result.
SMALL_N = 8
PIN_SMALL_N_DY = 3.3e-6         # measured 1.11e-6 of |gamma invstd g|_max (n = 2)


def _lib():
    from os2d_amd import _train_lib
    return _train_lib.load()


def _check(rc, what):
    from os2d_amd import _train_lib
    _train_lib.check(rc, what)


def _ptr(t):
    from os2d_amd import _lib as Lb
    return Lb.ptr(t)


def _stream(device):
    from os2d_amd import _lib as Lb
    return Lb.current_stream(device)


def dev(t, device):
    return t.detach().to(F32).contiguous().to(device)


def nan(device, *shape, dtype=F32):
    if dtype == torch.uint8:
        return torch.full(shape, 0xFF, dtype=dtype, device=device)       # an all-ones double is a NaN
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def report(stage, case, err):
    print("STAGE {:<18s} {:<44s} {:.3e}".format(stage, case, err))


def assert_planes(got, H, W, what):
    """A written plane buffer [N,C,PLANE]: finite everywhere, exactly +0.0 at the pad cells."""
    assert bool(torch.isfinite(got).all()), what + ": not every element was written"
    assert torch.count_nonzero(bits(got)[:, :, ~M.interior_mask(H, W)]) == 0, what + ": a pad cell is not +0.0"


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------------------------------------------------- (a) the convolution
@functools.lru_cache(maxsize=None)
def conv_case(layer, NB, shape):
    cout, cin, k = M.layer_shape(layer, 6)
    H, W = shape
    g = torch.Generator().manual_seed(5000 * layer + 100 * NB + 7 * H + W)
    x = torch.randn(NB, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    xp = M.pack_layer1_input(x) if layer == 1 else M.pack_planes(x)        # layer 1: plane 225 holds the sentinel
    return dict(xp=xp, w=w, b=b, z=L.conv_forward_model(xp, w, b, H, W), cout=cout, err={})


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("NB", NBS)
@pytest.mark.parametrize("layer", [1, 2])
@pytest.mark.parametrize("arith", [0, 1], ids=["f32", "f16x3"])
def test_conv_forward(device, arith, layer, NB, shape):
    c = conv_case(layer, NB, shape)
    lib, (H, W) = _lib(), shape
    PL = M.plane_geometry(H, W)[2]
    ws = nan(device, int(lib.os2d_train_conv_forward_workspace_floats(arith, layer, 6, NB)))
    z = nan(device, NB, c["cout"], PL)
    x, w, b = dev(c["xp"], device), dev(c["w"], device), dev(c["b"], device)
    _check(lib.os2d_train_conv_forward(arith, layer, 6, _ptr(w), _ptr(b), _ptr(x), NB, H, W, _ptr(z), _ptr(ws), ws.numel(), _stream(device)),
           "conv_forward")
    got = z.cpu()
    assert_planes(got, H, W, "z")
    err = M.rel_err(got, c["z"])
    c["err"][arith] = err
    report("conv_f16x3" if arith else "conv_f32", "layer {} NB {} {}x{}".format(layer, NB, H, W), err)
    assert err < PIN["conv_f16x3" if arith else "conv_f32"]
    if arith and 0 in c["err"]:         # within fp32 rounding of the fp32 route: the same order of magnitude on the same case
        report("conv_f16x3/f32", "layer {} NB {} {}x{}".format(layer, NB, H, W), err / c["err"][0])
        assert err < 4 * c["err"][0] + 2 * U32


# ---------------------------------------------------------------------------------------------------------- (b) the statistics
STATS_CASES = [(1, 1, 2), (3, 9, 13), (4, 38, 38), (1, 2, 209)]      # NB, H, W; the first: n = 2


@functools.lru_cache(maxsize=None)
def stats_case(layer, case):
    """z with a constant channel (0), a channel of mean 1e3 and standard deviation 1e-2 (1) and channels of every sign and scale."""
    NB, H, W = case
    C = CHANNELS[layer]
    g = torch.Generator().manual_seed(7000 * layer + 100 * NB + 7 * H + W)
    scale = torch.exp(2 * torch.randn(C, generator=g)).view(1, C, 1, 1)
    z = torch.randn(NB, C, H, W, generator=g) * scale + (torch.randn(C, generator=g).view(1, C, 1, 1) * scale)
    z[:, 0] = 0.75
    z[:, 1] = 1e3 + 1e-2 * torch.randn(NB, H, W, generator=g)
    zp = M.pack_planes(z)
    return zp, L.stats_model(zp, H, W)


@pytest.mark.parametrize("case", STATS_CASES, ids=ids)
@pytest.mark.parametrize("layer", [1, 2])
def test_bn_stats(device, layer, case):
    zp, (mean, var, invstd) = stats_case(layer, case)
    lib, (NB, H, W), C = _lib(), case, CHANNELS[layer]
    z = dev(zp, device)

    def run():
        ws = nan(device, int(lib.os2d_train_bn_workspace_bytes(layer, NB)), dtype=torch.uint8)
        out = [nan(device, C) for _ in range(3)]
        _check(lib.os2d_train_bn_stats(layer, _ptr(z), NB, H, W, ctypes.c_float(M.EPS32), *[_ptr(o) for o in out], _ptr(ws), ws.numel(),
                                       _stream(device)), "bn_stats")
        return [o.cpu() for o in out]

    got = run()
    assert all(bool(torch.isfinite(o).all()) for o in got)
    e_mean = ((got[0].to(F64) - mean).abs() / torch.maximum(mean.abs(), var.sqrt())).max()
    e_var = ((got[1].to(F64) - var).abs() / var.clamp_min(1e-300)).max()
    e_inv = ((got[2].to(F64) - invstd).abs() / invstd).max()
    tag = "layer {} NB {} {}x{}".format(layer, NB, H, W)
    for name, e in (("stats_mean", e_mean), ("stats_var", e_var), ("stats_invstd", e_inv)):
        report(name, tag, float(e))
    report("stats_var(ch 1)", tag, float((got[1][1].to(F64) - var[1]).abs() / var[1]))
    assert float(e_mean) <= STATS_BOUND and float(e_var) <= STATS_BOUND and float(e_inv) <= STATS_BOUND
    assert float(got[1][0]) == 0.0 and float(got[0][0]) == 0.75                     # the constant channel: var = 0 exactly
    assert float(got[2][0]) == float(torch.tensor(1.0 / M.EPS32 ** 0.5, dtype=F64).to(F32))
    again = run()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again))


# ---------------------------------------------------------------------------------------------------------- (c), (d)
@functools.lru_cache(maxsize=None)
def bn_case(layer, NB, shape):
    """z with |mean| <= 2 std per channel; gamma with a zero (channel 0) and negative entries; beta making channel 2 non-positive
    everywhere.  mean / invstd are the float64 statistics rounded to fp32; h is the float64 forward rounded to fp32, so that the
    mask h > 0 the kernel reads is the model's own."""
    H, W = shape
    C = CHANNELS[layer]
    g = torch.Generator().manual_seed(9000 * layer + 100 * NB + 7 * H + W)
    std = torch.exp(torch.randn(C, generator=g)).view(1, C, 1, 1)
    z = (torch.randn(NB, C, H, W, generator=g) + (4 * torch.rand(C, generator=g) - 2).view(1, C, 1, 1)) * std
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    gamma[0], gamma[1] = 0.0, -abs(float(gamma[1])) - 0.1
    beta = 0.3 * torch.randn(C, generator=g)
    beta[2] = -100.0 * (abs(float(gamma[2])) + 1.0)
    dh = torch.randn(NB, C, H, W, generator=g)
    zp, dhp = M.pack_planes(z), M.pack_planes(dh)
    mean, var, invstd = L.stats_model(zp, H, W)
    mean32, invstd32 = mean.to(F32), invstd.to(F32)
    h_apply = L.apply_model(zp, gamma, beta, mean32, invstd32, H, W)
    h = M.pack_planes(L.bn_relu_live_forward(z.to(F64), gamma.to(F64), beta.to(F64))).to(F32)
    dy, dg, db, _ = L.backward_model(dhp, zp, gamma, beta, H, W)
    k = (gamma.to(F64) * invstd).abs().view(1, C, 1)
    scale = float((k * (dhp.to(F64) * (h > 0)).abs()).max())
    return dict(zp=zp, dhp=dhp, gamma=gamma, beta=beta, mean=mean32, invstd=invstd32, h_apply=h_apply, h=h, dy=dy, dg=dg, db=db, C=C,
                n=NB * H * W, scale=scale)


BN_CASES = [(2, NB, s) for NB in NBS for s in SHAPES] + [(1, 3, (9, 13))]


@pytest.mark.parametrize("layer,NB,shape", BN_CASES, ids=ids)
def test_bn_relu_forward(device, layer, NB, shape):
    c = bn_case(layer, NB, shape)
    lib, (H, W) = _lib(), shape
    h = nan(device, NB, c["C"], M.plane_geometry(H, W)[2])
    args = [dev(c[k], device) for k in ("zp", "gamma", "beta", "mean", "invstd")]
    _check(lib.os2d_train_bn_relu_forward(layer, *[_ptr(a) for a in args], NB, H, W, _ptr(h), _stream(device)), "bn_relu_forward")
    got = h.cpu()
    assert_planes(got, H, W, "h")
    assert torch.count_nonzero(got[:, 2]) == 0 and float(got.min()) >= 0.0           # the non-positive channel; ReLU
    err = M.rel_err(got, c["h_apply"])
    report("apply", "layer {} NB {} {}x{}".format(layer, NB, H, W), err)
    assert err < PIN["apply"]


def _backward(device, lib, c, layer, NB, H, W, want_dg=True, want_db=True):
    C = c["C"]
    ws = nan(device, int(lib.os2d_train_bn_workspace_bytes(layer, NB)), dtype=torch.uint8)
    dy = nan(device, NB, C, M.plane_geometry(H, W)[2])
    dg = nan(device, C) if want_dg else None
    db = nan(device, C) if want_db else None
    args = [dev(c[k], device) for k in ("dhp", "zp", "h", "gamma", "mean", "invstd")]
    _check(lib.os2d_train_bn_relu_backward_batch(layer, *[_ptr(a) for a in args], NB, H, W, _ptr(dy), _ptr(dg), _ptr(db), _ptr(ws),
                                                 ws.numel(), _stream(device)), "bn_relu_backward_batch")
    return dy.cpu(), None if dg is None else dg.cpu(), None if db is None else db.cpu()


@pytest.mark.parametrize("layer,NB,shape", BN_CASES, ids=ids)
def test_bn_relu_backward_batch(device, layer, NB, shape):
    c = bn_case(layer, NB, shape)
    lib, (H, W) = _lib(), shape
    dy, dg, db = _backward(device, lib, c, layer, NB, H, W)
    assert_planes(dy, H, W, "dy")
    assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all())
    assert torch.count_nonzero(dy[:, 0]) == 0                                         # gamma = 0
    tag = "layer {} NB {} {}x{} n={}".format(layer, NB, H, W, c["n"])
    e_dg, e_db = M.rel_err(dg, c["dg"]), M.rel_err(db, c["db"])
    report("backward_dgamma", tag, e_dg)
    report("backward_dbeta", tag, e_db)
    assert e_dg < PIN["backward_dgamma"] and e_db < PIN["backward_dbeta"]
    if c["n"] < SMALL_N:
        e = float((dy.to(F64) - c["dy"]).abs().max()) / c["scale"]
        report("backward_dy/|kg|", tag, e)
        assert e < PIN_SMALL_N_DY
    else:
        e = M.rel_err(dy, c["dy"])
        report("backward_dy", tag, e)
        assert e < PIN["backward_dy"]
    again = _backward(device, lib, c, layer, NB, H, W)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((dy, dg, db), again))


@pytest.mark.parametrize("want_dg,want_db", [(True, False), (False, True), (False, False)])
def test_bn_relu_backward_batch_optional_outputs(device, want_dg, want_db):
    """Every NULL subset of the optional outputs: dy and the outputs that are asked for keep their bits."""
    layer, NB, (H, W) = 2, 3, (9, 13)
    c = bn_case(layer, NB, (H, W))
    lib = _lib()
    full = _backward(device, lib, c, layer, NB, H, W)
    part = _backward(device, lib, c, layer, NB, H, W, want_dg, want_db)
    assert torch.equal(bits(part[0]), bits(full[0]))
    assert (part[1] is None) == (not want_dg) and (part[2] is None) == (not want_db)
    for a, b in zip(part[1:], full[1:]):
        assert a is None or torch.equal(bits(a), bits(b))
