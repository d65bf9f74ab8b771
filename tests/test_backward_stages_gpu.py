"""GPU: every backward entry point of libos2d_train.so (include/os2d_train.h) on its own, called through os2d_amd/_train_lib.py with
tensors built on the host, against the float64 model of the same stage (tests/backward_model.py: torch autograd of the float64
forward stage).  tests/test_head_backward_gpu.py checks the same kernels end to end only.

In every test an output the header calls "written" is pre-filled with NaN (every element must come back finite, pad cells exactly
0) and an output it calls "added" with a non-zero pattern (the result is pattern + model).  Errors are relative max errors per
output tensor, |got - ref|_max / |ref|_max, never against another run of the kernel.
"""
import ctypes
import functools
import itertools

import pytest
import torch

import backward_model as M
from test_head_backward_gpu import PARAM_KEYS, TOL, _small, oracle_grads, rel_err as rel_err_head

pytestmark = pytest.mark.gpu

F32 = torch.float32
FRAGILE_CAP = 0.05           # the same cap as tests/test_backward_model.py

# Pins: 3x the largest relative max error measured on the MI355X over the cases of this file (measured value in the comment; the
# table is in DESIGN.md section 10).  The end-to-end pin of tests/test_head_backward_gpu.py is 6e-5: a smooth stage above it
# would be a finding, not a tolerance.
PIN = {
    "conv_data": 1.5e-5,          # measured 4.7e-6 (layer 1, 2x17x19: 6272 fp32 products per output)
    "conv_weight": 7.5e-6,        # measured 2.4e-6 with one slice (layer 1, 2x38x38), 1.2e-6 over every multi-slice case
    "params": 5e-7,               # measured 1.5e-7 (dbias; dy is an exact copy)
    "bn_relu": 1.8e-6,            # measured 6.0e-7 (dbias, layer 1)
    "norm225": 4.5e-7,            # measured 1.4e-7
    "corr": 4e-6,                 # measured 1.3e-6 (dfm, 1x5x64x17x19)
    "class": 9e-6,                # measured 2.9e-6 (C = 67, 33x40: the sampling positions are fp32)
    "decode_dcorr": 7.5e-6,       # measured 2.5e-6 (38x38, P = 6 with the inverse); 4.0e-7 on the smaller maps
    "decode_dparams": 5e-5,       # measured 1.6e-5 at the hand-placed x-clip location (per location); 1.7e-6 at 38x38, 7.4e-7 below
}
# d corr is scattered with atomicAdd: two calls on the same input may add a cell's addends in another order.  A cell collects a
# handful of addends (4 bilinear taps per point that lands near it; border cells the clamped points of a few columns or rows),
# all of the magnitude of the largest cell or below: a few dozen roundings of 2^-24.
ATOMIC_TOL = 64 * 2.0 ** -24


def _lib():
    from os2d_amd import _train_lib
    return _train_lib.load()


def _check(rc, what):
    from os2d_amd import _train_lib
    _train_lib.check(rc, what)


def _ptr(t):
    from os2d_amd import _lib as L
    return L.ptr(t)


def _stream(device):
    from os2d_amd import _lib as L
    return L.current_stream(device)


def dev(t, device):
    return t.detach().to(F32).contiguous().to(device)


def nan(device, *shape):
    return torch.full(shape, float("nan"), dtype=F32, device=device)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def report(stage, case, err):
    print("STAGE {:<15s} {:<40s} {:.3e}".format(stage, case, err))


def assert_planes(got, H, W, what):
    """A written plane buffer [N,C,PLANE]: finite everywhere, exactly 0 at the pad cells."""
    assert bool(torch.isfinite(got).all()), what + ": not every element was written"
    assert torch.count_nonzero(got[:, :, ~M.interior_mask(H, W)]) == 0, what + ": non-zero pad cell"


# ---------------------------------------------------------------------------------------------------------- convolutions
CONV_LAYERS = {"l1": (1, 6), "l2": (2, 6), "l3p6": (3, 6), "l3p4": (3, 4)}
CONV_SHAPES = [(1, 2, 2), (3, 9, 13), (2, 17, 19), (1, 2, 209), (1, 70, 2)]
CONV_CASES = [(k, s) for k in CONV_LAYERS for s in CONV_SHAPES] + [("l1", (2, 38, 38))]
SPLIT_SHAPES = {(3, 9, 13), (2, 17, 19)}
SPLIT_ROOMS = (1, 2, 3, 7, 64, 70)


@functools.lru_cache(maxsize=None)
def conv_case(key, shape):
    """Inputs (float32; the pads of x and dy are exact zeros, the header's precondition) and the float64 model, computed once."""
    layer, P = CONV_LAYERS[key]
    cout, cin, k = M.layer_shape(layer, P)
    NB, H, W = shape
    g = torch.Generator().manual_seed(1000 * layer + P + 7 * H + W)
    x = torch.randn(NB, cin, H, W, generator=g)
    dy = torch.randn(NB, cout, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    xp = M.pack_layer1_input(x) if layer == 1 else M.pack_planes(x)
    dyp = M.pack_planes(dy)
    dx_ref, dw_ref = M.conv_backward_model(xp, w, dyp, H, W)
    return dict(layer=layer, P=P, xp=xp, dyp=dyp, w=w, dx=dx_ref, dw=dw_ref, cin=cin)


@pytest.mark.parametrize("key,shape", CONV_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv_backward_data(device, key, shape):
    c = conv_case(key, shape)
    lib, (NB, H, W) = _lib(), shape
    PL = M.plane_geometry(H, W)[2]
    ws = nan(device, int(lib.os2d_train_conv_data_workspace_floats(c["layer"], c["P"])))
    dx = nan(device, NB, c["cin"], PL)
    w, dy = dev(c["w"], device), dev(c["dyp"], device)
    _check(lib.os2d_train_conv_backward_data(c["layer"], c["P"], _ptr(w), _ptr(dy), NB, H, W, _ptr(dx), _ptr(ws), ws.numel(),
                                             _stream(device)), "conv_backward_data")
    got = dx.cpu()
    assert_planes(got, H, W, "dx")
    err = M.rel_err(got, c["dx"])
    report("conv_data", "{} {}".format(key, shape), err)
    assert err < PIN["conv_data"]


@pytest.mark.parametrize("key,shape", CONV_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv_backward_weight(device, key, shape):
    """Every split-K slice count meets the same tolerance against float64; the same workspace gives the same bits twice."""
    from os2d_amd.modeling.head_train import _wgrad_splits
    c = conv_case(key, shape)
    lib, (NB, H, W) = _lib(), shape
    PL = M.plane_geometry(H, W)[2]
    n = int(lib.os2d_train_conv_weight_slice_floats(c["layer"], c["P"]))
    assert n == c["w"].numel()
    x, dy = dev(c["xp"], device), dev(c["dyp"], device)

    def run(room):
        ws = nan(device, n * room + (n // 2 if room > 1 else 0))        # room for exactly `room` slices (and a useless half)
        dw = nan(device, *c["w"].shape)
        _check(lib.os2d_train_conv_backward_weight(c["layer"], c["P"], _ptr(x), _ptr(dy), NB, H, W, _ptr(dw), _ptr(ws), ws.numel(),
                                                   _stream(device)), "conv_backward_weight")
        return dw.cpu()

    rooms = SPLIT_ROOMS if shape in SPLIT_SHAPES else (4, 64) if shape == (1, 2, 2) else (_wgrad_splits(NB, PL), 2)
    got = {}
    for room in rooms:
        got[room] = run(room)
        assert bool(torch.isfinite(got[room]).all()), "room {}: dw not fully written (or an unwritten slice was added)".format(room)
        err = M.rel_err(got[room], c["dw"])
        report("conv_weight", "{} {} room {}".format(key, shape, room), err)
        assert err < PIN["conv_weight"], room
        assert torch.equal(bits(run(room)), bits(got[room])), "room {}: two calls differ".format(room)
    if 70 in got:
        assert torch.equal(bits(got[70]), bits(got[64])), "more than 64 slices of room must behave as 64"
    if shape == (1, 2, 2):
        assert torch.equal(bits(got[64]), bits(got[4])), "64 positions allow 4 slices of one k-step"


# ---------------------------------------------------------------------------------------------------------- layer 3: parameters
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("P", [6, 4])
@pytest.mark.parametrize("shape", [(3, 9, 13), (1, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_params_backward(device, shape, P, with_bias):
    lib, (NB, H, W) = _lib(), shape
    PL = M.plane_geometry(H, W)[2]
    dparams = torch.randn(NB, P, H * W, generator=torch.Generator().manual_seed(P + H))
    dy_ref, db_ref = M.params_backward_model(dparams, H, W)
    dy, db = nan(device, NB, P, PL), nan(device, P) if with_bias else None
    src = dev(dparams, device)
    _check(lib.os2d_train_params_backward(_ptr(src), NB, P, H, W, _ptr(dy), _ptr(db), _stream(device)), "params_backward")
    got = dy.cpu()
    assert_planes(got, H, W, "dy")
    assert torch.equal(got.double(), dy_ref), "dy is a copy into the plane layout"
    if with_bias:
        assert bool(torch.isfinite(db).all())
        err = M.rel_err(db, db_ref)
        report("params", "{} P={}".format(shape, P), err)
        assert err < PIN["params"]


# ---------------------------------------------------------------------------------------------------------- BatchNorm + ReLU
@functools.lru_cache(maxsize=None)
def bn_case(layer, shape):
    NB, H, W = shape
    C = M.layer_shape(layer, 6)[0]
    g = torch.Generator().manual_seed(31 * layer + H)
    z = torch.randn(NB, C, H, W, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)     # a third of them < 0
    gamma[3] = 0.0
    beta = 0.3 * torch.randn(C, generator=g)
    beta[3] = 0.25                                      # the gamma = 0 channel is active everywhere: h = beta > 0
    mean = 0.2 * torch.randn(C, generator=g)
    var = 0.5 + torch.rand(C, generator=g)
    var[5] = 0.0                                        # only eps counts there
    h = M.bn_relu_forward(z.double(), gamma.double(), beta.double(), mean.double(), var.double()).float()
    assert 0.2 < float((h == 0).double().mean()) < 0.8  # the saved activation has exact zeros: the mask is h > 0
    dh = torch.randn(NB, C, M.plane_geometry(H, W)[2], generator=g)       # garbage at the pads too: the kernel masks them
    ref = M.bn_relu_backward_model(dh, z, gamma, beta, mean, var, H, W)
    return dict(C=C, hp=M.pack_planes(h), dh=dh, gamma=gamma, beta=beta, var=var, ref=ref)


@pytest.mark.parametrize("layer,shape", [(1, (3, 9, 13)), (2, (3, 9, 13)), (1, (1, 2, 2)), (2, (1, 2, 2))],
                         ids=lambda v: str(v) if isinstance(v, int) else "x".join(map(str, v)))
def test_bn_relu_backward(device, layer, shape):
    c = bn_case(layer, shape)
    lib, (NB, H, W), C = _lib(), shape, c["C"]
    PL = M.plane_geometry(H, W)[2]
    t = {k: dev(c[k], device) for k in ("dh", "hp", "gamma", "beta", "var")}

    def run(want):
        dy = nan(device, NB, C, PL)
        outs = [nan(device, C) if w else None for w in want]
        _check(lib.os2d_train_bn_relu_backward(layer, _ptr(t["dh"]), _ptr(t["hp"]), _ptr(t["gamma"]), _ptr(t["beta"]), _ptr(t["var"]),
                                               ctypes.c_float(M.EPS32), NB, H, W, _ptr(dy), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                               _stream(device)), "bn_relu_backward")
        return [dy.cpu()] + [o.cpu() if o is not None else None for o in outs]

    full = run((True, True, True))
    assert_planes(full[0], H, W, "dy")
    assert float(full[1][3]) == 0.0, "a channel with gamma = 0 gets dgamma = 0"
    live = torch.arange(C) != 3
    errs = {"dy": M.rel_err(full[0], c["ref"][0]), "dgamma": M.rel_err(full[1][live], c["ref"][1][live]),
            "dbeta": M.rel_err(full[2], c["ref"][2]), "dbias": M.rel_err(full[3], c["ref"][3])}
    for k, e in errs.items():
        assert bool(torch.isfinite(full[["dy", "dgamma", "dbeta", "dbias"].index(k)]).all()), k
        report("bn_relu", "layer {} {} {}".format(layer, shape, k), e)
    assert not {k: e for k, e in errs.items() if not e < PIN["bn_relu"]}, errs
    for want in itertools.product((True, False), repeat=3):
        if all(want):
            continue
        part = run(want)
        assert torch.equal(bits(part[0]), bits(full[0])), want
        for i, w in enumerate(want):
            assert part[1 + i] is None or torch.equal(bits(part[1 + i]), bits(full[1 + i])), (want, i)


# ---------------------------------------------------------------------------------------------------------- relu + L2 over 225
@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 17, 19)], ids=lambda s: "x".join(map(str, s)))       # HW = 4 / 323: one / two blocks
def test_norm225_backward(device, shape):
    lib, (NB, H, W) = _lib(), shape
    HW, PL = H * W, M.plane_geometry(H, W)[2]
    g = torch.Generator().manual_seed(HW)
    corr = torch.randn(NB, 225, H, W, generator=g)
    dead, single = (0, H - 1, 1), (1, 0, W - 1)
    corr[dead[0], :, dead[1], dead[2]] = -corr[dead[0], :, dead[1], dead[2]].abs()          # all 225 <= 0 ...
    corr[dead[0], ::7, dead[1], dead[2]] = 0.0                                               # ... some of them exactly 0
    corr[single[0], :, single[1], single[2]] = -corr[single[0], :, single[1], single[2]].abs()
    corr[single[0], 100, single[1], single[2]] = 0.7                                         # one positive channel
    dxn = torch.randn(NB, 225, PL, generator=g)
    prefill = 0.1 * torch.randn(NB, 225, HW, generator=g)          # of the magnitude of what is added
    ref = prefill.double() + M.norm225_backward_model(corr, dxn)
    dcorr = dev(prefill, device)
    c_d, dxn_d = dev(corr, device), dev(dxn, device)
    _check(lib.os2d_train_norm225_backward(_ptr(c_d), _ptr(dxn_d), NB, H, W, _ptr(dcorr), _stream(device)), "norm225_backward")
    got = dcorr.cpu()
    assert bool(torch.isfinite(got).all())
    n_dead = dead[1] * W + dead[2]
    assert torch.equal(bits(got[dead[0], :, n_dead]), bits(prefill[dead[0], :, n_dead])), "nothing is added where all 225 are <= 0"
    err = M.rel_err(got, ref)
    report("norm225", str(shape), err)
    assert err < PIN["norm225"]
    # the added part on its own, where it is not hidden behind the pattern: the single-channel position adds to channel 100 only
    n_single = single[1] * W + single[2]
    added = got[single[0], :, n_single].double() - prefill[single[0], :, n_single].double()
    assert torch.count_nonzero(added) <= 1 and torch.count_nonzero(added[torch.arange(225) != 100]) == 0


# ---------------------------------------------------------------------------------------------------------- correlation
@pytest.mark.parametrize("shape", [(1, 1, 1, 2, 2), (2, 3, 67, 9, 13), (3, 2, 130, 5, 7), (1, 5, 64, 17, 19)],
                         ids=lambda s: "x".join(map(str, s)))
def test_corr_backward(device, shape):
    from oracle import head_oracle as O
    lib, (A, B, C, H, W) = _lib(), shape
    HW = H * W
    g = torch.Generator().manual_seed(C + HW)
    fm = torch.randn(A, C, H, W, generator=g)
    zero = (A - 1, H - 1, 0)
    fm[zero[0], :, zero[1], zero[2]] = 0.0                       # an all-zero feature vector: the gradient there is g / eps
    qp = M.class_operand(O.l2_normalize_channels(torch.randn(B, C, 15, 15, generator=g).double(), 1e-5).float())
    dcorr = torch.randn(A * B, 225, HW, generator=g)
    dfm_ref, dq_ref = M.corr_backward_model(fm, qp, dcorr)
    n_ws = int(lib.os2d_train_corr_workspace_floats(A, C, H, W))
    t = [dev(x, device) for x in (fm, qp, dcorr)]

    def run(want_fm, want_q):
        ws = nan(device, n_ws)
        dfm = nan(device, A, C, H, W)
        dq = nan(device, B, C, 225)
        rc = lib.os2d_train_corr_backward(_ptr(t[0]), _ptr(t[1]), _ptr(t[2]), A, B, C, H, W, _ptr(dfm) if want_fm else None,
                                          _ptr(dq) if want_q else None, _ptr(ws), ws.numel(), _stream(device))
        _check(rc, "corr_backward")
        return dfm.cpu(), dq.cpu(), ws.cpu()

    dfm, dq, _ = run(True, True)
    assert bool(torch.isfinite(dfm).all()) and bool(torch.isfinite(dq).all())
    rest = torch.ones(A, H, W, dtype=torch.bool)
    rest[zero] = False
    at_zero = M.rel_err(dfm[zero[0], :, zero[1], zero[2]], dfm_ref[zero[0], :, zero[1], zero[2]])
    errs = {"dfm at the zero vector": at_zero, "dq": M.rel_err(dq, dq_ref),
            "dfm elsewhere": M.rel_err(dfm.permute(0, 2, 3, 1)[rest], dfm_ref.permute(0, 2, 3, 1)[rest])}
    for k, e in errs.items():
        report("corr", "{} {}".format(shape, k), e)
    assert not {k: e for k, e in errs.items() if not e < PIN["corr"]}, errs
    only_fm, untouched_q, _ = run(True, False)
    assert torch.equal(bits(only_fm), bits(dfm)) and bool(torch.isnan(untouched_q).all())
    untouched_fm, only_q, _ = run(False, True)
    assert torch.equal(bits(only_q), bits(dq)) and bool(torch.isnan(untouched_fm).all())
    none = run(False, False)                                      # returns 0 and launches nothing
    assert all(bool(torch.isnan(x).all()) for x in none)


# ---------------------------------------------------------------------------------------------------------- class maps
CLASS_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (15, 15), (12, 18), (33, 40)]


@pytest.mark.parametrize("C", [1, 67, 257])
def test_class_backward(device, C):
    from oracle import head_oracle as O
    lib, B = _lib(), len(CLASS_SIZES)
    g = torch.Generator().manual_seed(C)
    raws = [torch.randn(1, C, h, w, generator=g) for h, w in CLASS_SIZES]
    raws[3][:, :, 0, 0] = 0.0       # the 2x2 class: resized cell (0, 0) reads source cell (0, 0) alone: zero over all channels
    q15 = O.resize_class_maps([r.double() for r in raws]).float()
    assert torch.count_nonzero(q15[3, :, 0, 0]) == 0 and torch.count_nonzero(q15[3, :, 0, 1]) > 0
    dq = torch.randn(B, C, 225, generator=g)
    ref = M.class_backward_model(raws, dq)
    outs = [nan(device, *r.shape[1:]) for r in raws]
    ptrs = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64).to(device)
    sizes = torch.tensor(CLASS_SIZES, dtype=torch.int32).to(device)
    ws = nan(device, B * C * 225)
    q_d, dq_d = dev(q15.reshape(B, C, 225), device), dev(dq, device)
    _check(lib.os2d_train_class_backward(_ptr(q_d), _ptr(dq_d), B, C, _ptr(ptrs), _ptr(sizes), _ptr(ws), ws.numel(), _stream(device)),
           "class_backward")
    errs = {}
    for b, (o, r) in enumerate(zip(outs, ref)):
        assert bool(torch.isfinite(o).all()), CLASS_SIZES[b]
        errs[CLASS_SIZES[b]] = M.rel_err(o, r[0])                 # per class: the zero cell's g / eps stays in its own class
        report("class", "C={} {}".format(C, CLASS_SIZES[b]), errs[CLASS_SIZES[b]])
    assert not {k: e for k, e in errs.items() if not e < PIN["class"]}, errs


# ---------------------------------------------------------------------------------------------------------- decode backward
def run_decode(device, inp, P, inverse, stride, rec_field, use=(True, True, True), zeros_for_absent=False):
    lib = _lib()
    NB, _, H, W = inp["corr"].shape
    ups = []
    for name, on in zip(("dcls", "dcls_det", "dloc"), use):
        ups.append(dev(inp[name], device) if on else dev(torch.zeros_like(inp[name]), device) if zeros_for_absent else None)
    corr, params = dev(inp["corr"], device), dev(inp["params"], device)
    dcorr = dev(inp["prefill"], device)
    dparams = nan(device, NB, P, H * W)
    _check(lib.os2d_train_decode_backward(_ptr(corr), _ptr(params), _ptr(ups[0]), _ptr(ups[1]), _ptr(ups[2]), NB, H, W, P,
                                          1 if inverse else 0, stride, rec_field, _ptr(dcorr), _ptr(dparams), _stream(device)),
           "decode_backward")
    return dcorr.cpu(), dparams.cpu()


@pytest.mark.parametrize("name", sorted(M.DECODE_CASES))
def test_decode_backward(device, name):
    """d corr at EVERY location (the scatter is continuous across cell edges); d params at the non-fragile ones."""
    P, inverse, stride, rec_field, NB, H, W, _ = M.DECODE_CASES[name]
    inp = M.decode_inputs(name)
    dcorr_ref, dparams_ref, ratio = M.decode_backward_model(inp["corr"], inp["params"], inp["dcls"], inp["dcls_det"], inp["dloc"],
                                                            inverse, stride, rec_field)
    dcorr, dparams = run_decode(device, inp, P, inverse, stride, rec_field)
    assert bool(torch.isfinite(dcorr).all()) and bool(torch.isfinite(dparams).all())
    fragile = ratio < 1
    share = float(fragile.double().mean())
    print("STAGE decode fragile share {} {:.4f}".format(name, share))
    assert share <= FRAGILE_CAP
    err_c = M.rel_err(dcorr, inp["prefill"].double() + dcorr_ref)
    keep = (~fragile).view(NB, 1, H * W).expand(NB, P, H * W)
    err_p = M.rel_err(dparams[keep], dparams_ref[keep])
    report("decode_dcorr", name, err_c)
    report("decode_dparams", name, err_p)
    assert err_c < PIN["decode_dcorr"] and err_p < PIN["decode_dparams"]


@pytest.mark.parametrize("inverse", [True, False], ids=["inv", "fwd"])
def test_decode_backward_hand_placed_locations(device, inverse):
    """The branches random parameters never visit (backward_model.HAND_THETA), each location judged on its own: none is
    excluded as fragile."""
    inp = M.hand_inputs(inverse)
    dcorr_ref, dparams_ref, ratio = M.decode_backward_model(inp["corr"], inp["params"], inp["dcls"], inp["dcls_det"], inp["dloc"],
                                                            inverse, 16, 16)
    dcorr, dparams = run_decode(device, inp, 6, inverse, 16, 16)
    assert bool(torch.isfinite(dcorr).all()) and bool(torch.isfinite(dparams).all())
    print("distance to the nearest jump, in units of delta:", ["{:.3g}".format(float(r)) for r in ratio[0]])
    assert bool((ratio[0, 1:] > 100).all()), "hand-placed locations keep a margin far above delta (location 0 has exact ties)"
    err_c = M.rel_err(dcorr, inp["prefill"].double() + dcorr_ref)
    report("decode_dcorr", "hand inverse={}".format(inverse), err_c)
    assert err_c < PIN["decode_dcorr"]
    for n in range(9):
        err = M.rel_err(dparams[0, :, n], dparams_ref[0, :, n])
        report("decode_dparams", "hand inverse={} location {}".format(inverse, n), err)
        assert err < PIN["decode_dparams"], n
    # all 121 points clamped: with d cls alone, d params is exactly 0 there
    only_cls = dict(inp, dloc=torch.zeros_like(inp["dloc"]))
    _, dp = run_decode(device, only_cls, 6, inverse, 16, 16, use=(True, False, False))
    assert torch.count_nonzero(dp[0, :, 4]) == 0 and torch.count_nonzero(dp[0, :, 5]) > 0
    if not inverse:
        assert torch.count_nonzero(dp[0, :3, 1]) == 0           # location 1: every x coordinate clamped, the y's are not


@pytest.mark.parametrize("name", ["9x13_p6_inv_s16", "9x13_p4_fwd_s16"])
def test_decode_backward_null_upstream_gradients(device, name):
    P, inverse, stride, rec_field = M.DECODE_CASES[name][:4]
    inp = M.decode_inputs(name)
    for use in itertools.product((True, False), repeat=3):
        if all(use):
            continue
        dcorr, dparams = run_decode(device, inp, P, inverse, stride, rec_field, use=use)
        assert bool(torch.isfinite(dparams).all())
        if not any(use):
            assert torch.count_nonzero(dparams) == 0
            assert torch.equal(bits(dcorr), bits(inp["prefill"]))
            continue
        dcorr0, dparams0 = run_decode(device, inp, P, inverse, stride, rec_field, use=use, zeros_for_absent=True)
        assert torch.equal(bits(dparams), bits(dparams0)), use
        assert M.rel_err(dcorr, dcorr0) <= ATOMIC_TOL, use


# ---------------------------------------------------------------------------------------------------------- partial requires_grad
@functools.lru_cache(maxsize=None)
def _small_oracle():
    state, fm, class_fms, (gl, gc, gd) = _small(None)
    return state, fm, class_fms, (gl, gc, gd), oracle_grads(fm, class_fms, state, True, gl, gc, gd)


@pytest.mark.parametrize("only", ["fm", "class1", "linear.bias", "conv.1.weight"])
def test_partial_requires_grad_through_the_head(device, only):
    """The NULL outputs of the entry points as autograd reaches them; linear.bias alone gives need_below == False."""
    import util
    state, fm, class_fms, (gl, gc, gd), ref = _small_oracle()
    creator = util.make_head_creator(6, True, state, device)
    net = creator.aligner.parameter_regressor
    named = dict(net.named_parameters())
    for k, p in named.items():
        p.requires_grad_(k == only)
    fm_d = fm.to(device).requires_grad_(only == "fm")
    raws = [c.to(device).requires_grad_(only == "class{}".format(i)) for i, c in enumerate(class_fms)]
    loc, cls, cls_det, _ = creator.create_os2d_head(raws)(fm_d)
    loss = (loc.double() * gl.to(device)).sum() + (cls.double() * gc.to(device)).sum() + (cls_det.double() * gd.to(device)).sum()
    loss.backward()
    got = {"fm": fm_d.grad}
    got.update({"class{}".format(i): r.grad for i, r in enumerate(raws)})
    got.update({k: named[k].grad for k in PARAM_KEYS})
    want = {"fm": ref["fm"]}
    want.update({"class{}".format(i): g for i, g in enumerate(ref["class"])})
    want.update({k: ref[k] for k in PARAM_KEYS})
    for k, g in got.items():
        if k != only:
            assert g is None, k
    err = rel_err_head(got[only].cpu(), want[only])
    print("only", only, "{:.2e}".format(err))
    assert err < TOL
