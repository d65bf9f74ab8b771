"""GPU: the backward GEMMs of libos2d_train.so in split-fp16 ("f16x3") arithmetic - the *_ex entry points of include/os2d_train.h
at arith = 1 (os2d_amd/csrc_train/train_gemm.hip) - against the float64 models of tests/backward_model.py, on the shapes of
tests/test_backward_stages_gpu.py (whose inputs and cached float64 references are shared), and through autograd against the CPU
oracle on the small cases of tests/test_head_backward_gpu.py.

Outputs start as NaN and workspaces as NaN.  Errors are relative max errors per output tensor against float64."""
import pytest
import torch

import backward_model as M
import util
from test_backward_stages_gpu import (CONV_CASES, CONV_LAYERS, SPLIT_ROOMS, SPLIT_SHAPES, _check, _lib, _ptr, _stream, assert_planes, bits,
                                      conv_case, dev, nan)
from test_head_backward_gpu import CASES, PARAM_KEYS, TOL, _check_case, _small, hip_grads, oracle_grads

pytestmark = pytest.mark.gpu

F16X3 = 1
# The pins of the SAME stage on the fp32 route, copied from PIN of tests/test_backward_stages_gpu.py (3x what the fp32 kernels
# measure).  The split arithmetic adds less than fp32 rounding (tests/test_backward_f16x3_model.py) and the accumulation is fp32 on
# both routes, so the fp32 route's pins are the cap here: a value above one is a finding about the kernel, not a tolerance.
PIN = {"conv_data": 1.5e-5, "conv_weight": 7.5e-6, "corr": 4e-6}
IDS = dict(ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))


def report(stage, case, err):
    print("STAGE f16x3 {:<12s} {:<44s} {:.3e}".format(stage, case, err))


# ---------------------------------------------------------------------------------------------------------- convolutions
def data_gradient(device, c, shape, dyp=None, w=None, arith=F16X3):
    lib, (NB, H, W) = _lib(), shape
    PL = M.plane_geometry(H, W)[2]
    ws = nan(device, int(lib.os2d_train_conv_data_workspace_floats_ex(arith, c["layer"], c["P"], NB)))
    dx = nan(device, NB, c["cin"], PL)
    w_d, dy_d = dev(c["w"] if w is None else w, device), dev(c["dyp"] if dyp is None else dyp, device)
    _check(lib.os2d_train_conv_backward_data_ex(arith, c["layer"], c["P"], _ptr(w_d), _ptr(dy_d), NB, H, W, _ptr(dx), _ptr(ws), ws.numel(),
                                                _stream(device)), "conv_backward_data_ex")
    return dx.cpu()


def weight_gradient(device, c, shape, room, dyp=None, arith=F16X3):
    lib, (NB, H, W) = _lib(), shape
    n = int(lib.os2d_train_conv_weight_slice_floats_ex(arith, c["layer"], c["P"]))
    ws = nan(device, n * room + (n // 2 if room > 1 else 0))        # room for exactly `room` slices (and a useless half)
    dw = nan(device, *c["w"].shape)
    x, dy = dev(c["xp"], device), dev(c["dyp"] if dyp is None else dyp, device)
    _check(lib.os2d_train_conv_backward_weight_ex(arith, c["layer"], c["P"], _ptr(x), _ptr(dy), NB, H, W, _ptr(dw), _ptr(ws), ws.numel(),
                                                  _stream(device)), "conv_backward_weight_ex")
    return dw.cpu()


@pytest.mark.parametrize("key,shape", CONV_CASES, **IDS)
def test_conv_backward_data(device, key, shape):
    c = conv_case(key, shape)
    got = data_gradient(device, c, shape)
    assert_planes(got, shape[1], shape[2], "dx")
    err = M.rel_err(got, c["dx"])
    report("conv_data", "{} {}".format(key, shape), err)
    assert err < PIN["conv_data"]


@pytest.mark.parametrize("key,shape", CONV_CASES, **IDS)
def test_conv_backward_weight(device, key, shape):
    """Every split-K slice count meets the same tolerance against float64; the same workspace gives the same bits twice."""
    from os2d_amd.modeling.head_train import _wgrad_splits
    c = conv_case(key, shape)
    NB, H, W = shape
    PL = M.plane_geometry(H, W)[2]
    rooms = SPLIT_ROOMS if shape in SPLIT_SHAPES else (2, 64) if shape == (1, 2, 2) else (_wgrad_splits(NB, PL), 2)
    got = {}
    for room in rooms:
        got[room] = weight_gradient(device, c, shape, room)
        assert bool(torch.isfinite(got[room]).all()), "room {}: dw not fully written (or an unwritten slice was added)".format(room)
        err = M.rel_err(got[room], c["dw"])
        report("conv_weight", "{} {} room {}".format(key, shape, room), err)
        assert err < PIN["conv_weight"], room
        assert torch.equal(bits(weight_gradient(device, c, shape, room)), bits(got[room])), "room {}: two calls differ".format(room)
    if 70 in got:
        assert torch.equal(bits(got[70]), bits(got[64])), "more than 64 slices of room must behave as 64"
    if shape == (1, 2, 2):
        assert torch.equal(bits(got[64]), bits(got[2])), "64 positions allow 2 slices of one k-step of 32"


@pytest.mark.parametrize("key", sorted(CONV_LAYERS))
def test_arith_0_through_ex_is_the_old_entry_point(device, key):
    shape = (3, 9, 13)
    c = conv_case(key, shape)
    lib, (NB, H, W) = _lib(), shape
    PL = M.plane_geometry(H, W)[2]
    ws = nan(device, int(lib.os2d_train_conv_data_workspace_floats(c["layer"], c["P"])))
    dx = nan(device, NB, c["cin"], PL)
    w, x, dy = dev(c["w"], device), dev(c["xp"], device), dev(c["dyp"], device)
    _check(lib.os2d_train_conv_backward_data(c["layer"], c["P"], _ptr(w), _ptr(dy), NB, H, W, _ptr(dx), _ptr(ws), ws.numel(), _stream(device)),
           "conv_backward_data")
    assert torch.equal(bits(data_gradient(device, c, shape, arith=0)), bits(dx))
    n = int(lib.os2d_train_conv_weight_slice_floats(c["layer"], c["P"]))
    for room in (1, 3):
        ws = nan(device, n * room + (n // 2 if room > 1 else 0))
        dw = nan(device, *c["w"].shape)
        _check(lib.os2d_train_conv_backward_weight(c["layer"], c["P"], _ptr(x), _ptr(dy), NB, H, W, _ptr(dw), _ptr(ws), ws.numel(),
                                                   _stream(device)), "conv_backward_weight")
        assert torch.equal(bits(weight_gradient(device, c, shape, room, arith=0)), bits(dw)), room


# ---------------------------------------------------------------------------------------------------------- dynamic range, non-finite, zero
def test_small_pair_keeps_its_accuracy_in_the_data_gradient(device):
    """Layer 2, pair 1 of dy 2^-20 of its neighbours: one scale per pair, so each pair's dx is as accurate as on its own."""
    shape = (3, 9, 13)
    c = conv_case("l2", shape)
    dyp = c["dyp"].clone()
    dyp[1] *= 2.0 ** -20
    ref, _ = M.conv_backward_model(c["xp"], c["w"], dyp, shape[1], shape[2])
    got = data_gradient(device, c, shape, dyp=dyp)
    assert_planes(got, shape[1], shape[2], "dx")
    for nb in range(3):
        err = M.rel_err(got[nb], ref[nb])
        report("conv_data", "l2 {} pair {} (pair 1 x 2^-20)".format(shape, nb), err)
        assert err < PIN["conv_data"], nb


def test_one_nan_in_dy_stays_in_its_pair_and_reaches_the_weight_gradient(device):
    shape = (3, 9, 13)
    c = conv_case("l2", shape)
    dyp = c["dyp"].clone()
    cell = int(M.plane_index(shape[1], shape[2])[40])
    dyp[1, 5, cell] = float("nan")
    got = data_gradient(device, c, shape, dyp=dyp)
    assert not bool(torch.isfinite(got[1]).all()), "pair 1 read the NaN"
    assert torch.count_nonzero(got[1][:, ~M.interior_mask(shape[1], shape[2])].nan_to_num(1.0)) == 0, "pad cells stay exact zeros"
    for nb in (0, 2):
        assert bool(torch.isfinite(got[nb]).all()), nb
        err = M.rel_err(got[nb], c["dx"][nb])
        report("conv_data", "l2 {} pair {} (NaN in pair 1)".format(shape, nb), err)
        assert err < PIN["conv_data"], nb
    dw = weight_gradient(device, c, shape, 3, dyp=dyp)
    assert not bool(torch.isfinite(dw).all()), "dw sums over every pair"
    assert not bool(torch.isfinite(dw[5]).any()), "every weight of output channel 5 has the NaN among its addends"


def test_zero_dy_gives_exact_zeros(device):
    shape = (3, 9, 13)
    c = conv_case("l2", shape)
    zero = torch.zeros_like(c["dyp"])
    assert torch.count_nonzero(data_gradient(device, c, shape, dyp=zero)) == 0
    assert torch.count_nonzero(weight_gradient(device, c, shape, 3, dyp=zero)) == 0


# ---------------------------------------------------------------------------------------------------------- correlation
CORR_SHAPES = [(1, 1, 1, 2, 2), (2, 3, 67, 9, 13), (3, 2, 130, 5, 7), (1, 5, 64, 17, 19)]


def corr_inputs(shape):
    """The inputs of test_corr_backward of tests/test_backward_stages_gpu.py: a zero feature vector at (A-1, H-1, 0)."""
    from oracle import head_oracle as O
    A, B, C, H, W = shape
    g = torch.Generator().manual_seed(C + H * W)
    fm = torch.randn(A, C, H, W, generator=g)
    fm[A - 1, :, H - 1, 0] = 0.0
    qp = M.class_operand(O.l2_normalize_channels(torch.randn(B, C, 15, 15, generator=g).double(), 1e-5).float())
    dcorr = torch.randn(A * B, 225, H * W, generator=g)
    return fm, qp, dcorr


def corr_gradients(device, shape, fm, qp, dcorr, want_fm=True, want_q=True, arith=F16X3):
    lib, (A, B, C, H, W) = _lib(), shape
    t = [dev(x, device) for x in (fm, qp, dcorr)]
    ws = nan(device, int(lib.os2d_train_corr_workspace_floats_ex(arith, A, B, C, H, W)))
    dfm, dq = nan(device, A, C, H, W), nan(device, B, C, 225)
    _check(lib.os2d_train_corr_backward_ex(arith, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), A, B, C, H, W, _ptr(dfm) if want_fm else None,
                                           _ptr(dq) if want_q else None, _ptr(ws), ws.numel(), _stream(device)), "corr_backward_ex")
    return dfm.cpu(), dq.cpu()


def corr_errors(shape, dfm, dq, dfm_ref, dq_ref):
    A, B, C, H, W = shape
    zero = (A - 1, H - 1, 0)
    rest = torch.ones(A, H, W, dtype=torch.bool)
    rest[zero] = False
    return {"dfm at the zero vector": M.rel_err(dfm[zero[0], :, zero[1], zero[2]], dfm_ref[zero[0], :, zero[1], zero[2]]),
            "dq": M.rel_err(dq, dq_ref),
            "dfm elsewhere": M.rel_err(dfm.permute(0, 2, 3, 1)[rest], dfm_ref.permute(0, 2, 3, 1)[rest])}


@pytest.mark.parametrize("shape", CORR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_corr_backward(device, shape):
    fm, qp, dcorr = corr_inputs(shape)
    dfm_ref, dq_ref = M.corr_backward_model(fm, qp, dcorr)
    dfm, dq = corr_gradients(device, shape, fm, qp, dcorr)
    assert bool(torch.isfinite(dfm).all()) and bool(torch.isfinite(dq).all())
    errs = corr_errors(shape, dfm, dq, dfm_ref, dq_ref)
    for k, e in errs.items():
        report("corr", "{} {}".format(shape, k), e)
    assert not {k: e for k, e in errs.items() if not e < PIN["corr"]}, errs
    only_fm, untouched_q = corr_gradients(device, shape, fm, qp, dcorr, want_q=False)
    assert torch.equal(bits(only_fm), bits(dfm)) and bool(torch.isnan(untouched_q).all())
    untouched_fm, only_q = corr_gradients(device, shape, fm, qp, dcorr, want_fm=False)
    assert torch.equal(bits(only_q), bits(dq)) and bool(torch.isnan(untouched_fm).all())
    old = corr_gradients(device, shape, fm, qp, dcorr, arith=0)
    lib, (A, B, C, H, W) = _lib(), shape
    t = [dev(x, device) for x in (fm, qp, dcorr)]
    ws = nan(device, int(lib.os2d_train_corr_workspace_floats(A, C, H, W)))
    dfm0, dq0 = nan(device, A, C, H, W), nan(device, B, C, 225)
    _check(lib.os2d_train_corr_backward(_ptr(t[0]), _ptr(t[1]), _ptr(t[2]), A, B, C, H, W, _ptr(dfm0), _ptr(dq0), _ptr(ws), ws.numel(),
                                        _stream(device)), "corr_backward")
    assert torch.equal(bits(old[0]), bits(dfm0)) and torch.equal(bits(old[1]), bits(dq0)), "arith = 0 is the old entry point"


@pytest.mark.parametrize("which", ["image", "class"])
def test_small_slice_of_dcorr_keeps_its_accuracy(device, which):
    """One image's (class's) dcorr 2^-20 of the others: d fm is judged per image, d q per class."""
    shape = (2, 3, 67, 9, 13)
    A, B, C, H, W = shape
    fm, qp, dcorr = corr_inputs(shape)
    dcorr = dcorr.clone().view(A, B, 225, H * W)
    if which == "image":
        dcorr[1] *= 2.0 ** -20
    else:
        dcorr[:, 1] *= 2.0 ** -20
    dcorr = dcorr.view(A * B, 225, H * W)
    dfm_ref, dq_ref = M.corr_backward_model(fm, qp, dcorr)
    dfm, dq = corr_gradients(device, shape, fm, qp, dcorr)
    if which == "image":
        rest = torch.ones(A, H, W, dtype=torch.bool)
        rest[A - 1, H - 1, 0] = False                 # the zero feature vector: its own comparison in test_corr_backward
        errs = {a: M.rel_err(dfm[a].permute(1, 2, 0)[rest[a]], dfm_ref[a].permute(1, 2, 0)[rest[a]]) for a in range(A)}
    else:
        errs = {b: M.rel_err(dq[b], dq_ref[b]) for b in range(B)}
    for k, e in errs.items():
        report("corr", "{} {} {} (slice 1 x 2^-20)".format(shape, which, k), e)
    assert not {k: e for k, e in errs.items() if not e < PIN["corr"]}, errs


# ---------------------------------------------------------------------------------------------------------- through autograd
@pytest.fixture
def f16x3_env(monkeypatch):
    monkeypatch.setenv("OS2D_TRAIN_PRECISION", "f16x3")


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_match_oracle(device, f16x3_env, name):
    """The helpers of tests/test_head_backward_gpu.py build their own creator: its train_precision is None and follows the
    environment."""
    _check_case(device, name, *CASES[name])


def _heads(device, precision, monkeypatch=None):
    state, fm, class_fms, _ = _small(device)
    creator = util.make_head_creator(6, True, state, device)
    assert creator.train_precision is None
    if monkeypatch is not None:
        monkeypatch.setenv("OS2D_TRAIN_PRECISION", precision)
    else:
        creator.train_precision = precision
    head = creator.create_os2d_head([c.to(device).requires_grad_(True) for c in class_fms])
    return head, fm.to(device).requires_grad_(True)


def test_route_is_recorded_and_forward_is_the_f32_training_forward(device):
    head, fm = _heads(device, "f16x3")
    assert head.train_precision == "f16x3" and head.last_train_precision is None
    out = head(fm)
    assert head.last_train_precision == "f16x3" and head.last_precision == "f32"
    ref_head, ref_fm = _heads(device, "f32")
    ref = ref_head(ref_fm)
    assert ref_head.last_train_precision == "f32"
    for a, b in zip(out, ref):
        assert torch.equal(a.detach(), b.detach())
    # the two routes give different gradient bits (the backward really took another kernel) within the end-to-end tolerance
    out[1].sum().backward()
    ref[1].sum().backward()
    assert not torch.equal(fm.grad, ref_fm.grad)
    assert float((fm.grad - ref_fm.grad).abs().max()) < TOL * float(ref_fm.grad.abs().max())


def test_environment_is_honoured_by_a_creator_without_a_setting(device, monkeypatch):
    head, fm = _heads(device, "f16x3", monkeypatch)
    assert head.train_precision is None
    head(fm)
    assert head.last_train_precision == "f16x3"
    head.train_precision = "f32"                      # the head's own attribute overrides it
    head(fm)
    assert head.last_train_precision == "f32"


def test_unknown_train_precision_raises(device, monkeypatch):
    head, fm = _heads(device, "f16x2")
    with pytest.raises(ValueError, match="f16x2"):
        head(fm)
    with torch.no_grad():
        head(fm)                                      # the inference route does not look at it
    head, fm = _heads(device, "bf16", monkeypatch)
    with pytest.raises(ValueError, match="bf16"):
        head(fm)


def test_one_sgd_step_matches_oracle(device, f16x3_env):
    """test_one_sgd_step_matches_oracle of tests/test_head_backward_gpu.py with the f16x3 backward."""
    state, fm, class_fms, (gl, gc, gd) = _small(device, seed=21)
    lr = 0.05
    got, _, creator = hip_grads(device, fm, class_fms, state, 6, True, gl, gc, gd)
    net = creator.aligner.parameter_regressor
    torch.optim.SGD(net.parameters(), lr=lr).step()
    ref = oracle_grads(fm, class_fms, state, True, gl, gc, gd)
    named = dict(net.named_parameters())
    for k in PARAM_KEYS:
        want = state[k] - lr * ref[k]
        moved = named[k].detach().cpu()
        assert float((moved - want).abs().max()) <= lr * TOL * float(ref[k].abs().max()) + 1e-7, k


def test_pointers_that_are_not_16_byte_aligned(device):
    """The C ABI asks for fp32 alignment only: dy, w and the workspace one float off a 16-byte boundary take the loaders' and the
    maxima pass's element-wise forms and give the same bits."""
    shape = (3, 9, 13)
    c = conv_case("l2", shape)
    lib, (NB, H, W) = _lib(), shape
    PL = M.plane_geometry(H, W)[2]

    def off(t):                                   # the same values, one float further
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=device)
        buf[1:] = t.reshape(-1)
        return buf[1:]
    w, x, dy = dev(c["w"], device), dev(c["xp"], device), dev(c["dyp"], device)
    outs = []
    for shift in (False, True):
        w_, x_, dy_ = (off(w), off(x), off(dy)) if shift else (w, x, dy)
        n_ws = int(lib.os2d_train_conv_data_workspace_floats_ex(F16X3, c["layer"], c["P"], NB))
        ws = off(nan(device, n_ws)) if shift else nan(device, n_ws)
        dx = nan(device, NB, c["cin"], PL)
        _check(lib.os2d_train_conv_backward_data_ex(F16X3, c["layer"], c["P"], _ptr(w_), _ptr(dy_), NB, H, W, _ptr(dx), _ptr(ws), ws.numel(),
                                                    _stream(device)), "conv_backward_data_ex")
        n = int(lib.os2d_train_conv_weight_slice_floats_ex(F16X3, c["layer"], c["P"]))
        ws2 = off(nan(device, 3 * n)) if shift else nan(device, 3 * n)
        dw = nan(device, *c["w"].shape)
        _check(lib.os2d_train_conv_backward_weight_ex(F16X3, c["layer"], c["P"], _ptr(x_), _ptr(dy_), NB, H, W, _ptr(dw), _ptr(ws2), ws2.numel(),
                                                      _stream(device)), "conv_backward_weight_ex")
        outs.append((dx.cpu(), dw.cpu()))
    assert M.rel_err(outs[1][0], c["dx"]) < PIN["conv_data"] and M.rel_err(outs[1][1], c["dw"]) < PIN["conv_weight"]
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
