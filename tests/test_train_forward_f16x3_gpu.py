"""GPU: the split-fp16 ("f16x3") training forward of the head (``train_forward_precision``, os2d_amd/modeling/head_train.py) and its
bridge kernel os2d_train_planes_from_shb (include/os2d_train.h, os2d_amd/csrc_train/shb_planes.hip).

  1  the bridge kernel alone, bit for bit against the numpy model of tests/train_forward_f16x3_model.py;
  2  the outputs under autograd have the bits of ``head(fm, precision="f16x3")``; the default switch keeps those of "f32";
  3  the activations the autograd Function saved are the ones the f16x3 stage kernels produced;
  4  gradients against torch autograd of the CPU oracle (helpers and tolerances of tests/test_head_backward_gpu.py);
  5  partial requires_grad and a frozen TransformNet give the ``None`` pattern of the f32 forward;
  6  a non-finite feature reaches the loss; the other image keeps the bits of a clean run;
  7  one SGD step;  8  deterministic=True: two runs, the same bits.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import test_head_backward_gpu as HB
import train_forward_f16x3_model as M
import util

pytestmark = pytest.mark.gpu

PARAM_KEYS, TOL = HB.PARAM_KEYS, HB.TOL


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---------------------------------------------------------------------------------------------- 1: the bridge kernel alone
BRIDGE_SHAPES = [(1, 1, 1, 2, 2), (2, 9, 9, 3, 5), (2, 225, 226, 17, 19), (3, 128, 128, 2, 209), (1, 64, 64, 38, 38)]


def _finite_half_bits(rs, shape):
    """Raw fp16 bit patterns of finite values: every sign, exponent field 0 .. 30 (0: zeros and subnormals), every mantissa."""
    bits = rs.randint(0, 1 << 16, size=shape).astype(np.uint16)
    bad = (bits & 0x7C00) == 0x7C00
    bits[bad] &= np.uint16(0xBFFF)                  # exponent 31 -> 30
    bits[rs.uniform(size=shape) < 0.03] = 0         # exact zeros
    return bits


def _bridge_case(NB, channels, out_channels, H, W):
    rs = np.random.RandomState(NB * 1000 + channels + H * 7 + W)
    G, PL = M.groups(channels), M.plane(H, W)
    bits = _finite_half_bits(rs, (NB, G, 2, PL, 8))
    lo = bits[:, :, 1]
    small = rs.uniform(size=lo.shape) < 0.25
    lo[small] &= np.uint16(0x83FF)                  # a quarter of the lo halves subnormal (or zero)
    assert (bits[:, :, 0] & 0x8000).any() and (lo & 0x7C00 == 0).any()      # negative hi parts, subnormal lo parts
    # what the kernel must not look at: every pad cell, every padded channel of the last group
    bits[:, :, :, ~M.interior_mask(H, W), :] = 0xFFFF
    if channels % 8:
        bits[:, G - 1, :, :, channels % 8:] = 0xFFFF
    exp = rs.randint(-20, 31, size=channels).astype(np.int32)
    exp[channels // 2] = 0
    return bits, exp


@pytest.mark.parametrize("NB,channels,out_channels,H,W", BRIDGE_SHAPES)
def test_planes_from_shb_matches_the_model_bit_for_bit(device, NB, channels, out_channels, H, W):
    from os2d_amd import _lib, _train_lib
    tl = _train_lib.load()
    PL = int(_lib.load().os2d_plane_floats(H, W))
    assert PL == M.plane(H, W) and int(_lib.load().os2d_shb_bytes(channels, H, W)) == M.groups(channels) * 2 * PL * 16
    bits, exp = _bridge_case(NB, channels, out_channels, H, W)
    want = M.unpack(bits.view(np.float16), exp, channels, out_channels, H, W, np.float32)
    shb = torch.from_numpy(bits.view(np.uint8).reshape(-1)).to(device)
    exp_d = torch.from_numpy(exp).to(device)
    results = []
    for _ in range(2):
        out = torch.full((NB, out_channels, PL), float("nan"), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _train_lib.check(tl.os2d_train_planes_from_shb(_ptr(shb), _ptr(exp_d), NB, channels, out_channels, H, W, _ptr(out),
                                                           _stream(device)), "os2d_train_planes_from_shb")
        results.append(out.cpu().numpy())
    got = results[0]
    mask = M.interior_mask(H, W)
    assert np.array_equal(got[:, :channels][:, :, mask].view(np.uint32), want[:, :channels][:, :, mask].view(np.uint32))
    assert not got.view(np.uint32)[:, :, ~mask].any(), "a pad cell is not +0.0"
    assert not got.view(np.uint32)[:, channels:].any(), "an extra plane is not +0.0"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(results[1].view(np.uint32), got.view(np.uint32)), "a second call gives other bits"


def test_planes_from_shb_refuses_bad_arguments_and_launches_nothing(device):
    from os2d_amd import _train_lib
    tl = _train_lib.load()
    NB, channels, H, W = 2, 9, 3, 5
    PL = M.plane(H, W)
    bits, exp = _bridge_case(NB, channels, channels, H, W)
    shb = torch.from_numpy(bits.view(np.uint8).reshape(-1)).to(device)
    exp_d = torch.from_numpy(exp).to(device)
    out = torch.full((NB, channels, PL), float("nan"), dtype=torch.float32, device=device)

    def call(shb_=shb, exp_=exp_d, channels_=channels, out_channels_=channels, H_=H, out_=out):
        with torch.cuda.device(device):
            return tl.os2d_train_planes_from_shb(None if shb_ is None else _ptr(shb_), None if exp_ is None else _ptr(exp_), NB, channels_,
                                                 out_channels_, H_, W, None if out_ is None else _ptr(out_), _stream(device))

    for kw in (dict(shb_=None), dict(exp_=None), dict(out_=None), dict(out_channels_=channels - 1), dict(H_=0)):
        assert call(**kw) == -1, kw
        assert b"os2d_train_planes_from_shb" in tl.os2d_train_last_error()
    torch.cuda.synchronize(device)
    assert bool(torch.isnan(out).all()), "a refused call wrote to its output"


# ---------------------------------------------------------------------------------------------- the head under autograd
def _make(device, state, fm, class_fms, P, inverse, forward="f16x3", backward=None, deterministic=None, grad_fm=True, grad_class=True):
    creator = util.make_head_creator(P, inverse, state, device)
    creator.train_forward_precision, creator.train_precision, creator.deterministic = forward, backward, deterministic
    raws = [c.to(device).requires_grad_(grad_class) for c in class_fms]
    head = creator.create_os2d_head(raws)
    return creator, head, fm.to(device).requires_grad_(grad_fm), raws


def _grads(device, state, fm, class_fms, P, inverse, gl, gc, gd, **kw):
    """tests/test_head_backward_gpu.py: hip_grads, with the three switches of the creator."""
    creator, head, fm_d, raws = _make(device, state, fm, class_fms, P, inverse, **kw)
    net = creator.aligner.parameter_regressor
    loc, cls, cls_det, corners = head(fm_d)
    assert head.last_train_forward_precision == head.last_precision == kw.get("forward", "f16x3")
    loss = (loc.double() * gl.to(device)).sum() + (cls.double() * gc.to(device)).sum() + (cls_det.double() * gd.to(device)).sum()
    loss.backward()
    named = dict(net.named_parameters())
    out = {"fm": fm_d.grad.cpu(), "class": [r.grad.cpu() for r in raws]}
    out.update({k: named[k].grad.cpu() for k in PARAM_KEYS})
    return out, creator


def _case_inputs(name, seed=0):
    from os2d_amd.utils import synthetic
    P, inverse, A, C, H, W, sizes, B = HB.CASES[name]
    state = synthetic.make_transform_net_state(P, seed=seed + 3)
    fm = synthetic.make_feature_map(C, H, W, seed=seed + 5, A=A)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=sizes, seed=seed + 400)
    return state, fm, class_fms, HB.upstream(A, B, H, W, seed + 7)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The CPU oracle's gradients of a case of tests/test_head_backward_gpu.py: computed once, shared, never written."""
    state, fm, class_fms, (gl, gc, gd) = _case_inputs(name)
    return HB.oracle_grads(fm, class_fms, state, HB.CASES[name][1], gl, gc, gd)


def _errors(got, ref, B):
    pairs = {"fm": (got["fm"], ref["fm"])}
    pairs.update({"class{}".format(b): (got["class"][b], ref["class"][b]) for b in range(B)})
    pairs.update({k: (got[k], ref[k]) for k in PARAM_KEYS})
    return pairs, {k: HB.rel_err(*v) for k, v in pairs.items()}


# ---- 2: forward bits
@pytest.mark.parametrize("name", ["v2_affine_inverse", "odd_c67_9x13", "simple_affine_p4"])
def test_forward_has_the_bits_of_f16x3_inference(device, name):
    state, fm, class_fms, _ = _case_inputs(name)
    P, inverse = HB.CASES[name][:2]
    _, head, fm_d, _ = _make(device, state, fm, class_fms, P, inverse)
    with torch.no_grad():
        ref = head(fm_d.detach(), precision="f16x3")
    assert head.last_precision == "f16x3" and head.last_train_forward_precision is None
    out = head(fm_d)
    assert head.last_precision == "f16x3" and head.last_train_forward_precision == "f16x3" and head.last_train_precision == "f32"
    assert out[0].requires_grad and out[1].requires_grad and out[2].requires_grad and not out[3].requires_grad
    for i, what in ((0, "loc"), (1, "cls"), (3, "corners")):
        assert torch.equal(out[i].detach(), ref[i]), what
    assert out[2] is not out[1] and torch.equal(out[2].detach(), ref[1])
    assert head.range_status(synchronize=True) == 0
    # the default switch: today's route, the bits of precision="f32"
    _, head32, fm32, _ = _make(device, state, fm, class_fms, P, inverse, forward=None)
    with torch.no_grad():
        ref32 = head32(fm32.detach(), precision="f32")
    out32 = head32(fm32)
    assert head32.last_precision == "f32" and head32.last_train_forward_precision == "f32"
    for i in (0, 1, 3):
        assert torch.equal(out32[i].detach(), ref32[i]), i
    assert not torch.equal(out32[0].detach(), ref[0])          # (the two routes do differ: the test above is not vacuous)


def test_switch_resolution_on_the_head(device, monkeypatch):
    state, fm, class_fms, _ = _case_inputs("v2_affine_inverse")
    monkeypatch.delenv("OS2D_TRAIN_FORWARD_PRECISION", raising=False)
    creator, head, fm_d, _ = _make(device, state, fm, class_fms, 6, True, forward=None, backward="f16x3")
    assert creator.train_forward_precision is None and head.train_forward_precision is None
    head(fm_d)
    assert (head.last_train_forward_precision, head.last_precision, head.last_train_precision) == ("f32", "f32", "f16x3")
    monkeypatch.setenv("OS2D_TRAIN_FORWARD_PRECISION", "f16x3")
    head(fm_d)
    assert (head.last_train_forward_precision, head.last_precision, head.last_train_precision) == ("f16x3", "f16x3", "f16x3")
    head.train_forward_precision = "f32"                       # the head's own attribute overrides the environment
    head(fm_d)
    assert head.last_train_forward_precision == "f32"
    head.train_forward_precision = "fftx3"
    with pytest.raises(ValueError, match="train_forward_precision"):
        head(fm_d)
    with torch.no_grad():                                     # not the training route: the switch is not looked at
        head(fm_d)
    head.train_forward_precision = "f16x3"
    with pytest.raises(RuntimeError, match="209"):
        head(torch.rand(1, 64, 4, 210, device=device, requires_grad=True))


# ---- 3: the saved activations
def test_saved_activations_are_what_the_stage_kernels_produced(device):
    from os2d_amd import _lib
    lib = _lib.load()
    state, fm, class_fms, _ = _case_inputs("v2_affine_inverse")
    P, inverse, A, C, H, W, _, B = HB.CASES["v2_affine_inverse"]
    NB, PL = A * B, M.plane(H, W)
    creator, head, fm_d, _ = _make(device, state, fm, class_fms, P, inverse)
    head.keep_train_activations = True
    out = head(fm_d)
    saved = head.last_train_activations
    assert sorted(saved) == ["corr", "h1", "h2", "params", "rnorm"]
    net = creator.aligner.parameter_regressor
    w1, b1, w2, b2, w3, b3 = net.packed("f16x3")
    plan = net.range_plan()
    exps = [plan["in_exp"][0].cpu().numpy(), plan["out_exp"][0].cpu().numpy(), plan["out_exp"][1].cpu().numpy()]
    assert all(torch.equal(e.cpu(), torch.from_numpy(x)) for e, x in zip(net.activation_exponents(), exps))
    u8 = dict(dtype=torch.uint8, device=device)
    fm0 = fm_d.detach()
    with torch.cuda.device(device):
        s = _stream(device)
        qs = head._split_class_operand()
        ws = torch.empty(int(lib.os2d_corr_f16x3_workspace_bytes(A, C, H, W)), **u8)
        corr = torch.empty(NB, 225, H * W, dtype=torch.float32, device=device)
        bufs = [torch.empty(NB * int(lib.os2d_shb_bytes(c, H, W)), **u8) for c in (225, 128, 64)]
        params = torch.empty(NB, P, H * W, dtype=torch.float32, device=device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.check(lib.os2d_corr_f16x3(_ptr(fm0), _ptr(qs), _ptr(corr), _ptr(bufs[0]), A, B, C, H, W, _ptr(ws), ws.numel(), s), "corr")
        for layer, src, wp, bp, dst in ((1, bufs[0], w1, b1, bufs[1]), (2, bufs[1], w2, b2, bufs[2]), (3, bufs[2], w3, b3, params)):
            _lib.check(lib.os2d_transform_conv_f16x3(layer, _ptr(src), _ptr(wp), _ptr(bp), _ptr(dst), NB, P, H, W, 3, _ptr(status), s), "conv")
    assert int(status.item()) == 0
    assert torch.equal(saved["corr"], corr) and torch.equal(saved["params"], params)
    for key, buf, exp, channels, out_channels in (("rnorm", bufs[0], exps[0], 225, 226), ("h1", bufs[1], exps[1], 128, 128),
                                                  ("h2", bufs[2], exps[2], 64, 64)):
        shb = buf.cpu().numpy().view(np.float16).reshape(NB, M.groups(channels), 2, PL, 8)
        want = M.unpack(shb, exp, channels, out_channels, H, W, np.float32)
        got = saved[key].cpu().numpy().reshape(NB, out_channels, PL)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), key
        assert np.abs(want).max() > 0, key
        # exact: the float64 sum of the two halves is the fp32 value
        assert np.array_equal(got.astype(np.float64), M.unpack(shb, exp, channels, out_channels, H, W, np.float64)), key
    del out


# ---- 4: gradients against the CPU oracle
@pytest.mark.parametrize("backward,deterministic", [("f32", False), ("f16x3", False), ("f16x3", True)])
@pytest.mark.parametrize("name", sorted(HB.CASES))
def test_gradients_match_oracle(device, name, backward, deterministic):
    state, fm, class_fms, (gl, gc, gd) = _case_inputs(name)
    P, inverse = HB.CASES[name][:2]
    B = HB.CASES[name][7]
    got, _ = _grads(device, state, fm, class_fms, P, inverse, gl, gc, gd, backward=backward, deterministic=deterministic)
    _, errs = _errors(got, _oracle(name), B)
    print(name, "forward f16x3, backward", backward, "deterministic" if deterministic else "", "relative max errors:",
          {k: "{:.2e}".format(v) for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


def test_gradients_match_oracle_training_shape(device):
    """Reference training crops (2 images x 15 classes x 1024 channels x 38 x 38), f16x3 forward and f16x3 backward, at the pins of
    tests/test_head_backward_gpu.py: test_gradients_match_oracle_training_shape."""
    from os2d_amd.utils import synthetic
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    P, inverse, A, C, H, W, B, seed = 6, True, 2, 1024, 38, 38, 15, 11
    state = synthetic.make_transform_net_state(P, seed=seed + 3)
    fm = synthetic.make_feature_map(C, H, W, seed=seed + 5, A=A)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=[(15, 15), (20, 24), (13, 17)], seed=seed + 400)
    gl, gc, gd = HB.upstream(A, B, H, W, seed + 7)
    ref = HB.oracle_grads(fm, class_fms, state, inverse, gl, gc, gd)
    got, _ = _grads(device, state, fm, class_fms, P, inverse, gl, gc, gd, backward="f16x3")
    pairs, errs = _errors(got, ref, B)
    nerrs = {k: HB.rel_norm_err(*v) for k, v in pairs.items()}
    print("training_shape forward f16x3, backward f16x3 relative max errors:", {k: "{:.2e}".format(v) for k, v in errs.items()})
    print("training_shape forward f16x3, backward f16x3 relative norm errors:", {k: "{:.2e}".format(v) for k, v in nerrs.items()})
    bad = {k: v for k, v in errs.items() if not v < HB.TOL_TRAIN_MAX}
    assert not bad, bad
    bad = {k: v for k, v in nerrs.items() if not v < HB.TOL_TRAIN_NORM}
    assert not bad, bad
    assert sum(errs["class{}".format(b)] < TOL for b in range(B)) >= 8


# ---- 5: partial requires_grad, frozen TransformNet
def _none_pattern(device, forward, mode):
    from os2d_amd.modeling.model import Os2dModel
    state, fm, class_fms, (gl, gc, gd) = _case_inputs("v2_affine_inverse")
    creator, head, fm_d, raws = _make(device, state, fm, class_fms, 6, True, forward=forward, grad_fm=mode != "bias",
                                      grad_class=mode == "frozen")
    net = creator.aligner.parameter_regressor
    if mode == "frozen":
        Os2dModel.freeze_transform_params(types.SimpleNamespace(_transform_net=lambda: net))
    else:
        net.requires_grad_(False)
    if mode == "bias":
        net.linear.bias.requires_grad_(True)
    loc, cls, cls_det, _ = head(fm_d)
    assert head.last_precision == forward
    ((loc.double() * gl.to(device)).sum() + (cls.double() * gc.to(device)).sum() + (cls_det.double() * gd.to(device)).sum()).backward()
    named = dict(net.named_parameters())
    grads = {"fm": fm_d.grad}
    grads.update({"class{}".format(b): r.grad for b, r in enumerate(raws)})
    grads.update({k: named[k].grad for k in PARAM_KEYS})
    return grads


@pytest.mark.parametrize("mode", ["fm", "bias", "frozen"])
def test_partial_requires_grad_gives_the_same_none_pattern(device, mode):
    got, ref = _none_pattern(device, "f16x3", mode), _none_pattern(device, "f32", mode)
    assert {k for k, v in got.items() if v is None} == {k for k, v in ref.items() if v is None}
    present = {k for k, v in got.items() if v is not None}
    assert present == {"fm": {"fm"}, "bias": {"linear.bias"}, "frozen": {"fm", "class0", "class1", "class2"}}[mode]
    for k in present:
        assert got[k].shape == ref[k].shape and bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0, k


# ---- 6: non-finite input
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_feature_reaches_the_loss_and_spares_the_other_image(device, bad):
    state, fm, class_fms, _ = _case_inputs("v2_affine_inverse")
    _, head, fm_d, _ = _make(device, state, fm, class_fms, 6, True)
    clean = [t.detach().clone() for t in head(fm_d)]
    dirty_fm = fm.clone()
    dirty_fm[1, 5, 4, 6] = bad
    _, head2, fm2, _ = _make(device, state, dirty_fm, class_fms, 6, True)
    loc, cls, cls_det, corners = head2(fm2)
    assert head2.last_precision == "f16x3"
    assert not bool(torch.isfinite(cls[1]).all())
    loss = loc.sum() + cls.sum() + cls_det.sum()
    assert not bool(torch.isfinite(loss))
    for got, want, what in ((loc, clean[0], "loc"), (cls, clean[1], "cls"), (cls_det, clean[2], "cls_det"), (corners, clean[3], "corners")):
        assert torch.equal(got[0].detach(), want[0]), what


# ---- 7: one SGD step
def test_one_sgd_step_matches_oracle(device):
    """tests/test_head_backward_gpu.py: test_one_sgd_step_matches_oracle, on the f16x3 forward."""
    state, fm, class_fms, (gl, gc, gd) = HB._small(device, seed=21)
    lr = 0.05
    _, creator = _grads(device, state, fm, class_fms, 6, True, gl, gc, gd)
    net = creator.aligner.parameter_regressor
    torch.optim.SGD(net.parameters(), lr=lr).step()
    ref = HB.oracle_grads(fm, class_fms, state, True, gl, gc, gd)
    named = dict(net.named_parameters())
    for k in PARAM_KEYS:
        want = state[k] - lr * ref[k]
        moved = named[k].detach().cpu()
        assert float((moved - want).abs().max()) <= lr * TOL * float(ref[k].abs().max()) + 1e-7, k


# ---- 8: deterministic
@pytest.mark.parametrize("backward", ["f32", "f16x3"])
def test_deterministic_runs_give_the_same_bits(device, backward):
    state, fm, class_fms, (gl, gc, gd) = _case_inputs("v2_affine_inverse")
    runs = [_grads(device, state, fm, class_fms, 6, True, gl, gc, gd, backward=backward, deterministic=True)[0] for _ in range(2)]
    assert torch.equal(runs[0]["fm"], runs[1]["fm"])
    for a, b in zip(runs[0]["class"], runs[1]["class"]):
        assert torch.equal(a, b)
    for k in PARAM_KEYS:
        assert torch.equal(runs[0][k], runs[1][k]), k
