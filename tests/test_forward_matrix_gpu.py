"""GPU: the forward MATRIX kernels of libos2d_hip.so (include/os2d_hip.h) on their own - the three correlation entry points and
the inference convolutions of the TransformNet with their weight packing, fp32 and split-fp16 - called through os2d_amd/_lib.py
with tensors built on the host, against the float64 model of the same stage (tests/forward_matrix_model.py) at the edge shapes
of its case tables.  The head tests reach these kernels at the fixtures' shapes and under end-to-end tolerances only.
Counterpart of tests/test_forward_stages_gpu.py and tests/test_backward_stages_gpu.py, with their rules:

  * an output the header calls "written" is pre-filled with NaN (0xFF bytes for byte buffers: NaN as fp16 too), and so is
    every workspace;
  * every element must come back finite, every cell that is not a data cell exactly 0: plane borders and pad columns, the
    226th plane of rnorm, the channels 225..231 of the last SHB group; nothing is written past a compact output;
  * errors are computed against the float64 model, never against another run of a kernel;
  * bit-exact claims (the forms of the packed correlation, batch against slices, a second call, the two work-group shapes of the
    split-fp16 layers) are ``torch.equal`` on integer views;
  * a layer's input is built on the host: no test depends on another kernel's output.
"""
import ctypes

import pytest
import torch

import backward_model as M
import forward_matrix_model as FX
import freq_util

pytestmark = pytest.mark.gpu

F32 = torch.float32
GUARD = 64                           # NaN floats behind a compact output: nothing may be written there

# Pins: 3x the largest error measured on the MI355X over the cases of this file (measured value and its case in the comment; the
# table is in DESIGN.md section 10).  CEILINGS a pin may not exceed:
#   corr_*, rnorm_*   max |got - ref| of values <= 1: 2e-6, the bound of the correlation tests of tests/test_head_gpu.py
#   inv_norm_packed   max |got - ref| / ref: 3e-6, the bound of test_packed_correlation_stage_matches_reference
#   conv3_*           max |got - ref| of the transform parameters: 1e-5, the bound of test_transformation_net_stage_kernels
#   conv1_*, conv2_*  |got - ref|_max / |ref|_max: the forward bound of an fp32 accumulation of the case, computed from the model
#                     (forward_matrix_model.conv_error_ceiling; the smallest over the cases is 7.2e-4 for the 7x7 layer and 2.1e-4
#                     for the 5x5 layer) - checked per case in check_pins
CEILING = {"corr_f32": 2e-6, "rnorm_f32": 2e-6, "corr_f16x3": 2e-6, "rnorm_f16x3": 2e-6, "corr_packed": 2e-6, "inv_norm_packed": 3e-6,
           "conv3_f32": 1e-5, "conv3_f16x3": 1e-5}
PIN = {
    "corr_f32": 1.4e-6,           # measured 4.52e-7 (A1_B2_C67_1x257)
    "rnorm_f32": 3.9e-7,          # measured 1.29e-7 (A1_B2_C67_1x257)
    "corr_f16x3": 9.1e-7,         # measured 3.02e-7 (A1_B2_C67_1x257)
    "rnorm_f16x3": 3.3e-7,        # measured 1.10e-7 (A1_B2_C67_1x257)
    "corr_packed": 9.1e-7,        # measured 3.02e-7 (A1_B2_C67_1x257): the bits of corr_f16x3
    "inv_norm_packed": 7.8e-7,    # measured 2.60e-7 (A1_B97_C16_13x20)
    "conv1_f32": 6.3e-6,          # measured 2.09e-6 (adversarial 16x13)
    "conv2_f32": 1.5e-6,          # measured 5.12e-7 (adversarial 17x13)
    "conv3_f32": 3.7e-7,          # measured 1.25e-7 (edited 17x13, P = 6)
    "conv1_f16x3": 4.9e-6,        # measured 1.62e-6 (adversarial 16x13)
    "conv1_f16x2": 4.8e-4,        # measured 1.60e-4 (adversarial 8x13): the 7x7 weights as fp16 roundings
    "conv2_f16x3": 1.7e-6,        # measured 5.62e-7 (adversarial 17x13)
    "conv3_f16x3": 4.3e-7,        # measured 1.42e-7 (edited 17x13, P = 6)
}


def _L():
    from os2d_amd import _lib
    return _lib


def _call(name, *args):
    L = _L()
    L.check(getattr(L.load(), name)(*args), name)


def _ptr(t):
    return _L().ptr(t)


def _stream(device):
    return _L().current_stream(device)


def dev(t, device):
    return t.detach().to(F32).contiguous().to(device)


def nan(device, *shape):
    return torch.full(shape, float("nan"), dtype=F32, device=device)


def ff_bytes(device, n):
    return torch.full((int(n),), 0xFF, dtype=torch.uint8, device=device)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def report(stage, case, err):
    print("\nSTAGE {:<16s} {:<44s} {:.3e}".format(stage, case, err))


def check_pins(*items):
    """items: (stage, {case: error}[, {case: the case's own ceiling}]); without the third, CEILING[stage] (the convolution
    layers 1 and 2 have a ceiling per case).  Every line is printed before anything is asserted."""
    for stage, errs, *_ in items:
        for case, e in errs.items():
            report(stage, case, e)
    for stage, errs, *rest in items:
        for case in errs:
            ceiling = rest[0][case] if rest and rest[0] is not None else CEILING[stage]
            assert PIN[stage] <= ceiling, (stage, case, ceiling)
        bad = {k: e for k, e in errs.items() if not e < PIN[stage]}
        assert not bad, (stage, bad)


def maxabs(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max())


# ---------------------------------------------------------------------------------------------------------- correlation
def corr_operands(case, device):
    fm, q_hat = FX.corr_inputs(case)
    qp = M.class_operand(q_hat)
    return dev(fm, device), qp, dev(qp, device)


def split_operand(case, qp, device):
    A, B, C, H, W = case
    qs = FX.class_split_encode(qp)
    assert qs.numel() == int(_L().load().os2d_class_split_bytes(B, C))
    return qs.to(device)


def assert_corr_edges(case, corr, normalised=None, inv=None):
    """The zero feature vector: exact zeros for every class.  The dead column: normalised values exactly 0, inv_norm within
    rounding of 1 / 1e-6 (1e-6f is off by 2^-25 relative at most, the division rounds once)."""
    A, B, C, H, W = case
    a0, n0 = FX.corr_zero_at(case)
    assert torch.count_nonzero(corr.reshape(A, B, FX.K, H * W)[a0, :, :, n0]) == 0, "0 . q is not exactly 0"
    a1, b1, n1 = FX.corr_dead_at(case)
    assert float(corr[a1 * B + b1, :, n1].max()) < 0
    if normalised is not None:
        assert torch.count_nonzero(normalised[a1 * B + b1, :, n1]) == 0, "relu(negative) * inv_norm is not exactly 0"
        assert torch.count_nonzero(normalised.reshape(A, B, FX.K, H * W)[a0, :, :, n0]) == 0
    if inv is not None:
        for nb, n in [(a1 * B + b1, n1)] + [(a0 * B + b, n0) for b in range(B)]:
            assert abs(float(inv[nb, n]) - 1e6) <= 1e6 * 2.0 ** -22, (nb, n, float(inv[nb, n]))


@pytest.mark.parametrize("case", FX.CORR_CASES, ids=FX.corr_case_id)
def test_corr_f32(device, case):
    """os2d_fm_sumsq + os2d_corr into dirty buffers: the call zeroes the borders and the 226th plane of rnorm itself."""
    lib, (A, B, C, H, W) = _L().load(), case
    NB, HW, PL = A * B, H * W, int(lib.os2d_plane_floats(H, W))
    assert PL == M.plane_geometry(H, W)[2]
    fm_d, _, qp_d = corr_operands(case, device)
    ref_corr, ref_rn, _ = FX.corr_reference(case)
    sumsq, corr, rnorm = nan(device, A, HW), nan(device, NB, FX.K, HW), nan(device, NB, FX.K + 1, PL)
    _call("os2d_fm_sumsq", _ptr(fm_d), _ptr(sumsq), A, C, H, W, _stream(device))
    _call("os2d_corr", _ptr(fm_d), _ptr(qp_d), _ptr(sumsq), _ptr(corr), _ptr(rnorm), A, B, C, H, W, _stream(device))
    corr, rnorm = corr.cpu(), rnorm.cpu()
    assert bool(torch.isfinite(corr).all()) and bool(torch.isfinite(rnorm).all()), "not every element was written"
    assert torch.count_nonzero(rnorm[:, :, ~M.interior_mask(H, W)]) == 0, "non-zero border cell"
    assert torch.count_nonzero(rnorm[:, FX.K]) == 0, "the 226th plane"
    inner = M.unpack_planes(rnorm[:, :FX.K], H, W).reshape(NB, FX.K, HW)
    assert_corr_edges(case, corr, inner)
    name = FX.corr_case_id(case)
    check_pins(("corr_f32", {name: maxabs(corr, ref_corr)}), ("rnorm_f32", {name: maxabs(inner, ref_rn)}))


def run_corr_f16x3(case, fm_d, qs_d, device):
    lib, (A, B, C, H, W) = _L().load(), case
    NB, HW = A * B, H * W
    ws = ff_bytes(device, lib.os2d_corr_f16x3_workspace_bytes(A, C, H, W))
    corr = nan(device, NB, FX.K, HW)
    rshb = ff_bytes(device, NB * int(lib.os2d_shb_bytes(FX.K, H, W)))
    _call("os2d_corr_f16x3", _ptr(fm_d), _ptr(qs_d), _ptr(corr), _ptr(rshb), A, B, C, H, W, _ptr(ws), ws.numel(), _stream(device))
    return corr.cpu(), rshb.cpu()


@pytest.mark.parametrize("case", FX.CORR_CASES, ids=FX.corr_case_id)
def test_corr_f16x3(device, case):
    """os2d_corr_f16x3 with the class operand split on the host: corr and the split-half blocked normalised tensor
    [NB][29][hi|lo][PLANE][8] halves at 2^-os2d_rnorm_exp(); borders and the channels 225..231 of the last group exactly 0."""
    lib, (A, B, C, H, W) = _L().load(), case
    NB, HW = A * B, H * W
    assert int(lib.os2d_rnorm_exp()) == FX.SPLIT_EXP
    assert int(lib.os2d_shb_bytes(FX.K, H, W)) == 29 * 2 * M.plane_geometry(H, W)[2] * 16
    fm_d, qp, _ = corr_operands(case, device)
    ref_corr, ref_rn, _ = FX.corr_reference(case)
    corr, rshb = run_corr_f16x3(case, fm_d, split_operand(case, qp, device), device)
    assert bool(torch.isfinite(corr).all()), "not every element of corr was written"
    assert bool(torch.isfinite(rshb.view(torch.float16)).all()), "not every half was written"
    values, outside = freq_util.shb_decode(rshb, NB, 232, H, W)
    assert outside == 0.0, "non-zero border unit"
    assert torch.count_nonzero(values[:, FX.K:]) == 0, "channels 225..231 of the last group"
    inner = (values[:, :FX.K] * 2.0 ** -FX.SPLIT_EXP).reshape(NB, FX.K, HW)
    assert_corr_edges(case, corr, inner)
    name = FX.corr_case_id(case)
    check_pins(("corr_f16x3", {name: maxabs(corr, ref_corr)}), ("rnorm_f16x3", {name: maxabs(inner, ref_rn)}))


def run_corr_packed(case, fm_d, qs_d, form, device):
    lib, (A, B, C, H, W) = _L().load(), case
    ws = ff_bytes(device, lib.os2d_corr_f16x3_packed_workspace_bytes(A, B, C, H, W))
    corr, inv = nan(device, A * B, FX.K, H * W), nan(device, A * B, H * W)
    _call("os2d_corr_f16x3_packed", _ptr(fm_d), _ptr(qs_d), _ptr(corr), _ptr(inv), A, B, C, H, W, form, _ptr(ws), ws.numel(),
          _stream(device))
    return corr.cpu(), inv.cpu()


@pytest.mark.parametrize("case", FX.CORR_CASES, ids=FX.corr_case_id)
def test_corr_f16x3_packed(device, case):
    """os2d_corr_f16x3_packed: the packed form against the model; the padded form, both without half tiles and the head's own
    choice give the same bits, and the correlation values are those of os2d_corr_f16x3 - at the edge shapes, where a
    work-group of the packed form holds the rows of several classes (B = 9) or mostly padding (B = 1)."""
    A, B, C, H, W = case
    fm_d, qp, _ = corr_operands(case, device)
    qs_d = split_operand(case, qp, device)
    ref_corr, _, ref_inv = FX.corr_reference(case)
    corr, inv = run_corr_packed(case, fm_d, qs_d, 1, device)
    assert bool(torch.isfinite(corr).all()) and bool(torch.isfinite(inv).all()), "not every element was written"
    assert_corr_edges(case, corr, None, inv)
    name = FX.corr_case_id(case)
    check_pins(("corr_packed", {name: maxabs(corr, ref_corr)}),
               ("inv_norm_packed", {name: float(((inv.double() - ref_inv).abs() / ref_inv).max())}))
    for form in (0, 4, 5, -1):
        c2, i2 = run_corr_packed(case, fm_d, qs_d, form, device)
        assert torch.equal(bits(c2), bits(corr)) and torch.equal(bits(i2), bits(inv)), form
    assert torch.equal(bits(run_corr_f16x3(case, fm_d, qs_d, device)[0]), bits(corr)), "os2d_corr_f16x3 gives other correlation bits"


# ---------------------------------------------------------------------------------------------------------- convolutions
_PACKED = {}


def _bn_tensors(layer, state, device):
    conv, bn = FX.LAYER_KEYS[layer]
    w, b = dev(state[conv + ".weight"], device), dev(state[conv + ".bias"], device)
    bnp = [None] * 4 if bn is None else [dev(state[bn + k], device) for k in (".weight", ".bias", ".running_mean", ".running_var")]
    return w, b, bnp


def packed_f32(layer, kind, P, device):
    """os2d_pack_conv of the state's layer into NaN-prefilled buffers: every weight and the MT folded biases are written."""
    key = ("f32", layer, kind, P)
    if key not in _PACKED:
        lib = _L().load()
        w, b, bnp = _bn_tensors(layer, FX.conv_state(kind, P), device)
        pw, pb = nan(device, int(lib.os2d_packed_conv_floats(layer))), nan(device, int(lib.os2d_packed_bias_floats(layer)))
        _call("os2d_pack_conv", layer, P, _ptr(w), _ptr(b), *[_ptr(t) for t in bnp], ctypes.c_float(FX.O.BN_EPS), _ptr(pw), _ptr(pb),
              _stream(device))
        assert bool(torch.isfinite(pw).all()) and bool(torch.isfinite(pb[:pb.numel() // 3]).all()), "not every packed value was written"
        _PACKED[key] = (pw, pb)
    return _PACKED[key]


def packed_f16x3(layer, kind, P, device):
    """os2d_pack_conv_f16x3 with the exponents of ``range_plan``: (packed weights, packed bias, in_exp, out_exp | None)."""
    key = ("f16x3", layer, kind, P)
    if key not in _PACKED:
        lib = _L().load()
        plan = FX.conv_net(kind, P).range_plan()
        e_w, e_in, e_out = [plan[k][layer - 1] for k in ("weight_exp", "in_exp", "out_exp")]
        exps = [None if e is None else e.to(torch.int32).contiguous().to(device) for e in (e_w, e_in, e_out)]
        w, b, bnp = _bn_tensors(layer, FX.conv_state(kind, P), device)
        pw, pb = ff_bytes(device, lib.os2d_packed_conv_bytes(layer, 1)), nan(device, int(lib.os2d_packed_bias_floats(layer)))
        _call("os2d_pack_conv_f16x3", layer, P, _ptr(w), _ptr(b), *[_ptr(t) for t in bnp], ctypes.c_float(FX.O.BN_EPS),
              *[_ptr(e) for e in exps], _ptr(pw), _ptr(pb), _stream(device))
        assert bool(torch.isfinite(pw.cpu().view(torch.float16)).all()) and bool(torch.isfinite(pb).all()), "not every packed value was written"
        _PACKED[key] = (pw, pb, e_in, e_out)
    return _PACKED[key]


def conv_case_id(layer, kind, shape, P=6):
    return "{} {} NB={}{}".format(kind, FX.shape_id(shape), FX.CONV_NB, " P={}".format(P) if layer == 3 else "")


def run_conv_f32(layer, packed, xin, NB, P, H, W, device):
    """One os2d_transform_conv call into a NaN-prefilled output: planes [NB,Cout,PLANE], or [NB*P*H*W + GUARD] for layer 3."""
    PL = M.plane_geometry(H, W)[2]
    out = nan(device, NB * P * H * W + GUARD) if layer == 3 else nan(device, NB, FX.LAYER_CHANNELS[layer][1], PL)
    _call("os2d_transform_conv", layer, _ptr(xin), _ptr(packed[0]), _ptr(packed[1]), _ptr(out), NB, P, H, W, _stream(device))
    return out.cpu()


def check_compact(out, NB, P, H, W):
    """Layer 3: [NB,P,H*W] all written, the guard floats behind it untouched."""
    n = NB * P * H * W
    assert bool(torch.isfinite(out[:n]).all()), "not every element was written"
    assert bool(torch.isnan(out[n:]).all()), "written past the compact output"
    return out[:n].reshape(NB, P, H, W)


def check_planes(out, H, W):
    assert bool(torch.isfinite(out).all()), "not every element was written"
    assert torch.count_nonzero(out[:, :, ~M.interior_mask(H, W)]) == 0, "non-zero border cell"
    return M.unpack_planes(out, H, W)


def conv_error(layer, got, ref):
    err = float((got.double() - ref).abs().max())
    return err if layer == 3 else err / float(ref.abs().max())


def _conv_cases():
    out = []
    for layer in (1, 2, 3):
        for kind in FX.STATES:
            for shape in (FX.CONV_SHAPES if layer == 1 else FX.CONV_SHAPES_5X5):
                for P in ((6, 4) if layer == 3 else (6,)):
                    out.append(pytest.param(layer, kind, shape, P, id="L{}-{}-{}-P{}".format(layer, kind, FX.shape_id(shape), P)))
    return out


@pytest.mark.parametrize("layer,kind,shape,P", _conv_cases())
def test_transform_conv_f32(device, layer, kind, shape, P):
    """os2d_pack_conv + os2d_transform_conv, one layer on its own: the interior against the unfolded float64 layer, pads exactly 0,
    three pairs in one call = three calls bit for bit, a second call the same bits."""
    H, W = shape
    NB = FX.CONV_NB
    packed = packed_f32(layer, kind, P, device)
    xin = FX.pack_planes_input(layer, FX.conv_input(layer, kind, shape)).to(device)
    ref = FX.conv_reference(layer, kind, shape, P)
    out = run_conv_f32(layer, packed, xin, NB, P, H, W, device)
    got = check_compact(out, NB, P, H, W) if layer == 3 else check_planes(out, H, W)
    stage, name = "conv{}_f32".format(layer), conv_case_id(layer, kind, shape, P)
    check_pins((stage, {name: conv_error(layer, got, ref)}, None if layer == 3 else {name: FX.conv_error_ceiling(layer, kind, shape, "f32")}))
    for n in range(NB):
        one = run_conv_f32(layer, packed, xin[n:n + 1].contiguous(), 1, P, H, W, device)
        one = check_compact(one, 1, P, H, W) if layer == 3 else check_planes(one, H, W)
        assert torch.equal(bits(one), bits(got[n:n + 1])), "pair {} alone gives other bits".format(n)
    assert torch.equal(bits(run_conv_f32(layer, packed, xin, NB, P, H, W, device)), bits(out)), "a second call gives other bits"


def run_conv_f16x3(layer, packed, xin, NB, P, H, W, terms, device):
    """One os2d_transform_conv_f16x3 call into a 0xFF / NaN-prefilled output; the status word must stay 0."""
    lib = _L().load()
    if layer == 3:
        out = nan(device, NB * P * H * W + GUARD)
    else:
        out = ff_bytes(device, NB * int(lib.os2d_shb_bytes(FX.LAYER_CHANNELS[layer][1], H, W)))
    status = torch.zeros(1, dtype=torch.int32, device=device)
    _call("os2d_transform_conv_f16x3", layer, _ptr(xin), _ptr(packed[0]), _ptr(packed[1]), _ptr(out), NB, P, H, W, terms, _ptr(status),
          _stream(device))
    assert int(status.item()) == 0, "the range flag was raised on finite inputs inside the range plan"
    return out.cpu()


def check_shb(buf, exp, channels, H, W):
    import train_forward_f16x3_model as SHB
    values, halves = FX.shb_output(buf, exp, channels, H, W)
    assert bool(torch.isfinite(torch.from_numpy(halves.astype("float32"))).all()), "not every half was written"
    assert not halves[:, :, :, ~SHB.interior_mask(H, W)].any(), "non-zero border unit"
    return values


def _conv_cases_f16x3():
    return [pytest.param(*p.values, 3, id=p.id) for p in _conv_cases()] + \
           [pytest.param(*p.values, 2, id=p.id + "-terms2") for p in _conv_cases() if p.values[0] == 1]


@pytest.mark.parametrize("layer,kind,shape,P,terms", _conv_cases_f16x3())
def test_transform_conv_f16x3(device, layer, kind, shape, P, terms):
    """os2d_pack_conv_f16x3 + os2d_transform_conv_f16x3 with the exponents of ``range_plan``, one layer on its own, the input
    encoded on the host at the layer's in_exp: as test_transform_conv_f32, on the split-half blocked buffers."""
    H, W = shape
    NB = FX.CONV_NB
    pw, pb, e_in, e_out = packed_f16x3(layer, kind, P, device)
    cout = None if layer == 3 else FX.LAYER_CHANNELS[layer][1]
    xin = FX.shb_input(FX.conv_input(layer, kind, shape), e_in).to(device)
    ref = FX.conv_reference(layer, kind, shape, P)
    out = run_conv_f16x3(layer, (pw, pb), xin, NB, P, H, W, terms, device)
    got = check_compact(out, NB, P, H, W) if layer == 3 else check_shb(out, e_out, cout, H, W)
    mode = "f16x3" if terms == 3 else "f16x2"
    stage, name = "conv{}_{}".format(layer, mode), conv_case_id(layer, kind, shape, P)
    check_pins((stage, {name: conv_error(layer, got, ref)}, None if layer == 3 else {name: FX.conv_error_ceiling(layer, kind, shape, mode)}))
    per_pair = xin.view(NB, -1)
    for n in range(NB):
        one = run_conv_f16x3(layer, (pw, pb), per_pair[n].contiguous(), 1, P, H, W, terms, device)
        if layer == 3:
            assert torch.equal(bits(check_compact(one, 1, P, H, W)), bits(got[n:n + 1])), "pair {} alone gives other bits".format(n)
        else:
            check_shb(one, e_out, cout, H, W)
            assert torch.equal(one, out.view(NB, -1)[n]), "pair {} alone gives other bits".format(n)
    assert torch.equal(bits(run_conv_f16x3(layer, (pw, pb), xin, NB, P, H, W, terms, device)), bits(out)), "a second call gives other bits"


@pytest.mark.parametrize("layer,terms,copies", [(1, 3, 32), (1, 2, 32), (2, 3, 64)])
def test_transform_conv_f16x3_work_group_shapes_give_the_same_bits(device, layer, terms, copies):
    """os2d_launch_conv_f16x3 runs 128-position work-groups below 384 standard groups (two per tile for the 7x7 layer) and
    256-position ones from there on: three pairs take the fine shape, ``copies`` times the same three pairs the standard one -
    every copy must be the three-pair result bit for bit (which test_transform_conv_f16x3 holds against the model), at 17x13: a
    full 256-cell tile and one row in the next."""
    kind, (H, W), NB = "adversarial", (17, 13), FX.CONV_NB
    tiles = (H * (W + 3) + 255) // 256
    assert tiles * NB * (2 if layer == 1 else 1) < 384 <= tiles * NB * copies * (2 if layer == 1 else 1)
    pw, pb, e_in, e_out = packed_f16x3(layer, kind, 6, device)
    xin = FX.shb_input(FX.conv_input(layer, kind, (H, W)), e_in).to(device)
    few = run_conv_f16x3(layer, (pw, pb), xin, NB, 6, H, W, terms, device)
    many = run_conv_f16x3(layer, (pw, pb), xin.repeat(copies), NB * copies, 6, H, W, terms, device)
    check_shb(many, e_out, FX.LAYER_CHANNELS[layer][1], H, W)
    assert torch.equal(many.view(copies, -1), few.view(1, -1).expand(copies, -1)), "the two work-group shapes give other bits"


# ---------------------------------------------------------------------------------------------------------- refusals
# Arguments BOTH entry points reject on the host, before any launch: os2d_transform_conv in its argument check (P) and in
# os2d_launch_conv (the layer switch's default; the B-slab prefetch test 2 * (SLAB / 4) > 768 for W = 210, ahead of the launch),
# os2d_transform_conv_f16x3 in its argument checks (layer, P, terms, W > OS2D_MAX_W_DIRECT7).  Buffers have the sizes of the
# shape all the same.
REFUSALS = [("layer 0", 0, 6, 2, 5, 3), ("layer 4", 4, 6, 2, 5, 3), ("W = 210 for the direct 7x7 layer", 1, 6, 1, 210, 3),
            ("P = 5", 3, 5, 2, 5, 3)]
REFUSALS_F16X3 = REFUSALS + [("terms = 2 for layer 2", 2, 6, 2, 5, 2), ("terms = 4", 1, 6, 2, 5, 4)]


def assert_refused(rc, out, what):
    assert rc != 0, what + ": accepted"
    assert len(_L().load().os2d_last_error() or b"") > 0, what + ": no error text"
    assert bool(torch.isnan(out).all()), what + ": the output was touched"


@pytest.mark.parametrize("what,layer,P,H,W,terms", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_transform_conv_refuses(device, what, layer, P, H, W, terms):
    lib = _L().load()
    PL = int(lib.os2d_plane_floats(H, W))
    src = 3 if layer == 3 else 1                                          # the largest buffers: layer 1's
    xin = torch.zeros(1, FX.K + 1, PL, device=device)
    pw, pb = torch.zeros(int(lib.os2d_packed_conv_floats(src)), device=device), torch.zeros(int(lib.os2d_packed_bias_floats(src)), device=device)
    out = nan(device, 1, 128, PL)
    rc = lib.os2d_transform_conv(layer, _ptr(xin), _ptr(pw), _ptr(pb), _ptr(out), 1, P, H, W, _stream(device))
    torch.cuda.synchronize()
    assert_refused(rc, out, what)


@pytest.mark.parametrize("what,layer,P,H,W,terms", REFUSALS_F16X3, ids=[r[0] for r in REFUSALS_F16X3])
def test_transform_conv_f16x3_refuses(device, what, layer, P, H, W, terms):
    lib = _L().load()
    src = layer if layer in (2, 3) else 1
    xin = torch.zeros(int(lib.os2d_shb_bytes(FX.K, H, W)), dtype=torch.uint8, device=device)
    pw = torch.zeros(int(lib.os2d_packed_conv_bytes(src, 1)), dtype=torch.uint8, device=device)
    pb = torch.zeros(int(lib.os2d_packed_bias_floats(src)), device=device)
    out = nan(device, int(lib.os2d_shb_bytes(128, H, W)) // 4)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    rc = lib.os2d_transform_conv_f16x3(layer, _ptr(xin), _ptr(pw), _ptr(pb), _ptr(out), 1, P, H, W, terms, _ptr(status), _stream(device))
    torch.cuda.synchronize()
    assert_refused(rc, out, what)
    assert int(status.item()) == 0
