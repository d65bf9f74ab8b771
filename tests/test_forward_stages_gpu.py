"""GPU: the small forward entry points of libos2d_hip.so (include/os2d_hip.h) on their own, called through os2d_amd/_lib.py with
tensors built on the host, against the float64 model of the same stage (tests/forward_model.py).  The head tests reach these
kernels only through ``Os2dHead.forward``, at the fixtures' shapes and under end-to-end tolerances; the matrix kernels have
stage tests of their own (correlation and the inference convolutions: tests/test_forward_matrix_gpu.py; transforms and per-bin
GEMM: tests/test_dft_*_gpu.py, tests/test_spectral*_gpu.py).  Counterpart of
tests/test_backward_stages_gpu.py, with its rules:

  * an output the header calls "written" is pre-filled with NaN (0xFF bytes for byte buffers: NaN as fp16 too);
  * every element must come back finite, every pad exactly 0;
  * errors are computed against the float64 model, never against another run of a kernel;
  * bit-exact claims (pads, hi halves, the transposition, batch against slices) are ``torch.equal`` on integer views.
"""
import ctypes

import pytest
import torch

import backward_model as M
import forward_model as FM
import util

pytestmark = pytest.mark.gpu

F32 = torch.float32

# Pins: 3x the largest error measured on the MI355X over the cases of this file (measured value and its case in the comment;
# the table is in DESIGN.md section 10).  The project's own bounds are the CEILINGS a smooth stage has to stay under whatever
# the pin: 1e-6 on q15 (the golden head test), util.TOL_CLS, util.TOL_LOC / TOL_CORNERS with their relative parts, 1e-3 px on
# decoded boxes.
#   class_*    max |got - ref| of the normalised maps (values <= 1)
#   class_*_raw   normalize == 0 (values 1 +- 1, no bound of the project's applies): worst |got - ref| over what fp32 sampling
#              positions allow for the map, forward_model.resize_rounding_bound (1 = that bound)
#   split      worst |(hi + lo) 2^-12 - v| / bound, bound derived at test_class_split
#   sumsq, corr_norm*   relative max error |got - ref|_max / |ref|_max
#   decode_cls          max |got - ref|
#   decode_loc, decode_corners   worst |got - ref| / (atol + rtol |ref|) with util's tolerances (1 = the ceiling)
CEILING = {"class_single": 1e-6, "class_batch": 1e-6, "class_single_raw": 1.0, "class_batch_raw": 1.0, "split": 1.0, "sumsq": 1e-6,
           "corr_norm": 1e-6, "corr_norm_f16x3": 1e-6, "decode_cls": util.TOL_CLS, "decode_loc": 1.0, "decode_corners": 1.0,
           "boxes": 1e-3}
PIN = {
    "class_single": 9.4e-7,       # measured 3.1e-7 (C = 33, 64x3)
    "class_batch": 9.4e-7,        # measured 3.1e-7 (C = 33, 64x3)
    "class_single_raw": 0.62,     # measured 0.205 of the bound (C = 1, 2x2); 1.4e-6 of the largest value at C = 257, 64x3
    "class_batch_raw": 0.62,      # measured 0.205 of the bound (C = 1, 2x2)
    "split": 1.0,                 # measured 0.499 of the derived bound (C = 9): 3x would exceed the bound itself, so the bound
    "sumsq": 5.3e-7,              # measured 1.75e-7 (3x130x4x4)
    "corr_norm": 6e-7,            # measured 1.97e-7 (1x17x19)
    "corr_norm_f16x3": 7.2e-7,    # measured 2.39e-7 (2x3x5)
    "decode_cls": 4.4e-7,         # measured 1.45e-7 (38x38, P = 4, forward, stride 16)
    "decode_loc": 0.22,           # measured 0.072 of util's tolerance (17x19, P = 4 with the inverse, stride 8)
    "decode_corners": 0.2,        # measured 0.065 of util's tolerance (38x38, P = 6 with the inverse, stride 16)
    "boxes": 7.5e-6,              # measured 2.5e-6 px (candidate 15 of the clamp table)
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
    return t.detach().cpu().contiguous().view(torch.int32)


def report(stage, case, err):
    print("\nSTAGE {:<15s} {:<40s} {:.3e}".format(stage, case, err))


def check_pin(stage, errs):
    """errs: case -> error.  Every case is printed before anything is asserted."""
    for case, e in errs.items():
        report(stage, case, e)
    assert PIN[stage] <= CEILING[stage]
    bad = {k: e for k, e in errs.items() if not e < PIN[stage]}
    assert not bad, bad


def q_err(got, ref, raw, normalize):
    """Normalised maps: max |got - ref|; resized-only maps: the same over forward_model.resize_rounding_bound of the raw map."""
    err = float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max())
    if normalize:
        return err
    bound = FM.resize_rounding_bound(raw)
    return err / bound if bound > 0 else err            # the all-zero map: exactly 0 is asserted on its own


# ---------------------------------------------------------------------------------------------------------- class maps
def check_class_outputs(q15, qp, what):
    """q15 [.., C,15,15], qp [.., C,256] of one class or a batch: finite, the 31 pad rows exactly 0, qp the x-major
    transposition of q15 bit for bit."""
    q15, qp = q15.cpu(), qp.cpu()
    assert bool(torch.isfinite(q15).all()) and bool(torch.isfinite(qp).all()), what + ": not every element was written"
    assert torch.count_nonzero(qp[..., FM.K:]) == 0, what + ": non-zero pad row of qp"
    xmajor = qp[..., :FM.K].reshape(*qp.shape[:-1], 15, 15).transpose(-1, -2)        # [.., x, y] -> [.., y, x]
    assert torch.equal(bits(xmajor), bits(q15)), what + ": qp[c, x*15 + y] and q15[c, y, x] differ"


def class_errors(q15, qp, ref15, refp, raws, C, normalize):
    """case -> error of every class of the batch against the model, q15 and the 225 rows of qp."""
    return {"C={} n={} {}x{}".format(C, normalize, h, w): max(q_err(q15[b], ref15[b], raws[b], normalize),
                                                              q_err(qp[b, :, :FM.K], refp[b, :, :FM.K], raws[b], normalize))
            for b, (h, w) in enumerate(FM.BATCH_SIZES)}


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("C", FM.CLASS_CHANNELS_SINGLE)
def test_class_prepare_single(device, C, normalize):
    """os2d_class_prepare (no caller in os2d_amd/): every map of the ragged batch on its own; C = 257 wraps the 256-thread
    channel loop.  Against the model, not against the batch kernel: their sums run in different orders."""
    raws, ref15, refp = FM.class_case(C, normalize)
    q15s, qps = [], []
    for b, (h, w) in enumerate(FM.BATCH_SIZES):
        src = dev(raws[b][0], device)
        q15, qp = nan(device, C, 15, 15), nan(device, C, 256)
        _call("os2d_class_prepare", _ptr(src), C, h, w, normalize, _ptr(q15), _ptr(qp), _stream(device))
        check_class_outputs(q15, qp, "C={} n={} {}x{}".format(C, normalize, h, w))
        if b == FM.ZERO_AT:
            assert torch.count_nonzero(q15) == 0 and torch.count_nonzero(qp) == 0, "the all-zero map gives exact zeros"
        q15s.append(q15.cpu())
        qps.append(qp.cpu())
    check_pin("class_single" if normalize else "class_single_raw", class_errors(torch.stack(q15s), torch.stack(qps), ref15, refp, raws, C, normalize))


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("C", FM.CLASS_CHANNELS)
def test_class_prepare_batch(device, C, normalize):
    """os2d_class_prepare_batch: all nine sizes and an all-zero map in ONE launch; C around the 32-channel block."""
    raws, ref15, refp = FM.class_case(C, normalize)
    B = len(raws)
    srcs = [dev(r[0], device) for r in raws]
    ptrs = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64).to(device)
    sizes = torch.tensor(FM.BATCH_SIZES, dtype=torch.int32).to(device)
    n_ws = int(_L().load().os2d_class_prepare_workspace_floats(B, C))
    assert n_ws == B * ((C + 31) // 32) * FM.K
    ws = nan(device, n_ws)
    q15, qp = nan(device, B, C, 15, 15), nan(device, B, C, 256)
    _call("os2d_class_prepare_batch", _ptr(ptrs), _ptr(sizes), B, C, normalize, _ptr(q15), _ptr(qp), _ptr(ws), _stream(device))
    check_class_outputs(q15, qp, "batch C={} n={}".format(C, normalize))
    assert torch.count_nonzero(q15[FM.ZERO_AT]) == 0 and torch.count_nonzero(qp[FM.ZERO_AT]) == 0, "the all-zero class"
    # per class: the neighbours of the zero class match the model as every other class does
    check_pin("class_batch" if normalize else "class_batch_raw", class_errors(q15.cpu(), qp.cpu(), ref15, refp, raws, C, normalize))


# ---------------------------------------------------------------------------------------------------------- split operand
@pytest.mark.parametrize("C", FM.SPLIT_CHANNELS)
def test_class_split(device, C):
    """os2d_class_split: the fp16 hi|lo operand of every non-fp32 correlation, [B, G, hi|lo, 256, 8] halves of v' = v * 2^12.

    hi = rn16(v') bit for bit.  r = v' - hi is exact in fp32 (it has at most 13 significant bits), |r| <= ulp16(hi) / 2
    <= 2^-11 |hi|, and lo = rn16(r) is off by at most 2^-11 |lo| <= 2^-22 |hi| <= 2^-22 (1 + 2^-10) |v'| where lo is a normal
    fp16 number, and by at most the fp16 subnormal spacing 2^-24 where it is not (|v'| < 2^-14: hi itself is subnormal, lo 0 or
    one spacing).  So |(hi + lo) - v'| <= 2^-22 (1 + 2^-10) |v'| + 2^-24, times 2^-12 for v."""
    B = FM.SPLIT_B
    qp = FM.split_input(C)
    hi_ref, v, zero = FM.class_split_model(qp, C)
    G = FM.split_groups(C)
    nbytes = int(_L().load().os2d_class_split_bytes(B, C))
    assert nbytes == B * G * 2 * 256 * 16
    qs = ff_bytes(device, nbytes)
    qp_d = dev(qp, device)
    _call("os2d_class_split", _ptr(qp_d), _ptr(qs), B, C, _stream(device))
    got = qs.cpu().view(torch.int16).view(B, G, 2, 256, 8)
    halves = got.view(torch.float16)
    assert bool(torch.isfinite(halves).all()), "not every half was written"
    hi, lo = got[:, :, 0], got[:, :, 1]
    assert torch.equal(hi, hi_ref), "hi is not rn16(v * 4096)"
    assert torch.count_nonzero(halves[:, :, 0][zero]) == 0 and torch.count_nonzero(halves[:, :, 1][zero]) == 0, "non-zero pad"
    rec = (halves[:, :, 0].double() + halves[:, :, 1].double()) * 2.0 ** -FM.SPLIT_EXP
    bound = (2.0 ** -22 * (1 + 2.0 ** -10) * v.abs() * 2.0 ** FM.SPLIT_EXP + 2.0 ** -24) * 2.0 ** -FM.SPLIT_EXP
    tiny = (v != 0) & (v.abs() < FM.TINY)
    assert int(tiny.sum()) >= 3 and int(((v == 0) & ~zero).sum()) >= 3
    assert torch.count_nonzero(rec[v == 0]) == 0
    check_pin("split", {"C={}".format(C): float(((rec - v).abs() / bound).max()),
                        "C={} tiny values".format(C): float(((rec - v).abs() / bound)[tiny].max())})
    assert int(torch.count_nonzero(lo.view(torch.float16)[~zero])) > 0 or C == 1, "lo carries the second half of the bits"


# ---------------------------------------------------------------------------------------------------------- image norms
@pytest.mark.parametrize("shape", FM.SUMSQ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fm_sumsq(device, shape):
    """C beyond one 128-channel sweep, C no multiple of 16, H*W no multiple of 16."""
    A, C, H, W = shape
    fm = torch.randn(A, C, H, W, generator=torch.Generator().manual_seed(C + H * W))
    out = nan(device, A, H * W)
    fm_d = dev(fm, device)
    _call("os2d_fm_sumsq", _ptr(fm_d), _ptr(out), A, C, H, W, _stream(device))
    assert bool(torch.isfinite(out).all())
    check_pin("sumsq", {str(shape): M.rel_err(out, FM.sumsq_model(fm))})


# ---------------------------------------------------------------------------------------------------------- relu + L2 over 225
@pytest.mark.parametrize("shape", FM.CORR_NORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_corr_normalize(device, shape):
    """os2d_corr_normalize into a dirty buffer: the zero borders and the 226th plane are written by the call."""
    lib, (NB, H, W) = _L().load(), shape
    PL = int(lib.os2d_plane_floats(H, W))
    assert PL == M.plane_geometry(H, W)[2]
    corr = FM.corr_norm_input(shape)
    ref = FM.corr_normalize_model(corr)
    rnorm = nan(device, NB, 226, PL)
    corr_d = dev(corr.reshape(NB, FM.K, H * W), device)
    _call("os2d_corr_normalize", _ptr(corr_d), _ptr(rnorm), NB, H, W, _stream(device))
    got = rnorm.cpu()
    assert bool(torch.isfinite(got).all()), "not every element was written"
    assert torch.count_nonzero(got[:, :, ~M.interior_mask(H, W)]) == 0, "non-zero border cell"
    assert torch.count_nonzero(got[:, FM.K]) == 0, "the 226th plane"
    inner = M.unpack_planes(got[:, :FM.K], H, W)
    nb, h, w = FM.corr_norm_dead(shape)
    assert torch.count_nonzero(inner[nb, :, h, w]) == 0 and torch.count_nonzero(ref[nb, :, h, w]) == 0, "0 / (0 + 1e-6)"
    check_pin("corr_norm", {str(shape): M.rel_err(inner, ref)})


@pytest.mark.parametrize("shape", FM.CORR_NORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_corr_normalize_f16x3(device, shape):
    """The same into the split-half blocked buffer [NB][29][hi|lo][PLANE][8] halves, scaled by 2^12: borders, the channels
    225..231 of the last group and the dead location exactly 0; hi + lo against the model (2^-22 relative from the split)."""
    import freq_util
    lib, (NB, H, W) = _L().load(), shape
    assert int(lib.os2d_rnorm_exp()) == 12
    nbytes = int(lib.os2d_shb_bytes(FM.K, H, W))
    assert nbytes == 29 * 2 * M.plane_geometry(H, W)[2] * 16
    corr = FM.corr_norm_input(shape)
    ref = FM.corr_normalize_model(corr)
    rshb = ff_bytes(device, NB * nbytes)
    corr_d = dev(corr.reshape(NB, FM.K, H * W), device)
    _call("os2d_corr_normalize_f16x3", _ptr(corr_d), _ptr(rshb), NB, H, W, _stream(device))
    buf = rshb.cpu()
    assert bool(torch.isfinite(buf.view(torch.float16)).all()), "not every half was written"
    values, outside = freq_util.shb_decode(buf, NB, 232, H, W)
    assert outside == 0.0, "non-zero border unit"
    assert torch.count_nonzero(values[:, FM.K:]) == 0, "channels 225..231 of the last group"
    inner = values[:, :FM.K] * 2.0 ** -12
    nb, h, w = FM.corr_norm_dead(shape)
    assert torch.count_nonzero(inner[nb, :, h, w]) == 0
    check_pin("corr_norm_f16x3", {str(shape): M.rel_err(inner, ref)})


# ---------------------------------------------------------------------------------------------------------- alignment epilogue
def run_sample_decode(device, corr, params, inverse, stride, rec_field):
    NB, P, H, W = params.shape
    HW = H * W
    loc, cls, corners = nan(device, NB, 4, HW), nan(device, NB, 1, HW), nan(device, NB, 8, HW)
    c_d, p_d = dev(corr.reshape(NB, FM.K, HW), device), dev(params.reshape(NB, P, HW), device)
    _call("os2d_sample_decode", _ptr(c_d), _ptr(p_d), NB, H, W, P, 1 if inverse else 0, stride, rec_field, _ptr(loc), _ptr(cls),
          _ptr(corners), _stream(device))
    outs = [t.cpu().view(NB, -1, H, W) for t in (loc, cls, corners)]
    assert all(bool(torch.isfinite(t).all()) for t in outs), "not every element was written"
    return outs


def ratio(got, ref, atol, rtol, extra=None):
    """|got - ref| / (atol + rtol |ref| [+ extra]), elementwise."""
    tol = atol + rtol * ref.abs()
    return (got.double() - ref).abs() / (tol if extra is None else tol + extra)


def assert_batch_equals_slices(device, outs, corr, params, inverse, stride, rec_field):
    """A pair's outputs depend on nothing but its own slice: NB pairs in one call = NB calls, bit for bit."""
    for n in range(corr.size(0)):
        one = run_sample_decode(device, corr[n:n + 1], params[n:n + 1], inverse, stride, rec_field)
        for full, part in zip(outs, one):
            assert torch.equal(bits(full[n:n + 1]), bits(part)), n


@pytest.mark.parametrize("name", sorted(M.DECODE_CASES))
def test_sample_decode(device, name):
    """os2d_sample_decode on the 16 cases of the backward suite (both P, the inverse on and off, stride 16 / rec_field 16 and
    stride 8 / rec_field 32): cls, loc and corners at EVERY location - the forward values are continuous in the parameters
    (the clamp, min / max and the min-size rule have no jumps), so nothing is excluded as fragile."""
    P, inverse, stride, rec_field, NB, H, W, _ = M.DECODE_CASES[name]
    inp = M.decode_inputs(name)
    loc_ref, cls_ref, cor_ref, _ = FM.decode_forward_model(inp["corr"], inp["params"], inverse, stride, rec_field)
    outs = run_sample_decode(device, inp["corr"], inp["params"], inverse, stride, rec_field)
    loc, cls, corners = outs
    errs = {"decode_cls": float((cls.double() - cls_ref).abs().max()),
            "decode_loc": float(ratio(loc, loc_ref, util.TOL_LOC, util.RTOL_LOC).max()),
            "decode_corners": float(ratio(corners, cor_ref, util.TOL_CORNERS, util.RTOL_CORNERS).max())}
    for k, e in errs.items():
        report(k, name, e)
    assert not {k: e for k, e in errs.items() if not e < PIN[k]}, errs
    assert_batch_equals_slices(device, outs, inp["corr"], inp["params"], inverse, stride, rec_field)


@pytest.mark.parametrize("inverse", [True, False], ids=["inv", "fwd"])
def test_sample_decode_hand_placed_locations(device, inverse):
    """backward_model.HAND_THETA: exactly singular matrices, both min-size clips, all 121 points clamped; each location on its
    own.

    With the inverse on, locations 0 and 1 hold the inverse of a matrix regularised by 1e-5: theta ~ 1e5, corners ~ 1e7 px,
    where one fp32 ulp is a pixel.  They are judged against what fp32 rounding of theta allows there, derived as
    backward_model.fragility derives delta_c: the kernel rounds the three elements of a row of theta to fp32 and evaluates
    U = (t0 xj + t1 yi + t2) half_box + ecx with xj, yi = +-1: two additions, a multiplication and an addition - with theta's
    own roundings 8 roundings of at most 2^-24 of the magnitude they work at, which half_box (|t0| + |t1| + |t2|) + ecx
    bounds; with the factor 2 of fragility for the model's own path:
        delta = 16 * 2^-24 * (half_box * (|t0| + |t1| + |t2|) + stride * centre)          per corner coordinate.
    loc follows from the corners: the box centre is the mean of two corner coordinates (each within delta) and enters as
    10 (gcx - acx) / aw, the box size as 5 log(bw / aw): |d loc0| <= 10 delta / aw, |d loc2| <= 5 * 2 delta / bw (y alike).
    These terms are added to util's tolerances at the two singular locations only; everywhere else the pins hold."""
    stride, rec_field = 16, 16
    inp = M.hand_inputs(inverse)
    loc_ref, cls_ref, cor_ref, aux = FM.decode_forward_model(inp["corr"], inp["params"], inverse, stride, rec_field)
    outs = run_sample_decode(device, inp["corr"], inp["params"], inverse, stride, rec_field)
    loc, cls, corners = [t.reshape(t.size(1), 9) for t in outs]
    loc_ref, cls_ref, cor_ref = loc_ref.reshape(4, 9), cls_ref.reshape(1, 9), cor_ref.reshape(8, 9)
    delta = FM.theta_rounding_bound(aux, 1, 3, 3, stride, rec_field).reshape(2, 9)               # x, y
    singular = [n for n, th in enumerate(M.HAND_THETA) if th is None] if inverse else []
    assert singular == ([0, 1] if inverse else [])
    aw = float(stride * (FM.T - 1) + rec_field)
    xs, ys = cor_ref[0::2], cor_ref[1::2]
    bw = torch.stack([(xs.max(0)[0] - xs.min(0)[0]).clamp_min(1.0), (ys.max(0)[0] - ys.min(0)[0]).clamp_min(1.0)])   # [2,9]
    errs = {"decode_cls": {}, "decode_loc": {}, "decode_corners": {}}
    for n in range(9):
        case = "hand {} location {}".format("inv" if inverse else "fwd", n)
        extra_c = extra_l = None
        if n in singular:
            assert float(aux["theta"].reshape(9, 6)[n].abs().max()) > 5e4
            extra_c = delta[:, n].repeat(4)                                                         # x, y, x, y, ..
            extra_l = torch.cat([10 * delta[:, n] / aw, 5 * 2 * delta[:, n] / bw[:, n]])
        errs["decode_cls"][case] = float((cls[:, n].double() - cls_ref[:, n]).abs().max())
        errs["decode_loc"][case] = float(ratio(loc[:, n], loc_ref[:, n], util.TOL_LOC, util.RTOL_LOC, extra_l).max())
        errs["decode_corners"][case] = float(ratio(corners[:, n], cor_ref[:, n], util.TOL_CORNERS, util.RTOL_CORNERS, extra_c).max())
    for k, per_case in errs.items():
        for case, e in per_case.items():
            report(k, case, e)
    for k, per_case in errs.items():
        bad = {c: e for c, e in per_case.items() if not e < PIN[k]}
        assert not bad, bad
    # the clips of clip_to_min_size are visited: location 2 both, location 3 the x clip only
    if not inverse:
        assert float(bw[0, 2]) == 1.0 and float(bw[1, 2]) == 1.0 and float(bw[0, 3]) == 1.0 and float(bw[1, 3]) > 1.0


# ---------------------------------------------------------------------------------------------------------- box clamp
def _coder():
    from os2d_amd.modeling.box_coder import BoxGridGenerator, Os2dBoxCoder
    from os2d_amd.structures.feature_map import FeatureMapSize
    gen = BoxGridGenerator(box_size=FeatureMapSize(w=240, h=240), box_stride=FeatureMapSize(w=16, h=16))
    return Os2dBoxCoder(output_box_grid_generator=gen)


def test_box_clamp_and_empty_boxes(device):
    """The dw / dh clamp at log(1000/16) of os2d_decode_box (csrc/detect_common.h), shared by os2d_decode_boxes,
    os2d_detect_level* and os2d_detect_pyramid*, and what follows from it: a clamped box is clipped to the image, a box of
    exp(-large) width is empty and is dropped by the fused kernels exactly as the generic chain drops it.

    forward_model.CLAMP_TABLE: 24 hand-placed candidates on one 3x4 level.  The reference drops 10 of them as empty
    (forward_model.CLAMP_EMPTY): candidates 5, 6 and 20 by exp(-2000) = exp(-inf) = 0, candidates 7 - 10 and 19 because the
    CLAMPED box lies wholly outside the image (without the clamp they would reach back over it and survive), candidates 11 and
    18 as ordinary boxes pushed outside."""
    from oracle import decode_oracle as D
    from os2d_amd.structures.feature_map import FeatureMapSize
    from test_decode_gpu import _assert_same_detections
    H, W = FM.CLAMP_LEVEL
    iw, ih = FM.CLAMP_IMAGE
    HW, B = H * W, FM.CLAMP_B
    size = FeatureMapSize(w=iw, h=ih)
    loc, cls = FM.clamp_inputs()
    loc_d, cls_d = loc.to(device), cls.to(device)
    ref = FM.decode_boxes_model(loc, H, W, iw, ih)
    coder = _coder()
    assert (coder.get_feature_map_size(size).h, coder.get_feature_map_size(size).w) == (H, W)

    # 1. os2d_decode_boxes against decode_oracle.decode_level in float64
    boxes = nan(device, B, HW, 4)
    _call("os2d_decode_boxes", _ptr(loc_d), B, H, W, 16, 16, ctypes.c_float(iw), ctypes.c_float(ih), _ptr(boxes), _stream(device))
    assert bool(torch.isfinite(boxes).all())
    assert torch.equal(bits(coder.decode_level(loc_d, size)), bits(boxes))
    got = boxes.cpu().double()
    per_candidate = (got - ref).abs().reshape(B * HW, 4).max(1)[0]
    for k in range(B * HW):
        print("STAGE {:<15s} candidate {:<2d} {} {:.3e}".format("boxes", k, FM.CLAMP_TABLE[k][2:], float(per_candidate[k])))
    check_pin("boxes", {"3x4 clamp table": float(per_candidate.max())})
    flat = got.reshape(B * HW, 4)
    empty = ((flat[:, 2] <= flat[:, 0]) | (flat[:, 3] <= flat[:, 1])).nonzero().squeeze(1).tolist()
    assert empty == FM.CLAMP_EMPTY and len(empty) == 10
    for k in (0, 1, 4):                                  # clamped (or a rounding away from it) around the centre: the whole image
        assert flat[k].tolist() == [0.0, 0.0, float(iw), float(ih)], k

    # 2. + 3. the two fused routes against the generic chain, bit for bit, and the survivors against decode_oracle.decode_pyramid;
    # at IoU threshold 1 nothing is suppressed: exactly the 14 non-empty candidates survive
    corners = torch.rand(B, 8, HW, generator=torch.Generator().manual_seed(3)).mul(60).to(device)
    args = ([loc_d], [cls_d], [size], [0, 1])
    for iou_thr in (0.3, 1.0):
        coder.use_fused_level_kernel = True
        level = coder._decode_single_level_fused(*args, float("-inf"), iou_thr, None, [corners])
        pyramid = coder._decode_pyramid_fused(*args, float("-inf"), iou_thr, None, [corners])
        assert level is not None and pyramid is not None, "fused path not taken"
        coder.use_fused_level_kernel = False
        generic = coder.decode_pyramid(*args, nms_score_threshold=float("-inf"), nms_iou_threshold=iou_thr,
                                       transform_corners_pyramid=[corners])
        _assert_same_detections(level, generic)
        _assert_same_detections(pyramid, generic)
        rb, rs, rl = D.decode_pyramid([loc.double()], [cls], [(H, W)], [(iw, ih)], None, float("-inf"), iou_thr)
        assert torch.equal(generic.get_field("labels").cpu(), rl)
        assert torch.equal(generic.get_field("scores").cpu(), rs)
        assert util.maxdiff(generic.bbox_xyxy, rb) < 1e-3
        if iou_thr == 1.0:
            assert len(generic) == B * HW - len(FM.CLAMP_EMPTY) == 14
            alive = torch.ones(B * HW, dtype=torch.bool)
            alive[FM.CLAMP_EMPTY] = False
            assert sorted(generic.get_field("scores").cpu().tolist()) == sorted(cls.reshape(-1)[alive].tolist())
        else:
            assert 2 < len(generic) < 14, "NMS at 0.3 removes the duplicates of the whole-image box, not everything"
