"""Shared helpers for the parity tests."""
import glob
import os

import numpy as np
import torch

from os2d_amd.utils import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def head_fixture_names():
    return sorted(os.path.basename(p)[len("head_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "head_*.npz")))


def load_head_fixture(name):
    d = np.load(os.path.join(GOLDEN, "head_{}.npz".format(name)))
    P, inverse = int(d["P"]), bool(d["inverse"])
    state = synthetic.make_transform_net_state(P, seed=int(d["seed_net"]),
                                               linear_std=float(d["linear_std"]) if "linear_std" in d.files else 0.02,
                                               linear_bias=d["linear_bias"] if "linear_bias" in d.files else None)
    assert abs(synthetic.state_checksum(state) - float(d["net_checksum"])) < 1e-9, "regenerated weights differ"
    fx = dict(P=P, inverse=inverse, state=state, fm=torch.from_numpy(d["fm"]),
              class_fms=[torch.from_numpy(d["class_fm_{}".format(b)]) for b in range(int(d["n_classes"]))])
    for k in d.files:
        if k.startswith("ref_"):
            fx[k] = torch.from_numpy(d[k])
    # arrays kept beside the archive (head_<name>.ref_<key>.npy) so that no fixture file exceeds 1 MiB
    for path in glob.glob(os.path.join(GOLDEN, "head_{}.ref_*.npy".format(name))):
        fx[os.path.basename(path)[len("head_{}.".format(name)):-len(".npy")]] = torch.from_numpy(np.load(path))
    return fx


def make_head_creator(P, inverse, state, device, stride=16, rec_field=16):
    """Build the product head creator on `device` and load a TransformNet state dict into it."""
    from os2d_amd.modeling.head import build_os2d_head_creator
    from os2d_amd.structures.feature_map import FeatureMapSize
    creator = build_os2d_head_creator(P == 4, False, inverse, FeatureMapSize(w=stride, h=stride),
                                      FeatureMapSize(w=rec_field, h=rec_field))
    creator.aligner.parameter_regressor.load_state_dict(state)
    creator.to(device)
    creator.eval()
    return creator


def maxdiff(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


# ---- tolerances of the head parity tests (north_star: score maps within 1e-4 fp32)
#   cls      1e-5 absolute  (values ~0.3-0.45; measured ~3e-7)
#   loc      1e-4 absolute + 1e-5 relative (values up to ~1 near the identity; up to 35 / 5e5 for the extreme fixtures)
#   corners  2e-3 absolute + 2e-6 relative (pixel coordinates: ~600 near the identity, up to 1e5 .. 1e8 for the 1000x
#            zoom / near-singular fixtures, where one fp32 ulp is 0.008 .. 8 px)
TOL_CLS, TOL_LOC, TOL_CORNERS = 1e-5, 1e-4, 2e-3
RTOL_LOC, RTOL_CORNERS = 1e-5, 2e-6
# x_tiny_scale_inv zooms the template 1000x: a 1e-7 difference in the template grid coordinate (torch.linspace's middle
# element vs -1 + 7 * (2/14) in fp32) moves the sampling point by 1e-3 cells, i.e. the score by ~1e-5
CLS_TOL_OVERRIDE = {"x_tiny_scale_inv": 5e-5}


def assert_close(got, ref, atol, rtol=0.0, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, "{}: shape {} vs {}".format(what, tuple(got.shape), tuple(ref.shape))
    excess = (got - ref).abs() - (atol + rtol * ref.abs())
    assert torch.isfinite(got).all(), "{}: non-finite values".format(what)
    assert float(excess.max()) <= 0.0, "{}: max |diff| {:.3e} (worst excess over atol {:.1e} + rtol {:.1e}: {:.3e})".format(
        what, float((got - ref).abs().max()), atol, rtol, float(excess.max()))


# the fp32-equivalent modes at BASELINE.json's full size, pinned at <= 3x what is measured there (scores
# 2.4e-7, loc 1e-5): a regression of the default arithmetic by a factor of a few fails, long before north_star's 1e-4
PIN_CLS, PIN_LOC = 1e-6, 3e-5
FP32_EQUIVALENT = ("f32", "fft32", "fft", "fftx3", "f16x3")


def assert_head_outputs_close(name, loc, cls, corners, ref_loc, ref_cls, ref_corners, scale=1.0, corners_scale=1.0, pin=False):
    """The one place the head tolerances live.  ``corners_scale`` loosens the CORNER tolerance only (pixel coordinates: 2.5
    for levels whose coordinates reach 1400 - 2000 px, where one fp32 ulp is 1.2e-4 px); ``scale`` loosens all three and is
    for the opt-in reduced-precision mode (f16x2) only; ``pin``: scores and loc at the full-size pins above instead."""
    tol_cls, tol_loc = (PIN_CLS, PIN_LOC) if pin else (CLS_TOL_OVERRIDE.get(name, TOL_CLS) * scale, TOL_LOC * scale)
    assert_close(cls, ref_cls, tol_cls, 0.0, name + " cls")
    assert_close(loc, ref_loc, tol_loc, RTOL_LOC * scale, name + " loc")
    assert_close(corners, ref_corners, TOL_CORNERS * scale * corners_scale, RTOL_CORNERS * scale, name + " corners")


# ---- per-fixture pins: the error of every fp32-equivalent mode on every head fixture, MEASURED on an MI355X and
# recorded in tests/golden/head_fixture_pins.json as the worst ratio |diff| / (atol + rtol |ref|) per output (the tolerance formula
# above, so that fixtures whose coordinates reach 1e8 and those near the identity share one scale).  The golden test asserts at most
# 3x the recorded ratio (never tighter than PIN_FLOOR of the global tolerance: ~ an ulp of the scores) - a regression by a factor of a
# few in one of the 13 deformation cases fails, where the global 1e-5 / 1e-4 / 2e-3 let it pass.  The kernels are deterministic:
# the same bits on every box.  Regenerate on a GPU box:  OS2D_WRITE_FIXTURE_PINS=gpurun_out/head_fixture_pins.json pytest -m gpu -k golden
PINS_PATH = os.path.join(GOLDEN, "head_fixture_pins.json")
PIN_FACTOR, PIN_FLOOR = 3.0, 0.02
_PINS = None


def tolerance_ratio(got, ref, atol, rtol=0.0):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def head_error_ratios(name, loc, cls, corners, ref_loc, ref_cls, ref_corners):
    """[cls, loc, corners] as fractions of the generic tolerance of ``assert_head_outputs_close`` (scale 1)."""
    return [tolerance_ratio(cls, ref_cls, CLS_TOL_OVERRIDE.get(name, TOL_CLS)), tolerance_ratio(loc, ref_loc, TOL_LOC, RTOL_LOC),
            tolerance_ratio(corners, ref_corners, TOL_CORNERS, RTOL_CORNERS)]


def fixture_pins():
    global _PINS
    if _PINS is None:
        import json
        _PINS = json.load(open(PINS_PATH)) if os.path.exists(PINS_PATH) else {}
    return _PINS


def check_or_record_fixture_pin(name, precision, ratios):
    """Assert the recorded pin of (fixture, mode) - or, under $OS2D_WRITE_FIXTURE_PINS, record the measured ratios instead."""
    import json
    out = os.environ.get("OS2D_WRITE_FIXTURE_PINS")
    if out:
        d = json.load(open(out)) if os.path.exists(out) else {}
        d.setdefault(name, {})[precision] = [float("{:.4g}".format(r)) for r in ratios]
        with open(out, "w") as f:
            json.dump(d, f, indent=0, sort_keys=True)
        return
    pin = fixture_pins().get(name, {}).get(precision)
    if pin is None:
        return
    for what, r, p in zip(("cls", "loc", "corners"), ratios, pin):
        limit = max(PIN_FACTOR * p, PIN_FLOOR)
        assert r <= limit, "{} [{}] {}: error {:.4g} of the generic tolerance, pinned at {:.4g} (measured {:.4g})".format(name, precision, what, r, limit, p)


def route_head_inputs(A, B, H, W, C=32):
    """The network, class maps and feature maps of the head-route tests (tests/test_head_gpu.py: ROUTE_SHAPES;
    tests/test_range_flag_stages_gpu.py): (TransformNet state for P = 6, B class maps [C, h, w], feature maps [A, C, H, W]) on the
    CPU, fresh tensors on every call (a caller may edit them)."""
    state = synthetic.make_transform_net_state(6, seed=7)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=[(15, 15), (14, 16), (16, 14)], seed=500)
    return state, class_fms, synthetic.make_feature_map(C, H, W, seed=5, A=A)


def head_workspace_bytes(A, classes, C, H, W, precision, P=6):
    """os2d_head_workspace_bytes_ex: the workspace that takes ``classes`` classes per chunk."""
    import ctypes
    from os2d_amd import _lib
    from os2d_amd.modeling import head as head_mod
    n = ctypes.c_size_t()
    _lib.check(_lib.load().os2d_head_workspace_bytes_ex(A, classes, C, H, W, P, head_mod.PRECISIONS[precision], ctypes.byref(n)), "workspace bytes")
    return n.value


def head_forward_ex2(head, fm, precision, ws, status=None, conv2_freq=True):
    """os2d_head_forward_ex2 through ctypes on the CALLER's workspace ``ws`` (uint8 device tensor, used as it is: the range words
    at its start are the caller's to zero-fill and to read) and the caller's status word (int32 device tensor or None):
    (chunk_classes, [loc, cls, corners]), synchronised.  Outputs are NaN-prefilled.  conv2_freq: hand the fftx3 route the
    spectra of the 5x5 layer (wspec2) as well."""
    import ctypes
    from os2d_amd import _lib
    from os2d_amd.modeling import head as head_mod
    lib, ptr, dev = _lib.load(), _lib.ptr, fm.device
    A, C, H, W = fm.shape
    B = head.class_batch_size
    net = head.aligner.parameter_regressor
    spectra = net.spectra(H, W, split=precision == "fftx3")[:3] if precision in head_mod.FFT_MODES else (None, None, None)
    spectra2 = net.spectra2(H, W) if (precision == "fftx3" and conv2_freq) else None
    packed = net.packed(precision)
    qs = head._split_class_operand() if precision not in head_mod.FP32_MODES else None
    out = [torch.full((A, B, k, H, W), float("nan"), device=dev) for k in (4, 1, 8)]
    chunk = ctypes.c_int(0)
    _lib.check(lib.os2d_head_forward_ex2(
        ptr(fm), ptr(head._qp), *[ptr(t) for t in packed], A, B, C, H, W, 6, 1, head._stride, head._rec_field, *[ptr(t) for t in out],
        ptr(ws), ws.numel(), _lib.current_stream(dev), head_mod.PRECISIONS[precision], ptr(qs), None, ctypes.byref(chunk), ptr(status),
        *[ptr(t) for t in spectra], ptr(spectra2)), "os2d_head_forward_ex2")
    torch.cuda.synchronize()
    return chunk.value, out


def adversarial_transform_net_state(P, seed, lo1=-3.0, hi1=6.0, lo2=-3.0, hi2=3.0):
    """A TransformNet that computes the SAME function as ``make_transform_net_state(P, seed)`` but whose intermediate
    ranges are hostile to a fixed-range number format:
      * output channel o of conv 7x7 (+BN+ReLU) is scaled by s1[o] in 10^[lo1, hi1] (BN weight and bias; ReLU is
        positively homogeneous) and the 5x5 layer's input channel o by 1/s1[o]: activations span 1e-5 .. 1e5 (below 2^-14
        and beyond 65504), folded BN scales and the rows / columns of the weight tensors span nine decades;
      * the same between conv 5x5 128->64 and the last layer with s2 in 10^[lo2, hi2];
      * every fourth BatchNorm channel has running_var = 1e-6 (BN weight compensated so the folded scale is unchanged).
    In exact arithmetic the outputs are identical to the base network's; fp32 (the reference) loses nothing either."""
    import numpy as np
    st = {k: v.clone() for k, v in synthetic.make_transform_net_state(P, seed=seed).items()}
    rs = np.random.RandomState(seed + 7919)
    for bn, nxt, lo, hi in (("conv.1", "conv.3.weight", lo1, hi1), ("conv.4", "linear.weight", lo2, hi2)):
        c = st[bn + ".weight"].numel()
        s = torch.from_numpy((10.0 ** rs.uniform(lo, hi, size=c)).astype(np.float32))
        s[0], s[1] = 10.0 ** hi, 10.0 ** lo                     # both extremes are always present
        var = st[bn + ".running_var"].clone()
        small = torch.arange(c) % 4 == 0
        comp = torch.sqrt((torch.full_like(var, 1e-6) + 1e-5) / (var + 1e-5))
        st[bn + ".running_var"] = torch.where(small, torch.full_like(var, 1e-6), var)
        st[bn + ".weight"] = st[bn + ".weight"] * torch.where(small, comp, torch.ones_like(comp)) * s
        st[bn + ".bias"] = st[bn + ".bias"] * s
        st[nxt] = st[nxt] / s.view(1, -1, 1, 1)
    return st


class InverseTransformList(object):
    """A per-level inverse box transform shaped like the one the reference's dataloader hands to decode_pyramid (reference
    os2d/structures/transforms.py:12-27: closures appended in augmentation order, applied last-appended first)."""

    def __init__(self):
        self.steps = []

    def append(self, fn):
        self.steps.append(fn)

    def __call__(self, boxes):
        for fn in self.steps[::-1]:
            boxes = fn(boxes)
        return boxes


def dataloader_style_inverse(chain):
    """``chain`` [n,5] of tests/golden/decode_transforms.npz - the steps in the order the inverse applies them (kind 1: resize
    to (w, h); 4: crop (left, top, right, bottom); 2 / 3: horizontal / vertical flip) - as a list of lambdas calling
    BoxList.resize / crop / transpose, exactly what reference transforms.py:32-52, 78-79, 188-191 append."""
    from os2d_amd.structures.bounding_box import FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM
    from os2d_amd.structures.feature_map import FeatureMapSize
    t = InverseTransformList()
    for kind, a, b, c, d in list(chain)[::-1]:          # appended in augmentation order = reverse of the inverse's order
        kind = int(kind)
        if kind == 1:
            size = FeatureMapSize(w=int(a), h=int(b))
            t.append(lambda boxes, size=size: boxes.resize(size))
        elif kind == 4:
            region = (int(a), int(b), int(c), int(d))
            t.append(lambda boxes, region=region: boxes.crop(region))
        else:
            method = FLIP_LEFT_RIGHT if kind == 2 else FLIP_TOP_BOTTOM
            t.append(lambda boxes, method=method: boxes.transpose(method))
    return t
