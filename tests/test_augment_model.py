"""CPU: the numpy model of the training-image chain (tests/augment_model.py) equals every fixture recorded from the reference
and PIL byte for byte, the host side (structures/transforms.py, engine/augmentation.py: crop search, filter choice, colour draws,
box fates, inverse transforms) reproduces what the reference chose from the recorded seeds, and libos2d_augment.so is held to
what every library of the project is held to (tests/test_native_libs.py) and refuses bad arguments before any launch.

The host side runs here with the kernels' wrappers replaced by the model (``host_chain``): everything but the kernels."""
import ctypes
import glob
import os
import random

import numpy as np
import pytest
import torch

import augment_model as A
import image_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("augment_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "augment_*.npz"))
               if not p.endswith("augment_color_checksums.npz"))
PROBE = torch.tensor([[0.0, 0.0, 1.0, 1.0], [3.25, 7.5, 21.0, 15.75]])


def load(name):
    return np.load(os.path.join(GOLDEN, "augment_{}.npz".format(name)))


def model_levels(z):
    """the recorded run through the numpy model alone: window, padding, filters and colour operations as recorded"""
    pad = z["padding"]
    x0, y0, x1, y1 = z["window"]
    img = A.padded_window(z["image"], (x0 - pad[0], y0 - pad[1], x1 - pad[0], y1 - pad[1]), bool(z["hflip"]), bool(z["vflip"]))
    cw, ch = int(z["params"][0]), int(z["params"][1])
    img = A.resize_u8(img, cw, ch, A.FILTERS[z["filters"][0]])
    img = A.color_chain(img, [(int(k), float(f)) for k, f in z["color_ops"]])
    return [A.resize_u8(img, int(cw * s), int(ch * s), A.FILTERS[f]) for s, f in zip(z["scales"], z["filters"][1:])]


def test_the_cases_are_the_recorded_set():
    assert len(CASES) == 19 and {"random_boxes", "random_noboxes", "random_retry", "mined_all", "mined_flips", "color_csh", "color_shc",
                                 "color_none", "pyramid"} <= set(CASES)
    assert {"filter_" + f for f in A.FILTERS} <= set(CASES) and {"mined_" + s for s in ("left", "top", "right", "bottom")} <= set(CASES)
    assert [A.FILTERS[load("filter_" + f)["filters"][0]] for f in A.FILTERS] == list(A.FILTERS)
    assert load("color_csh")["color_ops"][:, 0].tolist() == [1, 2, 3, 4] and load("color_shc")["color_ops"][:, 0].tolist() == [1, 3, 4, 2]
    z = load("random_boxes")
    assert sorted(zip(z["mask_cutoff"].tolist(), z["mask_difficult"].tolist())) == [(False, False), (False, True), (True, True)]


@pytest.mark.parametrize("name", CASES)
def test_model_equals_the_fixture(name):
    z = load(name)
    levels = model_levels(z)
    assert len(levels) == len(z["scales"])
    for i, lvl in enumerate(levels):
        assert np.array_equal(lvl, z["u8_{}".format(i)]), (name, i)


@pytest.fixture(scope="module")
def all_colors():
    return A.all_colors()


@pytest.mark.parametrize("key", ["rgb_to_hsv", "hsv_to_rgb", "hue_23", "hue_231"])
def test_model_reproduces_pils_checksums_on_every_colour(key, all_colors):
    sums = np.load(os.path.join(GOLDEN, "augment_color_checksums.npz"))[key]
    if key == "rgb_to_hsv":
        got = A.rgb_to_hsv(all_colors)
    elif key == "hsv_to_rgb":
        got = A.hsv_to_rgb(all_colors)
    else:       # a factor whose int(f * 255) is the shift: 23, and -25 = 231 modulo 256
        got = A.color_chain(all_colors, [(A.HUE, {"hue_23": 0.0903, "hue_231": -0.0984}[key])])
    assert A.hue_shift(0.0903) == 23 and A.hue_shift(-0.0984) == 231
    assert np.array_equal(A.row_checksums(got), sums)


def test_host_tables_equal_the_model_for_every_filter():
    from os2d_amd.engine.image_pyramid import RANDOM_INTERPOLATION_FILTERS, resample_tables
    assert RANDOM_INTERPOLATION_FILTERS == A.FILTERS
    for name in A.FILTERS:
        for n, m in ((83, 200), (83, 40), (61, 7), (5, 80), (80, 5), (48, 48)):
            b, c = resample_tables(n, m, name)
            mb, mc = A.tables(n, m, name)
            assert np.array_equal(b, mb) and np.array_equal(c, mc) and b.dtype == c.dtype == np.int32, (name, n, m)
            assert c.shape[1] <= (1 if name == "nearest" else int(np.ceil(A.SUPPORT[name] * max(n / m, 1.0))) * 2 + 1)
    b, c = resample_tables(83, 40)
    assert np.array_equal(c, M.tables(83, 40)[1]) and np.array_equal(c, resample_tables(83, 40, "bilinear")[1])
    assert (resample_tables(83, 40, "lanczos")[1] < 0).any()          # negative lobes: rounded away from zero by -0.5
    with pytest.raises(ValueError, match="unknown filter"):
        resample_tables(8, 4, "gauss")


# ---- the host side, with the model standing in for the kernels
@pytest.fixture
def host_chain(monkeypatch):
    from os2d_amd.engine import image_pyramid as IP
    calls = []

    def resize_image(u8, target_size, crop_xyxy=None, hflip=False, vflip=False, device=None, filter="bilinear", pad=False):
        calls.append(("resize", tuple(crop_xyxy), filter))
        win = A.padded_window(u8.numpy(), crop_xyxy, hflip, vflip)
        return torch.from_numpy(A.resize_u8(win, target_size.w, target_size.h, filter))

    def distort_image(u8, ops, to_float=False, img_normalization=None, device=None):
        calls.append(("color", list(ops), to_float))
        out = A.color_chain(u8.numpy(), ops)
        return torch.from_numpy(M.to_float(out, img_normalization)) if to_float else torch.from_numpy(out)

    def _resample(x, window, hflip, vflip, ow, oh, lut, filter="bilinear", padded=False):
        calls.append(("level", tuple(window), filter))
        img = x[0].numpy()
        x0, y0, w, h = window
        assert not hflip and not vflip and (x0, y0, w, h) == (0, 0, img.shape[1], img.shape[0])
        return torch.from_numpy(M.to_float(A.resize_u8(img, ow, oh, filter), lut))[None]

    monkeypatch.setattr(IP, "upload_image", lambda u8, device=None: u8)
    monkeypatch.setattr(IP, "resize_image", resize_image)
    monkeypatch.setattr(IP, "distort_image", distort_image)
    monkeypatch.setattr(IP, "_resample", _resample)
    monkeypatch.setattr(IP, "_device_lut", lambda norm, device: norm)
    return calls


def run_case(z, image=None):
    """-> the 5-tuple of transform_image_to_pyramid for a recorded case, from its seed"""
    from os2d_amd.engine.augmentation import DataAugmentation, transform_image_to_pyramid
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    cw, ch, crop_scale, jitter_ar, scale_jitter, color, min_cov = z["params"].tolist()
    aug = DataAugmentation(random_flip_batches=False, random_crop_size=FeatureMapSize(w=int(cw), h=int(ch)), random_crop_scale=crop_scale,
                           jitter_aspect_ratio=jitter_ar, scale_jitter=scale_jitter, random_color_distortion=bool(color),
                           random_crop_label_images=False, min_box_coverage=min_cov)
    size = FeatureMapSize(w=z["image"].shape[1], h=z["image"].shape[0])
    boxes = BoxList(torch.from_numpy(z["boxes"]).clone(), size) if z["has_boxes"] else None
    mined = dict(crop_position_xyxy=BoxList(torch.from_numpy(z["mined"]).clone().view(1, 4), size)) if len(z["mined"]) else None
    random.seed(int(z["seed"]))
    torch.manual_seed(int(z["seed"]))
    image = torch.from_numpy(z["image"]) if image is None else image
    out = transform_image_to_pyramid(image, boxes, aug, hflip=bool(z["hflip"]), vflip=bool(z["vflip"]),
                                     pyramid_scales=tuple(z["scales"].tolist()), mined_data=mined, img_normalization=M.IMAGENET)
    if mined is not None:
        assert torch.equal(mined["crop_position_xyxy"].bbox_xyxy, torch.from_numpy(z["mined"]).view(1, 4))     # not shifted in place
    return out


def check_case(z, out, name):
    """everything but the image tensors: boxes, fates, inverse transforms (run, and traced as a box-op chain)"""
    from os2d_amd.modeling.box_ops import apply_box_ops, as_box_ops, trace_box_transform
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    levels, boxes_pyramid, cut, diff, inverse = out
    n = len(z["scales"])
    assert len(levels) == len(boxes_pyramid) == len(inverse) == n
    assert cut.dtype == diff.dtype == torch.bool
    assert np.array_equal(cut.numpy(), z["mask_cutoff"]) and np.array_equal(diff.numpy(), z["mask_difficult"]), name
    for i in range(n):
        u8 = z["u8_{}".format(i)]
        size = FeatureMapSize(w=u8.shape[1], h=u8.shape[0])
        assert boxes_pyramid[i].image_size == size and torch.equal(boxes_pyramid[i].bbox_xyxy, torch.from_numpy(z["boxes_{}".format(i)]))
        back = inverse[i](BoxList(PROBE.clone(), size))
        assert torch.equal(back.bbox_xyxy, torch.from_numpy(z["inv_probe_{}".format(i)])), (name, i)
        assert [back.image_size.w, back.image_size.h] == z["inv_size_{}".format(i)].tolist()
        traced = trace_box_transform(inverse[i], size)
        assert traced is not None and traced[2] == back.image_size
        assert torch.equal(apply_box_ops(PROBE, as_box_ops(inverse[i], size)), back.bbox_xyxy)


@pytest.mark.parametrize("name", CASES)
def test_host_search_reproduces_the_reference_from_the_seed(name, host_chain):
    z = load(name)
    out = run_case(z)
    check_case(z, out, name)
    pad = z["padding"]
    x0, y0, x1, y1 = z["window"].tolist()
    kind, window, crop_filter = host_chain[0]
    assert kind == "resize" and window == (x0 - pad[0], y0 - pad[1], x1 - pad[0], y1 - pad[1])       # the view's own coordinates
    chosen = [crop_filter] + [c[2] for c in host_chain if c[0] == "level"]
    colour = [c for c in host_chain if c[0] == "color"]
    assert len(colour) == (len(z["color_ops"]) > 0)
    expected = [A.FILTERS[i] for i in z["filters"]]
    if colour:
        assert colour[0][1] == [(int(k), float(f)) for k, f in z["color_ops"]]
        if colour[0][2]:            # one level of the image's own size: it comes out of the colour kernel as floats, its filter unused
            expected = expected[:1]
    assert chosen == expected
    for i, lvl in enumerate(out[0]):
        assert lvl.dtype == torch.float32 and torch.equal(lvl, torch.from_numpy(M.to_float(z["u8_{}".format(i)]))), (name, i)


def test_box_intersection_over_reference():
    from os2d_amd.structures.bounding_box import BoxList, box_intersection_over_reference
    from os2d_amd.structures.feature_map import FeatureMapSize
    size = FeatureMapSize(w=100, h=80)
    ref = BoxList(torch.tensor([[0.0, 0.0, 10.0, 10.0], [20.0, 20.0, 40.0, 30.0]]), size)
    win = BoxList(torch.tensor([[5.0, 0.0, 30.0, 25.0]]), size)
    assert torch.equal(box_intersection_over_reference(ref, win), torch.tensor([[0.5], [0.25]]))
    assert tuple(box_intersection_over_reference(BoxList.create_empty(size), win).shape) == (0, 1)
    with pytest.raises(RuntimeError, match="same image size"):
        box_intersection_over_reference(ref, BoxList(win.bbox_xyxy, FeatureMapSize(w=99, h=80)))


def test_mined_crop_that_does_not_fit_is_refused(host_chain):
    from os2d_amd.structures import transforms as T
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    img = torch.zeros(20, 30, 3, dtype=torch.uint8)
    view, _, _, _ = T.crop(img, crop_position=BoxList(torch.tensor([[-3.5, 2.0, 10.0, 25.75]]), FeatureMapSize(w=30, h=20)))
    assert view.window == (-3, 2, 10, 25)             # int() truncates towards zero: -3.5 pads 3 columns
    with pytest.raises(AssertionError, match="one box"):
        T.crop(img, crop_position=BoxList(torch.zeros(2, 4), FeatureMapSize(w=30, h=20)))


# ---- libos2d_augment.so: the record, the header, the binding and the built file agree; refusals before any launch (no GPU)
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KERNELS = ("resample_kernel", "color_kernel", "color_luma_kernel")


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import build, _augment_lib
    build.build_augment(verbose=False)
    return _augment_lib.load()


def test_augment_library_record_header_binding_and_exports_agree(lib):
    import re
    import subprocess
    from os2d_amd import build, _augment_lib, _image_lib
    rec = build.AUGMENT
    assert rec not in build.LIBRARIES and build.ALL_LIBRARIES == build.LIBRARIES + [rec] and _augment_lib.LIBRARY.record is rec
    assert (rec.name, rec.env, rec.header) == ("libos2d_augment.so", "OS2D_AUGMENT_LIB", "os2d_augment.h")
    assert build.up_to_date(rec) and os.path.exists(build.AUGMENT_LIB_PATH + ".srchash")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", rec.header)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(os2d_[a-z0-9_]+)\s*\(", text))) == sorted(_augment_lib.SIGNATURES)
    assert re.search(r"^#define OS2D_AUGMENT_ABI_VERSION (\d+)$", text, flags=re.M).group(1) == str(_augment_lib.ABI_VERSION) == "1"
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.AUGMENT_LIB_PATH]).decode()
    assert set(re.findall(r" T (os2d_\w+)", out)) == set(_augment_lib.SIGNATURES)
    assert "os2d_error_text" not in out and "os2d_set_error" not in out
    assert lib.os2d_augment_abi_version() == 1
    # the padded resample takes the arguments of the plain one
    assert _augment_lib.SIGNATURES["os2d_augment_resample_padded"] == _image_lib.SIGNATURES["os2d_image_resample"]
    for define, value in (("MAX_RATIO", 16), ("COLOR_MAX_OPS", _augment_lib.COLOR_MAX_OPS), ("COLOR_SLOTS", _augment_lib.COLOR_SLOTS),
                          ("COLOR_BRIGHTNESS", 1), ("COLOR_CONTRAST", 2), ("COLOR_SATURATION", 3), ("COLOR_HUE", 4), ("COLOR_TO_HSV", 5),
                          ("COLOR_FROM_HSV", 6)):
        assert re.search(r"^#define OS2D_AUGMENT_{} {}\b".format(define, value), text, flags=re.M), define


def test_augment_library_flags_includes_and_stamp(tmp_path):
    from os2d_amd import build
    rec = build.AUGMENT
    for s in rec.sources:           # the library's plain flags: no packed FP32, no per-unit contraction switch
        assert build.unit_flags(rec, s) == build.FLAGS + build.PACKED_OFF and os.path.exists(os.path.join(rec.csrc, s))
    assert all(not set(rec.sources) & set(other.sources) and rec.csrc != other.csrc for other in build.LIBRARIES)
    names = {os.path.basename(h) for h in build.headers(rec)}
    assert {"resample_kernel.h", "image_common.h", "abi_common.h", "os2d_augment.h"} <= names
    for path in [os.path.join(rec.csrc, s) for s in rec.sources] + build.headers(rec):
        for inc in build.local_includes(path):
            assert os.path.basename(inc) in names, (path, inc)
    assert not ({os.path.basename(h) for h in build.headers(build.HIP)} - {"abi_common.h"}) & names          # none of csrc/*.h
    h0 = build.source_hash(rec)
    assert build.source_hash(rec._replace(flags=rec.flags + ["-DX"])) != h0
    (tmp_path / "new_header.h").write_text("// new\n")
    assert build.source_hash(rec._replace(header_dirs=rec.header_dirs + [str(tmp_path)])) != h0
    # the image library is stamped with the shared kernel template too
    assert "resample_kernel.h" in {os.path.basename(h) for h in build.headers(build.IMAGE)}


def test_augment_kernels_are_the_listed_set_and_do_not_spill(lib):
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    ks = codeobj.kernels(build.AUGMENT_LIB_PATH)
    # padded resample: float planes and uint8 HWC; colour: float planes and uint8 HWC, the luma sum
    assert len(ks) == 5 and sum("resample_kernel" in n for n in ks) == 2
    for n, k in ks.items():
        assert any(name in n for name in KERNELS), n
        assert not (k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]), (n, k)
    assert len(codeobj.kernels(build.IMAGE_LIB_PATH)) == 2          # the image library keeps its two


def test_augment_sources_have_no_atomics_and_no_inline_assembly():
    import re
    from os2d_amd import build
    for path in [os.path.join(build.AUGMENT_CSRC, s) for s in build.AUGMENT_SOURCES] + [os.path.join(build.IMAGE_CSRC, "resample_kernel.h")]:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert not re.search(r"atomic\w*\s*\(", code) and "asm" not in code, path


def test_augment_library_keeps_its_own_error_text(lib):
    from os2d_amd import _image_lib
    image = _image_lib.load()
    before = image.os2d_image_last_error()
    assert _color(lib, ctypes.c_void_p(256), n_ops=-1) == -1 and b"operations" in lib.os2d_augment_last_error()
    assert image.os2d_image_last_error() == before


def _padded(lib, fake, **over):
    a = dict(src=fake, A=1, img_w=64, img_h=48, row_pitch=192, image_stride=192 * 48, x0=-4, y0=-6, w=64, h=48, hflip=0, vflip=0,
             xcoef=fake, xbounds=fake, xbounds_host=fake, kx=5, ycoef=fake, ybounds=fake, ybounds_host=fake, ky=5, ow=32, oh=24,
             lut=fake, out=fake, out_u8=0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.os2d_augment_resample_padded(*a.values())


def test_padded_resample_refuses_bad_arguments(lib):
    fake = ctypes.c_void_p(256)
    err = lib.os2d_augment_last_error
    for name in ("src", "xcoef", "xbounds", "xbounds_host", "ycoef", "ybounds", "ybounds_host", "out", "lut"):
        assert _padded(lib, fake, **{name: None}) == -1 and b"null" in err(), name
    for bad in (dict(x0=64), dict(y0=48), dict(x0=-64), dict(y0=-48), dict(x0=-100, w=100), dict(x0=10 ** 6), dict(y0=-(10 ** 6))):
        assert _padded(lib, fake, **bad) == -1 and b"no pixel inside the image" in err(), bad
    for bad in (dict(x0=-(2 ** 30) - 1), dict(w=2 ** 30 + 1, ow=2 ** 30), dict(h=2 ** 31 - 1, oh=2 ** 30)):
        assert _padded(lib, fake, **bad) == -1 and b"2^30" in err(), bad
    assert _padded(lib, fake, w=0) == -1 and b"shape" in err()
    assert _padded(lib, fake, ow=3) == -1 and b"ratio" in err()
    # an overhanging window passes the window rule: the next check (the host bounds table) refuses
    bad_bounds = np.stack([np.arange(32) * 2, np.full(32, 9)], 1).astype(np.int32)
    assert _padded(lib, fake, xbounds_host=ctypes.c_void_p(bad_bounds.ctypes.data), ybounds_host=ctypes.c_void_p(bad_bounds.ctypes.data)) == -1
    assert b"bounds" in err()
    # the plain entry point still refuses what leaves the image
    from test_image_abi import _call
    from os2d_amd import _image_lib
    image = _image_lib.load()
    assert _call(image, fake, x0=-1) == -1 and b"window outside the image" in image.os2d_image_last_error()


def _color(lib, fake, kinds=(1,), factors=(0.5,), null=(), **over):
    k = (ctypes.c_int * 8)(*kinds)
    f = (ctypes.c_double * 8)(*factors)
    a = dict(src=fake, w=64, h=48, row_pitch=192, n_ops=len(kinds), kinds=k, factors=f, lut=fake, out=fake, out_u8=0, sums=fake, stream=None)
    assert set(over) <= set(a) and set(null) <= set(a)
    a.update(over)
    a.update({name: None for name in null})
    return lib.os2d_augment_color(*a.values())


def test_color_refuses_bad_arguments(lib):
    fake = ctypes.c_void_p(256)
    err = lib.os2d_augment_last_error
    for name in ("src", "out", "lut", "kinds", "factors"):
        assert _color(lib, fake, null=(name,)) == -1 and b"null" in err(), name
    assert _color(lib, fake, kinds=(1, 2), factors=(1.0, 1.0), sums=None) == -1 and b"null" in err()        # contrast needs the workspace
    assert _color(lib, fake, kinds=(1, 2, 3, 4, 1), factors=(1.0,) * 5) == -1 and b"more than 4 operations" in err()
    assert _color(lib, fake, n_ops=-1) == -1 and b"operations" in err()
    for kind in (0, 7, -1):
        assert _color(lib, fake, kinds=(1, kind), factors=(1.0, 1.0)) == -1 and b"unknown operation kind" in err(), kind
    assert _color(lib, fake, kinds=(2, 3, 2), factors=(1.0,) * 3) == -1 and b"more than one contrast" in err()
    for f in (float("nan"), float("inf"), -2e6):
        assert _color(lib, fake, factors=(f,)) == -1 and b"factor" in err(), f
    for bad in (dict(w=0), dict(h=0), dict(row_pitch=191), dict(w=2 ** 16, h=2 ** 15, row_pitch=3 * 2 ** 16)):
        assert _color(lib, fake, **bad) == -1 and b"shape" in err(), bad
    assert _color(lib, fake, out=ctypes.c_void_p(264)) == -1 and b"aligned" in err()
    assert _color(lib, fake, lut=ctypes.c_void_p(258)) == -1 and b"aligned" in err()
    assert _color(lib, fake, kinds=(2,), factors=(1.0,), sums=ctypes.c_void_p(260)) == -1 and b"aligned" in err()
