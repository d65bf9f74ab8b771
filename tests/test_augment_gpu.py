"""GPU: the training images made on the device (libos2d_augment.so: os2d_augment_resample_padded, os2d_augment_color;
engine/augmentation.py) have exactly PIL's bits - against the fixtures recorded from the reference (tests/golden/augment_*.npz),
PIL's own checksums over all 2^24 colours, and tests/augment_model.py (held to both by tests/test_augment_model.py) where a
shape is not recorded.  Every comparison is ``torch.equal``."""
import os

import numpy as np
import pytest
import torch

import augment_model as A
import image_model as M
import test_augment_model as TA

pytestmark = pytest.mark.gpu

SRC_W, SRC_H = 83, 61
WINDOWS = dict(left_top=(-7, -5, 40, 33), right_bottom=(50, 35, 95, 70), all_sides=(-6, -4, 90, 66), one_pixel=(82, 60, 120, 90),
               whole=(0, 0, SRC_W, SRC_H))
FLIPS = ((False, False), (True, False), (False, True), (True, True))


def fms(w, h):
    from os2d_amd.structures.feature_map import FeatureMapSize
    return FeatureMapSize(w=w, h=h)


@pytest.fixture(scope="module")
def src():
    return np.random.RandomState(70).randint(0, 256, size=(SRC_H, SRC_W, 3)).astype(np.uint8)


def model_resize(img, window, hflip, vflip, ow, oh, name):
    return A.resize_u8(A.padded_window(img, window, hflip, vflip), ow, oh, name)


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_padded_windows_with_and_without_flips(window, src, device):
    from os2d_amd.engine.image_pyramid import resize_image
    win = WINDOWS[window]
    for hflip, vflip in FLIPS:
        got = resize_image(torch.from_numpy(src), fms(48, 40), crop_xyxy=win, hflip=hflip, vflip=vflip, device=device, pad=True)
        assert got.dtype == torch.uint8 and got.device == device and tuple(got.shape) == (40, 48, 3)
        assert torch.equal(got.cpu(), torch.from_numpy(model_resize(src, win, hflip, vflip, 48, 40, "bilinear"))), (window, hflip, vflip)
        if window == "whole":           # the padded instantiation on a window inside the image: the plain entry point's bits
            assert torch.equal(got, resize_image(torch.from_numpy(src), fms(48, 40), crop_xyxy=win, hflip=hflip, vflip=vflip, device=device))
    if window == "one_pixel":
        unit = resize_image(torch.from_numpy(src), fms(38, 30), crop_xyxy=win, device=device, pad=True)     # no resize: the pixel and zeros
        assert int(unit.sum()) == int(src[60, 82].sum()) and torch.equal(unit[0, 0].cpu(), torch.from_numpy(src[60, 82]))
    with pytest.raises(ValueError, match="no pixel"):
        resize_image(torch.from_numpy(src), fms(48, 40), crop_xyxy=(SRC_W, 0, SRC_W + 10, 10), device=device, pad=True)


@pytest.mark.parametrize("name", A.FILTERS)
def test_every_filter_up_and_down_on_an_overhanging_window(name, src, device):
    """200 output columns cross the seam of the 128-column tiles (with LANCZOS: the widest taps on both sides of it)."""
    from os2d_amd.engine.image_pyramid import resize_image
    win = WINDOWS["all_sides"]
    for (ow, oh), (hflip, vflip) in (((200, 150), (False, False)), ((31, 23), (True, True)), ((96, 23), (False, True))):
        got = resize_image(torch.from_numpy(src), fms(ow, oh), crop_xyxy=win, hflip=hflip, vflip=vflip, device=device, filter=name, pad=True)
        assert torch.equal(got.cpu(), torch.from_numpy(model_resize(src, win, hflip, vflip, ow, oh, name))), (name, ow, oh)
    inside = resize_image(torch.from_numpy(src), fms(200, 150), device=device, filter=name)         # the plain entry point, new tables
    assert torch.equal(inside.cpu(), torch.from_numpy(A.resize_u8(src, 200, 150, name)))


@pytest.mark.parametrize("w,h,ow,oh", [(160, 3, 10, 3), (3, 160, 3, 10)])
def test_lanczos_at_ratio_16(w, h, ow, oh, device):
    """97 taps per output position: the staged rows of one output row still fit"""
    from os2d_amd.engine.image_pyramid import resize_image
    img = np.random.RandomState(71).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    for name in ("lanczos", "bicubic"):
        got = resize_image(torch.from_numpy(img), fms(ow, oh), device=device, filter=name)
        assert torch.equal(got.cpu(), torch.from_numpy(A.resize_u8(img, ow, oh, name))), name


def test_batch_of_two_and_float_planes(src, device):
    from os2d_amd.engine import image_pyramid as IP
    other = np.random.RandomState(72).randint(0, 256, size=(SRC_H, SRC_W, 3)).astype(np.uint8)
    batch = torch.from_numpy(np.stack([src, other])).to(device)
    lut = IP._device_lut(M.IMAGENET, device)
    x0, y0, x1, y1 = WINDOWS["all_sides"]
    for name, (ow, oh) in (("lanczos", (200, 37)), ("box", (45, 150))):
        u8 = IP._resample(batch, (x0, y0, x1 - x0, y1 - y0), False, False, ow, oh, None, name, True)
        fl = IP._resample(batch, (x0, y0, x1 - x0, y1 - y0), False, False, ow, oh, lut, name, True)
        assert tuple(u8.shape) == (2, oh, ow, 3) and tuple(fl.shape) == (2, 3, oh, ow) and fl.dtype == torch.float32
        for a, img in enumerate((src, other)):
            ref = model_resize(img, WINDOWS["all_sides"], False, False, ow, oh, name)
            assert torch.equal(u8[a].cpu(), torch.from_numpy(ref)) and torch.equal(fl[a].cpu(), torch.from_numpy(M.to_float(ref))), (name, a)
    levels, _ = IP.ImagePyramidBuilder((0.5, 1.4), M.IMAGENET, device).build(batch, filters=("hamming", "nearest"))
    for lvl, s, name in zip(levels, (0.5, 1.4), ("hamming", "nearest")):
        for a, img in enumerate((src, other)):
            assert torch.equal(lvl[a].cpu(), torch.from_numpy(M.to_float(A.resize_u8(img, int(SRC_W * s), int(SRC_H * s), name))))


# ---- colour
def color_both(img, ops, device, norm=M.IMAGENET):
    """(uint8 HWC, float planes) of the device for a numpy image"""
    from os2d_amd.engine.image_pyramid import distort_image
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(img)
    return distort_image(t, ops, device=device), distort_image(t, ops, to_float=True, img_normalization=norm, device=device)


def check_color(img, ops, device, what):
    ref = A.color_chain(img, ops)
    u8, fl = color_both(img, ops, device)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == img.shape and tuple(fl.shape) == (3,) + img.shape[:2]
    assert torch.equal(u8.cpu(), torch.from_numpy(ref)), what
    assert torch.equal(fl.cpu(), torch.from_numpy(M.to_float(ref))), what


@pytest.fixture(scope="module")
def odd_image():
    """333x251: neither the pixel count nor a plane's start is a multiple of 4 elements"""
    return np.random.RandomState(73).randint(0, 256, size=(251, 333, 3)).astype(np.uint8)


@pytest.mark.parametrize("kind", [A.BRIGHTNESS, A.CONTRAST, A.SATURATION, A.HUE])
def test_each_operation_alone(kind, odd_image, device):
    for factor in (0.0, 1.0, 0.37, 1.73) if kind != A.HUE else (0.0, 1.0, 0.37, -0.21):
        check_color(odd_image, [(kind, factor)], device, (kind, factor))


@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (4, 1), (64, 64)])
def test_small_images_and_full_chains(w, h, device):
    img = np.random.RandomState(74 + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    for name in ("color_csh", "color_shc"):
        ops = [(int(k), float(f)) for k, f in TA.load(name)["color_ops"]]
        assert len(ops) == 4
        check_color(img, ops, device, (name, w, h))
    check_color(img, [], device, "empty chain")


def test_full_chains_contrast_positions_pitch_uniform_and_repeat(odd_image, device):
    from os2d_amd.engine.image_pyramid import distort_image
    csh = [(int(k), float(f)) for k, f in TA.load("color_csh")["color_ops"]]
    shc = [(int(k), float(f)) for k, f in TA.load("color_shc")["color_ops"]]
    first = [(A.CONTRAST, 1.4), (A.BRIGHTNESS, 0.8), (A.HUE, 0.07)]
    middle = [(A.SATURATION, 1.3), (A.CONTRAST, 0.6), (A.HUE, -0.05), (A.BRIGHTNESS, 1.1)]
    last = [(A.BRIGHTNESS, 1.12), (A.HUE, 0.09), (A.SATURATION, 0.5), (A.CONTRAST, 1.5)]
    for ops in (csh, shc, first, middle, last):
        check_color(odd_image, ops, device, ops)
    # a row pitch larger than the row: a view of a wider image
    wide = torch.zeros(251, 340, 3, dtype=torch.uint8, device=device)
    wide[:, 4:337] = torch.from_numpy(odd_image).to(device)
    view = wide[:, 4:337]
    assert view.stride(0) == 340 * 3
    a = distort_image(view, middle)
    assert torch.equal(a.cpu(), torch.from_numpy(A.color_chain(odd_image, middle)))
    assert torch.equal(distort_image(view, middle), a) and torch.equal(distort_image(view, middle, to_float=True), distort_image(view, middle, to_float=True))
    uniform = np.full((37, 53, 3), 0, np.uint8)
    uniform[:] = (12, 200, 77)
    for ops in (csh, last, [(A.CONTRAST, 0.0)], [(A.SATURATION, 0.0)]):
        check_color(uniform, ops, device, ("uniform", ops))
    with pytest.raises(RuntimeError, match="more than one contrast"):
        distort_image(view, [(A.CONTRAST, 1.0), (A.CONTRAST, 1.0)])


@pytest.mark.parametrize("key", ["rgb_to_hsv", "hsv_to_rgb", "hue_23", "hue_231"])
def test_every_colour_against_pils_checksums(key, device):
    from os2d_amd.engine import image_pyramid as IP
    sums = torch.from_numpy(np.load(os.path.join(TA.GOLDEN, "augment_color_checksums.npz"))[key])
    i = torch.arange(1 << 24, dtype=torch.int32, device=device).view(4096, 4096)
    allc = torch.stack([i >> 16, (i >> 8) & 255, i & 255], -1).to(torch.uint8)
    ops = dict(rgb_to_hsv=[(IP.TO_HSV, 0.0)], hsv_to_rgb=[(IP.FROM_HSV, 0.0)], hue_23=[(IP.HUE, 0.0903)], hue_231=[(IP.HUE, -0.0984)])[key]
    got = IP.distort_image(allc, ops)
    col = torch.arange(1, 4097, dtype=torch.int64, device=device)[None, :, None]
    assert torch.equal((got.to(torch.int64) * col).sum(1).cpu(), sums)


# ---- end to end
@pytest.mark.parametrize("name", TA.CASES)
def test_transform_image_to_pyramid_against_the_fixtures(name, device):
    z = TA.load(name)
    out = TA.run_case(z, torch.from_numpy(z["image"]).to(device))
    TA.check_case(z, out, name)
    for i, lvl in enumerate(out[0]):
        u8 = z["u8_{}".format(i)]
        assert lvl.dtype == torch.float32 and lvl.device == device and tuple(lvl.shape) == (3,) + u8.shape[:2]
        assert torch.equal(lvl.cpu(), torch.from_numpy(M.to_float(u8))), (name, i)


def test_second_call_does_not_synchronise(device):
    z = TA.load("pyramid")
    image = torch.from_numpy(z["image"]).to(device)
    first = TA.run_case(z, image)               # library load, tables of these sizes uploaded
    mined = TA.load("mined_all")
    first_mined = TA.run_case(mined, image)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):           # the mode is in force: a copy to the host is an error
            float(first[0][0].sum())
        second = TA.run_case(z, image)
        second_mined = TA.run_case(mined, image)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(second[0]) == 3 and all(torch.equal(a, b) for a, b in zip(first[0] + first_mined[0], second[0] + second_mined[0]))


def test_class_image_chain(device):
    """``transform_image_gt``: flips, colour, the label-image crop and the aspect-preserving resize, against the model with the
    same draws"""
    import random
    from os2d_amd.engine.augmentation import DataAugmentation, transform_image_gt
    from os2d_amd.engine.image_pyramid import class_image_size
    from os2d_amd.structures import transforms as T
    img = np.random.RandomState(75).randint(0, 256, size=(57, 90, 3)).astype(np.uint8)
    aug = DataAugmentation(random_flip_batches=False, random_crop_size=fms(48, 40), random_crop_scale=1.0, jitter_aspect_ratio=0.8,
                           scale_jitter=0.7, random_color_distortion=True, random_crop_label_images=True, min_box_coverage=0.7)
    plain = transform_image_gt(torch.from_numpy(img), None, hflip=True, gt_image_size=64, device=device)
    size = class_image_size(90, 57, 64)
    assert torch.equal(plain.cpu(), torch.from_numpy(M.to_float(A.resize_u8(np.ascontiguousarray(img[:, ::-1]), size.w, size.h))))
    for seed in range(4):
        random.seed(seed)
        torch.manual_seed(seed)
        got = transform_image_gt(torch.from_numpy(img), aug, vflip=True, gt_image_size=64, device=device)
        random.seed(seed)
        torch.manual_seed(seed)
        ops = aug.draw_distortion()
        ref = A.color_chain(np.ascontiguousarray(img[::-1]), ops)
        ar = 90 / 57
        new_ar = random.uniform(ar * 0.8, ar / 0.8)
        cw, ch = int(min(90, 57 * new_ar)), int(min(90 / new_ar, 57))
        view = T.crop(torch.from_numpy(ref), random_crop_size=fms(cw, ch), scale_jitter=0.7, jitter_aspect_ratio=0.8)[0]
        x0, y0, x1, y1 = view.window
        ref = ref[y0:y1, x0:x1]
        size = class_image_size(x1 - x0, y1 - y0, 64)
        ref = A.resize_u8(np.ascontiguousarray(ref), size.w, size.h, T.choose_filter(True))
        assert torch.equal(got.cpu(), torch.from_numpy(M.to_float(ref))), seed


def test_mined_records_go_in(device):
    """Records of ``mine_hard_patches`` (the recorded scores of tests/golden/mining_pyr.npz) on a synthetic image: every
    ``crop_position_xyxy`` gives a crop of the training size with the model's bits, whether or not it leaves the image."""
    import mining_cases as MC
    import test_mining_gpu as TM
    from os2d_amd.engine import mining
    from os2d_amd.engine.augmentation import DataAugmentation, transform_image_to_pyramid
    from os2d_amd.engine.objective import Os2dObjective
    name = "pyr"
    c, fx, coder = MC.CASES[name], MC.load(name), TM.make_coder(name)
    imgs, fm = TM.fms(name)
    L = range(len(imgs))
    scores = ([torch.from_numpy(fx["loc_{}".format(l)][0]).to(device) for l in L], [torch.from_numpy(fx["cls_{}".format(l)][0]).to(device) for l in L],
              [torch.from_numpy(fx["corners_{}".format(l)][0]).to(device) for l in L], fm)
    records, _ = mining.mine_hard_patches_for_image(None, Os2dObjective(MC.LOSS, **MC.CRITERION), coder, imgs, None, MC.CLASS_IDS, TM.gt_boxes(fx, 0),
                                                    fms(*MC.ORIG), fms(*MC.CROP), image_id=0, nms_iou_threshold=MC.NMS_IOU,
                                                    num_hard_patches=c["K"], scores=scores, box_transforms=TM.transforms(name))
    assert len(records) > 0
    image = np.random.RandomState(76).randint(0, 256, size=(MC.ORIG[1], MC.ORIG[0], 3)).astype(np.uint8)
    on_device = torch.from_numpy(image).to(device)
    aug = DataAugmentation(random_flip_batches=False, random_crop_size=fms(*MC.CROP), random_crop_scale=1.0, jitter_aspect_ratio=0.9,
                           scale_jitter=0.7, random_color_distortion=False, random_crop_label_images=False, min_box_coverage=0.7)
    gt = TM.gt_boxes(fx, 0)
    overhang = 0
    for rec in records:
        levels, boxes, cut, diff, inverse = transform_image_to_pyramid(on_device, gt, aug, mined_data=rec, img_normalization=M.IMAGENET)
        assert tuple(levels[0].shape) == (3, MC.CROP[1], MC.CROP[0]) and len(cut) == len(diff) == len(gt) == len(boxes[0])
        x0, y0, x1, y1 = [int(v) for v in rec["crop_position_xyxy"].bbox_xyxy[0]]
        overhang += x0 < 0 or y0 < 0 or x1 > MC.ORIG[0] or y1 > MC.ORIG[1]
    print("\n[augment] {} mined records, {} leave the image".format(len(records), overhang))
