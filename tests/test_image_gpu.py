"""GPU: the image pyramid built on the device from uint8 images (libos2d_image.so, engine/image_pyramid.py) has exactly the
reference's bits - the recorded fixtures of PIL + ToTensor + Normalize, and tests/image_model.py where a shape is too large to
store - and ``detect_raw_images`` / ``evaluate(pyramid_scales=...)`` give what the host-built pyramids give.  Every comparison
is ``torch.equal``."""
import os

import numpy as np
import pytest
import torch

import image_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PYRAMIDS = ("image_pyramid_small", "image_pyramid_ratios", "image_pyramid_thin")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def random_image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def model_levels(images, scales=M.DEFAULT_SCALES, norm=M.IMAGENET):
    """[A,3,h_l,w_l] float tensors of the numpy model for a list of equally sized uint8 images"""
    per_image = [M.pyramid(img, scales, norm) for img in images]
    return [torch.from_numpy(np.concatenate([p[i] for p in per_image], 0)) for i in range(len(scales))]


def builder(device, scales=M.DEFAULT_SCALES, norm=M.IMAGENET):
    from os2d_amd.engine.image_pyramid import ImagePyramidBuilder
    return ImagePyramidBuilder(scales=scales, img_normalization=norm, device=device)


@pytest.fixture(scope="module")
def seams():
    """333x251: widths and heights that are multiples of no tile size, several tiles per axis at the larger scales"""
    images = [random_image(333, 251, 7), random_image(333, 251, 8)]
    return dict(images=images, single=model_levels(images[:1]), both=model_levels(images))


@pytest.mark.parametrize("name", PYRAMIDS)
def test_pyramid_fixtures(name, device):
    from os2d_amd.engine.image_pyramid import resize_image
    from os2d_amd.engine.pyramid import pyramid_sizes
    from os2d_amd.structures.feature_map import FeatureMapSize
    z = load(name)
    img = torch.from_numpy(z["image"])
    scales = tuple(float(s) for s in z["scales"])
    levels, sizes = builder(device, scales).build(img)
    assert sizes == pyramid_sizes(FeatureMapSize(w=img.size(1), h=img.size(0)), scales) and len(levels) == len(scales)
    for i, (lvl, size) in enumerate(zip(levels, sizes)):
        u8 = z["u8_{}".format(i)]
        assert lvl.dtype == torch.float32 and lvl.device == device and tuple(lvl.shape) == (1, 3, size.h, size.w) == (1, 3) + u8.shape[:2]
        assert torch.equal(lvl.cpu()[0], torch.from_numpy(M.to_float(u8))), (name, i)
        if "float_{}".format(i) in z.files:
            assert torch.equal(lvl.cpu()[0], torch.from_numpy(z["float_{}".format(i)])), (name, i)
        got = resize_image(img, size, device=device)
        assert got.dtype == torch.uint8 and got.device == device and torch.equal(got.cpu(), torch.from_numpy(u8)), (name, i)
    if name == "image_pyramid_small":
        assert all("float_{}".format(i) in z.files for i in range(7))
        plain, _ = builder(device, scales, norm=None).build(img.to(device))          # ToTensor alone
        for i, lvl in enumerate(plain):
            assert torch.equal(lvl.cpu()[0], torch.from_numpy(M.to_float(z["u8_{}".format(i)], None)))


def test_flip_crop_chain_fixture(device):
    from os2d_amd.engine.image_pyramid import resize_image
    from os2d_amd.structures.feature_map import FeatureMapSize
    z = load("image_flip_crop")
    img = torch.from_numpy(z["image"])
    target = FeatureMapSize(w=int(z["target"][0]), h=int(z["target"][1]))
    resized = resize_image(img, target, crop_xyxy=tuple(int(v) for v in z["window"]), hflip=True, vflip=True, device=device)
    assert torch.equal(resized.cpu(), torch.from_numpy(z["resized"]))
    levels, sizes = builder(device, (1.0,)).build(resized)
    assert sizes == [target] and torch.equal(levels[0].cpu()[0], torch.from_numpy(M.to_float(z["u8_0"])))
    # the flips of the pyramid builder: the pyramid of the flipped image
    for hflip, vflip in ((True, False), (False, True), (True, True)):
        got, _ = builder(device, (0.625, 1.4)).build(img, hflip=hflip, vflip=vflip)
        ref = M.pyramid(z["image"], (0.625, 1.4), hflip=hflip, vflip=vflip)
        assert all(torch.equal(g.cpu(), torch.from_numpy(r)) for g, r in zip(got, ref)), (hflip, vflip)
    with pytest.raises(ValueError, match="inside"):
        resize_image(img, target, crop_xyxy=(5, 7, 65, 39), device=device)


def test_class_image_fixture(device):
    from os2d_amd.engine.image_pyramid import class_image_tensor
    z = load("image_class")
    for i in range(2):
        u8 = z["u8_{}".format(i)]
        got = class_image_tensor(torch.from_numpy(z["image_{}".format(i)]), gt_image_size=int(z["target_{}".format(i)]), device=device)
        assert tuple(got.shape) == (3,) + u8.shape[:2] and got.device == device
        assert torch.equal(got.cpu(), torch.from_numpy(M.to_float(u8)))
    got = class_image_tensor(torch.from_numpy(z["image_1"]).to(device), gt_image_size=64, img_normalization=None)
    assert torch.equal(got.cpu(), torch.from_numpy(M.to_float(z["u8_1"], None)))


def test_tile_seams_and_partial_tiles(seams, device):
    b = builder(device)
    one, sizes = b.build(torch.from_numpy(seams["images"][0]))
    assert [(s.w, s.h) for s in sizes] == M.pyramid_sizes(333, 251) and sizes[-1].w > 4 * 128 and sizes[-1].h > 16 * 16
    for lvl, (got, ref) in enumerate(zip(one, seams["single"])):
        assert torch.equal(got.cpu(), ref), lvl
    two, _ = b.build(torch.from_numpy(np.stack(seams["images"])))
    for lvl, (got, ref) in enumerate(zip(two, seams["both"])):
        assert tuple(got.shape) == tuple(ref.shape) and got.size(0) == 2 and torch.equal(got.cpu(), ref), lvl


@pytest.mark.parametrize("w,h", [(1, 1), (2, 3)])
def test_tiny_images(w, h, device):
    img = random_image(w, h, 20 + w)
    got, sizes = builder(device, (1.6,)).build(torch.from_numpy(img))
    assert [(s.w, s.h) for s in sizes] == [(int(w * 1.6), int(h * 1.6))]
    assert torch.equal(got[0].cpu(), torch.from_numpy(M.pyramid(img, (1.6,))[0]))


@pytest.mark.parametrize("w,h,ow,oh", [(160, 3, 10, 3), (3, 5, 48, 5), (3, 160, 3, 10), (5, 3, 5, 48)])
def test_ratio_16_on_one_axis(w, h, ow, oh, device):
    from os2d_amd.engine.image_pyramid import resize_image
    from os2d_amd.structures.feature_map import FeatureMapSize
    img = random_image(w, h, 30 + w)
    got = resize_image(torch.from_numpy(img), FeatureMapSize(w=ow, h=oh), device=device)
    assert torch.equal(got.cpu(), torch.from_numpy(M.resize_u8(img, ow, oh)))
    with pytest.raises(ValueError, match="ratio"):      # refused, not truncated
        resize_image(torch.from_numpy(random_image(w + (w > ow) * 16, h + (h > oh) * 16, 1)),
                     FeatureMapSize(w=ow + (ow > w) * 16, h=oh + (oh > h) * 16), device=device)


@pytest.mark.parametrize("w,h,scale", [(160, 16, 1 / 16), (3, 1, 16.0)])
def test_ratio_16_float_planes(w, h, scale, device):
    img = random_image(w, h, 40 + w)
    got, _ = builder(device, (scale,)).build(torch.from_numpy(img))
    assert torch.equal(got[0].cpu(), torch.from_numpy(M.pyramid(img, (scale,))[0]))


def test_batch_of_two_equals_two_singles_and_repeats_give_the_same_bits(seams, device):
    b = builder(device)
    batch = torch.from_numpy(np.stack(seams["images"])).to(device)
    two, _ = b.build(batch)
    again, _ = b.build(batch)
    # a batch that is a strided view: image stride and row pitch of a larger buffer
    big = torch.zeros(2, 260, 340, 3, dtype=torch.uint8, device=device)
    big[:, 4:255, 3:336] = batch
    view, _ = b.build(big[:, 4:255, 3:336])
    singles = [b.build(batch[a])[0] for a in range(2)]
    for lvl in range(len(two)):
        assert torch.equal(two[lvl], again[lvl]) and torch.equal(two[lvl], view[lvl])
        for a in range(2):
            assert torch.equal(two[lvl][a:a + 1], singles[a][lvl])


def test_second_build_does_not_synchronise(device):
    b = builder(device)
    img = torch.from_numpy(random_image(97, 61, 50)).to(device)
    first, _ = b.build(img)                 # library load, tables of this size uploaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second, sizes = b.build(img)
        other, _ = builder(device).build(img)       # the tables are cached per size, not per builder
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(sizes) == 7 and all(torch.equal(a, c) and torch.equal(a, d) for a, c, d in zip(first, second, other))


def test_detect_raw_images_and_evaluate_equal_the_host_pyramids(device, monkeypatch):
    """The small synthetic model of tests/test_model_gpu.py; two uint8 images; the host pyramids are tests/image_model.py's."""
    from test_model_gpu import _model
    from os2d_amd.engine import evaluate as E
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)       # the comparison is call to call through the backbone
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    net, _ = _model(device, seed=5)
    g = torch.Generator().manual_seed(2)
    class_ids = [0, 1, 2]
    head = E.build_class_head(net, [torch.randn(3, 96, 96, generator=g).to(device) for _ in class_ids])
    coder = net.build_box_coder()
    scales = (0.8, 1.2)
    images = [random_image(160, 120, 60), random_image(160, 120, 61)]
    host = [[torch.from_numpy(x) for x in M.pyramid(img, scales)] for img in images]
    assert [tuple(x.shape) for x in host[0]] == [(1, 3, 96, 128), (1, 3, 144, 192)]
    orig = [FeatureMapSize(w=320, h=240), FeatureMapSize(w=300, h=200)]
    kw = dict(orig_sizes=orig, nms_score_threshold=0.0)
    with torch.no_grad():
        list(E.detect_images(net, coder, host, head, class_ids, **kw))          # warm-up: kernel selection of the backbone
        ref = list(E.detect_images(net, coder, host, head, class_ids, **kw))
        got = list(E.detect_raw_images(net, coder, [torch.from_numpy(x) for x in images], head, class_ids, scales=scales,
                                       img_normalization=M.IMAGENET, **kw))
    assert len(got) == len(ref) == 2
    for a, b in zip(got, ref):
        assert len(a) == len(b) > 0 and a.image_size == b.image_size
        assert torch.equal(a.bbox_xyxy, b.bbox_xyxy)
        assert torch.equal(a.get_field("scores"), b.get_field("scores")) and torch.equal(a.get_field("labels"), b.get_field("labels"))
    gts = []
    for det, size in zip(ref, orig):
        top = det.get_field("scores").argsort(descending=True)[:3].cpu()
        b = BoxList(det.bbox_xyxy.cpu()[top], size)
        b.add_field("labels", det.get_field("labels").cpu()[top])
        gts.append(b)
    on_host = E.evaluate(net, coder, host, gts, head, class_ids, mAP_iou_thresholds=(0.5, 0.75), **kw)
    raw = E.evaluate(net, coder, [torch.from_numpy(x) for x in images], gts, head, class_ids, mAP_iou_thresholds=(0.5, 0.75),
                     pyramid_scales=scales, img_normalization=M.IMAGENET, **kw)
    assert list(raw) == list(on_host) and len(raw) == 9 and raw["recall@0.50"] > 0
    for key in raw:
        if key != "eval_time":
            assert raw[key] == on_host[key], key
