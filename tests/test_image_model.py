"""CPU: the numpy model of the image preprocessing (tests/image_model.py) equals every recorded fixture of the reference
(tests/golden/image_*.npz, made by make_image_golden.py with PIL) byte for byte and float bit for bit, and the product's host
tables (engine/image_pyramid.py) equal the model's."""
import os

import numpy as np
import pytest
import torch

import image_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PYRAMIDS = ("image_pyramid_small", "image_pyramid_ratios", "image_pyramid_thin")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_fixtures_are_small():
    for name in PYRAMIDS + ("image_flip_crop", "image_class"):
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 300 * 1024


@pytest.mark.parametrize("name", PYRAMIDS)
def test_model_equals_the_recorded_pyramids(name):
    z = load(name)
    img = z["image"]
    h, w = img.shape[:2]
    sizes = M.pyramid_sizes(w, h, z["scales"])
    for i, (ow, oh) in enumerate(sizes):
        got = M.resize_u8(img, ow, oh)
        assert same_bits(got, z["u8_{}".format(i)]), (name, i)
    if name == "image_pyramid_small":
        assert tuple(z["scales"]) == M.DEFAULT_SCALES
        norm = dict(mean=z["mean"], std=z["std"])
        levels = M.pyramid(img, z["scales"], norm)
        for i, lvl in enumerate(levels):
            assert same_bits(lvl[0], z["float_{}".format(i)]), i
    if name == "image_pyramid_ratios":
        assert [s[0] for s in sizes] == [5, 53, 153] and M.tables(53, 5)[0][:, 1].max() >= 19      # rows of 19 taps and more
        assert same_bits(z["u8_1"], img)                    # scale 1: the identity
    if name == "image_pyramid_thin":
        assert [s[0] for s in sizes] == [1, 6] and tuple(M.tables(13, 1)[0][0]) == (0, 13)    # the window is the whole row


def test_model_equals_the_recorded_flip_crop_chain():
    z = load("image_flip_crop")
    x = M.transpose_crop(z["image"], True, True, tuple(z["window"]))
    assert x.shape == (32, 40, 3)
    resized = M.resize_u8(x, *z["target"])
    assert same_bits(resized, z["resized"])
    assert same_bits(M.resize_u8(resized, 33, 33), z["u8_0"])


def test_model_equals_the_recorded_class_images():
    z = load("image_class")
    for i, expect in enumerate(((301, 190), (80, 50))):
        img = z["image_{}".format(i)]
        w, h = M.class_image_size(img.shape[1], img.shape[0], int(z["target_{}".format(i)]))
        assert (w, h) == expect == z["u8_{}".format(i)].shape[1::-1]
        assert same_bits(M.resize_u8(img, w, h), z["u8_{}".format(i)])
    assert M.class_image_size(1000, 1, 3) == (94, 1)        # a side never becomes 0


def test_product_tables_equal_the_model():
    from os2d_amd.engine import image_pyramid as P
    from os2d_amd.engine.pyramid import DEFAULT_SCALES, pyramid_sizes
    from os2d_amd.structures.feature_map import FeatureMapSize
    assert P.PRECISION_BITS == M.PRECISION_BITS == 22 and DEFAULT_SCALES == M.DEFAULT_SCALES
    for n, m in ((37, 18), (29, 46), (53, 5), (53, 153), (200, 22), (13, 1), (3, 48), (160, 10), (1, 1), (251, 351), (64, 64)):
        bounds, coef = P.resample_tables(n, m)
        mb, mc = M.tables(n, m)
        assert same_bits(bounds, mb) and same_bits(coef, mc), (n, m)
        assert bounds.min() >= 0 and (bounds.sum(1) <= n).all() and (bounds[:, 1] >= 1).all()
    assert P.resample_tables(37, 18) is P.resample_tables(37, 18)        # memoised
    assert same_bits(P.normalization_table(**M.IMAGENET).numpy(), M.normalization_table(M.IMAGENET))
    assert same_bits(P.normalization_table().numpy(), M.normalization_table(None))
    assert P.normalization_table().dtype == torch.float32 and tuple(P.normalization_table().shape) == (3, 256)
    assert tuple(P.IMAGENET_NORMALIZATION["mean"]) == M.IMAGENET["mean"] and tuple(P.IMAGENET_NORMALIZATION["std"]) == M.IMAGENET["std"]
    for w, h in ((1280, 960), (333, 251), (37, 29)):
        assert [(s.w, s.h) for s in pyramid_sizes(FeatureMapSize(w=w, h=h))] == M.pyramid_sizes(w, h)
    for w, h, t in ((30, 19, 240), (90, 57, 64), (1000, 1, 3)):
        s = P.class_image_size(w, h, t)
        assert (s.w, s.h) == M.class_image_size(w, h, t)


def test_the_product_does_not_import_pil():
    import re
    repo = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    for rel in ("os2d_amd/engine/image_pyramid.py", "os2d_amd/engine/evaluate.py", "os2d_amd/_image_lib.py"):
        assert not re.search(r"^\s*(import|from)\s+PIL\b", open(os.path.join(repo, rel)).read(), flags=re.M), rel
