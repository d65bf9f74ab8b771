#!/usr/bin/env python3
"""Generate the image-preprocessing fixtures by running the REFERENCE's transforms (PIL) in the development container.

Run only where the reference checkout exists:   python tests/golden/make_image_golden.py
It writes ``tests/golden/image_*.npz``: random uint8 inputs (fixed seeds) and what the reference's
``os2d.structures.transforms.transpose`` / ``resize`` (and PIL's ``crop``, as ``transforms.crop`` calls it) make of them.

torchvision is not installed here; the reference's modules import behind the stand-in of make_golden.py.  ``ToTensor`` and
``Normalize`` are restated from torchvision's published forms (torchvision/transforms/functional.py: ``to_tensor`` =
HWC uint8 -> CHW ``.float().div(255)``; ``normalize`` = ``.sub_(mean[:, None, None]).div_(std[:, None, None])`` with mean /
std as tensors of the image's dtype): parity at that boundary is to the published formula.

Only the first case stores float tensors; the others store the uint8 result of the resize (the float is then a table
lookup of it).  Every recorded size is asserted against the reference's ``FeatureMapSize``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

IMAGENET = dict(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
DEFAULT_SCALES = (0.5, 0.625, 0.8, 1.0, 1.2, 1.4, 1.6)


def to_tensor_normalize(pil_img, img_normalization):
    x = torch.from_numpy(np.array(pil_img, np.uint8, copy=True)).permute(2, 0, 1).contiguous().float().div(255)
    if img_normalization is not None:
        mean = torch.as_tensor(img_normalization["mean"], dtype=x.dtype)
        std = torch.as_tensor(img_normalization["std"], dtype=x.dtype)
        x.sub_(mean[:, None, None]).div_(std[:, None, None])
    return x


def random_image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def main():
    if not os.path.isdir(G.REFERENCE):
        raise SystemExit("the reference checkout {} is not present".format(G.REFERENCE))
    G.install_torchvision_standin()
    sys.path.insert(0, G.REFERENCE)
    from PIL import Image
    from os2d.structures import transforms as T
    from os2d.structures.feature_map import FeatureMapSize
    from os2d.utils.utils import get_image_size_after_resize_preserving_aspect_ratio

    def ref_pyramid(img, scales, hflip=False, vflip=False):
        """dataloader.py:293 + :325-338 without augmentation: the PIL images of the levels"""
        img, _ = T.transpose(img, hflip=hflip, vflip=vflip)
        size = FeatureMapSize(img=img)
        out = []
        for s in scales:
            p_size = FeatureMapSize(w=int(size.w * s), h=int(size.h * s))
            p_img, _ = T.resize(img, target_size=p_size)
            assert FeatureMapSize(img=p_img) == p_size
            out.append(p_img)
        return out

    def save(name, **arrays):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) <= 300 * 1024, (name, os.path.getsize(path))
        print(name, os.path.getsize(path), "bytes")

    # image_pyramid_small: 37x29, the seven default scales, ImageNet normalisation, float levels recorded
    src = random_image(37, 29, 101)
    levels = ref_pyramid(Image.fromarray(src), DEFAULT_SCALES)
    arrays = dict(image=src, scales=np.array(DEFAULT_SCALES), mean=np.array(IMAGENET["mean"]), std=np.array(IMAGENET["std"]))
    for i, p in enumerate(levels):
        arrays["u8_{}".format(i)] = np.array(p)
        arrays["float_{}".format(i)] = to_tensor_normalize(p, IMAGENET).numpy()
        assert arrays["float_{}".format(i)].shape == (3, p.size[1], p.size[0])
    save("image_pyramid_small", **arrays)

    # image_pyramid_ratios: 53x40 at 0.11 (19-tap rows), 1 (identity), 2.9 (up-scaling); image_pyramid_thin: 13x200
    for name, (w, h), scales, seed in (("image_pyramid_ratios", (53, 40), (0.11, 1.0, 2.9), 102),
                                       ("image_pyramid_thin", (13, 200), (0.11, 0.5), 103)):
        src = random_image(w, h, seed)
        arrays = dict(image=src, scales=np.array(scales))
        for i, p in enumerate(ref_pyramid(Image.fromarray(src), scales)):
            arrays["u8_{}".format(i)] = np.array(p)
        save(name, **arrays)

    # image_flip_crop: 64x48, both flips, window (5, 7, 45, 39), resized to 33x33, then pyramid scale 1
    src = random_image(64, 48, 104)
    window = (5, 7, 45, 39)
    img, _ = T.transpose(Image.fromarray(src), hflip=True, vflip=True)
    img = img.crop(window)                                   # transforms.crop(...): `img = img.crop(crop_xyxy)`
    assert FeatureMapSize(img=img) == FeatureMapSize(w=40, h=32)
    img, _ = T.resize(img, target_size=FeatureMapSize(w=33, h=33))
    assert FeatureMapSize(img=img) == FeatureMapSize(w=33, h=33)
    level, = ref_pyramid(img, (1.0,))
    save("image_flip_crop", image=src, window=np.array(window), target=np.array((33, 33)), resized=np.array(img), u8_0=np.array(level))

    # image_class: _transform_image_gt without augmentation (dataloader.py:357-385)
    arrays = {}
    for i, ((w, h), target, seed) in enumerate((((30, 19), 240, 105), ((90, 57), 64, 106))):
        src = random_image(w, h, seed)
        nh, nw = get_image_size_after_resize_preserving_aspect_ratio(h=h, w=w, target_size=target)
        img, _ = T.resize(Image.fromarray(src), target_size=FeatureMapSize(w=nw, h=nh))
        assert FeatureMapSize(img=img) == FeatureMapSize(w=nw, h=nh)
        arrays["image_{}".format(i)] = src
        arrays["target_{}".format(i)] = np.int64(target)
        arrays["u8_{}".format(i)] = np.array(img)
    save("image_class", **arrays)


if __name__ == "__main__":
    main()
