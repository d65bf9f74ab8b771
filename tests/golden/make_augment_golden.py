#!/usr/bin/env python3
"""Generate the training-image fixtures by running the REFERENCE's transforms (PIL) in the development container.

Run only where the reference checkout exists:   python tests/golden/make_augment_golden.py
It writes ``tests/golden/augment_*.npz``: small random uint8 images (96x72), boxes, seeds and what the reference's
``os2d.structures.transforms.transpose`` / ``crop`` / ``resize`` / ``random_distort`` and its ``DataAugmentation`` make of them
when called in the order of ``_transform_image_to_pyramid`` (os2d/data/dataloader.py:272-347), and
``augment_color_checksums.npz``: PIL's own RGB -> HSV, HSV -> RGB and hue shifts by 23 and 231 on the 4096x4096 image of all
2^24 colours, as per-row, per-channel int64 sums of value * (column + 1) (a single wrong byte always changes its row's sum).

torchvision is not installed here; the reference's modules import behind the stand-in of make_golden.py.  On top of it
``ColorJitter`` is restated from torchvision's published form (transforms.py ``ColorJitter.__init__`` / ``get_params`` /
``forward``, functional_pil.py ``adjust_*``): the ranges ``[max(0, 1 - d), 1 + d]`` and ``[-d, d]``, ``torch.randperm(4)``
then ``torch.empty(1).uniform_(lo, hi)`` per configured operation, ``ImageEnhance.Brightness / Contrast / Color`` and the hue
shift ``np_h += np.int32(hue_factor * 255).astype(np.uint8)`` on the H channel of ``convert("HSV")``.  Parity at that boundary
is to the published form.

Every case is found by searching Python ``random`` seeds until the reference, and the reference alone, takes the branch the
case is named for.  Asserted on the reference's run (a log of every ``random`` call its transforms module makes, and of every
PIL ``crop`` / ``resize``):
  * random_boxes        the first crop trial is accepted; 3 boxes; fates: one removed, one difficult (not removed), one kept
  * random_noboxes      no boxes: the first trial is taken without a coverage test
  * random_retry        at least one trial fails ``min_box_coverage`` and is drawn again
  * mined_left / _top / _right / _bottom / _all   the mined window leaves the image on exactly that side / on all four
  * mined_flips         a mined window that overhangs, with both flips
  * filter_<name>       the crop's resize draws that filter (one case per filter of the reference's list)
  * color_csh / color_shc   the order coin picks (contrast, saturation, hue) / (saturation, hue, contrast) and all four
                        operations are applied;  color_none  every operation's coin says no
  * pyramid             three scales, every level with a drawn filter
Every recorded level's size is asserted against the reference's ``FeatureMapSize``; every file is below 64 KB but the
checksums (393 KB of int64).
"""
import copy
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

FILTER_NAMES = ("box", "nearest", "hamming", "bicubic", "lanczos", "bilinear")


class LoggedRandom(object):
    """Stands in for the ``random`` module inside the reference's transforms module: same generator, every call logged."""

    def __init__(self):
        self.log = []

    def _do(self, name, *a):
        out = getattr(random, name)(*a)
        self.log.append((name, out))
        return out

    def uniform(self, a, b):
        return self._do("uniform", a, b)

    def randrange(self, n):
        return self._do("randrange", n)

    def choice(self, seq):
        return self._do("choice", seq)

    def random(self):
        return self._do("random")


def main():
    if not os.path.isdir(G.REFERENCE):
        raise SystemExit("the reference checkout {} is not present".format(G.REFERENCE))
    G.install_torchvision_standin()
    from PIL import Image, ImageEnhance
    color_log = []

    class ColorJitter(object):
        def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
            def rng(v, center, clip):
                lo, hi = center - float(v), center + float(v)
                if clip:
                    lo = max(lo, 0.0)
                return None if lo == hi == center else (float(lo), float(hi))
            self.ranges = [rng(brightness, 1, True), rng(contrast, 1, True), rng(saturation, 1, True), rng(hue, 0, False)]

        def __call__(self, img):
            order = torch.randperm(4)
            f = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in self.ranges]
            for fn in order.tolist():
                if f[fn] is None:
                    continue
                color_log.append((fn + 1, f[fn]))
                if fn == 0:
                    img = ImageEnhance.Brightness(img).enhance(f[fn])
                elif fn == 1:
                    img = ImageEnhance.Contrast(img).enhance(f[fn])
                elif fn == 2:
                    img = ImageEnhance.Color(img).enhance(f[fn])
                else:
                    h, s, v = img.convert("HSV").split()
                    np_h = np.array(h, dtype=np.uint8)
                    with np.errstate(over="ignore"):
                        np_h += np.int32(f[fn] * 255).astype(np.uint8)
                    img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
            return img

    sys.modules["torchvision.transforms"].ColorJitter = ColorJitter
    sys.path.insert(0, G.REFERENCE)
    from os2d.structures import transforms as T
    from os2d.structures.feature_map import FeatureMapSize
    from os2d.structures.bounding_box import BoxList
    from os2d.engine.augmentation import DataAugmentation

    pil_log = []
    orig_crop, orig_resize = Image.Image.crop, Image.Image.resize

    def logged_crop(self, box=None):
        pil_log.append(("crop", tuple(int(v) for v in box), self.size))
        return orig_crop(self, box)

    def logged_resize(self, size, resample=None, *a, **k):
        pil_log.append(("resize", tuple(size), int(resample)))
        return orig_resize(self, size, resample, *a, **k)

    Image.Image.crop, Image.Image.resize = logged_crop, logged_resize
    orig_expand = T.ImageOps.expand

    def logged_expand(img, border=0, fill=0):
        pil_log.append(("expand", tuple(int(v) for v in border), fill))
        return orig_expand(img, border=border, fill=fill)

    T.ImageOps = type("LoggedImageOps", (), dict(expand=staticmethod(logged_expand)))
    pil_filter = {int(getattr(Image, n.upper())): i for i, n in enumerate(FILTER_NAMES)}

    def run(image, boxes, seed, hflip, vflip, mined, scales, color, crop=(48, 40), crop_scale=1.0, jitter_ar=0.9, scale_jitter=0.7,
            min_cov=0.7):
        """the order of dataloader.py:272-347 with the reference's own functions -> dict of arrays, log"""
        rnd = LoggedRandom()
        T.random = rnd
        random.seed(seed)
        torch.manual_seed(seed)
        del pil_log[:], color_log[:]
        aug = DataAugmentation(random_flip_batches=False, random_crop_size=FeatureMapSize(w=crop[0], h=crop[1]), random_crop_scale=crop_scale,
                               jitter_aspect_ratio=jitter_ar, scale_jitter=scale_jitter, random_color_distortion=color,
                               random_crop_label_images=False, min_box_coverage=min_cov)
        img = Image.fromarray(image)
        size = FeatureMapSize(img=img)
        bl = BoxList(torch.from_numpy(boxes).clone(), size, mode="xyxy") if boxes is not None else BoxList.create_empty(size)
        inv = T.TransformList()
        img, bl = T.transpose(img, hflip=hflip, vflip=vflip, boxes=bl, transform_list=inv)
        if mined is not None:
            pos = BoxList(torch.tensor([mined], dtype=torch.float32), size, mode="xyxy")
            if hflip or vflip:
                _, pos = T.transpose(img, hflip=hflip, vflip=vflip, boxes=pos)
            img, bl, cut, diff = aug.crop_image(img, pos, boxes=bl, transform_list=inv)
        else:
            img, bl, cut, diff = aug.random_crop(img, boxes=bl, transform_list=inv)
        img, bl = T.resize(img, target_size=aug.random_crop_size, random_interpolation=True, boxes=bl, transform_list=inv)
        img = aug.random_distort(img)
        isz = FeatureMapSize(img=img)
        out = dict(image=image, boxes=boxes if boxes is not None else np.zeros((0, 4), np.float32), has_boxes=np.int64(boxes is not None),
                   seed=np.int64(seed), hflip=np.int64(hflip), vflip=np.int64(vflip),
                   mined=np.array(mined if mined is not None else [], np.float32), scales=np.array(scales, np.float64),
                   params=np.array([crop[0], crop[1], crop_scale, jitter_ar, scale_jitter, float(color), min_cov], np.float64),
                   mask_cutoff=cut.numpy(), mask_difficult=diff.numpy())
        probe = torch.tensor([[0.0, 0.0, 1.0, 1.0], [3.25, 7.5, 21.0, 15.75]])
        for i, s in enumerate(scales):
            p_size = FeatureMapSize(w=int(isz.w * s), h=int(isz.h * s))
            inv_i = copy.deepcopy(inv)
            p_img, p_bl = T.resize(img, target_size=p_size, random_interpolation=True, boxes=bl, transform_list=inv_i)
            assert FeatureMapSize(img=p_img) == p_size
            back = inv_i(BoxList(probe.clone(), p_size, mode="xyxy"))
            out["u8_{}".format(i)] = np.array(p_img)
            out["boxes_{}".format(i)] = p_bl.bbox_xyxy.numpy()
            out["inv_probe_{}".format(i)] = back.bbox_xyxy.numpy()
            out["inv_size_{}".format(i)] = np.array([back.image_size.w, back.image_size.h], np.int64)
        crops = [e for e in pil_log if e[0] == "crop"]
        resizes = [e for e in pil_log if e[0] == "resize"]
        assert len(crops) == 1 and len(resizes) == 1 + len(scales)
        out["window"] = np.array(crops[0][1], np.int64)             # in the padded image's coordinates
        out["padded_size"] = np.array(crops[0][2], np.int64)
        expands = [e for e in pil_log if e[0] == "expand"]
        assert len(expands) == (mined is not None) and all(e[2] == 0 for e in expands)
        out["padding"] = np.array(expands[0][1] if expands else (0, 0, 0, 0), np.int64)       # left, top, right, bottom
        out["filters"] = np.array([pil_filter[e[2]] for e in resizes], np.int64)
        out["color_ops"] = np.array(color_log, np.float64).reshape(-1, 2)
        return out, list(rnd.log)

    def find(name, accept, **kw):
        for seed in range(2000):
            out, log = run(seed=seed, **kw)
            if accept(out, log):
                path = os.path.join(HERE, "augment_{}.npz".format(name))
                np.savez_compressed(path, **out)
                assert os.path.getsize(path) <= 64 * 1024, (name, os.path.getsize(path))
                print(name, "seed", seed, os.path.getsize(path), "bytes; filters", out["filters"], "ops", out["color_ops"].tolist())
                return out
        raise SystemExit("no seed found for " + name)

    rs = np.random.RandomState(7)
    image = rs.randint(0, 256, size=(72, 96, 3)).astype(np.uint8)
    boxes3 = np.array([[10, 8, 30, 28], [40, 20, 70, 50], [60, 40, 90, 70]], np.float32)
    trials = lambda log: sum(1 for n, _ in log if n == "uniform") // 2
    base = dict(image=image, hflip=False, vflip=False, mined=None, scales=(1.0,), color=False)

    def fates(out, log):
        cut, diff = out["mask_cutoff"], out["mask_difficult"]
        return trials(log) == 1 and sorted(zip(cut.tolist(), diff.tolist())) == [(False, False), (False, True), (True, True)]

    find("random_boxes", fates, **dict(base, boxes=boxes3))
    find("random_noboxes", lambda o, log: trials(log) == 1, **dict(base, boxes=None))
    find("random_retry", lambda o, log: trials(log) >= 2, **dict(base, boxes=boxes3[:1], min_cov=0.9, scale_jitter=0.9))
    W, H = 96, 72
    mined = dict(left=(-9.6, 10.2, 38.4, 50.2), top=(20.3, -7.7, 68.3, 32.3), right=(60.5, 12.5, 108.5, 52.5), bottom=(30.0, 50.9, 78.0, 90.9),
                 all=(-10.5, -12.25, 110.75, 88.5))
    sides = dict(left=(1, 0, 0, 0), top=(0, 1, 0, 0), right=(0, 0, 1, 0), bottom=(0, 0, 0, 1), all=(1, 1, 1, 1))
    for side, pos in mined.items():
        def padded_there(o, log, side=side):
            pw, ph = o["padded_size"]
            x0, y0, x1, y1 = o["window"]
            got = (int(pos[0]) < 0, int(pos[1]) < 0, int(pos[2]) > W, int(pos[3]) > H)
            return got == tuple(bool(v) for v in sides[side]) and (pw > W or ph > H) and trials(log) == 0
        find("mined_" + side, padded_there, **dict(base, boxes=boxes3, mined=pos))
    find("mined_flips", lambda o, log: tuple(o["padded_size"]) != (W, H), **dict(base, boxes=boxes3, mined=(-6.5, 30.25, 50.5, 80.0), hflip=True, vflip=True))
    for i, name in enumerate(FILTER_NAMES):
        find("filter_" + name, lambda o, log, i=i: o["filters"][0] == i, **dict(base, boxes=boxes3[1:2], scales=(1.0,)))

    def order(first):
        def ok(o, log):
            kinds = [int(k) for k in o["color_ops"][:, 0]]
            return kinds == first
        return ok
    find("color_csh", order([1, 2, 3, 4]), **dict(base, boxes=boxes3[1:2], color=True))
    find("color_shc", order([1, 3, 4, 2]), **dict(base, boxes=boxes3[1:2], color=True))
    find("color_none", lambda o, log: len(o["color_ops"]) == 0 and sum(1 for n, _ in log if n == "random") == 5,
         **dict(base, boxes=boxes3[1:2], color=True))
    find("pyramid", lambda o, log: len(set(o["filters"].tolist())) >= 3, **dict(base, boxes=boxes3, scales=(0.5, 1.0, 1.6), color=True))

    # ---- PIL's colour conversions on every colour
    Image.Image.crop, Image.Image.resize = orig_crop, orig_resize
    i = np.arange(1 << 24, dtype=np.int64).reshape(4096, 4096)
    allc = np.stack([i >> 16, (i >> 8) & 255, i & 255], -1).astype(np.uint8)
    col = np.arange(1, 4097, dtype=np.int64)[None, :, None]
    sums = lambda a: (np.asarray(a).astype(np.int64) * col).sum(1)
    pil = Image.fromarray(allc)
    arrays = dict(rgb_to_hsv=sums(pil.convert("HSV")), hsv_to_rgb=sums(Image.fromarray(allc, "HSV").convert("RGB")))
    for shift in (23, 231):
        h, s, v = pil.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h += np.uint8(shift)
        arrays["hue_{}".format(shift)] = sums(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
    path = os.path.join(HERE, "augment_color_checksums.npz")
    np.savez_compressed(path, **arrays)
    assert all(a.shape == (4096, 3) and a.dtype == np.int64 for a in arrays.values()) and os.path.getsize(path) <= 1024 * 1024
    print("augment_color_checksums", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
