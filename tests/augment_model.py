"""Plain numpy restatement of what the training chain does to an image on the host with PIL (reference
os2d/structures/transforms.py, os2d/data/dataloader.py:272-385): ``ImageOps.expand`` + ``crop`` (a window that leaves the image
reads zeros), ``Image.resize`` with each of Pillow's six filters (Resample.c; NEAREST through the affine path), and the colour
operations torchvision's ``ColorJitter`` runs on a PIL image (``ImageEnhance`` = ``Image.blend`` with a degenerate image;
hue through Convert.c's rgb2hsv / hsv2rgb).  The comparator of the device kernels; tests/test_augment_model.py holds it to
the fixtures recorded from PIL itself."""
import math

import numpy as np

import image_model as M

PRECISION_BITS = M.PRECISION_BITS
BRIGHTNESS, CONTRAST, SATURATION, HUE, TO_HSV, FROM_HSV = 1, 2, 3, 4, 5, 6
FILTERS = ("box", "nearest", "hamming", "bicubic", "lanczos", "bilinear")          # the order ``transforms.resize`` draws from


def _sinc(x):
    if x == 0.0:
        return 1.0
    x *= math.pi
    return math.sin(x) / x


def weight(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    x = abs(x)
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    if name == "hamming":
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x *= math.pi
        return math.sin(x) / x * (float(np.float32(0.54)) + float(np.float32(0.46)) * math.cos(x))
    if name == "bicubic":
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    raise ValueError(name)


SUPPORT = dict(box=0.5, bilinear=1.0, hamming=1.0, bicubic=2.0, lanczos=3.0)


def tables(in_size, out_size, name="bilinear"):
    """(bounds int32 [out,2] = (first, count), coef int32 [out,ksize]) of one axis."""
    scale = in_size / out_size
    if name == "nearest":
        first = np.minimum(np.floor((np.arange(out_size) + 0.5) * scale).astype(np.int64), in_size - 1)
        return np.stack([first, np.ones_like(first)], 1).astype(np.int32), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32)
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [weight(name, (x + xmin - center + 0.5) * (1.0 / fs)) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        bounds[xx] = (xmin, xmax)
        coef[xx, :xmax] = [int((-0.5 if v < 0 else 0.5) + v * (1 << PRECISION_BITS)) for v in k]
    return bounds, coef


def resize_u8(img, ow, oh, name="bilinear"):
    """PIL ``img.resize((ow, oh), filter)`` of a uint8 [h,w,3] array."""
    h, w = img.shape[:2]
    if ow != w:
        img = M._pass(img, *tables(w, ow, name), axis=1)
    if oh != h:
        img = M._pass(img, *tables(h, oh, name), axis=0)
    return img


def padded_window(img, window_xyxy, hflip=False, vflip=False):
    """``transforms.transpose`` then ``ImageOps.expand(fill=0)`` + ``crop``: the window (x0, y0, x1, y1) of the flipped image,
    zeros where it leaves the image."""
    img = M.transpose_crop(img, hflip, vflip)
    h, w = img.shape[:2]
    x0, y0, x1, y1 = [int(v) for v in window_xyxy]
    pl, pt, pr, pb = max(-x0, 0), max(-y0, 0), max(x1 - w, 0), max(y1 - h, 0)
    big = np.pad(img, ((pt, pb), (pl, pr), (0, 0)))
    return np.ascontiguousarray(big[y0 + pt:y1 + pt, x0 + pl:x1 + pl])


# ---- colour
def luma(img):
    i = img.astype(np.int64)
    return ((19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16).astype(np.int64)


def blend(degenerate, img, factor):
    """``Image.blend(degenerate, image, factor)`` per byte in float32; degenerate broadcasts against img [h,w,3]."""
    f = np.float32(factor)
    d = np.asarray(degenerate, np.int64)
    t = d.astype(np.float32) + f * (img.astype(np.int64) - d).astype(np.float32)
    if not (0 <= f <= 1):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int64).astype(np.uint8)


def rgb_to_hsv(img):
    r, g, b = [img[..., c].astype(np.int64) for c in range(3)]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    s = cr / np.where(grey, 1, maxc).astype(np.float32)
    rc, gc, bc = [((maxc - c).astype(np.float32) / cr).astype(np.float64) for c in (r, g, b)]
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    h, s, v = [hsv[..., c].astype(np.int64) for c in range(3)]
    fh = h.astype(np.float64) * 6.0 / 255.0
    fl = np.floor(fh)
    i = fl.astype(np.int64) % 6
    f = (fh - fl).astype(np.float32)
    fs = s.astype(np.float32) / np.float32(255)
    fv = v.astype(np.float32)
    one = np.float32(1)
    p = np.clip(np.rint(fv * (one - fs)).astype(np.int64), 0, 255)
    q = np.clip(np.rint(fv * (one - fs * f)).astype(np.int64), 0, 255)
    t = np.clip(np.rint(fv * (one - fs * (one - f))).astype(np.int64), 0, 255)
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    grey = s == 0
    return np.stack([np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)], -1).astype(np.uint8)


def hue_shift(factor):
    return int(factor * 255) % 256


def color_chain(img, ops):
    """ops: [(kind, factor)] in order, on a uint8 [h,w,3] array."""
    for kind, factor in ops:
        if kind == BRIGHTNESS:
            img = blend(0, img, factor)
        elif kind == SATURATION:
            img = blend(luma(img)[..., None], img, factor)
        elif kind == CONTRAST:
            img = blend(int(luma(img).sum() / float(img.shape[0] * img.shape[1]) + 0.5), img, factor)
        elif kind == HUE:
            hsv = rgb_to_hsv(img)
            hsv[..., 0] = (hsv[..., 0].astype(np.int64) + hue_shift(factor)) % 256
            img = hsv_to_rgb(hsv)
        elif kind == TO_HSV:
            img = rgb_to_hsv(img)
        elif kind == FROM_HSV:
            img = hsv_to_rgb(img)
        else:
            raise ValueError(kind)
    return img


def all_colors():
    """The 4096x4096 image of all 2^24 colours: pixel index i = y * 4096 + x has (r, g, b) = (i >> 16, i >> 8 & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.int64).reshape(4096, 4096)
    return np.stack([i >> 16, (i >> 8) & 255, i & 255], -1).astype(np.uint8)


def row_checksums(img):
    """int64 [h,3]: sum over the row of value * (column + 1) per channel - a single wrong byte always changes its row's sum."""
    col = np.arange(1, img.shape[1] + 1, dtype=np.int64)[None, :, None]
    return (img.astype(np.int64) * col).sum(1)
