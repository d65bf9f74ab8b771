"""Plain numpy restatement of the reference's image preprocessing (os2d/data/dataloader.py:272-385): PIL's BILINEAR resize
of an 8-bit RGB image (precompute_coeffs / normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc / ...Vertical_8bpc of
Pillow's Resample.c), then ToTensor (``float32(u8) / 255``) and Normalize (``(x - mean) / std``).  The comparator of the
device kernel for shapes too large to store as fixtures; tests/test_image_model.py holds it to the recorded fixtures."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
DEFAULT_SCALES = (0.5, 0.625, 0.8, 1.0, 1.2, 1.4, 1.6)


def tables(in_size, out_size):
    """(bounds int32 [out,2] = (xmin, count), coef int32 [out,ksize]) of one axis; unused taps are 0."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = []
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            k.append(1.0 - a if a < 1.0 else 0.0)
        ww = sum(k)
        if ww != 0.0:
            k = [v / ww for v in k]
        bounds[xx] = (xmin, xmax)
        coef[xx, :xmax] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in k]
    return bounds, coef


def _pass(img, bounds, coef, axis):
    """One pass along `axis` (0 = vertical, 1 = horizontal) of a uint8 [h,w,3] image."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.int64)
    for i, (lo, n) in enumerate(bounds):
        k = coef[i, :n].astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        out[i] = (1 << (PRECISION_BITS - 1)) + (src[lo:lo + n] * k).sum(0)
    out = np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_u8(img, ow, oh):
    """PIL ``img.resize((ow, oh), Image.BILINEAR)`` of a uint8 [h,w,3] array."""
    h, w = img.shape[:2]
    if ow != w:
        img = _pass(img, *tables(w, ow), axis=1)
    if oh != h:
        img = _pass(img, *tables(h, oh), axis=0)
    return img


def transpose_crop(img, hflip=False, vflip=False, crop_xyxy=None):
    """``transforms.transpose`` then ``img.crop`` with a window inside the image."""
    if hflip:
        img = img[:, ::-1]
    if vflip:
        img = img[::-1]
    if crop_xyxy is not None:
        x0, y0, x1, y1 = crop_xyxy
        img = img[y0:y1, x0:x1]
    return np.ascontiguousarray(img)


def normalization_table(img_normalization=IMAGENET):
    """float32 [3,256]: ToTensor + Normalize of every byte per channel (only ToTensor for None)."""
    t = np.arange(256, dtype=np.float32) / np.float32(255)
    t = np.stack([t, t, t])
    if img_normalization is not None:
        mean = np.asarray(img_normalization["mean"], np.float32)[:, None]
        std = np.asarray(img_normalization["std"], np.float32)[:, None]
        t = (t - mean) / std
    return t.astype(np.float32)


def to_float(img_u8, img_normalization=IMAGENET):
    """uint8 [h,w,3] -> float32 [3,h,w]."""
    table = normalization_table(img_normalization)
    return np.stack([table[c][img_u8[:, :, c]] for c in range(3)])


def pyramid_sizes(w, h, scales=DEFAULT_SCALES):
    return [(int(w * s), int(h * s)) for s in scales]


def pyramid(img_u8, scales=DEFAULT_SCALES, img_normalization=IMAGENET, hflip=False, vflip=False):
    """The float32 [1,3,h_l,w_l] levels of ``_transform_image_to_pyramid`` without augmentation."""
    img = transpose_crop(img_u8, hflip, vflip)
    h, w = img.shape[:2]
    return [to_float(resize_u8(img, ow, oh), img_normalization)[None] for ow, oh in pyramid_sizes(w, h, scales)]


def class_image_size(w, h, target):
    """(w, h) of get_image_size_after_resize_preserving_aspect_ratio (os2d/utils/utils.py:32-37)."""
    ar = math.sqrt(h / w)
    return max(int(target / ar), 1), max(int(target * ar), 1)
