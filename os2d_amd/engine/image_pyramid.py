"""The normalised image pyramid from uint8 images, built on the device: what the reference's dataloader does on the host with
PIL and torchvision (os2d/data/dataloader.py:272-347 ``_transform_image_to_pyramid``, :357-385 ``_transform_image_gt``) - one
resize per scale (``Image.BILINEAR``, or a drawn filter under ``random_interpolation``), ``ToTensor``, ``Normalize`` - with the
same bits.  The augmentation search and the random draws on top of it are engine/augmentation.py.

    resample_tables       Pillow's precompute_coeffs + normalize_coeffs_8bpc for each of its filters (host, float64)
    normalization_table   ToTensor + Normalize of every byte value per channel, by the torch CPU operators the reference uses
    ImagePyramidBuilder   uint8 [h,w,3] / [A,h,w,3] -> the list of float32 [A,3,h_l,w_l] levels (one launch per level)
    resize_image          ``transforms.transpose`` / ``crop`` (``pad``: the window may leave the image and reads zeros there) /
                          ``resize`` -> uint8 HWC on the device
    distort_image         the colour operations of ``ColorJitter`` on a PIL image -> uint8 HWC or normalised float planes
    class_image_tensor    ``_transform_image_gt`` without augmentation

The integer filter and the lookup run in libos2d_image.so (include/os2d_image.h), padded windows and the colour arithmetic in
libos2d_augment.so (include/os2d_augment.h); there is no fallback.
Images are tensors: decoding files is the caller's business and nothing here imports PIL.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from .. import _augment_lib, _image_lib
from .._native import STREAM, raw_ptr
from ..structures.feature_map import FeatureMapSize
from .pyramid import DEFAULT_SCALES

IMAGENET_NORMALIZATION = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))   # reference os2d/config.py:28-29
PRECISION_BITS = 32 - 8 - 2       # Pillow Resample.c
MAX_RATIO = 16                    # include/os2d_image.h


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


_HAMMING_A, _HAMMING_B = float(np.float32(0.54)), float(np.float32(0.46))    # float constants in Resample.c


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_HAMMING_A + _HAMMING_B * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# Pillow's filters: name -> (weight function, support).  "nearest" is no filter of Resample.c: one tap (resample_tables).
FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}
# the list ``transforms.resize`` draws from when ``random_interpolation`` is on, in its order (reference transforms.py:65-71)
RANDOM_INTERPOLATION_FILTERS = ("box", "nearest", "hamming", "bicubic", "lanczos", "bilinear")


@functools.lru_cache(maxsize=None)
def resample_tables(in_size, out_size, filter="bilinear"):
    """Pillow's tables of one axis for a filter of ``FILTERS`` (``Image.BILINEAR`` unless named) or "nearest": ``(bounds, coef)``,
    numpy int32 ``[out,2]`` = (first source position, number of taps) and ``[out,ksize]`` fixed-point weights, unused taps 0.
    Python floats are C doubles and every operation below is the one of precompute_coeffs / normalize_coeffs_8bpc, in its
    order.  "nearest" (Pillow's affine path) is one tap of weight 1 at ``floor((i + 0.5) * in / out)``."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_tables: sizes must be positive, got {} -> {}".format(in_size, out_size))
    scale = in_size / out_size
    if filter == "nearest":
        first = [min(int(math.floor((xx + 0.5) * scale)), in_size - 1) for xx in range(out_size)]
        bounds = np.stack([np.array(first), np.ones(out_size, np.int64)], 1).astype(np.int32)
        coef = np.full((out_size, 1), 1 << PRECISION_BITS, np.int32)
        bounds.setflags(write=False)
        coef.setflags(write=False)
        return bounds, coef
    if filter not in FILTERS:
        raise ValueError("resample_tables: unknown filter {!r} (one of {})".format(filter, sorted(FILTERS) + ["nearest"]))
    weight, filter_support = FILTERS[filter]
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [0.0] * xmax
        ww = 0.0
        for x in range(xmax):
            k[x] = weight((x + xmin - center + 0.5) * ss)
            ww += k[x]
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
            coef[xx, x] = int((-0.5 if k[x] < 0 else 0.5) + k[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def normalization_table(mean=None, std=None):
    """float32 CPU tensor [3,256]: entry (c, b) is what ``ToTensor`` + ``Normalize(mean, std)`` make of byte b in channel c,
    computed by the same torch CPU operators (``.div(255)``, ``.sub_(mean).div_(std)``), so the lookup has their bits whatever
    the device would make of a division.  Without mean / std: ``ToTensor`` alone."""
    t = torch.arange(256).float().div(255).unsqueeze(0).repeat(3, 1)
    if mean is not None:
        t.sub_(torch.as_tensor(mean, dtype=t.dtype)[:, None]).div_(torch.as_tensor(std, dtype=t.dtype)[:, None])
    return t


@functools.lru_cache(maxsize=8)
def _cached_lut(mean, std, device_index):
    table = normalization_table() if mean is None else normalization_table(mean, std)
    return table.to(torch.device("cuda", device_index))


def _device_lut(img_normalization, device):
    """The table on the device: uploaded once per (normalisation, device), then only looked up."""
    if img_normalization is None:
        return _cached_lut(None, None, device.index)
    return _cached_lut(tuple(float(v) for v in img_normalization["mean"]), tuple(float(v) for v in img_normalization["std"]), device.index)


# ---- device copies of the per-axis tables, per (device, in, out, filter): made once (a blocking upload), then only looked up
_AXIS_TABLES = {}


def _axis_tables(device, in_size, out_size, filter="bilinear"):
    key = (device.index, in_size, out_size, "bilinear" if in_size == out_size else filter)
    hit = _AXIS_TABLES.get(key)
    if hit is None:
        if in_size > MAX_RATIO * out_size or out_size > MAX_RATIO * in_size:
            raise ValueError("image resize {} -> {}: size ratios beyond {} are not supported".format(in_size, out_size, MAX_RATIO))
        if in_size == out_size:         # PIL skips the pass of an axis that keeps its size: one tap of weight 1
            bounds = np.stack([np.arange(in_size), np.ones(in_size, np.int64)], 1).astype(np.int32)
            coef = np.full((in_size, 1), 1 << PRECISION_BITS, np.int32)
        else:
            bounds, coef = resample_tables(in_size, out_size, filter)
        bounds = np.ascontiguousarray(bounds)
        hit = (torch.from_numpy(np.array(coef)).to(device), torch.from_numpy(np.array(bounds)).to(device), bounds, int(coef.shape[1]))
        _AXIS_TABLES[key] = hit
    return hit


def _device_of(device):
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise ValueError("the image pyramid is built on a HIP device, got {}".format(device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def upload_image(image_u8, device=None):
    """A host image on the device (an asynchronous copy when its memory is pinned); a device tensor as it is."""
    return image_u8 if image_u8.is_cuda else image_u8.to(_device_of(device), non_blocking=True)


def _as_batch(image_u8, device):
    """-> (uint8 device tensor [A,h,w,3] whose pixels are 3 consecutive bytes, was_batched)"""
    if image_u8.dtype != torch.uint8 or image_u8.dim() not in (3, 4) or image_u8.size(-1) != 3:
        raise ValueError("expected a uint8 image [h,w,3] or [A,h,w,3], got {} {}".format(image_u8.dtype, tuple(image_u8.shape)))
    batched = image_u8.dim() == 4
    x = image_u8 if batched else image_u8.unsqueeze(0)
    if x.device != device:
        x = x.to(device, non_blocking=True)
    if x.stride(-1) != 1 or x.stride(-2) != 3 or x.stride(1) < 3 * x.size(2) or (x.size(0) > 1 and x.stride(0) < x.stride(1) * x.size(1)):
        x = x.contiguous()
    return x, batched


def _resample(x, window, hflip, vflip, ow, oh, lut, filter="bilinear", padded=False):
    """x: uint8 device [A,h,w,3]; window (x0, y0, w, h) in x's coordinates; lut: device float [3,256] -> float32 [A,3,oh,ow],
    or None -> uint8 [A,oh,ow,3].  padded: the window may leave the image, what lies outside reads as 0.  Enqueues one kernel
    on the current stream."""
    device = x.device
    A, img_h, img_w = x.size(0), x.size(1), x.size(2)
    x0, y0, w, h = window
    if ow < 1 or oh < 1:
        raise ValueError("image resize to an empty size {}x{}".format(ow, oh))
    xcoef, xb, xb_host, kx = _axis_tables(device, w, ow, filter)
    ycoef, yb, yb_host, ky = _axis_tables(device, h, oh, filter)
    if lut is None:
        out = torch.empty((A, oh, ow, 3), dtype=torch.uint8, device=device)
    else:
        out = torch.empty((A, 3, oh, ow), dtype=torch.float32, device=device)
    # a window that may leave the image: the same kernel template, instantiated in libos2d_augment.so
    lib, entry = (_augment_lib, "os2d_augment_resample_padded") if padded else (_image_lib, "os2d_image_resample")
    # x goes in by its strides (_as_batch lets padded rows through); the host copies of the bounds are numpy arrays
    lib.call(entry, raw_ptr(x), A, img_w, img_h, x.stride(1), x.stride(0), x0, y0, w, h, int(bool(hflip)), int(bool(vflip)), xcoef, xb,
             xb_host.ctypes.data, kx, ycoef, yb, yb_host.ctypes.data, ky, ow, oh, lut, out, int(lut is None), STREAM)
    return out


class ImagePyramidBuilder(object):
    """Builds the levels ``(int(w * s), int(h * s))`` of an image for every scale (reference dataloader.py:326), each by ONE
    resize of the source image as the reference does, normalised - one kernel launch per level on the current stream.
    ``img_normalization``: dict(mean, std), or None for ``ToTensor`` alone."""

    def __init__(self, scales=DEFAULT_SCALES, img_normalization=IMAGENET_NORMALIZATION, device=None):
        self.scales = tuple(float(s) for s in scales)
        self.device = _device_of(device)
        self.img_normalization = img_normalization
        self._lut = _device_lut(img_normalization, self.device)

    def sizes(self, img_size):
        return [FeatureMapSize(w=int(img_size.w * s), h=int(img_size.h * s)) for s in self.scales]

    def build(self, image_u8, hflip=False, vflip=False, filters=None):
        """image_u8: uint8 [h,w,3] or [A,h,w,3], on the host or the device.  Returns (levels, sizes): float32 device tensors
        [A,3,h_l,w_l] (A = 1 for a single image) and their ``FeatureMapSize``s.  After the first call at an image size the
        tables are on the device and a call only enqueues work (a device or pinned input given).  filters: one name of
        ``RANDOM_INTERPOLATION_FILTERS`` per level (``random_interpolation``), else bilinear."""
        x, _ = _as_batch(image_u8, self.device)
        h, w = x.size(1), x.size(2)
        sizes = self.sizes(FeatureMapSize(w=w, h=h))
        filters = ["bilinear"] * len(sizes) if filters is None else list(filters)
        if len(filters) != len(sizes):
            raise ValueError("one filter per pyramid level: got {} for {} levels".format(len(filters), len(sizes)))
        levels = [_resample(x, (0, 0, w, h), hflip, vflip, s.w, s.h, self._lut, f) for s, f in zip(sizes, filters)]
        return levels, sizes


def resize_image(image_u8, target_size, crop_xyxy=None, hflip=False, vflip=False, device=None, filter="bilinear", pad=False):
    """The reference's ``transforms.transpose(hflip, vflip)``, then ``img.crop(crop_xyxy)`` with the window inside the (flipped)
    image, then ``transforms.resize`` to ``target_size`` (a ``FeatureMapSize``): uint8 [h,w,3] (or [A,h,w,3]) -> uint8 HWC on
    the device - the intermediate image of the training chain crop -> resize -> pyramid.  filter: one of
    ``RANDOM_INTERPOLATION_FILTERS``.  pad: the window may leave the image on any side and reads zeros there (the
    ``ImageOps.expand(fill=0)`` + ``crop`` of a mined crop position); it must still contain a pixel of the image."""
    device = _device_of(device if device is not None else (image_u8.device if image_u8.is_cuda else None))
    x, batched = _as_batch(image_u8, device)
    h, w = x.size(1), x.size(2)
    if crop_xyxy is None:
        crop_xyxy = (0, 0, w, h)
    cx0, cy0, cx1, cy1 = [int(v) for v in crop_xyxy]
    if pad:
        if not (cx0 < cx1 and cy0 < cy1 and cx0 < w and cy0 < h and cx1 > 0 and cy1 > 0):
            raise ValueError("crop window {} has no pixel of the {}x{} image".format(tuple(crop_xyxy), w, h))
    elif not (0 <= cx0 < cx1 <= w and 0 <= cy0 < cy1 <= h):
        raise ValueError("crop window {} is not inside the {}x{} image".format(tuple(crop_xyxy), w, h))
    # the kernel flips inside its window: the window of the flipped image, in the coordinates of the stored one
    x0 = w - cx1 if hflip else cx0
    y0 = h - cy1 if vflip else cy0
    out = _resample(x, (x0, y0, cx1 - cx0, cy1 - cy0), hflip, vflip, int(target_size.w), int(target_size.h), None, filter, bool(pad))
    return out if batched else out[0]


# the colour operations of ``distort_image`` (OS2D_AUGMENT_COLOR_* of include/os2d_augment.h)
BRIGHTNESS, CONTRAST, SATURATION, HUE = _augment_lib.COLOR_BRIGHTNESS, _augment_lib.COLOR_CONTRAST, _augment_lib.COLOR_SATURATION, _augment_lib.COLOR_HUE
TO_HSV, FROM_HSV = _augment_lib.COLOR_TO_HSV, _augment_lib.COLOR_FROM_HSV          # the two halves of HUE, for checking them apart


def distort_image(image_u8, ops, to_float=False, img_normalization=IMAGENET_NORMALIZATION, device=None):
    """What torchvision's ``ColorJitter`` makes of a PIL image, operation by operation: ``ops`` is a sequence of at most four
    ``(kind, factor)`` - BRIGHTNESS / CONTRAST / SATURATION (``ImageEnhance.*.enhance(factor)``) and HUE (``adjust_hue``:
    H += int(factor * 255) modulo 256 in PIL's HSV) - applied in order with PIL's bits.  uint8 [h,w,3] -> uint8 [h,w,3] on the
    device, or with ``to_float`` the float32 [3,h,w] of ``ToTensor`` + ``Normalize`` (``img_normalization`` None: ``ToTensor``
    alone).  One launch; two when the chain has a contrast operation (the mean luma stays on the device)."""
    device = _device_of(device if device is not None else (image_u8.device if image_u8.is_cuda else None))
    if image_u8.dim() != 3:
        raise ValueError("expected one uint8 image [h,w,3], got {}".format(tuple(image_u8.shape)))
    x, _ = _as_batch(image_u8, device)
    ops = [(int(k), float(f)) for k, f in ops]
    h, w = x.size(1), x.size(2)
    if to_float:
        lut = _device_lut(img_normalization, device)
        out = torch.empty((3, h, w), dtype=torch.float32, device=device)
    else:
        lut = None
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=device)
    # the workspace of the mean: from the caching allocator, which hands it to nobody else before this stream is through with it
    sums = torch.empty(_augment_lib.COLOR_SLOTS, dtype=torch.int64, device=device) if any(k == CONTRAST for k, _ in ops) else None
    kinds = (ctypes.c_int * max(len(ops), 1))(*[k for k, _ in ops])
    factors = (ctypes.c_double * max(len(ops), 1))(*[f for _, f in ops])
    _augment_lib.call("os2d_augment_color", raw_ptr(x), w, h, x.stride(1), len(ops), kinds, factors, lut, out, int(lut is None), sums, STREAM)
    return out


def class_image_size(w, h, gt_image_size):
    """``get_image_size_after_resize_preserving_aspect_ratio`` (reference os2d/utils/utils.py:32-37) as a FeatureMapSize."""
    aspect_ratio_h_to_w = float(h) / w
    nw = int(gt_image_size / math.sqrt(aspect_ratio_h_to_w))
    nh = int(gt_image_size * math.sqrt(aspect_ratio_h_to_w))
    return FeatureMapSize(w=max(nw, 1), h=max(nh, 1))


def class_image_tensor(image_u8, gt_image_size=240, img_normalization=IMAGENET_NORMALIZATION, hflip=False, vflip=False, device=None,
                       filter="bilinear"):
    """``_transform_image_gt`` without augmentation: resize to area ~ gt_image_size^2 keeping the aspect ratio, ``ToTensor``,
    ``Normalize``.  uint8 [h,w,3] -> float32 device tensor [3,h',w']."""
    device = _device_of(device if device is not None else (image_u8.device if image_u8.is_cuda else None))
    x, batched = _as_batch(image_u8, device)
    h, w = x.size(1), x.size(2)
    size = class_image_size(w, h, gt_image_size)
    out = _resample(x, (0, 0, w, h), hflip, vflip, size.w, size.h, _device_lut(img_normalization, device), filter)
    return out if batched else out[0]
