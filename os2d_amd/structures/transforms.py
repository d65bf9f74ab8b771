"""The image + box transforms of the training dataloader over (uint8 device image, BoxList) pairs - what the reference's
os2d/structures/transforms.py does with PIL images on the host: ``TransformList``, ``transpose``, ``resize`` (with
``random_interpolation``), ``crop`` (the random-crop search, or a mined crop position that may leave the image) and
``random_distort``.

An image is a ``DeviceImage``: a uint8 [h,w,3] tensor on the device and a pending view of it (flips, then a window that may
overhang).  ``transpose`` and ``crop`` only change the view; ``resize`` runs the flips, the window with its zero padding and
the filter in ONE kernel (libos2d_image.so), ``random_distort`` the colour chain in one more.  Boxes stay on the host: an image
has a handful, the crop search breaks on their values, and torch on the CPU gives the reference's bits.

Random numbers: Python's ``random`` in the reference's call order (per crop trial ``uniform``, ``uniform``, ``randrange``,
``randrange``; ``choice`` of the six filters in the reference's list order; a ``random()`` coin per colour operation and for
the order of the two branches), so the same seed chooses what the reference chooses.  The colour factors are drawn as
torchvision's published ``ColorJitter`` draws them (``draw_color_factor``): torchvision itself is not a dependency, parity at
that boundary is to its published form.  Nothing here imports PIL.
"""
import random

import torch

from ..engine import image_pyramid as IP
from .bounding_box import BoxList, FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, box_intersection_over_reference
from .feature_map import FeatureMapSize


class TransformList(object):
    """Box transforms appended in the order the image went through them, run in the reverse order: the way back to the
    original image's coordinates (reference transforms.py:12-27).  ``trace_box_transform`` (modeling/box_ops.py) reads it."""

    def __init__(self):
        self._transforms = []

    def append(self, t):
        self._transforms.append(t)

    def __call__(self, x):
        for t in reversed(self._transforms):
            x = t(x)
        return x

    def copy(self):
        """A list of its own over the same (immutable) entries: what the reference's ``copy.deepcopy`` per level is for."""
        out = TransformList()
        out._transforms = list(self._transforms)
        return out


class DeviceImage(object):
    """uint8 [h,w,3] device tensor + the view of it that counts as the image: ``hflip`` / ``vflip`` of the whole tensor, then
    the window ``(x0, y0, x1, y1)`` of the flipped tensor; outside the tensor the window reads 0."""

    def __init__(self, u8, hflip=False, vflip=False, window=None, device=None):
        if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 3 or u8.size(2) != 3:
            raise ValueError("expected a uint8 image tensor [h,w,3]")
        self.u8 = IP.upload_image(u8, device)          # the one upload (a device tensor stays where it is)
        self.hflip, self.vflip = bool(hflip), bool(vflip)
        self.window = tuple(int(v) for v in window) if window is not None else (0, 0, u8.size(1), u8.size(0))

    @property
    def size(self):
        return FeatureMapSize(w=self.window[2] - self.window[0], h=self.window[3] - self.window[1])

    def is_plain(self):
        return not self.hflip and not self.vflip and self.window == (0, 0, self.u8.size(1), self.u8.size(0))

    def resized(self, target_size, filter="bilinear"):
        """-> DeviceImage of ``target_size`` without a pending view (one kernel)."""
        out = IP.resize_image(self.u8, target_size, crop_xyxy=self.window, hflip=self.hflip, vflip=self.vflip, filter=filter, pad=True)
        return DeviceImage(out)

    def materialized(self):
        return self if self.is_plain() else self.resized(self.size)


def as_image(img, device=None):
    return img if isinstance(img, DeviceImage) else DeviceImage(img, device=device)


def check_image_size(img, boxes):
    if boxes is not None:
        assert boxes.image_size == img.size, "Size of the image should match the size store in the accompanying BoxList"


def transpose(img, hflip=False, vflip=False, boxes=None, transform_list=None):
    """reference transforms.py:36-52.  A flip of a view: the other flip of the tensor, the window mirrored."""
    img = as_image(img)
    check_image_size(img, boxes)
    for flip, method in ((hflip, FLIP_LEFT_RIGHT), (vflip, FLIP_TOP_BOTTOM)):
        if not flip:
            continue
        x0, y0, x1, y1 = img.window
        full_h, full_w = img.u8.size(0), img.u8.size(1)
        if method == FLIP_LEFT_RIGHT:
            img = DeviceImage(img.u8, not img.hflip, img.vflip, (full_w - x1, y0, full_w - x0, y1))
        else:
            img = DeviceImage(img.u8, img.hflip, not img.vflip, (x0, full_h - y1, x1, full_h - y0))
        if boxes is not None:
            boxes = boxes.transpose(method)
            if transform_list is not None:
                transform_list.append(_Transpose(method))
    return img, boxes


class _Transpose(object):
    def __init__(self, method):
        self.method = method

    def __call__(self, boxes):
        return boxes.transpose(self.method)


class _Resize(object):
    def __init__(self, size):
        self.size = size

    def __call__(self, boxes):
        return boxes.resize(self.size)


class _Crop(object):
    def __init__(self, xyxy):
        self.xyxy = xyxy

    def __call__(self, boxes):
        return boxes.crop(self.xyxy)


def choose_filter(random_interpolation):
    """One ``random.choice`` of the six filters when ``random_interpolation``, else no draw and bilinear."""
    return random.choice(IP.RANDOM_INTERPOLATION_FILTERS) if random_interpolation else "bilinear"


def resize(img, target_size, random_interpolation=False, boxes=None, transform_list=None):
    """reference transforms.py:55-80: a number as ``target_size`` is the longer side."""
    img = as_image(img)
    image_size = img.size
    if not isinstance(target_size, FeatureMapSize):
        scale = float(target_size) / max(image_size.w, image_size.h)
        target_size = FeatureMapSize(w=int(image_size.w * scale + 0.5), h=int(image_size.h * scale + 0.5))
    img = img.resized(target_size, choose_filter(random_interpolation))
    if boxes is not None:
        boxes = boxes.resize(target_size)
        if transform_list is not None:
            transform_list.append(_Resize(image_size))
    else:
        assert transform_list is None
    return img, boxes


def _good_crop(xyxy, size):
    return max(int(xyxy[0]), 0), max(int(xyxy[1]), 0), min(int(xyxy[2]), size.w), min(int(xyxy[3]), size.h)


def crop(img, crop_size=None, crop_position=None, random_crop_size=None, random_crop_scale=1.0, scale_jitter=1.0,
         jitter_aspect_ratio=1.0, random_scale=1.0, coverage_keep_threshold=0.7, coverage_remove_threshold=0.3, max_trial=100,
         min_box_coverage=0.7, boxes=None, transform_list=None):
    """reference transforms.py:83-197.  ``crop_position`` (a BoxList of one box, a mined record's ``crop_position_xyxy``) may
    leave the image: the reference pads the image with zeros first, here the window simply overhangs.  As in the reference the
    boxes are NOT shifted by that padding: they are cropped by the window in the padded image's coordinates.  The caller's
    ``crop_position`` is left as it is (the reference shifts it in place)."""
    img = as_image(img)
    image_size = img.size
    assert 0 < random_crop_scale, "Crop scale has to be > 0, we have random_crop_scale = {0}".format(random_crop_scale)
    assert 0 < scale_jitter <= 1.0, "Scale jitter has to be in (0, 1], we have scale_jitter = {0}".format(scale_jitter)
    assert 0 < jitter_aspect_ratio <= 1.0, "Aspect ratio jitter has to be in (0, 1], we have jitter_aspect_ratio = {0}".format(jitter_aspect_ratio)
    imw, imh = image_size.w, image_size.h
    pad_left = pad_top = 0
    if crop_position is not None:
        assert len(crop_position) == 1, "Precomputed crop position should have only one box, but have {0}".format(crop_position)
        pos = crop_position.bbox_xyxy[0].detach().cpu().clone()
        if int(pos[0]) < 0:                 # padding on the left; int() truncates towards zero
            pad_left = -int(pos[0])
            pos[0] += pad_left
            pos[2] += pad_left
            imw += pad_left
        if int(pos[1]) < 0:                 # on the top
            pad_top = -int(pos[1])
            pos[1] += pad_top
            pos[3] += pad_top
            imh += pad_top
        if int(pos[2]) > imw:               # on the right
            imw += int(pos[2]) - imw
        if int(pos[3]) > imh:               # at the bottom
            imh += int(pos[3]) - imh
        crop_xyxy = _good_crop(pos, FeatureMapSize(w=imw, h=imh))
        for tuned, initial in zip(crop_xyxy, pos):
            assert abs(tuned - initial) <= 1.01, "Mined crop is not fitting: mined {0}, tuned {1}".format(pos, crop_xyxy)
    else:
        crop_width, crop_height = random_crop_size.w, random_crop_size.h
        crop_ar = crop_width / crop_height
        crop_xyxy = _good_crop((0, 0, crop_width / random_crop_scale, crop_height / random_crop_scale), image_size)
        for _ in range(max_trial):
            aspect_ratio = random.uniform(crop_ar * jitter_aspect_ratio, crop_ar / jitter_aspect_ratio)
            scale = random.uniform(random_crop_scale * scale_jitter, random_crop_scale / scale_jitter)
            w = min(crop_width / scale, imw)
            h = min(w / aspect_ratio, imh)
            w, h = int(w), int(h)
            assert imw - w >= 0, "Trying to sample a patch which is too wide: image width - {0}, patch width - {1}".format(imw, w)
            x = random.randrange(imw - w) if imw - w > 0 else 0
            assert imh - h >= 0, "Trying to sample a patch which is too high: image height - {0}, patch height - {1}".format(imh, h)
            y = random.randrange(imh - h) if imh - h > 0 else 0
            trial = _good_crop((x, y, x + w, y + h), image_size)
            if boxes is None:
                crop_xyxy = trial
                break
            coverage = box_intersection_over_reference(boxes, BoxList(torch.FloatTensor([trial]), image_size, mode="xyxy"))
            if len(boxes) == 0 or coverage.max() >= min_box_coverage:
                crop_xyxy = trial
                break

    # the image: the window of the (virtually padded) view, in the view's own coordinates
    vx0, vy0 = img.window[0], img.window[1]
    x0, y0, x1, y1 = crop_xyxy[0] - pad_left, crop_xyxy[1] - pad_top, crop_xyxy[2] - pad_left, crop_xyxy[3] - pad_top
    img = DeviceImage(img.u8, img.hflip, img.vflip, (vx0 + x0, vy0 + y0, vx0 + x1, vy0 + y1))

    if boxes is None:
        return img, None, None, None
    coverage = box_intersection_over_reference(boxes, BoxList(torch.FloatTensor([crop_xyxy]), image_size, mode="xyxy"))
    boxes = boxes.crop(crop_xyxy)
    coverage = coverage.squeeze()
    mask_cutoff_boxes = coverage < coverage_remove_threshold
    mask_difficult_boxes = coverage < coverage_keep_threshold
    if transform_list is not None:          # "uncrop" is a crop by the original image's frame seen from the window
        transform_list.append(_Crop((-crop_xyxy[0], -crop_xyxy[1], -crop_xyxy[0] + image_size.w, -crop_xyxy[1] + image_size.h)))
    return img, boxes, mask_cutoff_boxes, mask_difficult_boxes


def draw_color_factor(kind, delta):
    """The factor torchvision's ``ColorJitter(<kind>=delta)`` draws for one call (published ``__init__`` / ``get_params``):
    the range is ``[max(0, 1 - delta), 1 + delta]``, for hue ``[-delta, delta]``; ``get_params`` first draws the order of its
    four operations (``torch.randperm(4)``, of no effect with one operation) and then ``torch.empty(1).uniform_(lo, hi)``.
    None when the range is the single neutral value (the operation is then not applied)."""
    lo, hi = (-delta, delta) if kind == IP.HUE else (max(1 - delta, 0.0), 1 + delta)
    if lo == hi == (0 if kind == IP.HUE else 1):
        return None
    torch.randperm(4)
    return float(torch.empty(1).uniform_(float(lo), float(hi)))


def draw_distortion(brightness_delta=32 / 255., contrast_delta=0.5, saturation_delta=0.5, hue_delta=0.1):
    """The draws of reference transforms.py:200-248 -> the chain [(kind, factor)] that ``distort_image`` applies: brightness
    first; then a coin for the order (contrast, saturation, hue) or (saturation, hue, contrast); every operation behind a
    coin of its own, drawn just before its factor."""
    ops = []

    def maybe(kind, delta):
        if random.random() < 0.5:
            factor = draw_color_factor(kind, delta)
            if factor is not None:
                ops.append((kind, factor))

    maybe(IP.BRIGHTNESS, brightness_delta)
    if random.random() < 0.5:
        order = ((IP.CONTRAST, contrast_delta), (IP.SATURATION, saturation_delta), (IP.HUE, hue_delta))
    else:
        order = ((IP.SATURATION, saturation_delta), (IP.HUE, hue_delta), (IP.CONTRAST, contrast_delta))
    for kind, delta in order:
        maybe(kind, delta)
    return ops


def random_distort(img, brightness_delta=32 / 255., contrast_delta=0.5, saturation_delta=0.5, hue_delta=0.1):
    """The SSD colour augmentation (reference transforms.py:200-248) -> DeviceImage."""
    img = as_image(img).materialized()
    ops = draw_distortion(brightness_delta, contrast_delta, saturation_delta, hue_delta)
    return DeviceImage(IP.distort_image(img.u8, ops)) if ops else img
