"""The training images on the device: decoded uint8 images, boxes and mined records in, the reference's normalised tensors,
boxes, box fates and inverse box transforms out (reference os2d/engine/augmentation.py, os2d/data/dataloader.py:272-385).

    DataAugmentation             the reference's parameter record with its four methods, over structures/transforms.py
    transform_image_to_pyramid   ``_transform_image_to_pyramid``: flips, random or mined crop, resize, colour, pyramid levels
    transform_image_gt           ``_transform_image_gt``: the same for a class image

One upload of the uint8 image; flips + window + zero padding + filter are one kernel, the colour chain one more (two with a
contrast operation), every pyramid level one.  A level that keeps the image's size comes straight out of the colour kernel as
normalised float planes.  After the first call at a size (filter tables uploaded) nothing synchronises with the host.
"""
import random

import torch

from ..structures import transforms as T
from ..structures.bounding_box import BoxList
from ..structures.feature_map import FeatureMapSize
from . import image_pyramid as IP


class DataAugmentation(object):
    """The parameters of all data augmentations (reference engine/augmentation.py:6-86).  ``random_crop_size`` is a
    ``FeatureMapSize`` or None."""

    def __init__(self, random_flip_batches, random_crop_size, random_crop_scale, jitter_aspect_ratio, scale_jitter,
                 random_color_distortion, random_crop_label_images, min_box_coverage):
        self.batch_random_hflip = random_flip_batches
        self.batch_random_vflip = random_flip_batches
        self.do_random_color = random_color_distortion
        self.brightness_delta = 32 / 255.
        self.contrast_delta = 0.5
        self.saturation_delta = 0.5
        self.hue_delta = 0.1
        self.scale_jitter = scale_jitter
        self.jitter_aspect_ratio = jitter_aspect_ratio
        self.do_random_crop = random_crop_size is not None
        if self.do_random_crop:
            self.random_crop_size = random_crop_size
            self.random_crop_scale = random_crop_scale
            self.random_interpolation = True
            self.coverage_keep_threshold = 0.7
            self.coverage_remove_threshold = 0.3
            self.max_trial = 100
            self.min_box_coverage = min_box_coverage
        self.do_random_crop_label_images = random_crop_label_images

    def draw_distortion(self):
        """The colour chain of one image ([] when colour distortion is off: then nothing is drawn)."""
        if not self.do_random_color:
            return []
        return T.draw_distortion(self.brightness_delta, self.contrast_delta, self.saturation_delta, self.hue_delta)

    def random_distort(self, img):
        ops = self.draw_distortion()
        img = T.as_image(img)
        return T.DeviceImage(IP.distort_image(img.materialized().u8, ops)) if ops else img

    def random_crop(self, img, boxes=None, transform_list=None):
        if not self.do_random_crop:
            raise RuntimeError("Random crop data augmentation is not initialized")
        return self.crop_image(img, crop_position=None, boxes=boxes, transform_list=transform_list, random_crop_size=self.random_crop_size)

    def crop_image(self, img, crop_position, boxes=None, transform_list=None, random_crop_size=None):
        return T.crop(img, crop_position=crop_position, random_crop_size=random_crop_size, random_crop_scale=self.random_crop_scale,
                      crop_size=self.random_crop_size, scale_jitter=self.scale_jitter, jitter_aspect_ratio=self.jitter_aspect_ratio,
                      coverage_keep_threshold=self.coverage_keep_threshold, coverage_remove_threshold=self.coverage_remove_threshold,
                      max_trial=self.max_trial, min_box_coverage=self.min_box_coverage, boxes=boxes, transform_list=transform_list)

    def random_crop_label_image(self, img):
        img = T.as_image(img)
        if self.do_random_crop_label_images:
            size = img.size
            ar = size.w / size.h
            new_ar = random.uniform(ar * self.jitter_aspect_ratio, ar / self.jitter_aspect_ratio)
            w = int(min(size.w, size.h * new_ar))
            h = int(min(size.w / new_ar, size.h))
            img = self.crop_image(img, None, random_crop_size=FeatureMapSize(w=w, h=h))[0]
        return img


def _levels(img, ops, sizes, filters, img_normalization):
    """The float32 [3,h,w] tensor of every level of the view ``img`` after the colour chain ``ops``."""
    lut = IP._device_lut(img_normalization, img.u8.device)
    if ops:
        img = img.materialized()
        if all(s == img.size for s in sizes):         # PIL returns a copy for a resize to the same size: colour -> float planes
            return [IP.distort_image(img.u8, ops, to_float=True, img_normalization=img_normalization) for _ in sizes]
        img = T.DeviceImage(IP.distort_image(img.u8, ops))
    x = img.u8.unsqueeze(0)
    x0, y0, x1, y1 = img.window
    full_h, full_w = img.u8.size(0), img.u8.size(1)
    win = (full_w - x1 if img.hflip else x0, full_h - y1 if img.vflip else y0, x1 - x0, y1 - y0)   # in the stored tensor's frame
    return [IP._resample(x, win, img.hflip, img.vflip, s.w, s.h, lut, f, True)[0] for s, f in zip(sizes, filters)]


def transform_image_to_pyramid(image_u8, boxes=None, augmentation=None, hflip=False, vflip=False, pyramid_scales=(1,),
                               mined_data=None, img_normalization=IP.IMAGENET_NORMALIZATION, device=None):
    """``_transform_image_to_pyramid`` (reference dataloader.py:272-347) of a decoded image: uint8 [h,w,3] (host or device).
    augmentation: a ``DataAugmentation`` or None (``do_augmentation`` off).  mined_data: a record of
    ``mine_hard_patches_for_image`` (its ``crop_position_xyxy`` is used).  Returns (img_pyramid: float32 [3,h_l,w_l] device
    tensors, boxes_pyramid, mask_cutoff_boxes, mask_difficult_boxes, pyramid_box_inverse_transform)."""
    img = T.DeviceImage(image_u8, device=device)
    img_size = img.size
    if boxes is None:
        boxes = BoxList.create_empty(img_size)
    mask_cutoff_boxes = torch.zeros(len(boxes), dtype=torch.bool)
    mask_difficult_boxes = torch.zeros(len(boxes), dtype=torch.bool)
    box_inverse_transform = T.TransformList()
    img, boxes = T.transpose(img, hflip=hflip, vflip=vflip, boxes=boxes, transform_list=box_inverse_transform)
    crop_position = mined_data["crop_position_xyxy"] if mined_data is not None else None
    if crop_position is not None and (hflip or vflip):
        crop_position = crop_position.cpu()
        for flip, method in ((hflip, T.FLIP_LEFT_RIGHT), (vflip, T.FLIP_TOP_BOTTOM)):
            if flip:
                crop_position = crop_position.transpose(method)
    ops = []
    random_interpolation = False
    if augmentation is not None:
        if augmentation.do_random_crop:
            if crop_position is None:
                img, boxes, mask_cutoff_boxes, mask_difficult_boxes = augmentation.random_crop(img, boxes=boxes, transform_list=box_inverse_transform)
            else:
                img, boxes, mask_cutoff_boxes, mask_difficult_boxes = augmentation.crop_image(img, crop_position, boxes=boxes,
                                                                                              transform_list=box_inverse_transform)
            img, boxes = T.resize(img, target_size=augmentation.random_crop_size, random_interpolation=augmentation.random_interpolation,
                                  boxes=boxes, transform_list=box_inverse_transform)
        ops = augmentation.draw_distortion()
        random_interpolation = getattr(augmentation, "random_interpolation", False)    # set only with a random crop size
    img_size = img.size
    sizes = [FeatureMapSize(w=int(img_size.w * s), h=int(img_size.h * s)) for s in pyramid_scales]
    boxes_pyramid, inverse = [], []
    filters = []
    for p_size in sizes:
        chain = box_inverse_transform.copy()
        filters.append(T.choose_filter(random_interpolation))
        boxes_pyramid.append(boxes.resize(p_size))
        chain.append(T._Resize(img_size))
        inverse.append(chain)
    return _levels(img, ops, sizes, filters, img_normalization), boxes_pyramid, mask_cutoff_boxes, mask_difficult_boxes, inverse


def transform_image_gt(image_u8, augmentation=None, hflip=False, vflip=False, do_resize=True, gt_image_size=240,
                       img_normalization=IP.IMAGENET_NORMALIZATION, device=None):
    """``_transform_image_gt`` (reference dataloader.py:357-385) of a class image: flips, colour, the random crop of label
    images, the aspect-preserving resize -> float32 [3,h',w'] on the device."""
    img, _ = T.transpose(T.DeviceImage(image_u8, device=device), hflip=hflip, vflip=vflip)
    ops = []
    if augmentation is not None:
        ops = augmentation.draw_distortion()          # pointwise, except contrast's mean: applied before the crop, as drawn
        if ops:
            img = T.DeviceImage(IP.distort_image(img.materialized().u8, ops))
        img = augmentation.random_crop_label_image(img)
    size = img.size
    filter = "bilinear"
    if do_resize:
        size = IP.class_image_size(size.w, size.h, gt_image_size)
        filter = T.choose_filter(getattr(augmentation, "random_interpolation", False))
    return _levels(img, [], [size], [filter], img_normalization)[0]
