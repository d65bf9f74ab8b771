"""Anchor grids and the reference's box coder (os2d/modeling/box_coder.py) on the HIP libraries: decode + NMS for inference,
target assignment for training.

    create_strided_boxes_columnfirst / BoxGridGenerator   reference box_coder.py:16-76
    Os2dBoxCoder.build_boxes_from_loc_scores              reference box_coder.py:319-330   (os2d_decode_boxes)
    Os2dBoxCoder.decode_pyramid                           reference box_coder.py:448-536   (os2d_detect_level for one level,
                                                                                            os2d_detect_pyramid for several,
                                                                                            os2d_decode_boxes + os2d_nms otherwise)

    Os2dBoxCoder.encode / encode_pyramid / encode_batch   reference box_coder.py:332-421   (os2d_train_assign_targets, mode 0)
    Os2dBoxCoder.remap_anchor_targets                     reference box_coder.py:234-300   (os2d_train_assign_targets, mode 1)

    BoxGridGenerator.get_box_to_cut_anchor                reference box_coder.py:78-166    (os2d_train_crop_boxes)
    Os2dBoxCoder.encode_transformed / encode_pyramid_transformed / remap_anchor_targets_transformed
                                                          the same with the reference's box transforms (hard-patch mining,
                                                          reference box_coder.py:250-254, 352-354; os2d_train_assign_targets_ops)

The target side runs as one launch per call over every (image, label, anchor); the BoxLists are packed into four arrays on
the host once per batch.  A box transform reaches the kernels as the chain that box_ops.py records (its names are re-exported
here); the reference-named ``encode`` / ``encode_pyramid`` / ``remap_anchor_targets`` refuse transforms and name the
``_transformed`` methods.
"""
import ctypes
from functools import lru_cache

import torch

from .. import _lib
from .. import _train_lib
from .._native import STREAM
from ..structures.feature_map import FeatureMapSize
from ..structures.bounding_box import BoxList, FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM          # noqa: F401 (the flips: re-exported)
from .box_ops import (OP_SCALE, OP_HFLIP, OP_VFLIP, OP_SHIFT, MAX_BOX_OPS, MAX_DEFAULT_BOX_OPS,          # noqa: F401 (re-exported)
                      ResizeBoxes, _BoxTrace, apply_box_ops, _PROBE_BOXES, transform_level_boxes, trace_box_transform,
                      _TRACE_CACHE, _trace_chains, _probe_check, _trace_box_transform, ops_tables, _ops_tables,
                      traced_box_ops, as_box_ops)

BOX_ENCODING_WEIGHTS = (10.0, 10.0, 5.0, 5.0)   # reference box_coder.py:13


@lru_cache()
def create_strided_boxes_columnfirst(grid_size, box_size, box_stride):
    """Row-major (index h*W + w, despite the historical name) grid of xyxy anchor boxes with centres
    ((w+.5)*stride_w, (h+.5)*stride_h); CPU float tensor [H*W, 4] (reference box_coder.py:16-59)."""
    cy = (torch.arange(grid_size.h, dtype=torch.float32) + 0.5) * box_stride.h
    cx = (torch.arange(grid_size.w, dtype=torch.float32) + 0.5) * box_stride.w
    cx = cx.view(1, -1).expand(grid_size.h, grid_size.w).reshape(-1)
    cy = cy.view(-1, 1).expand(grid_size.h, grid_size.w).reshape(-1)
    hw, hh = box_size.w / 2.0, box_size.h / 2.0
    return torch.stack([cx - hw, cy - hh, cx + hw, cy + hh], dim=1)


class BoxGridGenerator(object):
    """reference box_coder.py:62-76: binds a box size and stride (both FeatureMapSize)."""

    def __init__(self, box_size, box_stride):
        self.box_size = box_size
        self.box_stride = box_stride

    def create_strided_boxes_columnfirst(self, fm_size):
        return create_strided_boxes_columnfirst(fm_size, self.box_size, self.box_stride)

    def get_box_to_cut_anchor(self, img_size, crop_size, fm_size, default_box_transform=None, device=None):
        """reference box_coder.py:78-166 with os2d_train_crop_boxes: per anchor of the level the stride-aligned crop window of
        ``crop_size`` around it that stays inside ``img_size``, and the anchor box, both through ``default_box_transform``.
        -> (crop_boxes BoxList, anchor_boxes BoxList, anchor_index int64 [H*W]) on the HIP device (``device``: default the
        current one).  A transform that is not a chain of BoxList.resize / transpose / crop raises ValueError."""
        if self.box_size.w != self.box_size.h or self.box_stride.w != self.box_stride.h:
            raise RuntimeError("anisotropic anchors are not supported")
        device = _hip_device() if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("get_box_to_cut_anchor runs on the HIP device only (no CPU fallback), got {}".format(device))
        ops, out_size = traced_box_ops(default_box_transform, img_size)
        HW = fm_size.h * fm_size.w
        crops = torch.empty(HW, 4, dtype=torch.float32, device=device)
        anchors = torch.empty(HW, 4, dtype=torch.float32, device=device)
        _, kinds, args = ops_tables([ops])
        _train_lib.call("os2d_train_crop_boxes", fm_size.h, fm_size.w, int(self.box_stride.w), int(self.box_size.w), int(img_size.w),
                        int(img_size.h), int(crop_size.w), int(crop_size.h), len(ops), kinds, args, crops, anchors, STREAM)
        return BoxList(crops, out_size), BoxList(anchors, out_size), torch.arange(HW, device=device)


def feature_map_size_c4(img_size):
    """Closed form of the ResNet-C4 output size (conv s2, maxpool s2, layer2 s2, layer3 s2, all with
    'same-ish' padding): four ceil-halvings.  Replaces the reference's dummy forward pass (model.py:91-114)."""
    def f(s):
        for _ in range(4):
            s = (s + 1) // 2
        return s
    return FeatureMapSize(w=f(img_size.w), h=f(img_size.h))


class Matcher(object):
    """torchvision's ``Matcher(high, low)`` without low-quality matches, as the kernels apply it: per column of an IoU matrix
    [n_gt, n_det] the row of the first maximum, -1 where it is below ``low``, -2 where it is in [low, high)."""
    BELOW_LOW_THRESHOLD, BETWEEN_THRESHOLDS = -1, -2

    def __init__(self, high_threshold, low_threshold):
        self.high_threshold, self.low_threshold = high_threshold, low_threshold

    def __call__(self, ious):
        best, index = ious.max(dim=0)
        index = torch.where(best < self.high_threshold, torch.full_like(index, self.BETWEEN_THRESHOLDS), index)
        return torch.where(best < self.low_threshold, torch.full_like(index, self.BELOW_LOW_THRESHOLD), index)


def _hip_device(boxes=None):
    """The device of these boxes when they are on one already, else the current HIP device."""
    on_device = boxes is not None and boxes.bbox_xyxy.is_cuda
    return boxes.bbox_xyxy.device if on_device else torch.device("cuda", torch.cuda.current_device())


def _label_rows(class_ids):
    """-> (ids, labels, rows_of): the class id of every head row, the labels in the order of the result, and per label the
    head rows that carry it, in row order (several for class-image views, reference box_coder.py:483-487)."""
    ids = [int(c) for c in class_ids]
    labels = list(set(ids))   # the reference iterates ``set(class_ids)`` (box_coder.py:483): same order, whatever it is
    rows_of = {l: [] for l in labels}
    for i, c in enumerate(ids):
        rows_of[c].append(i)
    return ids, labels, rows_of


def _require_device(loc, cls=None):
    """The decode kernels read float32 loc_scores (and the cls_scores, where they get them) on the HIP device."""
    if not (loc.is_cuda and (cls is None or cls.is_cuda) and loc.dtype == torch.float32):
        raise RuntimeError("decode runs on the HIP device only (no CPU fallback)")


def _level_inputs(loc, cls, B, hw, dev):
    """A level's loc_scores [B,4,hw] and cls_scores [B,hw] as the fused kernels get them: checked, contiguous, float32."""
    _require_device(loc, cls)
    assert loc.device == dev and cls.device == dev, "scores and boxes should be on the same device"
    loc, cls = loc.contiguous(), cls.float().contiguous()
    assert tuple(loc.shape) == (B, 4, hw) and tuple(cls.shape) == (B, hw), "level tensors do not match class_ids / feature map"
    return loc, cls


def _detections(boxes, scores, labels, default_boxes, corners, out_size):
    """What ``decode_pyramid`` returns, whichever route made it: boxes [n,4] on an image of ``out_size`` with the fields scores
    [n], labels [n] int64, default_boxes (a BoxList of the anchors) and, where corners [n,8] are given, transform_corners."""
    result = BoxList(boxes, out_size)
    result.add_field("scores", scores)
    result.add_field("labels", labels)
    result.add_field("default_boxes", BoxList(default_boxes, out_size))
    if corners is not None:
        result.add_field("transform_corners", corners)
    return result


class Os2dBoxCoder(object):
    """reference box_coder.py:169-536: decode + NMS for inference, encode / remap_anchor_targets for training."""

    def __init__(self, positive_iou_threshold=0.5, negative_iou_threshold=0.1,
                 remap_classification_targets_iou_pos=0.5, remap_classification_targets_iou_neg=0.1,
                 output_box_grid_generator=None, function_get_feature_map_size=None, do_nms_across_classes=False):
        self.get_feature_map_size = function_get_feature_map_size or feature_map_size_c4
        self.output_box_grid_generator = output_box_grid_generator
        self.positive_iou_threshold = positive_iou_threshold
        self.negative_iou_threshold = negative_iou_threshold
        self.remap_classification_targets_iou_pos = remap_classification_targets_iou_pos
        self.remap_classification_targets_iou_neg = remap_classification_targets_iou_neg
        self.do_nms_across_classes = do_nms_across_classes
        self.nms_max_batch = 10000          # reference bounding_box.py:344 (``nms_max_batch_size``)
        self.use_fused_level_kernel = True  # single-level calls go through os2d_detect_level when the level fits,
                                            # several levels through os2d_detect_pyramid
        self.fused_pyramid_passes = 3       # chunked-NMS passes launched by os2d_detect_pyramid (more -> generic path)
        self.weights = BOX_ENCODING_WEIGHTS
        g = output_box_grid_generator
        if g is None:
            raise RuntimeError("output_box_grid_generator is required (head_creator.box_grid_generator_image_level)")
        if g.box_size.w != g.box_size.h or g.box_stride.w != g.box_stride.h:
            raise RuntimeError("anisotropic anchors are not supported")
        self._stride = int(g.box_stride.w)
        self._rec_field = int(g.box_size.w - self._stride * 14)
        self.matcher = Matcher(self.positive_iou_threshold, self.negative_iou_threshold)
        self.matcher_remap = Matcher(self.remap_classification_targets_iou_pos, self.remap_classification_targets_iou_neg)

    def _get_default_boxes(self, img_size):
        """reference box_coder.py:191-203 (CPU anchors as a BoxList; the kernels use the closed form)."""
        fm = self.get_feature_map_size(img_size)
        return BoxList(self.output_box_grid_generator.create_strided_boxes_columnfirst(fm), image_size=img_size)

    # ------------------------------------------------------------------ decode of one level (os2d_decode_boxes)
    def decode_level(self, loc_scores, img_size):
        """loc_scores [NB,4,HW] device tensor -> boxes [NB,HW,4] xyxy clipped to the level image
        (reference box_coder.py:319-330 + bounding_box.py:261-265) with os2d_decode_boxes."""
        _require_device(loc_scores)
        loc_scores = loc_scores.contiguous()
        fm = self.get_feature_map_size(img_size)
        NB, four, HW = loc_scores.shape
        assert four == 4 and HW == fm.w * fm.h, "loc_scores {} do not match the feature map {}".format(tuple(loc_scores.shape), fm)
        boxes = torch.empty(NB, HW, 4, dtype=torch.float32, device=loc_scores.device)
        _lib.call("os2d_decode_boxes", loc_scores, NB, fm.h, fm.w, self._stride, self._rec_field, img_size.w, img_size.h, boxes, STREAM)
        return boxes

    def build_boxes_from_loc_scores(self, loc_scores, default_boxes):
        """reference box_coder.py:319-330 for ONE class: loc_scores [HW,4], default_boxes a BoxList carrying the
        level's image size.  Returns an (unclipped-to-nothing-smaller) BoxList like the reference."""
        img_size = default_boxes.image_size
        boxes = self.decode_level(loc_scores.t().contiguous().unsqueeze(0), img_size)[0]
        return BoxList(boxes, image_size=img_size, mode="xyxy")

    # ------------------------------------------------------------------ NMS (os2d_nms)
    @staticmethod
    def nms_sorted(boxes_sorted, counts, iou_threshold):
        """boxes_sorted [NC,N,4] (each list by decreasing score, counts[c] valid) -> keep mask [NC,N] bool."""
        if not boxes_sorted.is_cuda:
            raise RuntimeError("NMS runs on the HIP device only (no CPU fallback)")
        boxes_sorted = boxes_sorted.contiguous().float()
        NC, N, _ = boxes_sorted.shape
        dev = boxes_sorted.device
        counts = counts.to(device=dev, dtype=torch.int32).contiguous()
        keep = torch.empty(NC, N, dtype=torch.uint8, device=dev)
        num_keep = torch.empty(NC, dtype=torch.int32, device=dev)
        nbytes = ctypes.c_size_t()
        _lib.call("os2d_nms_workspace_bytes", NC, N, ctypes.byref(nbytes))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        _lib.call("os2d_nms", boxes_sorted, counts, NC, N, iou_threshold, keep, num_keep, ws, ws.numel(), STREAM)
        return keep.bool()

    def _nms_lists(self, boxes, scores, valid, iou_threshold, nms_max_batch=10000):
        """Batched equivalent of reference bounding_box.py:343-374 for NC independent lists padded to a common
        length: boxes [NC,N,4], scores [NC,N], valid [NC,N] bool.  Lists longer than ``nms_max_batch`` go through
        the reference's chunk-and-repeat scheme: the current id list (at first the valid entries in list order) is cut
        into consecutive chunks of ``nms_max_batch``, every chunk is NMS-ed on its own, the survivors are concatenated
        chunk by chunk in score order, until a list needed one chunk only or lost nothing.  Per pass: ONE stable sort
        by (chunk, descending score), ONE gather and ONE ``os2d_nms`` launch over all NC x chunks lists, one host
        synchronisation.  Lists that are finished are stable under further passes (an NMS of its own output removes
        nothing), so all lists simply iterate until the last one is done.  Returns a bool keep mask [NC,N]."""
        NC, N = scores.shape
        dev = scores.device
        M = int(nms_max_batch)
        # descending-score sort key as a non-negative int64 < 2^32 (smaller = higher score; -0 and +0 tie like in a float sort)
        bits = (scores.float() + 0.0).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        asc = torch.where((bits >> 31) == 1, bits ^ 0xFFFFFFFF, bits | 0x80000000)
        desc_key = 0xFFFFFFFF - asc
        cnt = valid.sum(1)
        n_max = int(cnt.max())
        if n_max == 0:
            return torch.zeros_like(valid)
        ids = torch.argsort((~valid).to(torch.uint8), dim=1, stable=True)[:, :n_max]      # valid entries, list order
        while True:
            L = ids.size(1)
            num_chunks = (n_max + M - 1) // M
            pos = torch.arange(L, device=dev).unsqueeze(0)
            inlist = pos < cnt.unsqueeze(1)
            key = torch.where(inlist, ((pos // M) << 32) | torch.gather(desc_key, 1, ids),
                              torch.full((1, 1), (num_chunks + 1) << 32, dtype=torch.int64, device=dev))
            order = torch.argsort(key, dim=1, stable=True)
            ids_sorted = torch.gather(ids, 1, order)          # chunk ch of a list = sorted positions [ch*M, ch*M + its count)
            Lp = num_chunks * M
            padded = ids_sorted if L == Lp else torch.cat(
                [ids_sorted[:, :Lp], torch.zeros(NC, max(Lp - L, 0), dtype=ids.dtype, device=dev)], 1)
            b_sorted = torch.gather(boxes, 1, padded.unsqueeze(-1).expand(-1, -1, 4)).view(NC * num_chunks, M, 4)
            cnt_ch = (cnt.unsqueeze(1) - torch.arange(num_chunks, device=dev).unsqueeze(0) * M).clamp(0, M).reshape(-1)
            keep_sorted = self.nms_sorted(b_sorted, cnt_ch, iou_threshold).view(NC, Lp)
            keep_sorted = keep_sorted[:, :L] if Lp >= L else torch.cat(
                [keep_sorted, torch.zeros(NC, L - Lp, dtype=torch.bool, device=dev)], 1)
            new_cnt = keep_sorted.sum(1)
            compact = torch.argsort((~keep_sorted).to(torch.uint8), dim=1, stable=True)   # survivors first, arrangement kept
            ids = torch.gather(ids_sorted, 1, compact)
            more = (((cnt + M - 1) // M > 1) & (new_cnt != cnt)).any()
            new_max, more = torch.stack([new_cnt.max(), more.to(new_cnt.dtype)]).tolist()  # the pass's one synchronisation
            cnt, n_max = new_cnt, int(new_max)
            ids = ids[:, :max(n_max, 1)]
            if not more:
                break
        alive = torch.zeros(NC, N + 1, dtype=torch.bool, device=dev)
        pos = torch.arange(ids.size(1), device=dev).unsqueeze(0)
        alive.scatter_(1, torch.where(pos < cnt.unsqueeze(1), ids, torch.full_like(ids, N)), True)
        return alive[:, :N]

    # ------------------------------------------------------------------ decode + NMS of a pyramid: three routes to one result
    def decode_pyramid(self, loc_scores_pyramid, cls_scores_pyramid, img_size_pyramid, class_ids,
                       nms_score_threshold=0.0, nms_iou_threshold=0.3, inverse_box_transforms=None,
                       transform_corners_pyramid=None):
        """reference box_coder.py:448-536 on the device, batched over classes:
        per level decode + clip (os2d_decode_boxes), score / empty-box mask, map to the original image
        (``inverse_box_transforms[l]`` is applied ONCE to a BoxList holding the level's boxes of all classes),
        concatenate levels, per-label NMS (os2d_nms), sort by score.  Entries of ``class_ids`` with the same id
        are merged before NMS, labels appear in the iteration order of ``set(class_ids)`` like in the reference (ascending
        for small ids).
        Returns a BoxList with fields scores, labels, default_boxes (and transform_corners if given)."""
        num_classes = len(class_ids)
        dev = cls_scores_pyramid[0].device
        if inverse_box_transforms is None:
            # the reference concatenates the levels of a label with cat_boxlist, which asserts one common image size
            # (bounding_box.py:390-437): levels of different sizes need transforms into a common frame
            if len({(s_.w, s_.h) for s_ in img_size_pyramid}) > 1:     # (not an ``assert``: must survive ``python -O``)
                raise ValueError("pyramid levels live on different image sizes ({}): pass inverse_box_transforms to map them to "
                                 "one image size before they are merged".format(sorted({(s_.w, s_.h) for s_ in img_size_pyramid})))
        fused = self._decode_single_level_fused(loc_scores_pyramid, cls_scores_pyramid, img_size_pyramid, class_ids,
                                                nms_score_threshold, nms_iou_threshold, inverse_box_transforms,
                                                transform_corners_pyramid)
        if fused is None:
            fused = self._decode_pyramid_fused(loc_scores_pyramid, cls_scores_pyramid, img_size_pyramid, class_ids,
                                               nms_score_threshold, nms_iou_threshold, inverse_box_transforms,
                                               transform_corners_pyramid)
        if fused is not None:
            return self._nms_across_classes(fused, nms_iou_threshold)
        boxes_l, scores_l, valid_l, dflt_l, corners_l = [], [], [], [], []
        for lvl, (loc, cls, img_size) in enumerate(zip(loc_scores_pyramid, cls_scores_pyramid, img_size_pyramid)):
            assert loc.device == dev and cls.device == dev, "scores and boxes should be on the same device"
            boxes = self.decode_level(loc, img_size)                                    # [B,HW,4]
            cls = cls.float()
            empty = (boxes[..., 3] <= boxes[..., 1]) | (boxes[..., 2] <= boxes[..., 0])
            valid = (cls > nms_score_threshold) & ~empty
            HW = boxes.size(1)
            dflt = self._get_default_boxes(img_size).bbox_xyxy.to(dev)                   # [HW,4]
            corners = None
            if transform_corners_pyramid is not None:
                corners = transform_corners_pyramid[lvl].transpose(1, 2).reshape(num_classes * HW * 2, 4)
            if inverse_box_transforms is not None:
                boxes, dflt, corners, _ = transform_level_boxes(inverse_box_transforms[lvl], boxes.reshape(-1, 4), dflt, corners, img_size)
                boxes = boxes.reshape(num_classes, HW, 4)
            boxes_l.append(boxes)
            scores_l.append(cls)
            valid_l.append(valid)
            dflt_l.append(dflt.unsqueeze(0).expand(num_classes, HW, 4))
            if corners is not None:
                corners_l.append(corners.reshape(num_classes, HW, 8))
        boxes = torch.cat(boxes_l, 1)
        scores = torch.cat(scores_l, 1)
        valid = torch.cat(valid_l, 1)
        dflt = torch.cat(dflt_l, 1)
        corners = torch.cat(corners_l, 1) if corners_l else None
        # merge rows that share a real label
        ids, labels_sorted, rows_of = _label_rows(class_ids)
        groups = [rows_of[l] for l in labels_sorted]
        if labels_sorted != ids:
            width = max(len(g) for g in groups) * boxes.size(1)

            def merge(t, fill):
                out = []
                for g in groups:
                    m = torch.cat([t[i] for i in g], 0)
                    pad = width - m.size(0)
                    if pad:
                        m = torch.cat([m, torch.full((pad,) + tuple(m.shape[1:]), fill, dtype=m.dtype, device=dev)], 0)
                    out.append(m)
                return torch.stack(out, 0)
            boxes, scores, valid, dflt = merge(boxes, 0.0), merge(scores, float("-inf")), merge(valid, False), merge(dflt, 0.0)
            corners = merge(corners, 0.0) if corners is not None else None
        if boxes.size(1) <= self.nms_max_batch:
            # every list fits one NMS batch (always true for a single level): ONE stable sort by score, NMS on the sorted
            # lists, and the survivors are already in the output order - no host synchronisation before the final
            # ``nonzero`` that sizes the result
            key = torch.where(valid, scores, torch.full_like(scores, float("-inf")))
            order = torch.argsort(key, dim=1, descending=True, stable=True)
            b_sorted = torch.gather(boxes, 1, order.unsqueeze(-1).expand(-1, -1, 4))
            keep_sorted = self.nms_sorted(b_sorted, valid.sum(1), nms_iou_threshold)
        else:
            keep = self._nms_lists(boxes, scores, valid, nms_iou_threshold, self.nms_max_batch)
            # per label: survivors by decreasing score (box_coder.py:431-437)
            key = torch.where(keep, scores, torch.full_like(scores, float("-inf")))
            order = torch.argsort(key, dim=1, descending=True, stable=True)
            keep_sorted = torch.gather(keep, 1, order)
        sel = keep_sorted.reshape(-1).nonzero().squeeze(1)
        flat = (order + torch.arange(order.size(0), device=dev).unsqueeze(1) * order.size(1)).reshape(-1)[sel]
        out_size = img_size_pyramid[0]
        if inverse_box_transforms is not None:
            out_size = inverse_box_transforms[0](BoxList(torch.zeros(1, 4, device=dev), img_size_pyramid[0])).image_size
        lab = torch.tensor(labels_sorted, dtype=torch.long, device=dev).unsqueeze(1).expand(-1, order.size(1)).reshape(-1)
        result = _detections(boxes.reshape(-1, 4)[flat], scores.reshape(-1)[flat], lab[sel], dflt.reshape(-1, 4)[flat],
                             corners.reshape(-1, 8)[flat] if corners is not None else None, out_size)
        return self._nms_across_classes(result, nms_iou_threshold)

    def _nms_across_classes(self, result, nms_iou_threshold):
        """reference box_coder.py:530-534 (``eval.nms_across_classes``, off by default)."""
        if self.do_nms_across_classes and len(result) > 0:
            b = result.bbox_xyxy.unsqueeze(0)
            s = result.get_field("scores").unsqueeze(0)
            k = self._nms_lists(b, s, torch.ones_like(s, dtype=torch.bool), nms_iou_threshold)[0]
            idx = k.nonzero().squeeze(1)
            idx = idx[torch.argsort(s[0][idx], descending=True, stable=True)]
            result = result[idx]
        return result

    def _decode_single_level_fused(self, loc_pyr, cls_pyr, size_pyr, class_ids, score_thr, iou_thr, inverse, corners_pyr):
        """One level, one row per label, an identity / ``ResizeBoxes`` mapping, and a level that fits the kernel's LDS:
        the whole per-class chain runs in ONE launch (os2d_detect_level); None when the generic path has to be used."""
        if not self.use_fused_level_kernel or len(loc_pyr) != 1:
            return None
        ids, labels, rows_of = _label_rows(class_ids)
        if len(labels) != len(ids):
            return None
        loc, cls, img_size = loc_pyr[0], cls_pyr[0], size_pyr[0]
        traced = trace_box_transform(inverse[0] if inverse is not None else None, img_size)
        if traced is None:
            return None
        ops, default_ops, out_size = traced
        fm = self.get_feature_map_size(img_size)
        lib = _lib.load()
        if not lib.os2d_detect_level_supported(fm.h, fm.w):
            return None
        dev = cls.device
        B, HW = len(ids), fm.h * fm.w
        loc, cls = _level_inputs(loc, cls, B, HW, dev)
        counts_c, kinds_c, args_c = ops_tables([ops])
        out_boxes = torch.empty(B, HW, 4, dtype=torch.float32, device=dev)
        out_scores = torch.empty(B, HW, dtype=torch.float32, device=dev)
        out_index = torch.empty(B, HW, dtype=torch.int32, device=dev)
        out_count = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.call("os2d_detect_level_ops", loc, cls, B, fm.h, fm.w, self._stride, self._rec_field, img_size.w, img_size.h, len(ops),
                  kinds_c, args_c, score_thr, iou_thr, out_boxes, out_scores, out_index, out_count, STREAM)
        # rows in the label order of the reference, survivors of a row by score
        order = [rows_of[l][0] for l in labels]
        perm = torch.tensor(order, dtype=torch.long, device=dev) if order != list(range(B)) else None
        counts = out_count[perm] if perm is not None else out_count
        mask = torch.arange(HW, device=dev).unsqueeze(0) < counts.unsqueeze(1)
        row, pos = mask.nonzero(as_tuple=True)                   # the one host synchronisation: sizes the result
        src_row = perm[row] if perm is not None else row
        flat = src_row * HW + pos
        boxes, scores = out_boxes.view(-1, 4)[flat], out_scores.view(-1)[flat]
        lab = torch.tensor(labels, dtype=torch.long, device=dev)[row]
        loc_idx = out_index.view(-1)[flat].long()
        dflt = apply_box_ops(self._get_default_boxes(img_size).bbox_xyxy.to(dev)[loc_idx], default_ops)
        corners = None
        if corners_pyr is not None:
            corners = corners_pyr[0][src_row, :, loc_idx]                                   # [n, 8]
            # like the reference, the corners go through the level's transform as the two "boxes" (x0, y0, x1, y1), (x2, y2, x3, y3)
            corners = apply_box_ops(corners.reshape(-1, 4), ops).view(-1, 8)
        return _detections(boxes, scores, lab, dflt, corners, out_size)

    def _slot_rows(self, ids, labels, rows_of, V, dev):
        """Device table [G][V] of the head rows of every label (-1: no such view), cached per (class ids, device): the rows of
        an evaluation's class batch are the same for every image, and building the table is a blocking host-to-device copy
        from pageable memory on the per-image path."""
        cache = self.__dict__.setdefault("_slot_rows_cache", {})
        key = (ids, V, str(dev))
        stream = torch.cuda.current_stream(dev)
        entry = cache.get(key)
        if entry is None:
            host = torch.tensor([(rows_of[l] + [-1] * V)[:V] for l in labels], dtype=torch.int32).pin_memory()
            table = host.to(dev, non_blocking=True)
            event = torch.cuda.Event()
            event.record(stream)
            if len(cache) >= 16:
                cache.pop(next(iter(cache)))
            # the pinned source lives as long as the copy may be in flight; the event marks the end of the copy
            entry = cache[key] = (table, host, event, stream.cuda_stream)
        table, _, event, producer = entry
        if stream.cuda_stream != producer:
            # a decode on ANOTHER stream than the one that filled the table: wait for the copy, and tell the caching
            # allocator that this stream reads the tensor too - an evicted entry must not be reused under a running kernel
            stream.wait_event(event)
            table.record_stream(stream)
        return table

    def _decode_pyramid_fused(self, loc_pyr, cls_pyr, size_pyr, class_ids, score_thr, iou_thr, inverse, corners_pyr):
        """Several levels and / or merged labels (class-image views: several head rows with one class id, reference
        box_coder.py:483-487), identity / ``ResizeBoxes`` mappings: the whole per-label chain, incl. the reference's
        chunk-and-repeat NMS for lists longer than ``nms_max_batch``, runs on the device (os2d_detect_pyramid /
        os2d_detect_pyramid_merged: one launch per NMS pass, a work-group per (chunk, label)); None when the generic path has
        to be used."""
        if not self.use_fused_level_kernel:
            return None
        # (a single level with one row per label normally took os2d_detect_level before this is called; levels beyond that
        # kernel's LDS budget - more than ~5,900 locations, e.g. 72 x 96 - come here as a pyramid of one level)
        ts = list(inverse) if inverse is not None else [None] * len(loc_pyr)
        traced = [trace_box_transform(t, s_) for t, s_ in zip(ts, size_pyr)]
        if any(t is None for t in traced):
            return None      # an entry that is not a chain of BoxList.resize / transpose / crop: generic path
        if len({(sz.w, sz.h) for _, _, sz in traced}) != 1:
            return None      # levels that end on different image sizes: the generic path fails like the reference's cat_boxlist
        lib = _lib.load()
        L = len(loc_pyr)
        fms = [self.get_feature_map_size(s) for s in size_pyr]
        hws = [fm.h * fm.w for fm in fms]
        N1 = sum(hws)                                         # candidates per head row
        ids, labels, rows_of = _label_rows(class_ids)
        G, V = len(labels), max(len(r) for r in rows_of.values())
        N = N1 * V                                            # candidates per label
        if N > (1 << 22) or not lib.os2d_detect_pyramid_supported(L, N, int(self.nms_max_batch)):
            return None
        dev = cls_pyr[0].device
        B = len(ids)
        locs, clss = [], []
        for loc, cls, hw in zip(loc_pyr, cls_pyr, hws):
            loc, cls = _level_inputs(loc, cls, B, hw, dev)
            locs.append(loc)
            clss.append(cls)
        out_size = traced[0][2]
        c_counts, c_kinds, c_args = ops_tables([t_[0] for t_ in traced])
        d_counts, d_kinds, d_args = ops_tables([t_[1] for t_ in traced], MAX_DEFAULT_BOX_OPS)
        passes = int(self.fused_pyramid_passes)
        nbytes = ctypes.c_size_t()
        _lib.call("os2d_detect_pyramid_workspace_bytes", G, N, passes, ctypes.byref(nbytes))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        out_boxes = torch.empty(G, N, 4, dtype=torch.float32, device=dev)
        out_scores = torch.empty(G, N, dtype=torch.float32, device=dev)
        out_index = torch.empty(G, N, dtype=torch.int32, device=dev)
        out_count = torch.empty(G, dtype=torch.int32, device=dev)
        out_default = torch.empty(G, N, 4, dtype=torch.float32, device=dev)
        unfinished = torch.empty(1, dtype=torch.int32, device=dev)
        c_loc = (ctypes.c_void_p * L)(*[t.data_ptr() for t in locs])
        c_cls = (ctypes.c_void_p * L)(*[t.data_ptr() for t in clss])
        c_cor, out_corners, cors = None, None, None
        if corners_pyr is not None:
            cors = [k.reshape(B, 8, hw).float().contiguous() for k, hw in zip(corners_pyr, hws)]
            c_cor = (ctypes.c_void_p * L)(*[t.data_ptr() for t in cors])
            out_corners = torch.empty(G, N, 8, dtype=torch.float32, device=dev)
        c_hw = (ctypes.c_int * (2 * L))(*[v for fm in fms for v in (fm.h, fm.w)])
        c_img = (ctypes.c_float * (2 * L))(*[float(v) for s_ in size_pyr for v in (s_.w, s_.h)])
        identity = labels == ids                         # one row per label, already in the reference's label order
        with torch.cuda.device(dev):                     # the table's upload and its event
            slot_rows = None if identity else self._slot_rows(tuple(ids), tuple(labels), rows_of, V, dev)
        _lib.call("os2d_detect_pyramid_ops", c_loc, c_cls, c_cor, B, L, c_hw, self._stride, self._rec_field, c_img, c_counts, c_kinds,
                  c_args, d_counts, d_kinds, d_args, score_thr, iou_thr, int(self.nms_max_batch), passes, G, V, slot_rows, out_boxes,
                  out_scores, out_index, out_default, out_corners, out_count, unfinished, ws, ws.numel(), STREAM)
        mask = torch.arange(N, device=dev).unsqueeze(0) < out_count.unsqueeze(1)
        row, pos = mask.nonzero(as_tuple=True)                   # the one host synchronisation: sizes the result
        if int(unfinished.item()) != 0:
            return None          # some label needs more NMS passes than were launched: generic path (exact, slower)
        flat = row * N + pos
        return _detections(out_boxes.view(-1, 4)[flat], out_scores.view(-1)[flat], torch.tensor(labels, dtype=torch.long, device=dev)[row],
                           out_default.view(-1, 4)[flat], out_corners.view(-1, 8)[flat] if out_corners is not None else None, out_size)

    # ------------------------------------------------------------------------------------------------ training targets
    @staticmethod
    def _pack_boxes(batch_boxes, device):
        """BoxLists (fields "labels", "difficult") -> gt_boxes [n,4] float32, gt_labels [n] int32, gt_difficult [n] uint8,
        image_offsets [A+1] int32 on ``device``; assembled on the host, once per batch."""
        boxes = [b.bbox_xyxy.detach().to("cpu", torch.float32).reshape(-1, 4) for b in batch_boxes]
        labels = [b.get_field("labels").detach().to("cpu", torch.int32).reshape(-1) for b in batch_boxes]
        difficult = [b.get_field("difficult").detach().to("cpu", torch.uint8).reshape(-1) if b.has_field("difficult")
                     else torch.zeros(len(b), dtype=torch.uint8) for b in batch_boxes]
        offsets = [0]
        for b in boxes:
            offsets.append(offsets[-1] + b.shape[0])
        n = offsets[-1]
        packed = (torch.cat(boxes).contiguous(), torch.cat(labels).contiguous(), torch.cat(difficult).contiguous(),
                  torch.tensor(offsets, dtype=torch.int32))
        return tuple(t.to(device, non_blocking=True) for t in packed) + (n,)

    def _assign(self, mode, batch_boxes, fm, num_labels, device, loc_scores=None, ops=None):
        """``ops``: None = the plain anchors (os2d_train_assign_targets), else a box-op chain (os2d_train_assign_targets_ops)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("target assignment runs on the HIP device only (no CPU fallback), got {}".format(device))
        A, HW = len(batch_boxes), fm.h * fm.w
        gt_boxes, gt_labels, gt_difficult, offsets, n = self._pack_boxes(batch_boxes, device)
        cls_targets = torch.empty(A, num_labels, HW, dtype=torch.int64, device=device)
        if mode == 0:
            outs = (torch.empty(A, num_labels, 4, HW, dtype=torch.float32, device=device), None, None)
            high, low = self.positive_iou_threshold, self.negative_iou_threshold
        else:
            outs = (None, torch.empty(A, num_labels, HW, dtype=torch.float32, device=device),
                    torch.empty(A, num_labels, HW, dtype=torch.float32, device=device))
            high, low = self.remap_classification_targets_iou_pos, self.remap_classification_targets_iou_neg
        head = (mode, gt_boxes if n else None, gt_labels if n else None, gt_difficult if n else None, offsets, n, loc_scores, A, num_labels,
                fm.h, fm.w, self._stride, self._rec_field, high, low)
        tail = (outs[0], cls_targets, outs[1], outs[2], STREAM)
        if ops is None:
            _train_lib.call("os2d_train_assign_targets", *(head + tail))
        else:
            if len(ops) > MAX_BOX_OPS:
                raise ValueError("a box-op chain of {} entries: at most {} are supported".format(len(ops), MAX_BOX_OPS))
            _, kinds, args = ops_tables([ops])
            _train_lib.call("os2d_train_assign_targets_ops", *(head + (len(ops), kinds, args) + tail))
        return cls_targets, outs

    def encode_batch(self, batch_boxes, img_size, num_labels, device):
        """``encode`` of every image of a batch in ONE launch: -> loc_targets [A,num_labels,4,HW] float32, cls_targets
        [A,num_labels,HW] int64 on ``device`` (what the reference's data loader stacks from per-image ``encode`` calls)."""
        cls_targets, outs = self._assign(0, batch_boxes, self.get_feature_map_size(img_size), num_labels, device)
        return outs[0], cls_targets

    def encode(self, boxes, img_size, num_labels, default_box_transform=None):
        """reference box_coder.py:332-389: -> loc_targets [num_labels,4,HW] float32, cls_targets [num_labels,HW] int64 (1
        positive, 0 negative, -1 ignored), on the HIP device (that of ``boxes`` when it is there already)."""
        if default_box_transform is not None:
            raise NotImplementedError("default_box_transform is not supported here: use encode_transformed")
        loc_targets, cls_targets = self.encode_batch([boxes], img_size, num_labels, _hip_device(boxes))
        return loc_targets[0], cls_targets[0]

    def encode_pyramid(self, boxes, img_size_pyramid, num_labels, default_box_transform_pyramid=None):
        """reference box_coder.py:391-421: ``encode`` per pyramid level -> (list of loc_targets, list of cls_targets)."""
        if default_box_transform_pyramid is not None and any(t is not None for t in default_box_transform_pyramid):
            raise NotImplementedError("default_box_transform_pyramid is not supported here: use encode_pyramid_transformed")
        levels = [self.encode(boxes, img_size, num_labels) for img_size in img_size_pyramid]
        return [l[0] for l in levels], [l[1] for l in levels]

    def remap_anchor_targets(self, loc_scores, batch_img_size, class_image_sizes, batch_boxes, box_reverse_transform=None):
        """reference box_coder.py:234-300: the targets after the model's localisation.  loc_scores [A,B,4,HW] on the HIP
        device -> cls_targets_remapped [A,B,HW] int64, ious_anchor, ious_anchor_corrected [A,B,HW] float32.  One launch,
        no host synchronisation.  The images of a batch share one size (they are one tensor)."""
        if box_reverse_transform is not None:
            raise NotImplementedError("box_reverse_transform is not supported here: use remap_anchor_targets_transformed")
        A, B, fm = self._remap_args("remap_anchor_targets", loc_scores, batch_img_size, batch_boxes)
        cls_targets, outs = self._assign(1, batch_boxes, fm, B, loc_scores.device, loc_scores.detach().contiguous())
        return cls_targets, outs[1], outs[2]

    def _remap_args(self, name, loc_scores, batch_img_size, batch_boxes):
        """The argument checks of ``remap_anchor_targets`` and its ``_transformed`` twin -> (A images, B labels, feature map size)."""
        if not (loc_scores.is_cuda and loc_scores.dtype == torch.float32):
            raise RuntimeError("{} runs on the HIP device only (no CPU fallback)".format(name))
        A, B = loc_scores.shape[0], loc_scores.shape[1]
        if len(batch_boxes) != A or len(batch_img_size) != A:
            raise ValueError("batch_boxes / batch_img_size must have one entry per image ({})".format(A))
        fm = self.get_feature_map_size(batch_img_size[0])
        if any(self.get_feature_map_size(s) != fm for s in batch_img_size[1:]) or fm.h * fm.w != loc_scores.shape[3]:
            raise ValueError("the images of a batch must share one feature map size that matches loc_scores")
        return A, B, fm

    # ---------------------------------------------------------------- targets under a box transform (hard-patch mining)
    def encode_transformed(self, boxes, img_size, num_labels, default_box_transform=None, device=None):
        """reference ``encode(..., default_box_transform=...)`` (box_coder.py:332-394): the anchors of ``img_size`` go through
        the transform before they are matched with ``boxes``, clipped to a minimal size and encoded.  The transform is a chain
        of BoxList.resize / transpose / crop calls (the reference's ``TransformList``) or a recorded chain of
        (kind, ax, ay) tuples; anything else raises ValueError.  -> loc_targets [num_labels,4,HW], cls_targets [num_labels,HW]."""
        ops = as_box_ops(default_box_transform, img_size)
        device = _hip_device(boxes) if device is None else device
        cls_targets, outs = self._assign(0, [boxes], self.get_feature_map_size(img_size), num_labels, device, ops=ops)
        return outs[0][0], cls_targets[0]

    def encode_pyramid_transformed(self, boxes, img_size_pyramid, num_labels, default_box_transform_pyramid=None, device=None):
        """reference ``encode_pyramid(..., default_box_transform_pyramid=...)`` (box_coder.py:396-422)."""
        ts = default_box_transform_pyramid if default_box_transform_pyramid is not None else [None] * len(img_size_pyramid)
        levels = [self.encode_transformed(boxes, s, num_labels, t, device=device) for s, t in zip(img_size_pyramid, ts)]
        return [l[0] for l in levels], [l[1] for l in levels]

    def remap_anchor_targets_transformed(self, loc_scores, batch_img_size, class_image_sizes, batch_boxes, box_reverse_transform=None):
        """reference ``remap_anchor_targets(..., box_reverse_transform=...)`` (box_coder.py:234-303): the box decoded from
        ``loc_scores`` against the plain anchor and the anchor itself go through the image's transform before they meet the
        ground truth.  ``box_reverse_transform``: one entry per image.  One launch when the images share a chain (mining
        handles one image at a time), else one per image; no host synchronisation."""
        A, B, fm = self._remap_args("remap_anchor_targets_transformed", loc_scores, batch_img_size, batch_boxes)
        ts = box_reverse_transform if box_reverse_transform is not None else [None] * A
        if len(ts) != A:
            raise ValueError("box_reverse_transform must have one entry per image ({})".format(A))
        chains = [as_box_ops(t, s) for t, s in zip(ts, batch_img_size)]
        loc_scores = loc_scores.detach().contiguous()
        if all(c == chains[0] for c in chains[1:]):
            cls_targets, outs = self._assign(1, batch_boxes, fm, B, loc_scores.device, loc_scores, ops=chains[0])
            return cls_targets, outs[1], outs[2]
        parts = [self._assign(1, [batch_boxes[a]], fm, B, loc_scores.device, loc_scores[a:a + 1], ops=chains[a]) for a in range(A)]
        return (torch.cat([p[0] for p in parts]), torch.cat([p[1][1] for p in parts]), torch.cat([p[1][2] for p in parts]))

    @staticmethod
    def _chain(transform, img_size):
        """``box_ops.as_box_ops`` under the coder's name for it."""
        return as_box_ops(transform, img_size)

    # ---------------------------------------------------------------- the reference's public helpers (plain tensors, no kernel)
    @staticmethod
    def apply_transform_to_corners(masked_transform_corners, transform, img_size):
        """reference box_coder.py:439-446: corners [n,8] (x,y,x,y,x,y,x,y) go through the transform as two boxes each."""
        ops = as_box_ops(transform, img_size)
        return apply_box_ops(masked_transform_corners.contiguous().view(-1, 4), ops).contiguous().view(-1, 8)

    @staticmethod
    def build_loc_targets(class_boxes, default_boxes):
        """reference box_coder.py:302-317 on two BoxLists of equal length (clip_to_min_size(1), then encode_boxes with
        weights (10, 10, 5, 5)): the reference's public helper.  ``encode`` does not come here - the kernel encodes against
        the closed-form anchors."""
        def clipped(b):
            b = b.bbox_xyxy
            x2 = torch.where(b[:, 0] + 1 > b[:, 2], b[:, 0] + 1, b[:, 2])
            y2 = torch.where(b[:, 1] + 1 > b[:, 3], b[:, 1] + 1, b[:, 3])
            return b[:, 0], b[:, 1], x2, y2
        gx1, gy1, gx2, gy2 = clipped(class_boxes)
        px1, py1, px2, py2 = clipped(default_boxes)
        ew, eh, gw, gh = px2 - px1, py2 - py1, gx2 - gx1, gy2 - gy1
        wx, wy, ww, wh = BOX_ENCODING_WEIGHTS
        return torch.stack([wx * ((gx1 + 0.5 * gw) - (px1 + 0.5 * ew)) / ew, wy * ((gy1 + 0.5 * gh) - (py1 + 0.5 * eh)) / eh,
                            ww * torch.log(gw / ew), wh * torch.log(gh / eh)], dim=1)

    @staticmethod
    def assign_anchors_to_boxes_threshold(detection_boxes, annotation_boxes, matcher):
        """reference box_coder.py:212-232 for arbitrary detection boxes: -> (index [n_det] of the matched annotation box, -1
        below the low threshold, -2 between the thresholds or matched to a difficult box; ious [n_gt, n_det]).  The
        reference's public helper; the kernels match against the closed-form anchors and do not come here."""
        a, d = annotation_boxes.bbox_xyxy, detection_boxes.bbox_xyxy
        wh = (torch.min(a[:, None, 2:], d[None, :, 2:]) - torch.max(a[:, None, :2], d[None, :, :2])).clamp(min=0)
        inter = wh[..., 0] * wh[..., 1]
        area_a, area_d = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
        ious = inter / (area_a[:, None] + area_d[None, :] - inter)
        index = matcher(ious)
        difficult = annotation_boxes.get_field("difficult").to(torch.bool)
        hit = index >= 0
        index = torch.where(hit & difficult[index.clamp(min=0)], torch.full_like(index, -2), index)
        return index, ious
