"""Hard-patch mining (reference os2d/engine/train.py:142-370) on the HIP kernels of libos2d_train.so.

Per training image the reference scores a small pyramid against the image's class batch, computes the per-anchor losses with
the criterion in patch-mining mode and keeps, for each of three roles - hard negatives ("neg"), hard positives ("pos") and
badly localised positives ("pos_loc") - the first ``num_hard_patches`` survivors of a greedy NMS over the stride-aligned crop
windows of the flagged (level, label, anchor) candidates.  Here the selection is one launch (os2d_train_mine_select): K rounds
of "take the best candidate alive, kill what overlaps it", the crop windows recomputed from (level, anchor); the records come
to the host in ONE copy per image, together with the scalar losses.

Differences from the reference, both deliberate: equal scores are taken in increasing (level, label,
anchor) order (the reference's sort leaves their order open), and the NMS is greedy over all candidates at any number of them
(the reference cuts lists longer than 10,000 into chunks, bounding_box.py:344-374; up to 10,000 the two agree).  Candidates
whose score is not finite are never selected.

The dataloader that consumes the records, the random choice of scales and negative classes, and visualisation are not here.
"""
import ctypes
from collections import OrderedDict

import torch

from .. import _train_lib
from .._native import STREAM
from ..modeling.box_ops import MAX_BOX_OPS, as_box_ops, ops_tables
from ..structures.bounding_box import BoxList
from ..structures.feature_map import FeatureMapSize

ROLES = ("neg", "pos", "pos_loc")
MAX_LEVELS, MAX_K = 8, 64                    # OS2D_MINE_MAX_LEVELS, OS2D_MINE_MAX_K
INDEX_INTS, VALUE_FLOATS = 3, 19             # OS2D_MINE_INDEX_INTS, OS2D_MINE_VALUE_FLOATS
F_POS, F_NEG, F_POSREG = 1, 2, 4             # flags of os2d_train_objective_forward


def _level_rows(t, A, B, hw, name):
    """A level's [A,B,hw] tensor as (tensor to keep alive, elements between two (image, label) rows): the level's slice of a
    merged pyramid is read in place, anything else is made dense."""
    if tuple(t.shape) != (A, B, hw):
        raise ValueError("{}: expected a [{}, {}, {}] tensor per level, got {}".format(name, A, B, hw, tuple(t.shape)))
    s = t.stride()
    if hw == 1 or s[2] == 1:
        row = s[1] if B > 1 else max(s[1], hw)
        if row >= hw and (A == 1 or s[0] == B * row):
            return t, int(row)
    return t.contiguous(), hw


def _flags_of(per_anchor):
    """The three masks of the criterion's per-anchor dictionary as the flag bytes the kernel reads (per level)."""
    out = []
    for pos, neg, reg in zip(per_anchor["pos_mask"], per_anchor["neg_mask"], per_anchor["pos_for_regression"]):
        out.append(pos.to(torch.uint8) * F_POS + neg.to(torch.uint8) * F_NEG + reg.to(torch.uint8) * F_POSREG)
    return out


def mine_select(per_anchor, cls_scores_pyramid, corners_pyramid, img_size_pyramid, fm_sizes, box_transforms, crop_size,
                nms_iou_threshold=0.5, num_hard_patches=10, box_grid_generator=None, out=None):
    """The K = ``num_hard_patches`` hardest patches per (image, role) of a pyramid, on the device, without synchronising.

    per_anchor          the criterion's patch-mining dictionary with per-level lists: "cls_loss", "loc_loss" float32 [A,B,HW_l]
                        and the flag bytes (bits 1 pos / 2 neg / 4 pos_for_regression) as its ``flags`` attribute (Os2dObjective
                        sets it) or a "flags" entry; without either they are rebuilt from the three bool masks "pos_mask",
                        "neg_mask", "pos_for_regression"
    cls_scores_pyramid  per level [A,B,HW_l] (or [B,HW_l] for one image)
    corners_pyramid     per level [A,B,8,HW_l] (or [B,8,HW_l]); None = zeros in the records
    img_size_pyramid    FeatureMapSize of every level's image; fm_sizes: FeatureMapSize of every level's feature map
    box_transforms      per level the transform into the original image: a chain of BoxList.resize / transpose / crop calls
                        (the reference's TransformList), a sequence of (kind, ax, ay), or None
    box_grid_generator  the BoxGridGenerator of the anchors (box size and stride)
    -> (count int32 [A,3], index int32 [A,3,K,3] = (level, label, anchor), values float32 [A,3,K,19] = crop xyxy, anchor xyxy,
    8 transformed corner values, cls_loss, loc_loss, score); roles in the order of ROLES."""
    if box_grid_generator is None:
        raise ValueError("mine_select needs the box_grid_generator of the anchors")
    L, K = len(img_size_pyramid), int(num_hard_patches)
    if not 1 <= L <= MAX_LEVELS:
        raise ValueError("mine_select handles 1 to {} pyramid levels, got {}".format(MAX_LEVELS, L))
    if not 1 <= K <= MAX_K:
        raise ValueError("num_hard_patches must be in 1..{}, got {}".format(MAX_K, K))
    if not (len(fm_sizes) == L and len(cls_scores_pyramid) == L and len(per_anchor["cls_loss"]) == L and len(per_anchor["loc_loss"]) == L):
        raise ValueError("every pyramid argument needs one entry per level ({})".format(L))
    transforms = list(box_transforms) if box_transforms is not None else [None] * L
    chains = [as_box_ops(t, s) for t, s in zip(transforms, img_size_pyramid)]     # ValueError for what cannot be expressed
    flags_l = per_anchor["flags"] if "flags" in per_anchor else getattr(per_anchor, "flags", None)
    if flags_l is None:
        flags_l = _flags_of(per_anchor)
    cls_scores = [t.unsqueeze(0) if t.dim() == 2 else t for t in cls_scores_pyramid]
    A, B = cls_scores[0].shape[0], cls_scores[0].shape[1]
    dev = cls_scores[0].device
    every = list(per_anchor["cls_loss"]) + list(per_anchor["loc_loss"]) + list(flags_l) + cls_scores + \
        (list(corners_pyramid) if corners_pyramid is not None else [])
    for t in every:
        if not (t.is_cuda and t.device == dev):
            raise RuntimeError("mine_select runs on the HIP device only (no CPU fallback): got a tensor on {}".format(t.device))
    keep, rows = [], []
    ptrs = {k: [] for k in ("cls_loss", "loc_loss", "flags", "cls_preds", "corners")}
    for l, fm in enumerate(fm_sizes):
        hw = fm.h * fm.w
        cl, row = _level_rows(per_anchor["cls_loss"][l].float(), A, B, hw, "cls_loss")
        ll, row_l = _level_rows(per_anchor["loc_loss"][l].float(), A, B, hw, "loc_loss")
        fl, row_f = _level_rows(flags_l[l], A, B, hw, "flags")
        if fl.dtype != torch.uint8:
            raise ValueError("flags must be uint8, got {}".format(fl.dtype))
        if not row == row_l == row_f:       # one stride per level in the ABI
            cl, ll, fl, row = cl.contiguous(), ll.contiguous(), fl.contiguous(), hw
        cp = cls_scores[l].float().contiguous()
        if tuple(cp.shape) != (A, B, hw):
            raise ValueError("cls_scores of level {}: expected {}, got {}".format(l, (A, B, hw), tuple(cp.shape)))
        level = [cl, ll, fl, cp]
        if corners_pyramid is not None:
            co = corners_pyramid[l].float().reshape(A, B, 8, hw).contiguous()
            level.append(co)
        keep.append(level)
        rows.append(row)
        for k, t in zip(("cls_loss", "loc_loss", "flags", "cls_preds", "corners"), level):
            ptrs[k].append(t.data_ptr())
    tl = _train_lib.load()
    c_hw = (ctypes.c_int * (2 * L))(*[v for fm in fm_sizes for v in (fm.h, fm.w)])
    c_img = (ctypes.c_int * (2 * L))(*[int(v) for s in img_size_pyramid for v in (s.w, s.h)])
    c_rows = (ctypes.c_int * L)(*rows)
    c_counts, c_kinds, c_args = ops_tables(chains, MAX_BOX_OPS)
    arrays = {k: (ctypes.c_void_p * L)(*v) if v else None for k, v in ptrs.items()}
    nbytes = int(tl.os2d_train_mine_select_workspace_bytes(A, B, L, c_hw))
    if nbytes == 0:
        raise ValueError("mine_select: unsupported shape A={} B={} levels={}".format(A, B, [(fm.h, fm.w) for fm in fm_sizes]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty(A, 3, dtype=torch.int32, device=dev), torch.empty(A, 3, K, INDEX_INTS, dtype=torch.int32, device=dev),
               torch.empty(A, 3, K, VALUE_FLOATS, dtype=torch.float32, device=dev))
    count, index, values = out
    g = box_grid_generator
    _train_lib.call("os2d_train_mine_select", A, B, L, c_hw, c_img, c_rows, int(g.box_stride.w), int(g.box_size.w), c_counts, c_kinds,
                    c_args, arrays["cls_loss"], arrays["loc_loss"], arrays["flags"], arrays["cls_preds"], arrays["corners"],
                    int(crop_size.w), int(crop_size.h), nms_iou_threshold, K, count, index, values, ws, ws.numel(), STREAM)
    return count, index, values


def records_from_host(count, index, values, out_size, class_ids, image_id, image=0):
    """The reference's list of OrderedDicts (train.py:328-361) from HOST copies of mine_select's outputs for one image."""
    data = []
    for r, role in enumerate(ROLES):
        for k in range(int(count[image, r])):
            level, label, anchor = [int(v) for v in index[image, r, k]]
            v = values[image, r, k]
            item = OrderedDict()
            item["pyramid_level"] = level
            item["label_local"] = label
            item["anchor_index"] = anchor
            item["role"] = role
            item["crop_position_xyxy"] = BoxList(v[0:4].clone().view(1, 4), out_size)
            item["anchor_position_xyxy"] = BoxList(v[4:8].clone().view(1, 4), out_size)
            item["transform_corners"] = v[8:16].clone()
            item["label_global"] = class_ids[label]
            item["loss"] = float(v[16])
            item["loss_loc"] = float(v[17])
            item["score"] = float(v[18])
            item["image_id"] = image_id
            data.append(item)
    return data


@torch.no_grad()
def mine_hard_patches_for_image(net, criterion, box_coder, image_levels, class_head, class_ids, gt_boxes, orig_size, crop_size,
                                image_id=None, nms_iou_threshold=0.5, num_hard_patches=10, scores=None, box_transforms=None):
    """Mining for ONE image (the body of the reference's loop, train.py:176-363).

    image_levels   the image resized to every pyramid level, [1,3,h_l,w_l] tensors on the HIP device
    class_head     the class batch as ``net.os2d_head_creator.create_os2d_head`` returns it; class_ids its global ids
    gt_boxes       BoxList in the original image (``orig_size``) with the LOCAL labels of ``class_ids`` and "difficult"
    scores         None: the levels are scored here with ``extract_scores``; else (loc_pyramid, cls_pyramid, corners_pyramid,
                   fm_sizes) with loc [B,4,HW_l], cls [B,HW_l], corners [B,8,HW_l] per level - ``net`` may then be None
    box_transforms per level the map from the level to the original image; None = ``resize(orig_size)``
    -> (hardnegdata, losses): the reference's list of OrderedDicts in the order neg, pos, pos_loc, each by decreasing score, and
    the scalar losses as floats.  The one copy that brings both to the host is the only synchronisation."""
    L = len(image_levels)
    img_size_pyramid = [s if isinstance(s, FeatureMapSize) else FeatureMapSize(img=s) for s in image_levels]
    if scores is None:
        from .evaluate import extract_scores
        s = extract_scores(net, image_levels, class_head)
        locs, clss, corners, fm_sizes = [t[0] for t in s["loc"]], [t[0] for t in s["cls"]], [t[0] for t in s["corners"]], s["fm_sizes"]
    else:
        locs, clss, corners, fm_sizes = scores
    if box_transforms is None:
        box_transforms = [((1, float(orig_size.w) / s.w, float(orig_size.h) / s.h),) for s in img_size_pyramid]
    B = len(class_ids)
    dev = clss[0].device
    loc_t, cls_t = box_coder.encode_pyramid_transformed(gt_boxes, img_size_pyramid, B, box_transforms, device=dev)
    loc_b = [t.reshape(B, 4, -1).unsqueeze(0) for t in locs]
    cls_b = [t.reshape(B, -1).unsqueeze(0) for t in clss]
    remapped = [box_coder.remap_anchor_targets_transformed(loc, [s], None, [gt_boxes], box_reverse_transform=[t])[0]
                for loc, s, t in zip(loc_b, img_size_pyramid, box_transforms)]
    keep_cpu, criterion.keep_class_loss_on_cpu = criterion.keep_class_loss_on_cpu, False
    try:
        losses, per_anchor = criterion(loc_b, [t.unsqueeze(0) for t in loc_t], cls_b, [t.unsqueeze(0) for t in cls_t],
                                       cls_targets_remapped=remapped, patch_mining_mode=True)
    finally:
        criterion.keep_class_loss_on_cpu = keep_cpu
    K = int(num_hard_patches)
    names = [k for k in losses]
    # one device blob = one copy: [counts 3 | index 3*K*3] as int32, then [values 3*K*19 | scalar losses] as float32
    n_int, n_val = 3 + 3 * K * INDEX_INTS, 3 * K * VALUE_FLOATS
    blob = torch.empty(n_int + n_val + len(names), dtype=torch.int32, device=dev)
    out = (blob[:3].view(1, 3), blob[3:n_int].view(1, 3, K, INDEX_INTS), blob[n_int:n_int + n_val].view(torch.float32).view(1, 3, K, VALUE_FLOATS))
    mine_select(per_anchor, cls_b, [c.reshape(1, B, 8, -1) for c in corners] if corners is not None else None, img_size_pyramid, fm_sizes,
                box_transforms, crop_size, nms_iou_threshold, K, box_grid_generator=box_coder.output_box_grid_generator, out=out)
    blob[n_int + n_val:].view(torch.float32).copy_(torch.stack([losses[k].detach().float().reshape(()) for k in names]))
    host = blob.cpu()                                           # the one synchronisation
    count, index = host[:3].view(1, 3), host[3:n_int].view(1, 3, K, INDEX_INTS)
    values = host[n_int:n_int + n_val].view(torch.float32).view(1, 3, K, VALUE_FLOATS)
    scalars = host[n_int + n_val:].view(torch.float32)
    data = records_from_host(count, index, values, orig_size, list(class_ids), image_id)
    return data, OrderedDict((k, float(v)) for k, v in zip(names, scalars))


def mine_hard_patches(net, criterion, box_coder, items, nms_iou_threshold=0.5, num_hard_patches=10):
    """reference train.py:142-370 over an iterable of per-image inputs: dictionaries with the keyword arguments of
    ``mine_hard_patches_for_image`` ("image_levels", "class_head", "class_ids", "gt_boxes", "orig_size", "crop_size",
    "image_id", optionally "scores" / "box_transforms").  -> (hardnegdata_per_imageid OrderedDict, list of the images' losses)."""
    if net is not None:
        net.eval()
    per_image, all_losses = OrderedDict(), []
    for item in items:
        data, losses = mine_hard_patches_for_image(net, criterion, box_coder, nms_iou_threshold=nms_iou_threshold,
                                                   num_hard_patches=num_hard_patches, **item)
        per_image[item.get("image_id")] = data
        all_losses.append(losses)
    return per_image, all_losses
