"""Plain-torch restatement of hard-patch mining: the crop placement of the reference's get_box_to_cut_anchor
(os2d/modeling/box_coder.py:78-166) and the selection as K rounds of "take the best candidate still alive, kill what overlaps
it" - what greedy NMS + sort + take K amounts to.  Runs on any device; the oracle of the kernels beyond the fixtures' sizes.
Test infrastructure only."""
import torch

BRANCHES = ("floor", "zero", "shift", "full")      # "move right / down" cannot occur: the corner is never negative after the first step


def apply_ops(boxes, ops):
    x1, y1, x2, y2 = boxes.unbind(1)
    for kind, ax, ay in ops:
        if kind == 1:
            x1, y1, x2, y2 = x1 * ax, y1 * ay, x2 * ax, y2 * ay
        elif kind == 2:
            x1, x2 = ax - x2, ax - x1
        elif kind == 3:
            y1, y2 = ay - y2, ay - y1
        else:
            x1, y1, x2, y2 = x1 - ax, y1 - ay, x2 - ax, y2 - ay
    return torch.stack([x1, y1, x2, y2], dim=1)


def crop_axis(c, crop, img, stride):
    """centres c [n] float32 -> (lo, hi, branch sets): the reference's expressions with torch.where for its masked writes."""
    raw = c - crop / 2
    floored = (torch.floor(raw) // stride) * stride
    lo = torch.where(raw > 0, floored, torch.zeros_like(raw))
    hi = lo + crop
    neg = lo < 0
    hi = torch.where(neg, hi - lo, hi)
    lo = torch.where(neg, torch.zeros_like(lo), lo)
    over = hi > img
    shift = torch.floor(torch.ceil(torch.floor(hi - img) / stride)) * stride
    fit = (lo - shift) >= 0
    lo2 = torch.where(over & fit, lo - shift, lo)
    hi2 = torch.where(over & fit, hi - shift, hi)
    lo2 = torch.where(over & ~fit, torch.zeros_like(lo), lo2)
    hi2 = torch.where(over & ~fit, torch.full_like(hi, float(crop)), hi2)
    hit = set()
    for name, m in (("floor", (raw > 0) & ~over), ("zero", ~(raw > 0) & ~over), ("shift", over & fit), ("full", over & ~fit)):
        if bool(m.any()):
            hit.add(name)
    return lo2, hi2, hit


def crop_boxes(H, W, stride, box_size, img_w, img_h, crop_w, crop_h, ops=(), device="cpu"):
    """-> (crops [HW,4], anchors [HW,4], branches hit on either axis)."""
    idx = torch.arange(H * W, device=device)
    cx = ((idx % W).float() + 0.5) * stride
    cy = ((idx // W).float() + 0.5) * stride
    left, right, hx = crop_axis(cx, crop_w, img_w, stride)
    top, bottom, hy = crop_axis(cy, crop_h, img_h, stride)
    half = box_size / 2
    anchors = torch.stack([cx - half, cy - half, cx + half, cy + half], 1)
    return apply_ops(torch.stack([left, top, right, bottom], 1), ops), apply_ops(anchors, ops), hx | hy


def select(scores, mask, crops, iou_thr, K):
    """scores [N], mask [N] bool, crops [N,4] -> flat indices of the first K survivors of greedy NMS in order of decreasing score;
    equal scores in increasing index; non-finite scores never."""
    alive = mask & torch.isfinite(scores)
    area = (crops[:, 2] - crops[:, 0]) * (crops[:, 3] - crops[:, 1])
    kept = []
    for _ in range(K):
        if not bool(alive.any()):
            break
        s = torch.where(alive, scores, torch.full_like(scores, float("-inf")))
        i = int(torch.nonzero((s == s.max()) & alive)[0])
        kept.append(i)
        b = crops[i]
        w = (torch.min(crops[:, 2], b[2]) - torch.max(crops[:, 0], b[0])).clamp(min=0)
        h = (torch.min(crops[:, 3], b[3]) - torch.max(crops[:, 1], b[1])).clamp(min=0)
        inter = w * h
        iou = inter / (area[i] + area - inter)
        alive = alive & ~(iou > iou_thr)
        alive[i] = False
    return kept


def mine(cls_loss, loc_loss, flags, levels, stride, box_size, img_sizes, crop, chains, iou_thr, K, image=0):
    """cls_loss / loc_loss / flags: per level [A,B,HW_l] tensors; levels [(H, W)]; img_sizes [(w, h)]; crop (w, h).
    -> per role (neg, pos, pos_loc) a list of (level, label, anchor, crop box [4], anchor box [4])."""
    dev = cls_loss[0].device
    B = cls_loss[0].shape[1]
    tables = [crop_boxes(H, W, stride, box_size, iw, ih, crop[0], crop[1], ops, dev)[:2]
              for (H, W), (iw, ih), ops in zip(levels, img_sizes, chains)]
    crops = torch.cat([t[0].unsqueeze(0).expand(B, -1, 4).reshape(-1, 4) for t in tables])
    anchors = torch.cat([t[1].unsqueeze(0).expand(B, -1, 4).reshape(-1, 4) for t in tables])
    where = [(l, b, p) for l, (H, W) in enumerate(levels) for b in range(B) for p in range(H * W)] if crops.shape[0] < 50000 else None
    offsets = [0]
    for H, W in levels:
        offsets.append(offsets[-1] + B * H * W)
    out = []
    for bit, src in ((2, cls_loss), (1, cls_loss), (4, loc_loss)):
        scores = torch.cat([t[image].reshape(-1) for t in src]).float()
        mask = torch.cat([(t[image].reshape(-1) & bit) != 0 for t in flags])
        recs = []
        for i in select(scores, mask, crops, iou_thr, K):
            if where is not None:
                l, b, p = where[i]
            else:
                l = max(k for k in range(len(levels)) if offsets[k] <= i)
                hw = levels[l][0] * levels[l][1]
                b, p = (i - offsets[l]) // hw, (i - offsets[l]) % hw
            recs.append((l, b, p, crops[i].clone(), anchors[i].clone()))
        out.append(recs)
    return out
