"""Plain torch restatement of the target assignment and of the OS2D objective, test infrastructure only (as
tests/f16x3_model.py): what the kernels of os2d_amd/csrc_train/objective.hip have to compute, written from the formulas and
vectorised over anchors, with no BoxList, no Matcher object and no sort-of-a-sort.  It reproduces the fixtures recorded
from the reference (tests/test_objective_model.py) and is the comparator for shapes too large to store.  Runs on any
device; gradients come from autograd."""
import math

import torch

XFORM_CLIP = math.log(1000.0 / 16)


def anchors(H, W, stride, box_size, device="cpu"):
    """[HW,4] xyxy, row-major cells, centres ((x+0.5)*stride, (y+0.5)*stride)."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device),
                            torch.arange(W, dtype=torch.float32, device=device), indexing="ij")
    cx, cy = (xs.reshape(-1) + 0.5) * stride, (ys.reshape(-1) + 0.5) * stride
    half = 0.5 * box_size
    return torch.stack([cx - half, cy - half, cx + half, cy + half], 1)


def iou_one_to_many(g, b):
    """g [4] one box, b [...,4] -> IoU [...], fp32, inter / (area_g + area_b - inter)."""
    w = (torch.minimum(g[2], b[..., 2]) - torch.maximum(g[0], b[..., 0])).clamp(min=0)
    h = (torch.minimum(g[3], b[..., 3]) - torch.maximum(g[1], b[..., 1])).clamp(min=0)
    inter = w * h
    return inter / ((g[2] - g[0]) * (g[3] - g[1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter)


def decode(loc, anc):
    """loc [B,4,HW], anc [HW,4] -> boxes [B,HW,4]; weights (10,10,5,5), dw / dh clamped at log(1000/16)."""
    w, h = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    cx, cy = anc[:, 0] + 0.5 * w, anc[:, 1] + 0.5 * h
    pcx, pcy = loc[:, 0] / 10.0 * w + cx, loc[:, 1] / 10.0 * h + cy
    pw = torch.exp((loc[:, 2] / 5.0).clamp(max=XFORM_CLIP)) * w
    ph = torch.exp((loc[:, 3] / 5.0).clamp(max=XFORM_CLIP)) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 2)


def _best_box(det, boxes, labels, B):
    """det [B,HW,4] (or [HW,4], shared by the labels); -> best IoU [B,HW], index of the first best box [B,HW] (-1 = the
    label has no box), index of each label's first box [B]."""
    dev = boxes.device
    if det.dim() == 2:
        det = det.unsqueeze(0).expand(B, -1, -1)
    best = torch.full(det.shape[:2], -1.0, device=dev)
    index = torch.full(det.shape[:2], -1, dtype=torch.long, device=dev)
    first = torch.full((B,), -1, dtype=torch.long, device=dev)
    for j in range(boxes.shape[0]):
        lab = int(labels[j])
        iou = iou_one_to_many(boxes[j], det[lab])
        better = (iou > best[lab]) | (index[lab] < 0)
        best[lab] = torch.where(better, iou, best[lab])
        index[lab] = torch.where(better, torch.full_like(index[lab], j), index[lab])
        if first[lab] < 0:
            first[lab] = j
    return best, index, first


def _class_targets(best, index, difficult, high, low):
    """-> (class targets [B,HW] int64 in {1, 0, -1}, matched [B,HW] bool)."""
    has = index >= 0
    diff = torch.zeros_like(has)
    if difficult.numel():
        diff = difficult[index.clamp(min=0)] & has
    matched = has & (best >= high) & ~diff
    ignored = has & (best >= low) & ~matched
    return matched.long() - ignored.long(), matched


def encode_image(boxes, labels, difficult, B, H, W, stride, box_size, high, low):
    """One image: -> loc_targets [B,4,HW] float32, cls_targets [B,HW] int64."""
    anc = anchors(H, W, stride, box_size, boxes.device)
    best, index, first = _best_box(anc, boxes, labels, B)
    cls, matched = _class_targets(best, index, difficult, high, low)
    loc = torch.zeros(B, 4, H * W, device=boxes.device)
    if boxes.shape[0] == 0:
        return loc, cls
    use = torch.where(matched, index, first.view(B, 1).expand_as(index)).clamp(min=0)     # unmatched: the label's first box
    g = boxes[use]                                                                         # [B,HW,4]
    gx2 = torch.where(g[..., 0] + 1 > g[..., 2], g[..., 0] + 1, g[..., 2])                 # clip_to_min_size(1)
    gy2 = torch.where(g[..., 1] + 1 > g[..., 3], g[..., 1] + 1, g[..., 3])
    ew, eh = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    ecx, ecy = anc[:, 0] + 0.5 * ew, anc[:, 1] + 0.5 * eh
    gw, gh = gx2 - g[..., 0], gy2 - g[..., 1]
    gcx, gcy = g[..., 0] + 0.5 * gw, g[..., 1] + 0.5 * gh
    enc = torch.stack([10.0 * (gcx - ecx) / ew, 10.0 * (gcy - ecy) / eh, 5.0 * torch.log(gw / ew), 5.0 * torch.log(gh / eh)], 1)
    has = (first >= 0).view(B, 1, 1)
    return torch.where(has, enc, loc), cls


def remap_image(loc_scores, boxes, labels, difficult, B, H, W, stride, box_size, high, low):
    """One image, loc_scores [B,4,HW]: -> cls_targets_remapped [B,HW] int64, ious_anchor, ious_anchor_corrected [B,HW]."""
    anc = anchors(H, W, stride, box_size, loc_scores.device)
    best_a, index_a, _ = _best_box(anc, boxes, labels, B)
    best_d, index_d, _ = _best_box(decode(loc_scores, anc), boxes, labels, B)
    cls, _ = _class_targets(best_d, index_d, difficult, high, low)
    has = index_a >= 0
    zero = torch.zeros_like(best_a)
    return cls, torch.where(has, best_a, zero), torch.where(has, best_d, zero)


def objective(class_loss, loc_preds, loc_targets, cls_preds, cls_targets, cls_targets_remapped=None, cls_preds_for_neg=None,
              patch_mining_mode=False, margin=0.5, margin_pos=0.6, class_loss_neg_weight=1.0, localization_weight=0.2,
              neg_to_pos_ratio=3, rll_neg_weight_ratio=0.001, **_):
    """-> dict: loss, loc, cls, cls_pos, cls_neg (scalars, attached to the graph), cls_loss / loc_loss [A,B,HW], pos / neg /
    pos_reg masks.  RLL uses every negative (none when there is no positive); ContrastiveLoss keeps the
    k = neg_to_pos_ratio * num_pos largest candidate losses, equal ones by increasing flat index."""
    pos_reg = cls_targets > 0
    tgt = cls_targets if cls_targets_remapped is None else cls_targets_remapped
    pos = tgt > 0
    cand = ~(pos | (tgt == -1))
    num_pos, num_reg = pos.sum(), pos_reg.sum()
    np1, nr1 = num_pos.clamp(min=1).float(), num_reg.clamp(min=1).float()
    zero = torch.zeros((), device=cls_preds.device)

    d = (loc_preds - loc_targets).abs()
    loc_loss = torch.where(d < 1, 0.5 * d * d, d - 0.5).sum(2)
    loc_loss = torch.where(pos_reg, loc_loss, zero)

    score_neg = cls_preds if cls_preds_for_neg is None else cls_preds_for_neg
    lneg = torch.where(cand, 0.5 * (score_neg - margin).clamp(min=0), zero)
    lpos = torch.where(pos, 0.5 * (margin_pos - cls_preds).clamp(min=0), zero)
    if class_loss == "ContrastiveLoss":
        cls_loss = lneg * lneg + lpos * lpos
    else:
        if not patch_mining_mode:
            nontrivial = ((lpos > 0) & pos).sum().float()
            lpos = lpos * torch.where(nontrivial > 0, num_pos.float() / nontrivial.clamp(min=1), zero)
            l = lneg.detach()
            max_l = l.amax(dim=(0, 2), keepdim=True)                                    # per label
            live = max_l > 1e-5
            T = torch.where(live, float(-math.log(rll_neg_weight_ratio)) / max_l, zero)
            w = torch.exp((l - max_l) * T) * ((l > 0) & cand & live).float()
            norm = 1.0 / (w.sum(dim=(0, 2), keepdim=True) * live.sum())
            norm = torch.where((norm <= 1e-8) | ~live, zero, norm)
            w = w * norm * np1
            lneg = torch.where(w > 1e-8, lneg, zero) * w
        cls_loss = lneg + lpos

    if patch_mining_mode:
        neg = cand
    elif class_loss == "RLL":
        neg = cand & (num_pos > 0)
    else:
        k = (float(neg_to_pos_ratio) * num_pos.float()).long()
        key = torch.where(cand, cls_loss.detach(), torch.full_like(cls_loss, -1.0)).reshape(-1)
        order = torch.sort(key, descending=True, stable=True)[1]
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=order.device)
        neg = (rank.view(cand.shape) < k) & cand
    cls_pos = torch.where(pos, cls_loss, zero).sum() / np1
    cls_neg = torch.where(neg, cls_loss, zero).sum() / np1
    loc = loc_loss.sum() / nr1
    cls = cls_pos + cls_neg * class_loss_neg_weight
    return dict(loss=cls + loc * localization_weight, loc=loc, cls=cls, cls_pos=cls_pos, cls_neg=cls_neg,
                cls_loss=cls_loss, loc_loss=loc_loss, pos=pos, neg=neg, pos_reg=pos_reg)
