"""Models and case tables for the stage tests of os2d_amd/csrc_train/objective.hip (tests/test_objective_stages_gpu.py), test
infrastructure only, as tests/forward_matrix_model.py is for the forward matrix kernels.

Two evaluations of ONE set of formulas:

  * float64: the judge of every VALUE (loc_targets, both IoUs, the five scalars, cls_loss, loc_loss, coef, the gradients).  Inputs
    are the fp32 inputs cast up; scalar arguments enter as the fp32 values the ABI receives (``f32``: margin_pos = 0.6 is not 0.6).
  * float32: the judge of every DECISION.  The IoU against its thresholds, the first maximum, the contrastive per-element loss
    (0.5 * max(x - m, 0))^2, the mining cut and the smooth-L1 branch are made in fp32 by the kernels; the unit is built with
    -ffp-contract=off, so each is a chain of single IEEE operations that CPU torch reproduces bit for bit.  This evaluation gives
    the expected integer outputs, the flags and the zero pattern of the gradients, and the contrastive cls_loss / coef bits.

The objective is tests/objective_model.py's ``objective`` called with double or float tensors - its formulas are not restated
here; ``objective_outputs`` only adds what the kernels return besides (flags, coef, gradients by autograd).  Target assignment is
written once, generic in the dtype (objective_model's ``encode_image`` keeps its running maximum in a float32 buffer), with the
box-op chain applied as ``os2d_apply_box_ops`` documents: op by op, one rounding per product / difference.

Case tables: the smallest shapes that still reach each path (OBJ_THREADS = 256: HW = 257 is two work-groups per row).  The
conditions the cases must meet are asserted on the models alone in tests/test_objective_stage_model.py."""
import functools
import math

import numpy as np
import torch

import objective_model as M

F32, F64 = torch.float32, torch.float64
OBJ_THREADS = 256
F_POS, F_NEG, F_POSREG, F_CAND, F_HINGE = 1, 2, 4, 8, 16
SCALARS = ("loss", "loc", "cls", "cls_pos", "cls_neg")
REL_MARGIN = 1e-3                       # no value that is not a deliberate boundary case is this close (relative) to a threshold
RLL_LIVE, RLL_WEIGHT_CUT = 1e-5, 1e-8   # the RLL cuts: per-label maximum, weight / normalisation


def f32(v):
    """The fp32 value a C float argument receives."""
    return float(np.float32(v))


def next_up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def next_down(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t


XFORM_CLIP = f32(math.log(1000.0 / 16))         # the kernel's constant 4.135166556742356f
CLIP_SCORE = f32(5.0 * math.log(1000.0 / 16))   # loc_scores[2:] / 5 reaches the clamp about here


# ------------------------------------------------------------------------------------------------------ target assignment
def apply_ops(b, ops):
    """The chain (kind, ax, ay) of include/os2d_hip.h's OS2D_BOX_OP_* on [...,4] xyxy boxes, in the dtype of ``b``."""
    x1, y1, x2, y2 = b.unbind(-1)
    for kind, ax, ay in ops:
        ax, ay = torch.tensor(f32(ax), dtype=b.dtype), torch.tensor(f32(ay), dtype=b.dtype)
        if kind == 1:
            x1, y1, x2, y2 = x1 * ax, y1 * ay, x2 * ax, y2 * ay
        elif kind == 2:
            x1, x2 = ax - x2, ax - x1
        elif kind == 3:
            y1, y2 = ay - y2, ay - y1
        elif kind == 4:
            x1, y1, x2, y2 = x1 - ax, y1 - ay, x2 - ax, y2 - ay
        else:
            raise ValueError(kind)
    return torch.stack([x1, y1, x2, y2], -1)


def plain_anchors(case, dtype):
    H, W = case["H"], case["W"]
    stride, box = torch.tensor(float(case["stride"]), dtype=dtype), torch.tensor(float(case["rec_field"] + 14 * case["stride"]), dtype=dtype)
    p = torch.arange(H * W)
    cx, cy = ((p % W).to(dtype) + 0.5) * stride, ((p // W).to(dtype) + 0.5) * stride
    half = 0.5 * box
    return torch.stack([cx - half, cy - half, cx + half, cy + half], -1)


def decode(loc, anc, clip):
    """objective_model.decode for one label (loc [4,HW]) with the clamp constant as the fp32 value the kernel holds."""
    w, h = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    cx, cy = anc[:, 0] + 0.5 * w, anc[:, 1] + 0.5 * h
    pcx, pcy = loc[0] / 10.0 * w + cx, loc[1] / 10.0 * h + cy
    pw, ph = torch.exp(torch.minimum(loc[2] / 5.0, clip)) * w, torch.exp(torch.minimum(loc[3] / 5.0, clip)) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)


def _first_maximum(boxes, det):
    best = torch.full(det.shape[:1], -1.0, dtype=det.dtype)
    index = torch.full(det.shape[:1], -1, dtype=torch.long)
    for j in range(boxes.shape[0]):
        iou = M.iou_one_to_many(boxes[j], det)
        better = (iou > best) | (index < 0)
        best, index = torch.where(better, iou, best), torch.where(better, torch.full_like(index, j), index)
    return best, index


def assign(case, mode, dtype):
    """-> dict: cls [A,B,HW] int64; mode 0: loc [A,B,4,HW]; mode 1: ia, ic [A,B,HW] (the outputs the other mode leaves alone are
    absent).  ``has`` [A,B] marks the (image, label) pairs with a box."""
    A, B, HW = case["A"], case["B"], case["H"] * case["W"]
    T = lambda v: torch.tensor(f32(v), dtype=dtype)   # noqa: E731
    high, low, ops = T(case["high"]), T(case["low"]), case["ops"] or ()
    plain = plain_anchors(case, dtype)
    anc = apply_ops(plain, ops)
    out = dict(cls=torch.zeros(A, B, HW, dtype=torch.long), has=torch.zeros(A, B, dtype=torch.bool))
    if mode == 0:
        out["loc"] = torch.zeros(A, B, 4, HW, dtype=dtype)
    else:
        out["ia"], out["ic"] = torch.zeros(A, B, HW, dtype=dtype), torch.zeros(A, B, HW, dtype=dtype)
    for a, (boxes, labels, difficult) in enumerate(case["gt"]):
        boxes = boxes.to(dtype)
        for b in range(B):
            js = [j for j in range(boxes.shape[0]) if int(labels[j]) == b]
            if not js:
                continue
            out["has"][a, b] = True
            mine, hard = boxes[js], difficult[js].bool()
            best_a, index_a = _first_maximum(mine, anc)
            if mode == 1:
                det = apply_ops(decode(case["loc_scores"][a, b].to(dtype), plain, T(XFORM_CLIP)), ops)
                best, index = _first_maximum(mine, det)
                out["ia"][a, b], out["ic"][a, b] = best_a, best
            else:
                best, index = best_a, index_a
            neg = best < low                                           # torchvision's Matcher, then the difficult flag
            matched = ~neg & ~(best < high) & ~hard[index]
            out["cls"][a, b] = torch.where(neg, 0, torch.where(matched, 1, -1))
            if mode == 1:
                continue
            g = mine[torch.where(matched, index, torch.zeros_like(index))]   # unmatched: the label's first box
            gx1, gy1 = g[:, 0], g[:, 1]
            gx2, gy2 = torch.where(gx1 + 1 > g[:, 2], gx1 + 1, g[:, 2]), torch.where(gy1 + 1 > g[:, 3], gy1 + 1, g[:, 3])
            px1, py1 = anc[:, 0], anc[:, 1]
            px2, py2 = torch.where(px1 + 1 > anc[:, 2], px1 + 1, anc[:, 2]), torch.where(py1 + 1 > anc[:, 3], py1 + 1, anc[:, 3])
            ew, eh, gw, gh = px2 - px1, py2 - py1, gx2 - gx1, gy2 - gy1
            ecx, ecy, gcx, gcy = px1 + 0.5 * ew, py1 + 0.5 * eh, gx1 + 0.5 * gw, gy1 + 0.5 * gh
            out["loc"][a, b] = torch.stack([10.0 * (gcx - ecx) / ew, 10.0 * (gcy - ecy) / eh, 5.0 * torch.log(gw / ew), 5.0 * torch.log(gh / eh)])
    return out


_ASSIGNED = {}


def assigned(case, mode, dtype):
    """``assign`` of a case of the tables below, computed once."""
    key = (id(case), mode, dtype)
    if key not in _ASSIGNED:
        _ASSIGNED[key] = (assign(case, mode, dtype), case)
    return _ASSIGNED[key][0]


def _gt(rows):
    """rows: [(box, label, difficult)] -> (boxes [n,4] float32, labels [n] int32, difficult [n] uint8)."""
    return (torch.tensor([r[0] for r in rows], dtype=F32).reshape(-1, 4), torch.tensor([r[1] for r in rows], dtype=torch.int32),
            torch.tensor([r[2] for r in rows], dtype=torch.uint8))


def ground_truth(H, W, stride, rec_field, boundary=True):
    """Three images, four labels, every coordinate a small integer or a multiple of 1/4 (exact in fp32, so the encode-mode IoUs
    are quotients of exactly computed integers):

      image 0   label 0: anchor 0 shifted left by a third of its width - IoU with anchor 0 = (2/3) / (4/3) = 0.5 EXACTLY = iou_high
                label 1: two identical boxes on the middle anchor, only the SECOND difficult: the first maximum decides
                label 2: the last anchor as a difficult box (matched, then ignored); this label has a box in this image only
                label 3: a box half a pixel wide (clip_to_min_size)
      image 1   no box (equal offsets)
      image 2   label 0: a box far outside the image; label 1: anchor 0 shifted left by three fifths of its width - IoU with anchor
                0 = (2/5) / (8/5) = 0.25 EXACTLY = iou_low; label 3: a box in general position
    ``boundary`` False (the box-op cases, where the transformed coordinates round): the shifts are 1/4 and 2/3 of the width, IoU
    0.6 and 0.2, away from both thresholds.  (Both thresholds are exact in fp32 AND as real numbers, so the float64 evaluation
    decides these elements as the fp32 one does; with iou_low = fp32(0.2) it could not.)"""
    box, HW = rec_field + 14 * stride, H * W
    assert box % 60 == 0

    def anc(p):
        cx, cy = (p % W + 0.5) * stride, (p // W + 0.5) * stride
        return [cx - box / 2, cy - box / 2, cx + box / 2, cy + box / 2]

    def sh(b, dx, dy=0.0):
        return [b[0] + dx, b[1] + dy, b[2] + dx, b[3] + dy]
    mid, last = HW // 2, HW - 1
    mcx, mcy = (mid % W + 0.5) * stride, (mid // W + 0.5) * stride
    s_high, s_low = (box // 3, 3 * box // 5) if boundary else (box // 4, 2 * box // 3)
    img0 = [(sh(anc(0), -s_high), 0, 0), (anc(mid), 1, 0), (anc(mid), 1, 1), (anc(last), 2, 1), ([mcx, mcy - 20, mcx + 0.5, mcy + 20], 3, 0)]
    img2 = [([1e5, 1e5, 1e5 + 100, 1e5 + 50], 0, 0), (sh(anc(0), -s_low), 1, 0), ([mcx - 50.5, mcy - 30.25, mcx + 61.75, mcy + 44.5], 3, 0)]
    return [_gt(img0), _gt([]), _gt(img2)]


GRIDS = [(1, 1), (15, 17), (16, 16), (1, 257)]          # HW = 1, 255, 256, 257
OPS_ALONE = [(1, 1.25, 0.75), (2, 272.0, 0.0), (3, 0.0, 240.0), (4, 24.0, -40.0)]
OPS_CHAIN = [(1, 1.25, 0.75), (2, 340.0, 0.0), (4, 24.0, -40.0), (3, 0.0, 180.0), (1, 0.5, 2.0), (4, -8.0, 16.0)]
HIGH0, LOW0 = 0.5, 0.25                                 # encode thresholds: the exact IoUs of ground_truth
HIGH1, LOW1 = 0.6, 0.3                                  # remap thresholds
SPECIAL_ROWS = [(0, 1), (0, 0), (0, 3), (2, 1)]         # (image, label) pairs with a box that take the mode-1 specials


def _assign_case(name, H, W, gt, B, stride=16, rec_field=16, high=HIGH0, low=LOW0, ops=None, boundary=None):
    return dict(name=name, A=len(gt), B=B, H=H, W=W, stride=stride, rec_field=rec_field, high=high, low=low, ops=ops, gt=gt,
                boundary=boundary, loc_scores=None, special=None)


def _transformed(gt, ops):
    """Ground truth of the box-op cases: the boxes go through the chain as the anchors do, so the overlaps keep their pattern."""
    return [(apply_ops(b, ops) if b.shape[0] else b, l, d) for b, l, d in gt]


@functools.lru_cache(maxsize=None)
def encode_cases():
    """Mode 0.  ``boundary``: (image, label, anchor, threshold name) of the elements whose IoU sits exactly on a threshold."""
    out = []
    for H, W in GRIDS:
        gid = "{}x{}".format(H, W)
        gt = ground_truth(H, W, 16, 16)
        at = [(0, 0, 0, "high"), (2, 1, 0, "low")]
        out.append(_assign_case(gid + " at", H, W, gt, 4, boundary=at))
        out.append(_assign_case(gid + " below", H, W, gt, 4, high=next_up(HIGH0), low=next_up(LOW0), boundary=at))
    out.append(_assign_case("16x16 B=1", 16, 16, [_gt([([33.5, 20.25, 240.0, 251.75], 0, 0)])], 1))
    out.append(_assign_case("15x17 no boxes", 15, 17, [_gt([]), _gt([]), _gt([])], 4))
    out.append(_assign_case("15x17 stride 8 rec_field 8", 15, 17, ground_truth(15, 17, 8, 8), 4, stride=8, rec_field=8,
                            boundary=[(0, 0, 0, "high"), (2, 1, 0, "low")]))
    return out


@functools.lru_cache(maxsize=None)
def ops_cases():
    """Both modes through os2d_train_assign_targets_ops at 15x17: every op kind alone, the 6-op chain with both flips, and
    nops = 0 (which must equal the plain entry point bit for bit)."""
    gt = ground_truth(15, 17, 16, 16, boundary=False)
    chains = [("nops=0", [])] + [("op kind {}".format(o[0]), [o]) for o in OPS_ALONE] + [("6-op chain", OPS_CHAIN)]
    return [_assign_case("15x17 " + n, 15, 17, _transformed(gt, ops), 4, ops=ops) for n, ops in chains]


def _remap_margin(case):
    """Smallest relative distance of a corrected IoU to a remap threshold, and of loc_scores[2:] / 5 to the clamp (the deliberate
    clamp entries excluded), over the (image, label) pairs with a box; and where the closest IoUs are."""
    m = assign(case, 1, F32)
    has = m["has"][:, :, None].expand_as(m["ic"])
    dist = torch.minimum((m["ic"] - f32(case["high"])).abs() / case["high"], (m["ic"] - f32(case["low"])).abs() / case["low"])
    dist = torch.where(has, dist, torch.ones_like(dist))
    clamp = ((case["loc_scores"][:, :, 2:] / 5.0 - XFORM_CLIP).abs() / XFORM_CLIP)[~case["special"][:, :, 2:]]
    return float(dist.min()), float(clamp.min()), dist


def with_loc_scores(case, seed):
    """The case with mode-1 inputs: loc_scores ~ N(0, 1.5), the four special entries (below), and every anchor whose corrected IoU
    came within REL_MARGIN of a threshold redrawn - the decision there would hang on the device's expf."""
    case = dict(case, high=HIGH1, low=LOW1, boundary=None)
    A, B, HW = case["A"], case["B"], case["H"] * case["W"]
    g = torch.Generator().manual_seed(seed)
    loc = torch.randn(A, B, 4, HW, generator=g) * 1.5
    special = torch.zeros(A, B, 4, HW, dtype=torch.bool)
    values = [(next_up(CLIP_SCORE), next_down(CLIP_SCORE)),    # one fp32 step either side of 5 log(1000/16)
              (1e4, -1e4), (-1e4, 1e4),                        # far beyond the clamp / an exp that underflows
              (-600.0, -600.0)]                                # expf(-120) = 0: a decoded box of zero area
    rows = [r for r in SPECIAL_ROWS if r[0] < A and r[1] < B and any(int(l) == r[1] for l in case["gt"][r[0]][1])]
    for s, (v2, v3) in enumerate(values if rows else []):
        a, b = rows[s % len(rows)]
        p = min(s // len(rows), HW - 1)
        loc[a, b, 2, p], loc[a, b, 3, p] = v2, v3
        special[a, b, 2:, p] = True
    case["loc_scores"], case["special"] = loc, special
    for _ in range(50):
        iou_margin, _, dist = _remap_margin(case)
        if iou_margin > REL_MARGIN:
            return case
        for a, b, p in (dist <= REL_MARGIN).nonzero().tolist():
            loc[a, b, :2, p] = torch.randn(2, generator=g) * 1.5
    raise AssertionError("no margin: " + case["name"])


@functools.lru_cache(maxsize=None)
def remap_cases():
    out = []
    for i, (H, W) in enumerate(GRIDS):
        out.append(with_loc_scores(_assign_case("{}x{}".format(H, W), H, W, ground_truth(H, W, 16, 16), 4), 100 + i))
    out.append(with_loc_scores(_assign_case("16x16 B=1", 16, 16, [_gt([([33.5, 20.25, 240.0, 251.75], 0, 0)])], 1), 110))
    out.append(with_loc_scores(_assign_case("15x17 no boxes", 15, 17, [_gt([]), _gt([]), _gt([])], 4), 111))
    out.append(with_loc_scores(_assign_case("15x17 stride 8 rec_field 8", 15, 17, ground_truth(15, 17, 8, 8), 4, stride=8, rec_field=8), 112))
    return out


@functools.lru_cache(maxsize=None)
def remap_ops_cases():
    return [with_loc_scores(c, 120 + i) for i, c in enumerate(ops_cases())]


def one_image(case, a):
    """Image ``a`` of a case as a case of its own (a batch must equal the per-image calls bit for bit)."""
    sub = dict(case, A=1, gt=[case["gt"][a]])
    if case["loc_scores"] is not None:
        sub["loc_scores"], sub["special"] = case["loc_scores"][a:a + 1].contiguous(), case["special"][a:a + 1]
    return sub


# ------------------------------------------------------------------------------------------------------ objective
OBJ_SHAPES = [(1, 1, 1), (2, 3, 255), (2, 3, 256), (2, 3, 257), (3, 100, 1), (1, 257, 3), (1, 300, 5)]
CRITERION = dict(margin=0.5, margin_pos=0.6, class_loss_neg_weight=0.7, localization_weight=0.2)
MARGIN, MARGIN_POS = f32(CRITERION["margin"]), f32(CRITERION["margin_pos"])
PLATEAU_SCORE, ABOVE_SCORES, BELOW_SCORE = 0.8125, (0.95, 0.96875, 1.0), 0.78


def shape_id(shape):
    return "A{}_B{}_HW{}".format(*shape)


def _effective(inp):
    return inp["cls_targets"] if inp["cls_targets_remapped"] is None else inp["cls_targets_remapped"]


def _neg_scores(inp):
    return inp["cls_preds"] if inp["cls_preds_for_neg"] is None else inp["cls_preds_for_neg"]


def masks(inp):
    """(pos, cand, pos_reg) [A,B,HW] of the inputs: what the targets alone decide."""
    eff = _effective(inp)
    pos = eff > 0
    return pos, ~(pos | (eff == -1)), inp["cls_targets"] > 0


def base_inputs(shape, remap, seed):
    """Random inputs with the fixed elements every scenario keeps (flat index over [A,B,HW]; N = 1 holds one of them only):

      0   class and regression positive with cls_preds == margin_pos EXACTLY (the hinge's kink); its four loc differences are
          1, 1 + ulp, 1 - ulp, -1 (the smooth-L1 branch and the clamp of the backward)
      1   candidate with its score == margin EXACTLY
      2   candidate; with ``remap`` a regression positive that the remapped target turned into a class negative
      3   regression positive with differences -(1 + ulp), -(1 - ulp)
      the last (image, label) row: all -1 (ignored) in the targets the class loss uses."""
    A, B, HW = shape
    N = A * B * HW
    rs = np.random.RandomState(seed)
    t = lambda a, dt=F32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)   # noqa: E731
    inp = dict(cls_targets=t(rs.choice([1, 0, -1], size=shape, p=[0.15, 0.7, 0.15]), torch.long),
               cls_targets_remapped=t(rs.choice([1, 0, -1], size=shape, p=[0.15, 0.7, 0.15]), torch.long) if remap else None,
               loc_targets=t(rs.randn(A, B, 4, HW)), loc_preds=t(rs.randn(A, B, 4, HW) * 1.5),
               cls_preds=t(rs.rand(*shape) * 1.4 - 0.4),
               cls_preds_for_neg=t(rs.rand(*shape) * 1.4 - 0.6) if remap else None)
    cls_t, eff, x, xn = inp["cls_targets"].view(-1), _effective(inp).view(-1), inp["cls_preds"].view(-1), _neg_scores(inp).view(-1)
    loc, loc_t = inp["loc_preds"].view(A * B, 4, HW), inp["loc_targets"].view(A * B, 4, HW)

    def diffs(i, values):
        for c, v in enumerate(values):
            loc_t[i // HW, c, i % HW], loc[i // HW, c, i % HW] = 0.0, v
    if N == 1:
        if remap:       # a regression positive that the remap turned into a candidate at the margin
            cls_t[0], eff[0], xn[0] = 1, 0, MARGIN
        else:
            cls_t[0], x[0] = 1, MARGIN_POS
        diffs(0, (1.0, next_up(1.0), next_down(1.0), -1.0))
        return inp
    _effective(inp)[A - 1, B - 1] = -1
    cls_t[0], eff[0], x[0] = 1, 1, MARGIN_POS
    eff[1], xn[1] = 0, MARGIN
    eff[2] = 0
    if remap:
        cls_t[2] = 1
    cls_t[3] = 1
    diffs(0, (1.0, next_up(1.0), next_down(1.0), -1.0))
    diffs(3, (-next_up(1.0), -next_down(1.0)))
    return inp


def _clone(inp):
    return {k: None if v is None else v.clone() for k, v in inp.items()}


def _params(loss, patch=False, ratio=3.0, rll_ratio=0.001):
    return dict(CRITERION, loss=loss, patch=patch, ratio=float(ratio), rll_ratio=rll_ratio)


def ratio_for(k, num_pos):
    """neg_to_pos_ratio with (fp32(ratio) * fp32(num_pos)).long() == k."""
    if k == 0:
        return 0.0
    r = f32((k + 0.5) / num_pos)
    assert int(np.float32(r) * np.float32(num_pos)) == k
    return r


def contrastive_loss_bits(x):
    """fp32 pattern of (0.5 * max(x - margin, 0))^2, as the kernel and objective_model compute it."""
    h = np.float32(0.5) * np.maximum(np.float32(x) - np.float32(MARGIN), np.float32(0))
    return int(np.float32(h * h).view(np.uint32))


def low_byte_pair():
    """Two candidate scores whose losses differ, and differ in the lowest byte of the fp32 pattern only: every radix pass but the
    last sees one prefix.  Found by stepping down from 0.9 one fp32 value at a time."""
    hi = np.float32(0.9)
    lo = hi
    while contrastive_loss_bits(lo) == contrastive_loss_bits(hi):
        lo = np.nextafter(lo, np.float32(0))
    assert contrastive_loss_bits(lo) >> 8 == contrastive_loss_bits(hi) >> 8
    return float(hi), float(lo)


def plateau_window(shape):
    """Flat indices [start, start + 18): across the (image, label) row boundary, and for HW = 257 across the 256-element boundary
    inside the row as well."""
    HW = shape[2]
    start = 250 if HW == 257 else (HW if HW >= 8 else 96) - 7
    return start, start + 18


def _order_candidates(inp, top, hold=()):
    """Scores of the candidates: ``top`` (index -> score) as given, three more above everything, all others at most BELOW_SCORE."""
    _, cand, _ = masks(inp)
    xn, free = _neg_scores(inp).view(-1), [i for i in cand.view(-1).nonzero().view(-1).tolist() if i not in top and i not in hold]
    above = free[len(free) // 2:][:3]
    for i in free:
        xn[i] = min(float(xn[i]), BELOW_SCORE)
    for i, v in zip(above, ABOVE_SCORES):
        xn[i] = v
    for i, v in top.items():
        xn[i] = v
    return above


def contrastive_scenarios(shape, remap):
    """[(name, inputs, params, facts)] of ContrastiveLoss: the mining counts k = 0, 1, total - 1, total, total + 1, a plateau of
    equal losses cut at krem = 1, plateau - 1 and plateau, the low-byte pair with the cut between the two, all losses 0 with the
    cut among them, and patch mode.  ``facts`` is what tests/test_objective_stage_model.py asserts of the scenario."""
    base = base_inputs(shape, remap, 11 + 2 * OBJ_SHAPES.index(shape) + remap)
    pos, cand, _ = masks(base)
    num_pos, total = int(pos.sum()), int(cand.sum())
    out = [("patch", base, _params("ContrastiveLoss", patch=True), {})]
    ks = [0] + ([k for k in (1, total - 1, total, total + 1) if k > 0] if num_pos else [])
    for k in sorted(set(ks)):
        out.append(("k={}".format(k), base, _params("ContrastiveLoss", ratio=ratio_for(k, num_pos)), dict(k=k, total=total)))
    if num_pos == 0 or total < 16:
        return out
    lo, hi = plateau_window(shape)
    inp = _clone(base)
    plateau = [i for i in range(lo, hi) if bool(masks(inp)[1].view(-1)[i])]
    above = _order_candidates(inp, {i: PLATEAU_SCORE for i in plateau})
    for krem in sorted({1, len(plateau) - 1, len(plateau)}):
        out.append(("plateau krem={}".format(krem), inp, _params("ContrastiveLoss", ratio=ratio_for(len(above) + krem, num_pos)),
                    dict(plateau=plateau, krem=krem, above=above)))
    inp = _clone(base)
    idx = masks(inp)[1].view(-1).nonzero().view(-1).tolist()
    x_hi, x_lo = low_byte_pair()
    pair = (idx[-1], idx[2])                       # the LARGER loss at the higher flat index: the index rule cannot pick it
    above = _order_candidates(inp, {pair[0]: x_hi, pair[1]: x_lo})
    out.append(("low byte", inp, _params("ContrastiveLoss", ratio=ratio_for(len(above) + 1, num_pos)), dict(pair=pair, above=above)))
    inp = _clone(base)
    xn = _neg_scores(inp).view(-1)
    for i in idx:
        xn[i] = min(float(xn[i]), 0.45)
    xn[1] = MARGIN
    out.append(("all zero", inp, _params("ContrastiveLoss", ratio=ratio_for(total // 2, num_pos)), dict(all_zero=True, k=total // 2)))
    return out


def rll_threshold_quantities(inp, par):
    """What the RLL cuts compare, in float64, for the margin checks only: per-label maxima of the half-margins (against 1e-5), the
    per-label normalisation and the final weights of the candidates with a positive half-margin (against 1e-8)."""
    pos, cand, _ = masks(inp)
    l = torch.where(cand, 0.5 * (_neg_scores(inp).double() - MARGIN).clamp(min=0), torch.zeros((), dtype=F64))
    max_l = l.amax(dim=(0, 2), keepdim=True)
    live = max_l > RLL_LIVE
    T = torch.where(live, f32(-math.log(par["rll_ratio"])) / max_l.clamp(min=1e-300), torch.zeros((), dtype=F64))
    w = torch.exp((l - max_l) * T) * ((l > 0) & live).double()
    norm = 1.0 / (w.sum(dim=(0, 2), keepdim=True) * max(int(live.sum()), 1))
    weights = (w * norm * max(int(pos.sum()), 1))[(l > 0) & live.expand_as(l)]
    return max_l.view(-1), norm.view(-1)[live.view(-1)], weights


def rll_margin(inp, par):
    """Smallest relative distance of any of the above to its cut."""
    max_l, norm, weights = rll_threshold_quantities(inp, par)
    d = [((max_l[max_l > 0] - RLL_LIVE).abs() / RLL_LIVE), ((norm - RLL_WEIGHT_CUT).abs() / RLL_WEIGHT_CUT),
         ((weights - RLL_WEIGHT_CUT).abs() / RLL_WEIGHT_CUT)]
    return min([float(x.min()) for x in d if x.numel()] + [1.0])


def rll_scenarios(shape, remap):
    """[(name, inputs, params, facts)] of RLL (neg_to_pos_ratio = inf, as Os2dObjective sets it):

      live      from B = 3: label 0 has its largest half-margin below 1e-5 (2e-6, one candidate) next to live labels, and with
                A >= 2 label 1 has candidates in image 0 only
      trivial   num_pos > 0 and every positive at or above margin_pos: no non-trivial positive, positive scale 0
      no pos    num_pos = 0: no negative is used either
      1e-12     rll_neg_weight_ratio = 1e-12: weights on both sides of the 1e-8 cut
      patch     patch mode: no normalisation; the kinks of BOTH hinges have a gradient
    The seed is the first whose scenario keeps every cut REL_MARGIN away (rll_margin)."""
    A, B, HW = shape

    def build(seed):
        inp = base_inputs(shape, remap, seed)
        if B >= 3:
            eff, xn = _effective(inp), _neg_scores(inp)
            if (A - 1) * B * HW + HW - 1 > 3:         # not one of the fixed elements: label 0 has a candidate for certain
                eff[A - 1, 0, HW - 1] = 0
            xn[:, 0] = torch.where(eff[:, 0] == 0, xn[:, 0].clamp(max=0.45), xn[:, 0])
            a, p = (eff[:, 0] == 0).nonzero()[-1].tolist()
            xn[a, 0, p] = MARGIN + 4e-6
            if A >= 2:
                eff[1:, 1][eff[1:, 1] == 0] = -1
            if HW > 1:
                xn.view(-1)[1] = MARGIN               # the kink candidate lives in label 0
        return inp

    def settle(name, make, par, facts):
        for seed in range(300, 340):
            inp = make(build(seed + 40 * OBJ_SHAPES.index(shape) + 20 * remap))
            if rll_margin(inp, par) > REL_MARGIN:
                return (name, inp, par, facts)
        raise AssertionError("no margin: " + name)

    def trivial(inp):
        pos = masks(inp)[0]
        inp["cls_preds"][pos] = inp["cls_preds"][pos].clamp(min=0.7)
        if pos.view(-1)[0]:
            inp["cls_preds"].view(-1)[0] = MARGIN_POS
        return inp

    def no_pos(inp):
        eff = _effective(inp)
        eff[eff > 0] = 0
        return inp
    inf = float("inf")
    out = [settle("live", lambda i: i, _params("RLL", ratio=inf), dict(dead_label=B >= 3, one_image_label=B >= 3 and A >= 2)),
           settle("patch", lambda i: i, _params("RLL", patch=True, ratio=inf), {}),
           settle("1e-12", lambda i: i, _params("RLL", ratio=inf, rll_ratio=1e-12), dict(both_sides=A * B * HW > 16))]
    if bool(masks(out[0][1])[0].any()):
        out.append(settle("trivial", trivial, _params("RLL", ratio=inf), dict(trivial=True)))
    out.append(settle("no pos", no_pos, _params("RLL", ratio=inf), dict(no_pos=True)))
    return out


@functools.lru_cache(maxsize=None)
def scenarios(shape, remap):
    return [("ContrastiveLoss " + s[0],) + s[1:] for s in contrastive_scenarios(shape, remap)] + \
           [("RLL " + s[0],) + s[1:] for s in rll_scenarios(shape, remap)]


_OUTPUTS = {}


def objective_outputs(inp, par, dtype, grad_loss=1.0):
    """objective_model.objective on the inputs cast to ``dtype`` plus what the kernels return besides: -> dict with the five
    scalars (python floats), cls_loss, loc_loss, flags (bits 1 | 2 | 4 | 8 | 16), coef = d cls_loss_i / d score_i (the RLL weights
    and counts as constants: autograd of the model, not a formula of its own) and dloc, dcls, dcls_for_neg = grad_loss * d loss.
    Without cls_preds_for_neg both class terms are in dcls and dcls_for_neg is None."""
    key = (id(inp), id(par), dtype, grad_loss)
    if key in _OUTPUTS:
        return _OUTPUTS[key][0]
    leaf = lambda v: None if v is None else v.to(dtype).clone().requires_grad_()   # noqa: E731
    loc, cls, det = leaf(inp["loc_preds"]), leaf(inp["cls_preds"]), leaf(inp["cls_preds_for_neg"])
    out = M.objective(par["loss"], loc, inp["loc_targets"].to(dtype), cls, inp["cls_targets"], inp["cls_targets_remapped"], det,
                      patch_mining_mode=par["patch"], margin=f32(par["margin"]), margin_pos=f32(par["margin_pos"]),
                      class_loss_neg_weight=f32(par["class_loss_neg_weight"]), localization_weight=f32(par["localization_weight"]),
                      neg_to_pos_ratio=f32(par["ratio"]), rll_neg_weight_ratio=math.exp(-f32(-math.log(par["rll_ratio"]))))
    wrt = [t for t in (loc, cls, det) if t is not None]
    zeros = lambda g, t: torch.zeros_like(t) if g is None else g   # noqa: E731
    coef = [zeros(g, t) for g, t in zip(torch.autograd.grad(out["cls_loss"].sum(), wrt[1:], retain_graph=True, allow_unused=True), wrt[1:])]
    grads = [zeros(g, t) for g, t in zip(torch.autograd.grad(out["loss"] * grad_loss, wrt, allow_unused=True), wrt)]
    pos, cand, pos_reg = masks(inp)
    x, xn = inp["cls_preds"], _neg_scores(inp)                              # the clamp arguments' signs, in fp32 as the kernel
    hinge = torch.where(pos, f32(par["margin_pos"]) - x >= 0, cand & (xn - f32(par["margin"]) >= 0))
    assert torch.equal(pos, out["pos"]) and torch.equal(pos_reg, out["pos_reg"])
    res = dict({k: float(out[k].detach()) for k in SCALARS}, cls_loss=out["cls_loss"].detach(), loc_loss=out["loc_loss"].detach(),
               flags=(pos * F_POS + out["neg"] * F_NEG + pos_reg * F_POSREG + cand * F_CAND + hinge * F_HINGE).to(torch.uint8),
               neg=out["neg"], coef=sum(coef), dloc=grads[0], dcls=grads[1], dcls_for_neg=grads[2] if det is not None else None)
    _OUTPUTS[key] = (res, inp, par)          # the inputs are kept alive with it: the ids stay unique
    return res


def rel_err(got, ref):
    """max |got - ref| / max |ref| (absolute when the reference is all zero): tests/objective_util.rel_err on tensors."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    return err / scale if scale > 0 else err


def scalar_err(got, ref):
    return abs(got - ref) / abs(ref) if ref != 0 else abs(got)
