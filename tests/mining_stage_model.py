"""Loop model of hard-patch mining for the stage suite (tests/test_mining_stage_model.py on the CPU, tests/test_mining_stages_gpu.py
on the GPU): crop placement one anchor at a time in numpy.float32 scalars with the reference's expressions operation for operation
(os2d/modeling/box_coder.py:78-166, torch's floor_divide included), box-op chains with one rounding per operation, and the
selection as an explicit greedy loop over the candidates in flat (level, label, anchor) order.  Plain NumPy and Python: nothing of
os2d_amd, no torch, nothing of tests/mining_model.py - that is the point of it.  Test infrastructure only.

Besides the records the model reports what a case reached: the branch of the placement per axis and anchor, and for the
selection every (kept window, window tested against it) pair that the loop evaluated, with its float32 operands, its decision and
its float64 IoU - ``band_gap`` is the smallest |IoU - thr| over these pairs."""
import numpy as np

F32 = np.float32
BRANCHES = ("floor", "zero", "shift", "full")
ROLE_BITS = (2, 1, 4)                      # neg, pos, pos_loc: flag bits of the objective kernel
INDEX_INTS, VALUE_FLOATS = 3, 19
OP_SCALE, OP_HFLIP, OP_VFLIP, OP_SHIFT = 1, 2, 3, 4
_ZERO, _ONE, _HALF = F32(0), F32(1), F32(0.5)


# ------------------------------------------------------------------------------------------------------------ crop placement
def floor_div(a, b):
    """torch.floor_divide of two float32 scalars (c10::div_floor_floating): fmod, divide, correct, floor, round."""
    a, b = F32(a), F32(b)
    if b == 0:
        return a / b
    mod = F32(np.fmod(a, b))
    div = F32(F32(a - mod) / b)
    if mod != 0 and ((b < 0) != (mod < 0)):
        div = F32(div - _ONE)
    if div != 0:
        fl = F32(np.floor(div))
        if F32(div - fl) > _HALF:
            fl = F32(fl + _ONE)
        return fl
    return F32(np.copysign(_ZERO, F32(a / b)))


def crop_axis(c, crop, img, stride):
    """One axis of one anchor: centre c (float32), window length, image length, stride -> (lo, hi, branch)."""
    stride_f, crop_f, img_f = F32(stride), F32(crop), F32(img)
    raw = F32(c - F32(crop / 2))                                             # box_left = cx - crop_size.w / 2
    if raw > 0:                                                              # masked_select_or_fill_constant(floor_to_stride(..), .. > 0, 0)
        lo = F32(floor_div(F32(np.floor(raw)), stride_f) * stride_f)
        branch = "floor"
    else:
        lo = _ZERO
        branch = "zero"
    hi = F32(lo + crop_f)
    if lo < 0:                                                               # "have to move right": cannot happen, kept as the reference has it
        hi = F32(hi - lo)
        lo = _ZERO
        branch = "moved"
    if hi > img_f:
        over = F32(np.floor(F32(hi - img_f)))
        shift = F32(F32(np.floor(F32(np.ceil(F32(over / stride_f))))) * stride_f)    # ceil_to_stride
        if F32(lo - shift) >= 0:
            lo, hi, branch = F32(lo - shift), F32(hi - shift), "shift"
        else:
            lo, hi, branch = _ZERO, crop_f, "full"
    return lo, hi, branch


def apply_ops(box, ops):
    """A box-op chain on one box (4 float32 scalars): kinds 1 scale, 2 h-flip, 3 v-flip, 4 shift; one rounding per operation."""
    x1, y1, x2, y2 = [F32(v) for v in box]
    for kind, ax, ay in ops:
        ax, ay = F32(ax), F32(ay)
        if kind == OP_SCALE:
            x1, y1, x2, y2 = F32(x1 * ax), F32(y1 * ay), F32(x2 * ax), F32(y2 * ay)
        elif kind == OP_HFLIP:
            x1, x2 = F32(ax - x2), F32(ax - x1)
        elif kind == OP_VFLIP:
            y1, y2 = F32(ay - y2), F32(ay - y1)
        elif kind == OP_SHIFT:
            x1, y1, x2, y2 = F32(x1 - ax), F32(y1 - ay), F32(x2 - ax), F32(y2 - ay)
        else:
            raise ValueError("box-op kind {}".format(kind))
    return x1, y1, x2, y2


def crop_box(p, W, stride, box_size, img_w, img_h, crop_w, crop_h, ops=()):
    """Anchor p of a level -> (crop window [4], anchor box [4], (branch on x, branch on y)), both boxes through ``ops``."""
    y, x = divmod(int(p), int(W))
    cx = F32(F32(F32(x) + _HALF) * F32(stride))
    cy = F32(F32(F32(y) + _HALF) * F32(stride))
    left, right, bx = crop_axis(cx, crop_w, img_w, stride)
    top, bottom, by = crop_axis(cy, crop_h, img_h, stride)
    half = F32(F32(box_size) / F32(2))                                       # cx_cy_w_h -> xyxy: cx - w / 2 on a float32 tensor
    anchor = (F32(cx - half), F32(cy - half), F32(cx + half), F32(cy + half))
    return apply_ops((left, top, right, bottom), ops), apply_ops(anchor, ops), (bx, by)


def crop_table(H, W, stride, box_size, img_w, img_h, crop_w, crop_h, ops=()):
    """-> (crops [HW,4] float32, anchors [HW,4] float32, branches on x [HW], branches on y [HW])."""
    crops, anchors = np.zeros((H * W, 4), F32), np.zeros((H * W, 4), F32)
    bx, by = [], []
    for p in range(H * W):
        crops[p], anchors[p], (x, y) = crop_box(p, W, stride, box_size, img_w, img_h, crop_w, crop_h, ops)
        bx.append(x), by.append(y)
    return crops, anchors, bx, by


# ------------------------------------------------------------------------------------------------------------------ selection
def area(b):
    return F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))


def iou_pair(a, b):
    """-> (float32 IoU as the reference's tensor expressions round it, float64 IoU of the same float32 boxes, the float32 operands)."""
    w = max(F32(min(a[2], b[2]) - max(a[0], b[0])), _ZERO)
    h = max(F32(min(a[3], b[3]) - max(a[1], b[1])), _ZERO)
    inter = F32(w * h)
    area_a, area_b = area(a), area(b)
    total = F32(area_a + area_b)
    union = F32(total - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = F32(inter / union)
    a64, b64 = [float(v) for v in a], [float(v) for v in b]
    w64 = max(min(a64[2], b64[2]) - max(a64[0], b64[0]), 0.0)
    h64 = max(min(a64[3], b64[3]) - max(a64[1], b64[1]), 0.0)
    i64 = w64 * h64
    u64 = (a64[2] - a64[0]) * (a64[3] - a64[1]) + (b64[2] - b64[0]) * (b64[3] - b64[1]) - i64
    return q, (i64 / u64 if u64 > 0 else float("nan")), (w, h, inter, area_a, area_b, total, union)


def select(scores, flagged, window_of, windows, thr, K):
    """Greedy selection over candidates 0..N-1 in flat order.

    scores [N] float32; flagged [N] bool; window_of [N]: index of the candidate's window in ``windows`` [T,4].
    -> (kept flats, pairs): at most K rounds of "take the best candidate alive (finite scores only; on equality - -0 equals +0 -
    the smaller flat), remove it, kill every candidate alive whose window has float32 inter / union > thr with the kept one".
    pairs: one entry (round, kept flat, window index, killed, float32 IoU, float64 IoU, operands) per window tested in a round."""
    N = len(scores)
    thr = F32(thr)
    alive = [bool(flagged[i]) and bool(np.isfinite(scores[i])) for i in range(N)]
    kept, pairs = [], []
    for r in range(K):
        best = -1
        for i in range(N):
            if alive[i] and (best < 0 or scores[i] > scores[best]):           # strict: the smaller flat wins equality; -0 == +0
                best = i
        if best < 0:
            break
        kept.append(best)
        alive[best] = False                                                  # the kept candidate is removed
        if r + 1 == K:
            break
        verdict = {}
        for i in range(N):
            if not alive[i]:
                continue
            t = window_of[i]
            if t not in verdict:
                q, q64, operands = iou_pair(windows[window_of[best]], windows[t])
                verdict[t] = bool(q > thr)
                pairs.append((r, best, t, verdict[t], q, q64, operands))
            if verdict[t]:
                alive[i] = False
    return kept, pairs


def mine(case):
    """A case of tests/mining_stage_cases.py -> dict(count [A,3] int32, index [A,3,K,3] int32, values [A,3,K,19] float32 - the
    layout os2d_train_mine_select writes, unfilled records -1 and 0 -, kept [A][3] flat lists, candidates [A][3], pairs [A][3],
    band_gap, exact, branches_x / branches_y per level)."""
    A, B, K, levels = case["A"], case["B"], case["K"], case["levels"]
    tables, branches_x, branches_y = [], [], []
    for (H, W), (iw, ih), ops in zip(levels, case["imgs"], case["chains"]):
        crops, anchors, bx, by = crop_table(H, W, case["stride"], case["box"], iw, ih, case["crop"][0], case["crop"][1], ops)
        tables.append((crops, anchors))
        branches_x.append(bx), branches_y.append(by)
    windows = np.concatenate([t[0] for t in tables])
    where, window_of, base = [], [], 0
    for l, (H, W) in enumerate(levels):
        for b in range(B):
            for p in range(H * W):
                where.append((l, b, p))
                window_of.append(base + p)
        base += H * W
    count = np.zeros((A, 3), np.int32)
    index = np.full((A, 3, K, INDEX_INTS), -1, np.int32)
    values = np.zeros((A, 3, K, VALUE_FLOATS), F32)
    kept_all, cand_all, pairs_all = [], [], []
    gap, exact = float("inf"), True
    for a in range(A):
        kept_a, cand_a, pairs_a = [], [], []
        for r, bit in enumerate(ROLE_BITS):
            src = case["loc_loss"] if r == 2 else case["cls_loss"]
            scores = np.concatenate([np.asarray(t[a], F32).reshape(-1) for t in src])
            flagged = np.concatenate([(np.asarray(t[a]).reshape(-1) & bit) != 0 for t in case["flags"]])
            kept, pairs = select(scores, flagged, window_of, windows, case["thr"], K)
            count[a, r] = len(kept)
            for k, flat in enumerate(kept):
                l, b, p = where[flat]
                index[a, r, k] = (l, b, p)
                v = values[a, r, k]
                v[0:4], v[4:8] = tables[l][0][p], tables[l][1][p]
                if case["corners"] is not None:
                    q = case["corners"][l][a, b, :, p]
                    v[8:12], v[12:16] = apply_ops(q[0:4], case["chains"][l]), apply_ops(q[4:8], case["chains"][l])
                v[16], v[17], v[18] = case["cls_loss"][l][a, b, p], case["loc_loss"][l][a, b, p], case["cls_preds"][l][a, b, p]
            for pr in pairs:
                gap = min(gap, abs(pr[5] - float(F32(case["thr"]))))
                exact = exact and all(float(o) == int(o) and 0 <= float(o) < 2 ** 24 for o in pr[6])
            kept_a.append(kept), cand_a.append(int((flagged & np.isfinite(scores)).sum())), pairs_a.append(pairs)
        kept_all.append(kept_a), cand_all.append(cand_a), pairs_all.append(pairs_a)
    return dict(count=count, index=index, values=values, kept=kept_all, candidates=cand_all, pairs=pairs_all, band_gap=gap, exact=exact,
                branches_x=branches_x, branches_y=branches_y, where=where)
