"""Plain NumPy model of the detection stage (os2d_nms, os2d_detect_level*, os2d_detect_pyramid* of include/os2d_hip.h):
candidate list, decode, validity, box-op chains and the reference's chunk-and-repeat NMS, written as loops over candidates.
TEST INFRASTRUCTURE ONLY; it imports nothing of os2d_amd.

  * decode follows oracle/decode_oracle.decode_level in float64 (the box comparison of the GPU tests);
  * the op chains are applied in float32 as well, every product / difference rounded on its own (NumPy never contracts), which
    is what os2d_apply_box_ops computes bit for bit;
  * NMS is reference os2d/structures/bounding_box.py:343-374 (restated in decode_oracle.nms_chunked): IoU in float32 as
    inter / (area_a + area_b - inter) > thr, one vectorised test of a candidate against the boxes kept so far.

The kernels' geometry (steps of 64, batches of 1024, caches of 2048, the staging window) appears here ONLY to classify what a
case covers (``ChunkRun.classify``): no decision of the model depends on it.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TEMPLATE = 15
XFORM_CLIP = math.log(1000.0 / 16)
OP_SCALE, OP_HFLIP, OP_VFLIP, OP_SHIFT = 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------------------ decode and chains
def anchors(H, W, stride=16, rec_field=16):
    """[HW,4] float64 xyxy, row-major; every value is a small integer or half-integer, exact in float32 as well."""
    half = 0.5 * (stride * (TEMPLATE - 1) + rec_field)
    cx = np.tile((np.arange(W, dtype=F64) + 0.5) * stride, H)
    cy = np.repeat((np.arange(H, dtype=F64) + 0.5) * stride, W)
    return np.stack([cx - half, cy - half, cx + half, cy + half], 1)


def decode_level(loc, H, W, img_w, img_h, stride=16, rec_field=16):
    """loc [4,HW] float32 -> [HW,4] float64, clipped to the level's image (decode_oracle.decode_level)."""
    loc = np.asarray(loc, F64)
    a = anchors(H, W, stride, rec_field)
    aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    acx, acy = a[:, 0] + 0.5 * aw, a[:, 1] + 0.5 * ah
    with np.errstate(over="ignore"):
        pw = np.exp(np.minimum(loc[2] / 5.0, XFORM_CLIP)) * aw
        ph = np.exp(np.minimum(loc[3] / 5.0, XFORM_CLIP)) * ah
    pcx, pcy = loc[0] / 10.0 * aw + acx, loc[1] / 10.0 * ah + acy
    return np.stack([np.clip(pcx - 0.5 * pw, 0, img_w), np.clip(pcy - 0.5 * ph, 0, img_h),
                     np.clip(pcx + 0.5 * pw, 0, img_w), np.clip(pcy + 0.5 * ph, 0, img_h)], 1)


def apply_ops(boxes, ops, dtype):
    """ops: [(kind, ax, ay)] with float32 arguments (the ABI's); boxes [n,4]; every op in ``dtype``, rounded on its own."""
    b = np.array(boxes, dtype=dtype)
    for kind, ax, ay in ops:
        ax, ay = dtype(F32(ax)), dtype(F32(ay))
        if kind == OP_SCALE:
            b = b * np.array([ax, ay, ax, ay], dtype)
        elif kind == OP_HFLIP:
            b = np.stack([ax - b[:, 2], b[:, 1], ax - b[:, 0], b[:, 3]], 1)
        elif kind == OP_VFLIP:
            b = np.stack([b[:, 0], ay - b[:, 3], b[:, 2], ay - b[:, 1]], 1)
        elif kind == OP_SHIFT:
            b = b - np.array([ax, ay, ax, ay], dtype)
        else:
            raise ValueError(kind)
    return b


def chain_scale(ops):
    """Largest factor by which the chain stretches a length (the product of its SCALE ops' larger factors)."""
    f = 1.0
    for kind, ax, ay in ops:
        if kind == OP_SCALE:
            f *= max(abs(float(F32(ax))), abs(float(F32(ay))))
    return f


def label_candidates(levels, rows, score_thr):
    """The candidate list of one label: its head rows in slot order (-1: nothing), each row level by level, each level location
    by location.  levels: dicts H, W, img_w, img_h, loc [B,4,HW], cls [B,HW], corners [B,8,HW] or None, ops, dops.
    Returns arrays over V * N1 candidates (those of a -1 slot are invalid and hold NaN)."""
    N1 = sum(lv["H"] * lv["W"] for lv in levels)
    n = len(rows) * N1
    out = {"N1": N1, "scores": np.full(n, np.nan, F32), "valid": np.zeros(n, bool), "boxes64": np.full((n, 4), np.nan),
           "boxes32": np.full((n, 4), np.nan, F32), "default32": np.full((n, 4), np.nan, F32), "scale": np.ones(n),
           "corners32": None if levels[0].get("corners") is None else np.full((n, 8), np.nan, F32)}
    for v, row in enumerate(rows):
        off = v * N1
        for lv in levels:
            H, W = lv["H"], lv["W"]
            sl = slice(off, off + H * W)
            off += H * W
            out["scale"][sl] = chain_scale(lv["ops"])
            if row < 0:
                continue
            box = decode_level(lv["loc"][row], H, W, lv["img_w"], lv["img_h"])
            s = np.asarray(lv["cls"][row], F32)
            empty = (box[:, 3] <= box[:, 1]) | (box[:, 2] <= box[:, 0])
            with np.errstate(invalid="ignore"):
                out["valid"][sl] = (s > F32(score_thr)) & ~empty
            out["scores"][sl] = s
            out["boxes64"][sl] = apply_ops(box, lv["ops"], F64)
            out["boxes32"][sl] = apply_ops(box.astype(F32), lv["ops"], F32)
            out["default32"][sl] = apply_ops(anchors(H, W).astype(F32), lv["dops"], F32)
            if out["corners32"] is not None:
                c = np.asarray(lv["corners"][row], F32).T                                   # [HW,8]
                out["corners32"][sl] = np.concatenate([apply_ops(c[:, :4], lv["ops"], F32), apply_ops(c[:, 4:], lv["ops"], F32)], 1)
    return out


# ------------------------------------------------------------------------------------------------------------ NMS
def stable_descending(scores):
    """Positions by decreasing score, ties (+0 against -0 too) in list order."""
    return np.argsort(-np.asarray(scores, F64), kind="stable")


def _iou(kept, cand, dtype):
    """IoU of the candidate with every kept box, in ``dtype``, with the reference's roundings; 0/0 is NaN (compares false)."""
    k, c = kept.astype(dtype, copy=False), cand.astype(dtype, copy=False)
    w = np.maximum(np.minimum(k[:, 2], c[2]) - np.maximum(k[:, 0], c[0]), dtype(0))
    h = np.maximum(np.minimum(k[:, 3], c[3]) - np.maximum(k[:, 1], c[1]), dtype(0))
    inter = w * h
    area_k = (k[:, 2] - k[:, 0]) * (k[:, 3] - k[:, 1])
    area_c = (c[2] - c[0]) * (c[3] - c[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((area_k + area_c) - inter)


class ChunkRun:
    """Greedy NMS of one chunk in sorted order, with what the coverage conditions need.
    kept_pos [K]   sorted positions of the kept boxes (index = kept rank)
    victim_pos, sup_rank [S]   every suppressed candidate: its sorted position, the kept rank of its FIRST suppressor
    hits           per suppressed candidate the kept ranks of ALL its suppressors
    band           min over the tested pairs of |IoU64 - thr|;  pairs: how many were tested"""

    def __init__(self, boxes32, iou_thr, boxes64=None):
        n = len(boxes32)
        thr = F32(iou_thr)
        b64 = boxes32.astype(F64) if boxes64 is None else boxes64
        kept32, kept64 = np.empty((n, 4), F32), np.empty((n, 4), F64)
        kept_pos, victim, sup, hits_all = [], [], [], []
        self.band, self.pairs = math.inf, 0
        k = 0
        for p in range(n):
            if k:
                with np.errstate(invalid="ignore"):
                    hit = _iou(kept32[:k], boxes32[p], F32) > thr
                    d = np.abs(_iou(kept64[:k], b64[p], F64) - float(thr))
                self.pairs += k
                d = d[~np.isnan(d)]
                if d.size:
                    self.band = min(self.band, float(d.min()))
                if hit.any():
                    victim.append(p)
                    sup.append(int(np.argmax(hit)))
                    hits_all.append(np.nonzero(hit)[0])
                    continue
            kept32[k], kept64[k] = boxes32[p], b64[p]
            kept_pos.append(p)
            k += 1
        self.n = n
        self.kept_pos = np.array(kept_pos, np.int64)
        self.victim_pos, self.sup_rank, self.hits = np.array(victim, np.int64), np.array(sup, np.int64), hits_all

    @property
    def kept_count(self):
        return len(self.kept_pos)

    def kept_before(self, pos):
        """How many boxes were kept among the sorted positions < pos."""
        return np.searchsorted(self.kept_pos, pos)

    def classify(self, win, batch=1024, group=64):
        """COVERAGE ONLY.  A kernel that works candidates off in batches (``batch`` candidates of a staging window of ``win``,
        survivors of the boxes kept before the batch resolved ``group`` at a time) meets each suppressed candidate in one of
        these ways; per suppressed candidate:
          earlier     its first suppressor was kept in an earlier batch
          between     same batch: candidates between the two that survived the boxes kept before the batch (-1 if ``earlier``)
          same_group  same batch and both in one resolve group of the batch's survivors"""
        def batch_of(p):
            return (p // win) * ((win + batch - 1) // batch) + (p % win) // batch
        nb = int(batch_of(self.n - 1)) + 1 if self.n else 0
        start = [None] * nb                                        # first sorted position of every batch
        for p in range(self.n):
            if start[batch_of(p)] is None:
                start[batch_of(p)] = p
        dead_before = np.zeros(self.n, bool)                       # killed by a box kept before its batch started
        for p, h in zip(self.victim_pos, self.hits):
            dead_before[p] = bool((h < self.kept_before(start[batch_of(p)])).any())
        surv_index = np.zeros(self.n, np.int64)                    # index among the batch's survivors
        for s in start:
            e = min([x for x in start if x > s] + [self.n])
            surv_index[s:e] = np.cumsum(~dead_before[s:e]) - 1
        sup_pos = self.kept_pos[self.sup_rank] if len(self.sup_rank) else np.zeros(0, np.int64)
        earlier = np.array([batch_of(a) < batch_of(b) for a, b in zip(sup_pos, self.victim_pos)], bool)
        between = np.where(earlier, -1, surv_index[self.victim_pos] - surv_index[sup_pos] - 1)
        same_group = ~earlier & (surv_index[self.victim_pos] // group == surv_index[sup_pos] // group)
        return {"earlier": earlier, "between": between, "same_group": same_group, "sup_pos": sup_pos}


def nms_chunked(boxes32, scores, valid, iou_thr, max_batch, boxes64=None):
    """The reference's memory-bounded NMS.  Returns dict: order (surviving candidate numbers, final order), passes (how many
    were run), runs [pass][chunk] -> ChunkRun, ended ('one chunk' | 'nothing removed'), band, pairs."""
    ids = np.nonzero(valid)[0]
    M = int(max_batch)
    runs = []
    while True:
        n = len(ids)
        out, this = [], []
        for s in range(0, n, M):
            chunk = ids[s:s + M]
            chunk = chunk[stable_descending(scores[chunk])]
            run = ChunkRun(boxes32[chunk], iou_thr, None if boxes64 is None else boxes64[chunk])
            this.append(run)
            out.append(chunk[run.kept_pos])
        runs.append(this)
        ids = np.concatenate(out) if out else np.zeros(0, np.int64)
        if len(this) <= 1 or len(ids) == n:
            ended = "one chunk" if len(this) <= 1 else "nothing removed"
            break
    order = ids[stable_descending(scores[ids])]
    every = [r for p in runs for r in p]
    return {"order": order, "passes": len(runs), "runs": runs, "ended": ended, "final_chunks": sum(1 for r in runs[-1] if r.kept_count),
            "band": min([r.band for r in every] + [math.inf]), "pairs": sum(r.pairs for r in every)}


def detect_label(levels, rows, score_thr, iou_thr, max_batch):
    """One label end to end: candidates + NMS.  Adds ``cand`` (label_candidates) to the result of nms_chunked."""
    cand = label_candidates(levels, rows, score_thr)
    res = nms_chunked(cand["boxes32"], cand["scores"], cand["valid"], iou_thr, max_batch, cand["boxes64"])
    res["cand"] = cand
    return res


def nms_sorted_list(boxes32, count, iou_thr):
    """os2d_nms on one list already sorted by score: the keep mask over the first min(count, N) boxes, and the run."""
    n = min(int(count), len(boxes32))
    run = ChunkRun(np.asarray(boxes32[:n], F32), iou_thr)
    keep = np.zeros(len(boxes32), np.uint8)
    keep[run.kept_pos] = 1
    return keep, run
