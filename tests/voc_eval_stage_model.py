"""A plain statement of every entry point of libos2d_eval.so (include/os2d_eval.h): numpy arrays, Python integers and
floats, written as loops in the order of the reference's os2d/data/voc_eval.py.  It is deliberately NOT the parallel
formulation of tests/voc_eval_model.py (keys, atomics, scans): two independent statements of the metric should agree
(tests/test_voc_eval_stage_model.py), and the kernels are compared with this one (tests/test_voc_eval_stages_gpu.py).

Floats: an IoU is a chain of np.float32 operations, each rounded on its own; prec, rec and the terms of the average precision
are single IEEE fp64 operations (a Python float is an IEEE double).  Sums are not formed here where their order is the
kernel's business: ``ap`` returns the terms of a segment and the caller takes ``math.fsum``."""
import math

import numpy as np

F32 = np.float32
NAN = float("nan")


def count_gt(gt_labels, gt_difficult, L):
    """n_pos [L+1] (boxes per label that are not difficult, slot L their total) and gt_count [L] (all boxes per label).  A label
    outside [0, L) is skipped; any nonzero byte is difficult."""
    n_pos, gt_count = [0] * (L + 1), [0] * L
    for l, d in zip(np.asarray(gt_labels).tolist(), np.asarray(gt_difficult).tolist()):
        if l < 0 or l >= L:
            continue
        gt_count[l] += 1
        if d == 0:
            n_pos[l] += 1
            n_pos[L] += 1
    return np.array(n_pos, np.int32), np.array(gt_count, np.int32)


def iou_f32(a, b):
    """IoU of two boxes (xmin, ymin, xmax, ymax) with +1 on xmax / ymax of both, every operation rounded to fp32."""
    one = F32(1)
    ax1, ay1, ax2, ay2 = F32(a[0]), F32(a[1]), F32(a[2]) + one, F32(a[3]) + one
    bx1, by1, bx2, by2 = F32(b[0]), F32(b[1]), F32(b[2]) + one, F32(b[3]) + one
    area_a = (ax2 - ax1) * (ay2 - ay1)
    area_b = (bx2 - bx1) * (by2 - by1)
    w = max(min(ax2, bx2) - max(ax1, bx1), F32(0))
    h = max(min(ay2, by2) - max(ay1, by1), F32(0))
    inter = F32(w) * F32(h)
    return inter / (area_a + area_b - inter)


def score_order(scores, rows):
    """``rows`` in descending score, equal scores (-0.0 == +0.0 included) in the order given."""
    return sorted(rows, key=lambda i: -float(scores[i]))     # sorted() is stable; -(-0.0) == -(+0.0) as floats


def match(det_boxes, det_scores, det_labels, det_offsets, gt_boxes, gt_labels, gt_difficult, gt_offsets, thr):
    """The reference's loop (voc_eval.py:81-140): per image, per label, the detections in (descending score, increasing index
    in the image); the best ground-truth box of the label by IoU, the first of equal maxima; no box when the maximum is below
    the threshold rounded to fp32; the first detection to reach a plain box gets 1, later ones 0, any on a difficult box -1.
    -> match [D] int8, gt_index [D] int32 (row of the matched box in the packed ground truth, or -1)."""
    D, N = len(det_scores), len(det_offsets) - 1
    thr = F32(thr)
    out, index = np.zeros(D, np.int8), np.full(D, -1, np.int32)
    det_labels, gt_labels = np.asarray(det_labels).tolist(), np.asarray(gt_labels).tolist()
    for n in range(N):
        rows = list(range(int(det_offsets[n]), int(det_offsets[n + 1])))
        boxes = list(range(int(gt_offsets[n]), int(gt_offsets[n + 1])))
        for label in sorted(set(det_labels[d] for d in rows)):
            mine = [g for g in boxes if gt_labels[g] == label]
            selec = {g: False for g in mine}
            for d in score_order(det_scores, [d for d in rows if det_labels[d] == label]):
                best, arg = None, -1
                for g in mine:
                    iou = iou_f32(det_boxes[d], gt_boxes[g])
                    if best is None or iou > best:           # the first argmax
                        best, arg = iou, g
                if arg >= 0 and best < thr:
                    arg = -1
                index[d] = arg
                if arg < 0:
                    out[d] = 0
                elif gt_difficult[arg] != 0:
                    out[d] = -1
                else:
                    out[d] = 0 if selec[arg] else 1
                    selec[arg] = True
    return out, index


def label_key(label, L):
    """The key of the per-class ordering: the label, or L for a label outside [0, L) (such rows follow every class)."""
    return label if 0 <= label < L else L


def sort(scores, labels, L):
    """perm_joint: the rows in descending score, ties (+-0 included) in increasing index.  perm_class: perm_joint in
    increasing label key, otherwise unchanged.  sorted_labels: the key along perm_class; class_offsets [L+1]: the first
    position whose key is >= l.  Not defined for NaN scores."""
    D = len(scores)
    labels = np.asarray(labels).tolist()
    joint = score_order(scores, list(range(D)))
    by_class = sorted(joint, key=lambda i: label_key(labels[i], L))
    keys = [label_key(labels[i], L) for i in by_class]
    offsets = [sum(1 for k in keys if k < l) for l in range(L + 1)] if L <= 64 else np.searchsorted(np.array(keys, np.int64), np.arange(L + 1)).tolist()
    return np.array(joint, np.uint32), np.array(by_class, np.uint32), np.array(keys, np.int32), np.array(offsets, np.int32)


def divide(num, den):
    """One IEEE fp64 division per element of two integer lists: 0 / 0 is NaN, x / 0 is inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array(num, np.float64) / np.array(den, np.float64)


def prec_rec(match_, perm, seg, n_pos, L):
    """Per segment (a run of equal values of ``seg``; one segment when it is None) the running counts tp of match == 1 and fp of
    match == 0 along ``perm``; prec = tp / (tp + fp), rec = tp / n_pos[segment] (0 for a label outside [0, L)).
    -> tp, fp (int64), prec, rec (fp64), rec_last {label: the recall at the last position of its segment, only where
    n_pos > 0}."""
    D = len(perm)
    m = np.asarray(match_)[np.asarray(perm, np.int64)].tolist()
    s = [0] * D if seg is None else np.asarray(seg).tolist()
    n_pos = np.asarray(n_pos).tolist()
    tps, fps, den = [0] * D, [0] * D, [0] * D
    tp = fp = 0
    tails = []
    for j in range(D):
        if j == 0 or s[j] != s[j - 1]:
            tp = fp = 0
        if m[j] == 1:
            tp += 1
        elif m[j] == 0:
            fp += 1
        tps[j], fps[j] = tp, fp
        den[j] = n_pos[s[j]] if 0 <= s[j] < L else 0
        if j == D - 1 or s[j + 1] != s[j]:
            tails.append(j)
    prec = divide(tps, [a + b for a, b in zip(tps, fps)])
    rec = divide(tps, den)
    rec_last = {s[j]: float(rec[j]) for j in tails if den[j] > 0}
    return np.array(tps, np.int64), np.array(fps, np.int64), prec, rec, rec_last


def ap(prec, rec, seg, L, use_07):
    """mpre [D]: the maximum of nan_to_num(prec) from a position to the end of its segment.  Then per segment whose label is
    in [0, L): use_07 false -> the list of the terms (rec[i] - before) * mpre[i] at the positions where rec[i] != before
    (before = 0 at the head of a segment), for the caller's math.fsum; use_07 true -> 11 values, mpre at the first position with
    rec >= 0.1 * t, or the 0.0 the caller wrote when no position reaches the level.  -> mpre, {label: list}."""
    D = len(prec)
    p, r = np.asarray(prec, np.float64).tolist(), np.asarray(rec, np.float64).tolist()
    s = [0] * D if seg is None else np.asarray(seg).tolist()
    mpre = [0.0] * D
    for j in range(D - 1, -1, -1):
        x = 0.0 if p[j] != p[j] else p[j]
        tail = j == D - 1 or s[j + 1] != s[j]
        mpre[j] = x if tail or x > mpre[j + 1] else mpre[j + 1]
    out = {}
    for j in range(D):
        if s[j] < 0 or s[j] >= L:
            continue
        head = j == 0 or s[j] != s[j - 1]
        if head:
            out[s[j]] = [0.0] * 11 if use_07 else []
            reached = [False] * 11
        before = 0.0 if head else r[j - 1]
        if not use_07:
            if r[j] != before:
                out[s[j]].append((r[j] - before) * mpre[j])
            continue
        for t in range(11):
            if not reached[t] and r[j] >= 0.1 * t:
                reached[t] = True
                out[s[j]][t] = mpre[j]
    return np.array(mpre, np.float64), out


def class_ap(row, use_07):
    if not use_07:
        return float(row[0])
    total = 0.0
    for t in range(11):
        total += float(row[t]) / 11.0
    return total


def finalise(acc, rec_last, n_pos, L, use_07):
    """acc [(L+1), 11], rec_last [L+1], n_pos [L+1] (slot L: the joint class) -> ap_per_class, recall_per_class, n_pos_out
    [L] fp64 (NaN for a class without positives) and [map, map_weighted, recall, ap_joint_classes].  The sums are math.fsum
    of the products the kernel forms: ap * n_pos / total (two operations) and n_pos * recall (one)."""
    acc = np.asarray(acc, np.float64).reshape(L + 1, 11)
    n_pos = np.asarray(n_pos).tolist()
    total = float(n_pos[L])
    aps, recs = [NAN] * L, [NAN] * L
    seen, weighted, good = [], [], []
    for l in range(L):
        if n_pos[l] > 0:
            aps[l], recs[l] = class_ap(acc[l], use_07), float(rec_last[l])
            seen.append(aps[l])
            weighted.append(float(np.float64(aps[l] * float(n_pos[l])) / np.float64(total)))
            good.append(float(n_pos[l]) * recs[l])
    scalars = [math.fsum(seen) / len(seen) if seen else NAN,        # nanmean
               math.fsum(weighted),                                 # nansum: 0.0 when no class has positives
               math.fsum(good) / total if total > 0 else NAN,
               class_ap(acc[L], use_07) if total > 0 else NAN]
    return np.array(aps), np.array(recs), np.array(n_pos[:L], np.float64), np.array(scalars)


def fill_acc(acc, per_segment, use_07, row=None):
    """What os2d_eval_ap leaves in the caller's zeroed acc [(L+1), 11], with math.fsum as the sum of a segment's terms."""
    for s, v in per_segment.items():
        if use_07:
            acc[s if row is None else row, :] = v
        else:
            acc[s if row is None else row, 0] = math.fsum(v)
    return acc


def evaluate(c, L, thr, use_07):
    """The stages chained as VocEvaluator.compute chains the entry points.  c: det_boxes, det_scores, det_labels, det_offsets,
    gt_boxes, gt_labels, gt_difficult, gt_offsets (numpy)."""
    n_pos, gt_count = count_gt(c["gt_labels"], c["gt_difficult"], L)
    m, gt_index = match(c["det_boxes"], c["det_scores"], c["det_labels"], c["det_offsets"], c["gt_boxes"], c["gt_labels"], c["gt_difficult"],
                        c["gt_offsets"], thr)
    joint, by_class, keys, offsets = sort(c["det_scores"], c["det_labels"], L)
    tp, fp, prec, rec, last = prec_rec(m, by_class, keys, n_pos, L)
    mpre, per_class = ap(prec, rec, keys, L, use_07)
    jtp, jfp, jprec, jrec, jlast = prec_rec(m, joint, None, n_pos[L:], 1)
    jmpre, per_joint = ap(jprec, jrec, None, 1, use_07)
    acc = fill_acc(fill_acc(np.zeros((L + 1, 11)), per_class, use_07), per_joint, use_07, row=L)
    rec_last = np.zeros(L + 1)
    for s, v in last.items():
        rec_last[s] = v
    for s, v in jlast.items():
        rec_last[L] = v
    aps, recalls, n_pos_out, scalars = finalise(acc, rec_last, n_pos, L, use_07)
    return dict(match=m, gt_index=gt_index, n_pos=n_pos, gt_count=gt_count, perm_joint=joint, perm_class=by_class, sorted_labels=keys,
                class_offsets=offsets, tp=tp, fp=fp, prec=prec, rec=rec, mpre=mpre, tp_joint=jtp, fp_joint=jfp, prec_joint=jprec,
                rec_joint=jrec, terms=per_class, ap_per_class=aps, recall_per_class=recalls, n_pos_out=n_pos_out, scalars=scalars)


def same_bits(a, b):
    """Equal shape, NaN at the same positions, equal bits everywhere else (the sign and payload of a NaN are the divider's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def bits(a):
    """Integer view of an fp64 / fp32 array for equality of bits (NaN payloads included)."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
