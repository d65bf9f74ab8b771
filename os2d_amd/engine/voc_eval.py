"""PASCAL VOC detection metric (mAP, recall) of a whole dataset, computed on the device by libos2d_eval.so: the
counterpart of the reference's ``os2d/data/voc_eval.py`` with its function names, arguments and result dictionary.

The reference copies every image's detections to the host and loops over images x labels in numpy.  Here detections stay
on the device from ``decode_pyramid`` to the final numbers:

    match      one thread per detection: IoU against the ground truth of its image and label (+1 on xmax / ymax, fp32, first
               argmax, threshold rounded to fp32), the best-scoring detection of every ground-truth box found by a 64-bit
               integer atomicMin of (score key, index in image)
    sort       stable radix sort of all detections by descending score (joint classes) and by (label, descending score);
               independent of the IoU threshold, so computed once per ``VocEvaluator`` and reused
    curves     segmented scans over the sorted array: tp / fp counts, prec = tp / (tp + fp), rec = tp / n_pos in fp64, the
               reversed running maximum, the area under the curve (or the 11-point form)
    finalise   map, map_weighted, recall, ap_joint_classes

Tie order.  The reference sorts with numpy's unstable ``argsort()[::-1]`` and so defines no order among equal scores; here
equal scores are taken in increasing (image order, index within the image), both inside an image and in the dataset-wide
sort.

Labels are non-negative integers below ``num_labels``.  The arrays have length ``num_labels``; when it is not given it is
the reference's "largest label seen + 1", which needs the largest detection label from the device (one synchronisation).
Labels that were never seen have AP NaN and ``prec`` / ``rec`` None, so a larger ``num_labels`` changes no scalar.

Detection labels live on the device and are not validated.  A detection whose label is outside ``[0, num_labels)`` (a
``num_labels`` that is too small) can match only a ground-truth box of the same label - none when the ground-truth labels
are in range, which host-side ground truth is checked for; it then counts as a false positive of the joint class - and is sorted
behind every class with the key ``num_labels`` (``sorted_labels`` holds ``num_labels`` for those rows, and
``class_offsets[num_labels]`` is the number of detections in range): the per-class numbers are those without it.
"""
import torch

from .. import _eval_lib
from .._native import STREAM
from ..structures.bounding_box import BoxList  # noqa: F401  (the type of the arguments)


def _n(t):
    """The kernels take NULL for an array without elements (no detections, no ground truth)."""
    return t if t is not None and t.numel() else None


def _to_device(host, device):
    """Host tensor -> device without a synchronisation: through pinned memory, non_blocking."""
    pinned = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
    pinned.copy_(host)
    return pinned.to(device, non_blocking=True)


def _resized(pred, size):
    """``pred.resize(size)``.  BoxList.resize builds the unequal-ratio factor with ``torch.tensor(..., device=...)``, a
    blocking copy; for device boxes the same product is formed here from a factor uploaded without one."""
    rw = float(size.w) / pred.image_size.w
    rh = float(size.h) / pred.image_size.h
    if rw == rh or not pred.bbox_xyxy.is_cuda:
        return pred.resize(size)
    factor = _to_device(torch.tensor([rw, rh, rw, rh], dtype=torch.float32), pred.bbox_xyxy.device)
    out = BoxList(pred.bbox_xyxy * factor, size)
    out.extra_fields = dict(pred.extra_fields)
    return out


class VocEvaluator(object):
    """Accumulates (detections, ground truth) per image and computes the VOC metric on the device.

    ``add`` keeps device tensors and host ground truth as they are; nothing is copied or synchronised there.  ``compute``
    packs everything once, sorts once, and evaluates one IoU threshold per call; packing and the sorted orders are cached on
    the object until the next ``add``.  With host-side ground truth and ``num_labels`` given, the only device-to-host
    transfer is the copy of the class offsets at the end of ``compute`` (needed to cut ``prec`` / ``rec`` into per-class
    views); ``compute(..., with_curves=False)`` leaves those lists out and transfers nothing."""

    def __init__(self, num_labels=None, device=None):
        self.num_labels = num_labels
        self.device = torch.device(device) if device is not None else None
        self._pred, self._gt = [], []
        self._packed = None
        self.last = None      # device arrays of the last compute(): match, tpfp / prec / rec of both orders (tests, tools)

    def __len__(self):
        return len(self._pred)

    def add(self, pred_boxlist, gt_boxlist):
        pred = _resized(pred_boxlist, gt_boxlist.image_size)
        self._pred.append((pred.bbox_xyxy, pred.get_field("scores"), pred.get_field("labels")))
        difficult = gt_boxlist.get_field("difficult") if gt_boxlist.has_field("difficult") else None
        self._gt.append((gt_boxlist.bbox_xyxy, gt_boxlist.get_field("labels"), difficult))
        self._packed = None

    # ------------------------------------------------------------------------------------------------ packing + sort
    def _device(self):
        if self.device is not None:
            return self.device
        for b, _, _ in self._pred:
            if b.is_cuda:
                return b.device
        return torch.device("cuda", torch.cuda.current_device())

    def _cat(self, parts, dtype, device, tail=()):
        """Concatenation of per-image tensors on ``device``; host parts are joined on the host and uploaded once."""
        parts = [p.reshape((-1,) + tuple(tail)) for p in parts]
        if not parts:
            return torch.empty((0,) + tuple(tail), dtype=dtype, device=device)
        if all(not p.is_cuda for p in parts):
            return _to_device(torch.cat(parts, 0).to(dtype).contiguous(), device)
        return torch.cat([p if p.is_cuda else _to_device(p.contiguous(), device) for p in parts], 0).to(dtype).contiguous()

    def _pack(self):
        if self._packed is not None:
            return self._packed
        if not self._pred:
            raise RuntimeError("VocEvaluator.compute: no image was added")
        lib = _eval_lib.load()
        dev = self._device()
        N = len(self._pred)
        det_counts = [int(b.shape[0]) for b, _, _ in self._pred]
        gt_counts = [int(b.shape[0]) for b, _, _ in self._gt]
        D, G = sum(det_counts), sum(gt_counts)
        if D >= 2 ** 31 or G >= 2 ** 31:
            raise RuntimeError("VocEvaluator: more than 2^31 - 1 boxes")
        offsets = torch.zeros(2, N + 1, dtype=torch.int32)
        offsets[0, 1:] = torch.tensor(det_counts, dtype=torch.int64).cumsum(0)
        offsets[1, 1:] = torch.tensor(gt_counts, dtype=torch.int64).cumsum(0)
        offsets = _to_device(offsets, dev)
        p = dict(N=N, D=D, G=G, device=dev, det_offsets=offsets[0], gt_offsets=offsets[1])
        p["det_boxes"] = self._cat([b for b, _, _ in self._pred], torch.float32, dev, (4,))
        p["det_scores"] = self._cat([s for _, s, _ in self._pred], torch.float32, dev)
        p["det_labels"] = self._cat([l for _, _, l in self._pred], torch.int32, dev)
        p["gt_boxes"] = self._cat([b for b, _, _ in self._gt], torch.float32, dev, (4,))
        p["gt_labels"] = self._cat([l for _, l, _ in self._gt], torch.int32, dev)
        p["gt_difficult"] = self._cat([(d != 0) if d is not None else torch.zeros(l.shape, dtype=torch.bool, device=l.device)
                                       for _, l, d in self._gt], torch.uint8, dev)
        L = self.num_labels
        if L is None:    # the reference's length: largest label seen + 1
            seen = [l.max() for _, l, _ in self._gt if l.numel()] + ([p["det_labels"].max()] if D else [])
            L = int(max(int(v) for v in seen)) + 1 if seen else 1
        L = int(L)
        host_gt = [l for _, l, _ in self._gt if l.numel() and not l.is_cuda]
        if host_gt and (max(int(l.max()) for l in host_gt) >= L or min(int(l.min()) for l in host_gt) < 0):
            raise ValueError("VocEvaluator: a ground-truth label lies outside [0, num_labels = {})".format(L))
        p["L"] = L
        # [class_offsets (L+1) | n_pos (L+1) | gt_count (L)]: one buffer, one device-to-host copy when the curves are asked for
        meta = torch.empty(3 * L + 2, dtype=torch.int32, device=dev)
        p["meta"] = meta
        p["class_offsets"], p["n_pos"], p["gt_count"] = meta[:L + 1], meta[L + 1:2 * L + 2], meta[2 * L + 2:]
        _eval_lib.call("os2d_eval_count_gt", _n(p["gt_labels"]), _n(p["gt_difficult"]), G, L, _n(p["n_pos"]), _n(p["gt_count"]), STREAM)
        p["perm_joint"] = torch.empty(D, dtype=torch.int32, device=dev)
        p["perm_class"] = torch.empty(D, dtype=torch.int32, device=dev)
        p["sorted_labels"] = torch.empty(D, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.os2d_eval_sort_workspace_bytes(D), dtype=torch.uint8, device=dev)
        _eval_lib.call("os2d_eval_sort", _n(p["det_scores"]), _n(p["det_labels"]), D, L, max(L - 1, 0).bit_length(), _n(p["perm_joint"]),
                       _n(p["perm_class"]), _n(p["sorted_labels"]), _n(p["class_offsets"]), _n(ws), ws.numel(), STREAM)
        p["scan_ws"] = torch.empty(lib.os2d_eval_scan_workspace_bytes(D), dtype=torch.uint8, device=dev)
        self._packed = p
        return p

    # ------------------------------------------------------------------------------------------------ stages
    def _match(self, p, iou_thresh):
        dev, D, G = p["device"], p["D"], p["G"]
        match = torch.empty(D, dtype=torch.int8, device=dev)
        gt_index = torch.empty(D, dtype=torch.int32, device=dev)
        winner = torch.empty(G, dtype=torch.int64, device=dev)
        _eval_lib.call("os2d_eval_match", _n(p["det_boxes"]), _n(p["det_scores"]), _n(p["det_labels"]), _n(p["det_offsets"]), D, p["N"],
                       _n(p["gt_boxes"]), _n(p["gt_labels"]), _n(p["gt_difficult"]), _n(p["gt_offsets"]), G, float(iou_thresh),
                       _n(gt_index), _n(winner), _n(match), STREAM)
        return match

    def _curves(self, p, match, joint, rec_last):
        """tp/fp, prec and rec of the per-class (joint=False) or the joint-classes ordering."""
        dev, D, L = p["device"], p["D"], p["L"]
        tpfp = torch.empty(D, dtype=torch.int64, device=dev)
        prec = torch.empty(D, dtype=torch.float64, device=dev)
        rec = torch.empty(D, dtype=torch.float64, device=dev)
        perm = p["perm_joint"] if joint else p["perm_class"]
        seg = None if joint else p["sorted_labels"]
        n_pos = p["n_pos"][L:] if joint else p["n_pos"]
        _eval_lib.call("os2d_eval_prec_rec", _n(match), _n(perm), _n(seg), _n(n_pos), 1 if joint else L, D, _n(tpfp), _n(prec), _n(rec),
                       _n(rec_last[L:] if joint else rec_last), _n(p["scan_ws"]), p["scan_ws"].numel(), STREAM)
        return tpfp, prec, rec

    def _ap(self, p, prec, rec, joint, use_07_metric, acc):
        dev, D, L = p["device"], p["D"], p["L"]
        mpre = torch.empty(D, dtype=torch.float64, device=dev)
        seg = None if joint else p["sorted_labels"]
        _eval_lib.call("os2d_eval_ap", _n(prec), _n(rec), _n(seg), 1 if joint else L, D, int(bool(use_07_metric)), _n(mpre),
                       _n(acc[L:] if joint else acc), _n(p["scan_ws"]), p["scan_ws"].numel(), STREAM)
        return mpre

    def compute(self, iou_thresh=0.5, use_07_metric=False, with_curves=True):
        """The reference's result dictionary (``eval_detection_voc``) on the device: ``ap_per_class``, ``recall_per_class``,
        ``n_pos`` are fp64 tensors of length num_labels, ``map``, ``map_weighted``, ``recall``, ``ap_joint_classes`` 0-dim
        fp64 tensors, ``prec`` / ``rec`` lists of per-class views into the class-sorted arrays (None where the reference has
        None; left out with ``with_curves=False``)."""
        p = self._pack()
        dev, L = p["device"], p["L"]
        match = self._match(p, iou_thresh)
        rec_last = torch.zeros(L + 1, dtype=torch.float64, device=dev)
        acc = torch.zeros(L + 1, 11, dtype=torch.float64, device=dev)
        tpfp, prec, rec = self._curves(p, match, False, rec_last)
        mpre = self._ap(p, prec, rec, False, use_07_metric, acc)
        tpfp_j, prec_j, rec_j = self._curves(p, match, True, rec_last)
        mpre_j = self._ap(p, prec_j, rec_j, True, use_07_metric, acc)
        out = torch.empty(3 * L + 4, dtype=torch.float64, device=dev)
        ap, recall_pc, n_pos, scalars = out[:L], out[L:2 * L], out[2 * L:3 * L], out[3 * L:]
        _eval_lib.call("os2d_eval_finalise", _n(acc), _n(rec_last), _n(p["n_pos"]), L, int(bool(use_07_metric)), _n(ap), _n(recall_pc),
                       _n(n_pos), _n(scalars), STREAM)
        self.last = dict(match=match, tpfp=tpfp, prec=prec, rec=rec, mpre=mpre, tpfp_joint=tpfp_j, prec_joint=prec_j, rec_joint=rec_j,
                         mpre_joint=mpre_j, perm_class=p["perm_class"], perm_joint=p["perm_joint"], class_offsets=p["class_offsets"],
                         n_pos_joint=p["n_pos"][L])
        result = {"ap_per_class": ap, "map": scalars[0], "map_weighted": scalars[1], "recall_per_class": recall_pc, "recall": scalars[2],
                  "n_pos": n_pos, "ap_joint_classes": scalars[3]}
        if with_curves:
            result["prec"], result["rec"] = self._curve_lists(p, prec, rec)
        return result

    def _curve_lists(self, p, prec, rec):
        L = p["L"]
        if "meta_host" not in p:
            p["meta_host"] = p["meta"].cpu()       # the one device-to-host transfer
        meta = p["meta_host"].tolist()
        offsets, n_pos, gt_count = meta[:L + 1], meta[L + 1:2 * L + 1], meta[2 * L + 2:]
        precs, recs = [None] * L, [None] * L
        for l in range(L):
            lo, hi = offsets[l], offsets[l + 1]
            if hi > lo or gt_count[l] > 0:         # the label was seen among predictions or ground truth
                precs[l] = prec[lo:hi]
                if n_pos[l] > 0:
                    recs[l] = rec[lo:hi]
        return precs, recs


# ---------------------------------------------------------------------------------------------------- reference functions
def _evaluator(gt_boxlists, pred_boxlists):
    assert len(gt_boxlists) == len(pred_boxlists), "Length of gt and pred lists need to be same."
    ev = VocEvaluator()
    for pred, gt in zip(pred_boxlists, gt_boxlists):
        ev.add(pred, gt)
    return ev


def do_voc_evaluation(predictions, gt_boxes, iou_thresh=0.5, use_07_metric=False):
    """Reference voc_eval.py:14-37: resizes every prediction BoxList to its ground truth's image size and evaluates."""
    return eval_detection_voc([p.resize(g.image_size) for p, g in zip(predictions, gt_boxes)], gt_boxes, iou_thresh=iou_thresh,
                              use_07_metric=use_07_metric)


def eval_detection_voc(pred_boxlists, gt_boxlists, iou_thresh=0.5, use_07_metric=False):
    """Reference voc_eval.py:39-68 (boxes already in the ground truth's image size)."""
    return _evaluator(gt_boxlists, pred_boxlists).compute(iou_thresh=iou_thresh, use_07_metric=use_07_metric)


def calc_detection_voc_prec_rec(gt_boxlists, pred_boxlists, iou_thresh=0.5, merge_classes_together=False):
    """Reference voc_eval.py:71-171.  Returns (prec, rec, n_pos): lists of device tensors (None as in the reference) and
    n_pos as an int32 device tensor indexed by label (one entry, the total, with ``merge_classes_together``)."""
    ev = _evaluator(gt_boxlists, pred_boxlists)
    p = ev._pack()
    L = p["L"]
    match = ev._match(p, iou_thresh)
    rec_last = torch.zeros(L + 1, dtype=torch.float64, device=p["device"])
    if merge_classes_together:
        _, prec, rec = ev._curves(p, match, True, rec_last)
        n_pos = p["n_pos"][L:]
        return [prec], [rec if int(n_pos[0]) > 0 else None], n_pos
    _, prec, rec = ev._curves(p, match, False, rec_last)
    precs, recs = ev._curve_lists(p, prec, rec)
    return precs, recs, p["n_pos"][:L]


def calc_detection_voc_ap(prec, rec, use_07_metric=False):
    """Reference voc_eval.py:174-230 for lists of device tensors: fp64 device tensor of len(prec), NaN where an entry is None."""
    lib = _eval_lib.load()
    n = len(prec)
    have = [l for l in range(n) if prec[l] is not None and rec[l] is not None]
    dev = prec[have[0]].device if have else torch.device("cuda", torch.cuda.current_device())
    ap = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    if not have:
        return ap
    lengths = [int(prec[l].numel()) for l in have]
    D = sum(lengths)
    acc = torch.zeros(n, 11, dtype=torch.float64, device=dev)
    if D:
        p = torch.cat([prec[l].to(torch.float64) for l in have]).contiguous()
        r = torch.cat([rec[l].to(torch.float64) for l in have]).contiguous()
        seg = _to_device(torch.repeat_interleave(torch.tensor(have, dtype=torch.int32), torch.tensor(lengths)), dev)
        mpre = torch.empty(D, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.os2d_eval_scan_workspace_bytes(D), dtype=torch.uint8, device=dev)
        _eval_lib.call("os2d_eval_ap", _n(p), _n(r), _n(seg), n, D, int(bool(use_07_metric)), _n(mpre), _n(acc), _n(ws), ws.numel(), STREAM)
    if use_07_metric:
        total = torch.zeros(n, dtype=torch.float64, device=dev)
        for t in range(11):
            total = total + acc[:, t] / 11
    else:
        total = acc[:, 0]
    idx = torch.tensor(have, dtype=torch.int64, device=dev)
    ap[idx] = total[idx]
    return ap


def calc_detection_recall(rec, n_pos):
    """Reference voc_eval.py:232-253: (recall, recall_per_class, n_pos) as fp64 device tensors."""
    n = len(rec)
    n_pos = torch.as_tensor(n_pos)[:n].to(torch.float64)
    dev = n_pos.device
    last = [r[-1:].to(torch.float64) if r is not None and r.numel() else torch.zeros(1, dtype=torch.float64, device=dev) for r in rec]
    last = torch.cat(last) if last else torch.zeros(0, dtype=torch.float64, device=dev)
    absent = torch.tensor([r is None for r in rec], dtype=torch.bool, device=dev) | (n_pos == 0)
    per_class = torch.where(absent, torch.full_like(last, float("nan")), last)
    weight = torch.where(absent, torch.zeros_like(n_pos), n_pos)
    total = weight.sum()
    recall = (weight * torch.where(absent, torch.zeros_like(last), last)).sum() / total      # 0 / 0 = NaN as in the reference
    return recall, per_class, n_pos
