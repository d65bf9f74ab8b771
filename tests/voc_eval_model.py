"""The VOC detection metric restated in vectorised torch, in the parallel formulation of the HIP kernels (DESIGN.md
section 12): packed detections, an order-free match (first argmax, the winner of a ground-truth box = its best-ranked
detection), two stable sorts, segmented scans.  It reproduces every fixture recorded from the reference
(tests/test_voc_eval_model.py) and is the comparator on shapes too large to record; it runs on any device.

Ties between equal scores: descending score, then increasing packed index (image order, index within the image)."""
import torch


def pack(images_boxes, images_scores, images_labels, gt_boxes, gt_labels, gt_difficult, device):
    """Per-image lists of tensors -> packed tensors with an image index per row."""
    def cat(parts, dtype, tail=()):
        parts = [torch.as_tensor(p).reshape((-1,) + tail) for p in parts]
        return torch.cat(parts, 0).to(device=device, dtype=dtype) if parts else torch.zeros((0,) + tail, dtype=dtype, device=device)
    image = lambda parts: torch.repeat_interleave(torch.arange(len(parts)), torch.tensor([len(p) for p in parts], dtype=torch.long)).to(device)  # noqa: E731
    return dict(boxes=cat(images_boxes, torch.float32, (4,)), scores=cat(images_scores, torch.float32), labels=cat(images_labels, torch.int64),
                image=image(images_labels), gt_boxes=cat(gt_boxes, torch.float32, (4,)), gt_labels=cat(gt_labels, torch.int64),
                gt_difficult=cat(gt_difficult, torch.bool), gt_image=image(gt_labels), N=len(images_labels))


def match(p, iou_thresh):
    """match [D] int8 in packed order and the stable descending-score order of the detections."""
    dev = p["boxes"].device
    D, G, N = p["boxes"].shape[0], p["gt_boxes"].shape[0], p["N"]
    order = torch.sort(p["scores"], descending=True, stable=True).indices
    out = torch.zeros(D, dtype=torch.int8, device=dev)
    if D == 0 or G == 0:
        return out, order
    rank = torch.empty(D, dtype=torch.int64, device=dev)
    rank[order] = torch.arange(D, device=dev)
    # ground truth of every image as a padded table [N, M]
    counts = torch.bincount(p["gt_image"], minlength=N)
    M = int(counts.max())
    first = torch.cumsum(counts, 0) - counts
    slot = torch.arange(G, device=dev) - first[p["gt_image"]]
    table = torch.full((N, M), -1, dtype=torch.int64, device=dev)
    table[p["gt_image"], slot] = torch.arange(G, device=dev)
    cand = table[p["image"]]                                      # [D, M] global ground-truth index or -1
    safe = cand.clamp(min=0)
    ok = (cand >= 0) & (p["gt_labels"][safe] == p["labels"][:, None])
    one = torch.tensor([0, 0, 1, 1], dtype=torch.float32, device=dev)
    a = (p["boxes"] + one)[:, None, :]
    b = (p["gt_boxes"] + one)[safe]
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    w = (torch.min(a[..., 2], b[..., 2]) - torch.max(a[..., 0], b[..., 0])).clamp(min=0)
    h = (torch.min(a[..., 3], b[..., 3]) - torch.max(a[..., 1], b[..., 1])).clamp(min=0)
    inter = w * h
    iou = inter / (area_a + area_b - inter)
    iou = torch.where(ok, iou, torch.full_like(iou, -1.0))
    best = iou.max(1).values
    col = torch.where(iou == best[:, None], torch.arange(M, device=dev)[None, :], M).min(1).values      # FIRST argmax
    arg = torch.gather(cand, 1, col.clamp(max=M - 1)[:, None])[:, 0]
    arg = torch.where(best < torch.tensor(iou_thresh, dtype=torch.float32, device=dev), torch.full_like(arg, -1), arg)
    has = arg >= 0
    winner = torch.full((G,), D, dtype=torch.int64, device=dev)
    winner.scatter_reduce_(0, arg[has], rank[has], reduce="amin")
    safe_arg = arg.clamp(min=0)
    value = torch.where(p["gt_difficult"][safe_arg], -1, (winner[safe_arg] == rank).to(torch.int64))
    out = torch.where(has, value, torch.zeros_like(value)).to(torch.int8)
    return out, order


def curves(m_sorted, seg, n_pos, L):
    """tp, fp (int64), prec, rec, mpre (fp64) over an array sorted by (segment, descending score)."""
    dev = m_sorted.device
    D = m_sorted.shape[0]
    counts = torch.bincount(seg, minlength=L)
    start = (torch.cumsum(counts, 0) - counts)[seg]
    def seg_cumsum(flag):
        c = torch.cumsum(flag.to(torch.int64), 0)
        before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), c])[start]
        return c - before
    tp, fp = seg_cumsum(m_sorted == 1), seg_cumsum(m_sorted == 0)
    prec = tp.double() / (tp + fp).double()
    rec = tp.double() / n_pos[seg].double()
    # reversed running maximum inside every segment, exactly: on (segment, dense rank of the value) integer keys
    x = torch.nan_to_num(prec, nan=0.0)
    values, dense = torch.unique(x, return_inverse=True)
    U = values.numel() + 1
    block = (L - 1 - seg) * U                       # grows along the flipped array: the maximum restarts in every segment
    key = (block + dense).flip(0)
    run = torch.cummax(key, 0).values.flip(0)
    mpre = values[run - block] if D else x
    return tp, fp, prec, rec, mpre


def average_precision(rec, mpre, seg, L, use_07_metric):
    dev = rec.device
    D = rec.shape[0]
    ap = torch.zeros(L, dtype=torch.float64, device=dev)
    if D == 0:
        return ap
    head = torch.ones(D, dtype=torch.bool, device=dev)
    head[1:] = seg[1:] != seg[:-1]
    before = torch.where(head, torch.zeros_like(rec), torch.roll(rec, 1))
    if not use_07_metric:
        term = torch.where(rec != before, (rec - before) * mpre, torch.zeros_like(rec))
        return ap.index_add_(0, seg, term)
    for t in range(11):
        level = 0.1 * t
        first = (rec >= level) & (head | ~(before >= level))
        p = torch.zeros(L, dtype=torch.float64, device=dev)
        p[seg[first]] = mpre[first]
        ap = ap + p / 11
    return ap


def evaluate(p, L, iou_thresh=0.5, use_07_metric=False):
    """Everything the reference's result dictionary holds, plus the intermediates, as tensors on p's device."""
    dev = p["boxes"].device
    m, order = match(p, iou_thresh)
    plain = p["gt_labels"][~p["gt_difficult"]]
    n_pos = torch.bincount(plain, minlength=L)[:L]
    by_class = order[torch.sort(p["labels"][order], stable=True).indices]
    seg = p["labels"][by_class]
    tp, fp, prec, rec, mpre = curves(m[by_class], seg, n_pos, L)
    nan = torch.full((L,), float("nan"), dtype=torch.float64, device=dev)
    ap = torch.where(n_pos > 0, average_precision(rec, mpre, seg, L, use_07_metric), nan)
    counts = torch.bincount(seg, minlength=L)
    last = torch.zeros(L, dtype=torch.float64, device=dev)
    ends = torch.cumsum(counts, 0) - 1
    last[counts > 0] = rec[ends[counts > 0]]
    recall_pc = torch.where(n_pos > 0, last, nan)
    total = n_pos.sum()
    zero = torch.zeros_like(seg)
    jtp, jfp, jprec, jrec, jmpre = curves(m[order], zero, total.reshape(1), 1)
    ap_joint = average_precision(jrec, jmpre, zero, 1, use_07_metric)[0] if int(total) > 0 else nan[0]
    seen = (n_pos > 0)
    return dict(match=m, order_joint=order, order_class=by_class, n_pos=n_pos, tp=tp, fp=fp, prec=prec, rec=rec, class_counts=counts,
                gt_counts=torch.bincount(p["gt_labels"], minlength=L)[:L], ap_per_class=ap, recall_per_class=recall_pc,
                map=ap[seen].sum() / seen.sum(), map_weighted=(ap[seen] * n_pos[seen].double() / total.double()).sum(),
                recall=(n_pos[seen].double() * recall_pc[seen]).sum() / total.double() if int(total) > 0 else nan[0],
                ap_joint_classes=ap_joint, tp_joint=jtp, fp_joint=jfp, prec_joint=jprec, rec_joint=jrec)
