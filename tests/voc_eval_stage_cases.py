"""Case tables of the stage tests of libos2d_eval.so, shared by tests/test_voc_eval_stage_model.py (CPU) and
tests/test_voc_eval_stages_gpu.py.  Every case is derived from the geometry of the kernels (os2d_amd/csrc_eval/eval_common.h,
sort.hip, metric.hip) and its name says which edge it sits on.  Everything is numpy, drawn from fixed seeds."""
import numpy as np

# ------------------------------------------------------------------------------------------------------------- the geometry
ITEMS = 8                      # consecutive positions of one thread in a scan (EVAL_ITEMS)
WAVE = 64 * ITEMS              # 512: positions of one wave - in the sort, the 8 runs of 64 keys a wave ranks
TILE = 256 * ITEMS             # 2,048: positions of one work-group (EVAL_TILE)
CARRY_ROUND = 256              # tiles per round of scan_carries_kernel (one per thread)
RADIX_ROUND = 4096             # counts per round of radix_scan_kernel (4 per thread, 1,024 threads)
RADIX_TILES = RADIX_ROUND // 256                          # 16 tiles fill one round: 256 digit counts per tile
SORT_SECOND_ROUND = RADIX_TILES * TILE + TILE + 1         # 34,817: 18 tiles, 4,608 counts
SCAN_SECOND_ROUND = CARRY_ROUND * TILE + TILE + 3         # 526,339: 258 tiles, two of them in the second round
EDGES = (ITEMS, WAVE, TILE)


def around(n):
    return (n - 1, n, n + 1)


# ----------------------------------------------------------------------------------------------------------------- count_gt
COUNT_G = (0, 1) + around(256) + (600,)     # none, one, the work-group size +-1, three work-groups
COUNT_L = (1, 5, 1024)
DIFFICULT_BYTES = (0, 1, 2, 255)


def count_cases():
    out = []
    for G in COUNT_G:
        for L in COUNT_L:
            rng = np.random.RandomState(1000 * L + G)
            labels = rng.randint(-1, L + 1, G)               # -1 and L: outside [0, L)
            if G >= 2:
                labels[0], labels[-1] = L, -1
            difficult = rng.choice(DIFFICULT_BYTES, G)
            out.append(dict(name="G{}_L{}_spread".format(G, L), L=L, gt_labels=labels.astype(np.int32), gt_difficult=difficult.astype(np.uint8)))
            one = np.full(G, L - 1)                          # every box on one label: contended atomics
            cyc = np.array(DIFFICULT_BYTES * (G // 4 + 1))[:G]
            out.append(dict(name="G{}_L{}_one_label".format(G, L), L=L, gt_labels=one.astype(np.int32), gt_difficult=cyc.astype(np.uint8)))
    return out


# -------------------------------------------------------------------------------------------------------------------- match
def pack_images(images):
    """images: list of (detections [[x1, y1, x2, y2, score, label]], ground truth [[x1, y1, x2, y2, label, difficult]])."""
    det = [np.asarray(d, np.float64).reshape(-1, 6) for d, _ in images]
    gt = [np.asarray(g, np.float64).reshape(-1, 6) for _, g in images]
    d, g = np.concatenate(det), np.concatenate(gt)
    return dict(det_boxes=d[:, :4].astype(np.float32), det_scores=d[:, 4].astype(np.float32), det_labels=d[:, 5].astype(np.int32),
                det_offsets=np.cumsum([0] + [len(x) for x in det]).astype(np.int32),
                gt_boxes=g[:, :4].astype(np.float32), gt_labels=g[:, 4].astype(np.int32), gt_difficult=g[:, 5].astype(np.uint8),
                gt_offsets=np.cumsum([0] + [len(x) for x in gt]).astype(np.int32))


def _m(name, images, thr, match=None, gt_index=None):
    c = pack_images(images)
    c.update(name=name, thr=float(thr), expect_match=match, expect_index=gt_index)
    return c


def up32(x):
    """The next fp32 above x."""
    return float(np.nextafter(np.float32(x), np.float32(1)))


TALL = [0, 0, 9, 19]       # 10 x 20 = 200 with the +1 convention
HALF = [0, 0, 9, 9]        # 10 x 10 = 100 inside TALL: IoU 100 / 200 = 0.5 exactly
THREEQ = [0, 0, 9, 14]     # 10 x 15 = 150 inside TALL: IoU 150 / 200 = 0.75 exactly
FAR = [100, 100, 109, 119]
BOX = [10, 10, 50, 50]
INF = float("inf")
TIE_CROWD = 300            # more than one work-group of 256 detections


def match_cases():
    out = []
    # the decision best < thr on its edge
    for box, v in ((HALF, 0.5), (THREEQ, 0.75)):
        out.append(_m("iou_equals_thr_{}".format(v), [([TALL + [0.9, 0]], [box + [0, 0]])], v, [1], [0]))
        out.append(_m("iou_one_ulp_below_thr_{}".format(v), [([TALL + [0.9, 0]], [box + [0, 0]])], up32(v), [0], [-1]))
    out.append(_m("thr_0_disjoint", [([TALL + [0.9, 0]], [FAR + [1, 0], FAR + [0, 0], BOX + [0, 0]])], 0.0, [1], [1]))
    out.append(_m("thr_1_identical", [([BOX + [0.9, 0], [10, 10, 50, 49, 0.95, 0]], [BOX + [0, 0]])], 1.0, [1, 0], [0, -1]))
    out.append(_m("thr_above_1", [([BOX + [0.9, 0]], [BOX + [0, 0]])], 1.5, [0], [-1]))
    # equal maxima: the first box
    out.append(_m("duplicate_gt_first_difficult", [([BOX + [0.9, 0], BOX + [0.8, 0]], [BOX + [0, 1], BOX + [0, 0]])], 0.5, [-1, -1], [0, 0]))
    out.append(_m("duplicate_gt_second_difficult", [([BOX + [0.9, 0], BOX + [0.8, 0]], [BOX + [0, 0], BOX + [0, 1]])], 0.5, [1, 0], [0, 0]))
    # ties for one box: descending score, then the index in the image
    gt = [BOX + [0, 0]]
    ties = dict(equal=([0.5, 0.5, 0.5], 0), zero_plus_minus=([0.0, -0.0], 0), zero_minus_plus=([-0.0, 0.0], 0),
                zero_minus_plus_late=([-1.0, -0.0, 0.0, -0.0], 1), negative=([-1.0, -0.5, -0.5], 1), infinities=([-INF, 1.0, INF, INF], 2),
                subnormal=([1e-45, 0.0, -1e-45, 1e-45], 0), subnormal_above_zero=([0.0, -0.0, 1e-45], 2),
                subnormal_below_zero=([-1e-45, -0.0, 0.0], 1))
    for name, (scores, win) in ties.items():
        expect = [1 if i == win else 0 for i in range(len(scores))]
        # a first image shifts the packed rows: the tie is decided by the index IN THE IMAGE
        out.append(_m("tie_" + name, [([FAR + [0.1, 0]], []), ([BOX + [s, 0] for s in scores], gt)], 0.5, [0] + expect, [-1] + [0] * len(scores)))
    out.append(_m("tie_crowd", [([BOX + [0.25, 0]] * TIE_CROWD, gt)], 0.5, [1] + [0] * (TIE_CROWD - 1), [0] * TIE_CROWD))
    out.append(_m("tie_crowd_difficult", [([BOX + [0.25, 0]] * TIE_CROWD, [BOX + [0, 1]])], 0.5, [-1] * TIE_CROWD, [0] * TIE_CROWD))
    # image_of: empty images at the start, in the middle, at the end; detections without ground truth and the reverse.  Every
    # image has its own place for the box, so a detection looked up in another image finds nothing.
    at = lambda n: [100 * n, 0, 100 * n + 40, 40]            # noqa: E731
    images = [([], []), ([], [at(1) + [0, 0]]), ([at(2) + [0.9, 0], at(2) + [0.9, 0]], [at(2) + [0, 0]]), ([], []), ([at(4) + [0.8, 0]], []),
              ([], [at(5) + [0, 0]]), ([at(6) + [0.7, 0], at(5) + [0.6, 0], at(6) + [0.7, 1]], [at(6) + [1, 0], at(6) + [0, 0]]), ([], []), ([], [])]
    out.append(_m("image_lookup", images, 0.5, [1, 0, 0, 1, 0, 1], [1, 1, -1, 4, -1, 3]))
    out.append(_m("label_only_in_another_image", [([BOX + [0.9, 1]], [BOX + [0, 0]]), ([], [BOX + [1, 0]])], 0.5, [0], [-1]))
    # the match step has no L: a label is only compared.  7 has a box, -1 and 1 << 20 have none.
    out.append(_m("labels_outside", [([BOX + [0.9, 7], BOX + [0.8, -1], BOX + [0.7, 1 << 20], BOX + [0.6, 0]], [BOX + [0, 0], BOX + [7, 0]])], 0.5,
                  [1, 0, 0, 1], [1, -1, -1, 0]))
    # boxes of one pixel: area 1; [5,5,6,5] has area 2 and holds [5,5,5,5]: IoU 0.5 exactly
    out.append(_m("one_pixel", [([[5, 5, 5, 5, 0.9, 0], [5, 5, 5, 5, 0.8, 1], [7, 7, 7, 7, 0.7, 0]], [[5, 5, 5, 5, 0, 0], [5, 5, 6, 5, 1, 0]])], 0.5,
                  [1, 1, 0], [0, 1, -1]))
    out.append(_m("one_pixel_above", [([[5, 5, 5, 5, 0.8, 1]], [[5, 5, 6, 5, 1, 0]])], up32(0.5), [0], [-1]))
    # shapes: one image, D around the work-group size; integer boxes and few score values: equal IoUs and equal scores abound
    for D in (1,) + around(256):
        out.append(_drawn_match("drawn_N1_D{}".format(D), 500 + D, [D], [12], 0.5))
    out.append(_drawn_match("drawn_N5", 77, [40, 0, 90, 3, 130], [6, 4, 0, 9, 5], 0.3))
    c = _drawn_match("no_ground_truth_D257", 78, [200, 57], [0, 0], 0.5)     # G = 0: null pointers
    c["expect_match"], c["expect_index"] = [0] * 257, [-1] * 257
    out.append(c)
    return out


def _drawn_match(name, seed, det_counts, gt_counts, thr):
    rng = np.random.RandomState(seed)
    images = []
    for nd, ng in zip(det_counts, gt_counts):
        xy = rng.randint(0, 12, (ng, 2)) * 4
        gt = np.concatenate([xy, xy + rng.randint(0, 6, (ng, 2)) * 4, rng.randint(0, 3, (ng, 1)), (rng.rand(ng, 1) < 0.25)], 1)
        src = gt[rng.randint(0, ng, nd)][:, :4] if ng else rng.randint(0, 40, (nd, 4))
        jit = rng.randint(-1, 2, (nd, 4)) * 4 * (rng.rand(nd, 1) < 0.6)
        boxes = src + jit
        boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2])                      # xmax >= xmin: inside the contract
        det = np.concatenate([boxes, rng.choice([0.0, -0.0, 0.25, 0.5, 0.5, 0.75, -1.0], (nd, 1)), rng.randint(0, 3, (nd, 1))], 1)
        images.append((det, gt))
    return _m(name, images, thr)


# --------------------------------------------------------------------------------------------------------------------- sort
SORT_D = (1,) + around(64) + around(WAVE) + around(TILE) + (SORT_SECOND_ROUND,)
RUN = 64


def from_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def scores_of(pattern, D, rng):
    if pattern == "all_equal":
        return np.full(D, 0.5, np.float32)
    if pattern == "two_values":
        return np.where(np.arange(D) % 2 == 0, 0.25, 0.75).astype(np.float32)
    if pattern == "lowest_byte":          # only the digit of the first pass differs
        return from_bits(0x3F000000 | rng.randint(0, 256, D))
    if pattern == "highest_byte":         # only the digit of the fourth pass differs: sign and seven exponent bits, all finite
        return from_bits((rng.randint(0, 256, D).astype(np.uint32) << 24) | 0x00400000)
    if pattern == "zeros":
        return rng.choice(np.array([0.0, -0.0], np.float32), D)
    if pattern == "infinities":
        return rng.choice(np.array([INF, -INF, 1.0, -1.0], np.float32), D)
    if pattern == "negative_subnormal":
        return rng.choice(np.array([-1.5, -1e-45, 1e-45, -3e-39, 3e-39, 0.0, -0.0, 2.0], np.float32), D)
    if pattern == "few_values":
        return rng.choice(np.linspace(-1, 1, 37).astype(np.float32), D)
    if pattern == "runs_on_edges":        # distinct scores, but 64 equal ones across a wave-run edge and 64 across a tile edge
        s = rng.permutation(D).astype(np.float32)
        s[WAVE - RUN // 2:WAVE + RUN // 2] = -5.0
        s[TILE - RUN // 2:TILE + RUN // 2] = D + 5.0
        return s
    raise KeyError(pattern)


PATTERNS = ("all_equal", "two_values", "lowest_byte", "highest_byte", "zeros", "infinities", "negative_subnormal", "few_values")


def _s(name, scores, labels, L, label_bits):
    return dict(name=name, scores=np.asarray(scores, np.float32), labels=np.asarray(labels, np.int32), L=L, label_bits=label_bits)


def bits_for(L):
    return max(L - 1, 0).bit_length()


def sort_cases():
    out = []
    for D in SORT_D:                       # every size: equal scores (stability alone), two values, many ties
        for pattern in ("all_equal", "two_values", "few_values") if D != SORT_SECOND_ROUND else ("all_equal", "lowest_byte"):
            rng = np.random.RandomState(D % 9973 + len(pattern))
            L = 257 if D == SORT_SECOND_ROUND else 5
            out.append(_s("D{}_{}".format(D, pattern), scores_of(pattern, D, rng), rng.randint(0, L, D), L, bits_for(L)))
    for D in (WAVE + 1, TILE + 1):         # every pattern past one wave and past one tile
        for pattern in PATTERNS:
            rng = np.random.RandomState(D + 7 * len(pattern))
            out.append(_s("D{}_{}".format(D, pattern), scores_of(pattern, D, rng), rng.randint(0, 5, D), 5, 3))
    D = TILE + WAVE + 1
    rng = np.random.RandomState(3)
    out.append(_s("D{}_runs_on_edges".format(D), scores_of("runs_on_edges", D, rng), rng.randint(0, 2, D), 2, 1))
    # the label passes
    D = TILE + 1
    rng = np.random.RandomState(4)
    scores = scores_of("few_values", D, rng)
    out.append(_s("L1_bits0", scores, np.zeros(D), 1, 0))
    out.append(_s("L256_bits8", scores, rng.randint(0, 256, D), 256, 8))
    out.append(_s("L257_bits9", scores, rng.choice([0, 1, 255, 256], D), 257, 9))
    out.append(_s("L65537_bits17", scores, rng.choice([0, 1, 255, 256, 257, 511, 65535, 65536], D), 65537, 17))
    for name, absent in (("start", (0, 1)), ("middle", (2, 3)), ("end", (5, 6)), ("all_but_one", (0, 1, 2, 3, 5, 6))):
        present = [l for l in range(7) if l not in absent]
        out.append(_s("labels_absent_" + name, scores[:70], rng.choice(present, 70), 7, 3))
    return out


def pass_count_cases():
    """L = 5 with label_bits 3, 9, 17, 25: one to four label passes must give the same outputs."""
    D = TILE + 1
    scores, labels = scores_of("few_values", D, np.random.RandomState(5)), np.random.RandomState(6).randint(0, 5, D)
    return [_s("L5_bits{}".format(b), scores, labels, 5, b) for b in (3, 9, 17, 25)]


# More work-groups than the device holds at once (256 compute units x 8 work-groups of four waves), three times over: a
# label pass that read and wrote ONE index buffer is harmless while every work-group reads before any writes, and shows
# only here.  Equal scores and the label MANY_LABELS[i % 6] (all three digits permute): the orders are known in closed form.
MANY_TILES_D = 3 * 256 * 8 * TILE + 1
MANY_LABELS = (0, 256, 65536, 1, 257, 512)
MANY_L = 65537


def many_tiles_order(D):
    """perm_class of the many-tiles case as per-residue (first row, label) in output order: rows first, first + 6, .."""
    return [(r, MANY_LABELS[r]) for r in sorted(range(6), key=lambda r: MANY_LABELS[r])]


def nan_case():
    rng = np.random.RandomState(8)
    D = WAVE + 1
    scores = scores_of("few_values", D, rng)
    scores[rng.rand(D) < 0.2] = np.nan
    scores[::97] = -np.float32(np.nan)
    return _s("nan_scores", scores, rng.randint(0, 5, D), 5, 3)


def out_of_range_case():
    """L = 5; labels 0 .. 4 plus 256, 261, 65536 + 2 and -1 whose low bytes are 0, 5, 2 and 255, with scores interleaved with
    those of the classes 0 and 2.  Written out so that the expected outputs can be too."""
    rows = [(0.90, 0), (0.85, 256), (0.80, 0), (0.75, 2), (0.70, 65538), (0.65, 2), (0.60, 1), (0.55, -1), (0.50, 0), (0.45, 261),
            (0.40, 3), (0.35, 4), (0.30, 256), (0.25, 0), (0.20, 65538), (0.15, 2), (0.10, 4), (0.05, -1)]
    order = [7, 2, 11, 0, 16, 5, 9, 14, 1, 3, 17, 12, 4, 8, 10, 6, 13, 15]       # packed order: not sorted by anything
    rows = [rows[i] for i in order]
    c = _s("out_of_range_labels", [r[0] for r in rows], [r[1] for r in rows], 5, 3)
    # match by hand: class 0 hits (1), misses (0); class 2 hits; one difficult (-1); the rows outside are 0, as match_kernel
    # leaves a detection whose label has no ground truth
    hand = {0.90: 1, 0.80: 0, 0.50: 1, 0.25: 0, 0.75: 0, 0.65: 1, 0.15: -1, 0.60: 1, 0.40: 0, 0.35: 1, 0.10: 0}
    c["match"] = np.array([hand.get(round(float(s), 2), 0) for s in c["scores"]], np.int8)
    c["n_pos"] = np.array([3, 1, 2, 0, 1, 7], np.int32)
    return c


# ------------------------------------------------------------------------------------------------------------ prec_rec and ap
SCAN_D = (1,) + around(ITEMS) + around(WAVE) + around(TILE) + (2 * TILE + 1, SCAN_SECOND_ROUND)
SEGMENT_LENGTHS = tuple(n for e in EDGES for n in around(e))      # 7, 8, 9, 511, 512, 513, 2047, 2048, 2049


def segments(lengths, D):
    """seg [D] from a cycle of segment lengths: segment k has label k - 1 and L = segments - 3 when there are at least four
    (the first label is -1, the last two are L and L + 1: outside [0, L)), else label k and L = segments."""
    ends, k, total = [], 0, 0
    while total < D:
        ends.append(lengths[k % len(lengths)])
        total += ends[-1]
        k += 1
    seg = np.repeat(np.arange(len(ends)), ends)[:D]
    n = len(ends)
    return (seg - 1, n - 3) if n >= 4 else (seg, n)


def scan_case(name, D, lengths, seed):
    """lengths: None = seg NULL (one segment, L = 1).  Segment k: k % 4 == 1 begins with a run of -1 (prec NaN until the first
    0 or 1), k % 4 == 2 holds -1 only, k % 5 == 3 has n_pos 0 (rec NaN, then inf)."""
    rng = np.random.RandomState(seed)
    m = rng.choice(np.array([-1, 0, 0, 1, 1], np.int8), D)
    if lengths is None:
        seg, L = None, 1
        labels = np.zeros(D, np.int64)
        m[:min(3, D - 1)] = -1
    else:
        seg, L = segments(lengths, D)
        labels = seg - seg[0]
        start = np.concatenate([[0], np.flatnonzero(np.diff(labels)) + 1, [D]])
        for k in range(len(start) - 1):
            a, b = start[k], start[k + 1]
            if k % 4 == 1:
                m[a:a + max(1, (b - a) // 2)] = -1
            elif k % 4 == 2:
                m[a:b] = -1
    n_pos = np.zeros(L, np.int32)
    hits = np.bincount(labels[m == 1], minlength=int(labels[-1]) + 1)
    for k in range(int(labels[-1]) + 1):
        s = k + (0 if seg is None else int(seg[0]))
        if 0 <= s < L:
            n_pos[s] = 0 if k % 5 == 3 else int(hits[k]) + k % 3 + (1 if hits[k] == 0 else 0)
    perm = rng.permutation(D).astype(np.uint32)
    match = np.empty(D, np.int8)
    match[perm] = m
    return dict(name=name, D=D, L=L, seg=None if seg is None else seg.astype(np.int32), n_pos=n_pos, match=match, perm=perm)


SPAN = 3 * TILE + ITEMS + 1     # a segment over three whole tiles, then segments of length 1: tiles 1 and 2 hold no segment
#                                 start, tile 3 starts one at its first position


def scan_cases(D):
    """The layouts at one D of SCAN_D."""
    out = [scan_case("D{}_one_segment".format(D), D, None, D)]
    if D == SCAN_SECOND_ROUND:      # the carry of a segment crosses the rounds of scan_carries_kernel; then every edge length
        out.append(scan_case("D{}_long_then_edges".format(D), D, (CARRY_ROUND * TILE + 5,) + SEGMENT_LENGTHS, 11))
        return out
    out.append(scan_case("D{}_every_position".format(D), D, (1,), D + 1))
    for n in SEGMENT_LENGTHS:
        if n < D + 1:
            out.append(scan_case("D{}_segments_of_{}".format(D, n), D, (n,), D + n))
    return out


def span_case():
    return scan_case("D{}_three_tiles_then_singles".format(SPAN), SPAN, (3 * TILE,) + (1,) * (ITEMS + 1), 12)


def scan_table():
    return [c for D in SCAN_D for c in scan_cases(D)] + [span_case(), ap07_levels_case()]


_REFERENCE = {}


def scan_reference(c):
    """The stage model's prec_rec and both forms of ap for a scan case, computed once and shared by every test; read only."""
    import voc_eval_stage_model as S
    if c["name"] not in _REFERENCE:
        tp, fp, prec, rec, last = S.prec_rec(c["match"], c["perm"], c["seg"], c["n_pos"], c["L"])
        for a in (tp, fp, prec, rec):
            a.setflags(write=False)
        _REFERENCE[c["name"]] = dict(tp=tp, fp=fp, prec=prec, rec=rec, last=last, ap=S.ap(prec, rec, c["seg"], c["L"], False),
                                     ap07=S.ap(prec, rec, c["seg"], c["L"], True))
    return _REFERENCE[c["name"]]


def ap07_levels_case():
    """Class 0: n_pos 10, three hits - 3 / 10.0 >= 0.1 * 3 is false in fp64, so the levels 3 .. 10 stay 0.  Class 1: n_pos 2,
    one hit: 1 / 2.0 == 0.1 * 5 exactly, level 5 is reached.  Class 2: n_pos 3, no hit: only level 0."""
    m = np.array([1, 0, 1, 1, 0, 0, 1, 0, 0, 0], np.int8)
    seg = np.array([0, 0, 0, 0, 0, 1, 1, 1, 2, 2], np.int32)
    return dict(name="ap07_levels", D=10, L=3, seg=seg, n_pos=np.array([10, 2, 3], np.int32), match=m, perm=np.arange(10, dtype=np.uint32))


# ----------------------------------------------------------------------------------------------------------------- finalise
FINALISE_L = (1,) + around(256) + (1024,)      # one class; the work-group size +-1 (a thread takes l, l + 256, ..); four each


def finalise_cases():
    out = []
    for L in FINALISE_L:
        for kind in ("no_positives", "one_class", "mixed"):
            rng = np.random.RandomState(L + len(kind))
            n_pos = np.zeros(L + 1, np.int32)
            if kind == "one_class":
                n_pos[L // 2] = 7
            elif kind == "mixed":
                n_pos[:L] = rng.randint(0, 4, L) * rng.randint(1, 50, L)
                n_pos[L - 1] = 3
            n_pos[L] = n_pos[:L].sum()
            acc = rng.rand(L + 1, 11)
            hits = rng.randint(0, 1 << 20, L + 1) % (n_pos + 1)
            with np.errstate(invalid="ignore"):
                rec_last = np.nan_to_num(hits / n_pos.astype(np.float64))
            if kind == "mixed":          # classes with positives and no detection: the zeros the caller wrote
                quiet = rng.rand(L + 1) < 0.3
                quiet[L - 1], quiet[L] = True, False
                acc[quiet], rec_last[quiet] = 0.0, 0.0
            out.append(dict(name="L{}_{}".format(L, kind), L=L, n_pos=n_pos, acc=acc, rec_last=rec_last))
    return out
