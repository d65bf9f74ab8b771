"""Case tables of the detection stage suite (tests/test_detect_stage_model.py on the CPU, tests/test_detect_stages_gpu.py on the
GPU), each case with the regime of the kernels it exists for; tests/detect_stage_model.py tells whether a case reaches it.
Plain NumPy, nothing of os2d_amd.

Box families
  grid     loc[2:] = 5 ln(8/240): 8-px boxes on the stride-16 anchor centres, disjoint from every neighbour.
  twins    the same box moved 1 px in x: IoU 56/72 with its original, 0 with everything else.  In another view of a merged label
           the twin sits at the original's location (loc[0] = 10/240); inside one level it sits at the location to the right
           (loc[0] = 10 * (1 - 16) / 240).  The twin's score puts it a chosen number of ranks behind its original.
  random   target boxes inside a 256-px square, sides of 8 - 64 px (8 - 16 px beyond 128 locations), written as loc of whatever
           anchor the location has.

For every case that goes through a decoding kernel no tested pair's float64 IoU may lie within BAND of the threshold and no
valid box may have a side under MIN_SIDE (so that "empty" is the same in float32): a random case takes the first seed for which
both hold, recorded in SEEDS.  Nothing is ever excluded from a comparison.
"""
import functools
import math

import numpy as np

import detect_stage_model as DM

F32 = np.float32
BAND = 1e-4
MIN_SIDE = 1e-2
EXCLUDED = 0                                   # candidates or pairs left out of a comparison: none, ever
INF = float("inf")
LN8 = F32(5.0 * math.log(8.0 / 240.0))
TWIN_VIEW = F32(10.0 / 240.0)                  # loc[0] of a twin at its original's location
TWIN_RIGHT = F32(10.0 * (1 - 16) / 240.0)      # loc[0] of a twin at the location right of its original
SUB = float(np.frombuffer(np.uint32(1).tobytes(), F32)[0])          # smallest subnormal
NEG_NAN = float(np.frombuffer(np.uint32(0xFFC00000).tobytes(), F32)[0])
LEVEL_MAX_HW = 6115       # 6 * 8192 + align16(2 HW) + 16 HW + 4608 <= 160 KiB; the GPU test asks os2d_detect_level_supported
FINALIZE_SORT = 16384     # os2d_hip.h: a multi-chunk result beyond it is reported unfinished

# first seeds that keep BAND and MIN_SIDE (tests/test_detect_stage_model.py::test_seeds recomputes every one)
SEEDS = {("level", "hw1024"): 5, ("level", "hw1025"): 2, ("pyramid", "n1023"): 7, ("pyramid", "n1024"): 14, ("pyramid", "n1025"): 2,
         # every other seeded case: seed 0.  The four labels of the pyramid case "passes" (first_pass_seed):
         ("passes", 0): 96, ("passes", 1): 1000, ("passes", 2): 2001, ("passes", 3): 3000}


def shape_for(n):
    h = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    return h, n // h


def scale_ops(sx, sy):
    return [(DM.OP_SCALE, sx, sy)]


def make_level(H, W, loc, cls, ops=None, dops=None, corners=None, img=None):
    ops = scale_ops(1.0, 1.0) if ops is None else ops
    img = (16 * W, 16 * H) if img is None else img
    return {"H": H, "W": W, "loc": np.ascontiguousarray(loc, F32), "cls": np.ascontiguousarray(cls, F32), "ops": ops,
            "dops": ops if dops is None else dops, "corners": None if corners is None else np.ascontiguousarray(corners, F32),
            "img_w": float(img[0]), "img_h": float(img[1])}


def grid_loc(B, HW):
    loc = np.zeros((B, 4, HW), F32)
    loc[:, 2:] = LN8
    return loc


def rank_scores(times):
    """Scores that sort the entries by ascending ``times``: 1 - rank 2^-16, distinct and exact in float32."""
    rank = np.empty(len(times), np.int64)
    rank[np.argsort(times, kind="stable")] = np.arange(len(times))
    assert len(times) < 65536
    return (1.0 - rank * 2.0 ** -16).astype(F32)


GAPS = (0, 100, 1500)     # ranks of originals between an original and its twin: resolve, vote, earlier batch


def twin_level(H, W, every=4, seed=1):
    """A grid level whose pairs of locations (2k, 2k+1) of a row are two grid boxes, or - every ``every``-th pair - an original
    and its twin, the twin GAPS[..] originals behind.  Returns loc [1,4,HW], cls [1,HW], number of twins."""
    HW = H * W
    loc = grid_loc(1, HW)
    order = np.random.RandomState(seed).permutation(HW).astype(np.float64)       # rank of every location without twins
    times = order.copy()
    twins = 0
    for h in range(H):
        for k in range(W // 2):
            left = h * W + 2 * k
            pair = h * (W // 2) + k
            if pair % every == 0:
                loc[0, 0, left + 1] = TWIN_RIGHT
                times[left + 1] = order[left] + GAPS[(pair // every) % len(GAPS)] + 0.5
                twins += 1
    return loc, rank_scores(times)[None], twins


def random_level(rs, B, H, W, lo=-1.0):
    """Random overlap: target boxes inside [0, 256)^2, sides 8 - 64 px (8 - 16 px beyond 128 locations); the level's image is at
    least 256 px."""
    HW = H * W
    a = DM.anchors(H, W)
    acx, acy = 0.5 * (a[:, 0] + a[:, 2]), 0.5 * (a[:, 1] + a[:, 3])
    w, h = rs.uniform(8, 64 if HW <= 128 else 16, (2, B, HW))      # many boxes: small ones, or no seed keeps the band empty
    cx, cy = rs.uniform(0, 1, (2, B, HW)) * (256 - np.stack([w, h])) + 0.5 * np.stack([w, h])
    loc = np.stack([10 * (cx - acx) / 240, 10 * (cy - acy) / 240, 5 * np.log(w / 240), 5 * np.log(h / 240)], 1).astype(F32)
    cls = rs.uniform(lo, 1, (B, HW)).astype(F32)
    return loc, cls, (max(16 * W, 256), max(16 * H, 256))


# ------------------------------------------------------------------------------------------------------------------ os2d_nms
def grid_box(i, dx=0.0, cols=64):
    x, y = 16.0 * (i % cols) + 4 + dx, 16.0 * (i // cols) + 4
    return [x, y, x + 8, y + 8]


def nms_list_across_2048():
    """One sorted list: 2040 originals and 8 twins in the first 2048 places (4 twins right behind their original, 4 of them 70
    places behind), then 64 disjoint boxes - the kept count goes 2040 -> 2104 inside the step at 2048 -, then originals whose
    kept rank is beyond 2048 with twins next to them and 70 places behind, and twins of two early originals at the very end."""
    items = [(float(k), k, 0.0) for k in range(2300)]
    for k in (5, 200, 400, 600, 2110, 2150, 2190, 2230):
        items.append((k + 0.5, k, 1.0))
    for k in (20, 220, 420, 620, 2105, 2140, 2180, 2220):
        items.append((k + 70.5, k, 1.0))
    for k in (1000, 1500):
        items.append((5000.0 + k, k, 1.0))
    items.sort()
    return np.array([grid_box(k, dx) for _, k, dx in items], F32)


def _nms_cases():
    rs = np.random.RandomState(11)
    N = 130
    ctr, wh = rs.uniform(0, 120, (8, N, 2)), rs.uniform(8, 40, (8, N, 2))
    cases = {"counts": {"boxes": np.concatenate([ctr - wh / 2, ctr + wh / 2], -1).astype(F32),
                        "counts": [0, 1, 63, 64, 65, N, N + 1, 100000], "iou_thr": 0.3}}
    a = nms_list_across_2048()
    cases["across_2048"] = {"boxes": np.stack([a, a, a]), "counts": [len(a), 2112, 2047], "iou_thr": 0.3}
    touch = np.array([[0, 0, 8, 8], [8, 0, 16, 8], [16, 8, 24, 16], [0, 8, 8, 16], [4, 4, 12, 12], [40, 40, 48, 48],
                      [47.5, 40, 56, 48], [100, 100, 108, 108]], F32)
    cases["iou_thr_0"] = {"boxes": touch[None], "counts": [8], "iou_thr": 0.0}
    same = np.array([[0, 0, 8, 8], [0, 0, 8, 8], [3, 3, 20, 9], [3, 3, 20, 9], [0, 0, 8, 8.5]], F32)
    cases["iou_thr_1"] = {"boxes": same[None], "counts": [5], "iou_thr": 1.0}
    flat = np.array([[5, 5, 5, 5], [5, 5, 5, 5], [3, 3, 3, 9], [3, 3, 3, 9], [0, 0, 8, 8], [0, 0, 8, 8]], F32)
    cases["zero_area"] = {"boxes": np.stack([flat, flat]), "counts": [6, 2], "iou_thr": 0.3}
    return cases


NMS_CASES = _nms_cases()


@functools.lru_cache(maxsize=None)
def nms_model(name):
    """Per list of the case: (keep mask, ChunkRun)."""
    c = NMS_CASES[name]
    return [DM.nms_sorted_list(b, n, c["iou_thr"]) for b, n in zip(c["boxes"], c["counts"])]


# ------------------------------------------------------------------------------------------------- os2d_detect_level[_ops]
LEVEL_HW = (1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025)
SIX_OPS = [(DM.OP_SCALE, 1.5, 0.75), (DM.OP_HFLIP, 384.0, 0.0), (DM.OP_SHIFT, 10.0, -7.0), (DM.OP_VFLIP, 0.0, 192.0),
           (DM.OP_SCALE, 2.0, 1.25), (DM.OP_SHIFT, -3.0, 4.0)]


def score_table():
    """16 scores on a 4x4 grid level, twins at locations 1, 5 and 11 (of 0, 4 and 10).  At threshold -inf: NaN, -NaN and -inf are
    not valid; +0 and -0 tie, so location 0 (-0) is met before its twin 1 (+0) and the twin dies; 11 is the next float above
    10's 0.5, so the twin wins there.  At threshold 0 the smallest subnormal is valid, zero and the negative subnormal are not;
    at 0.5 a score equal to the threshold is not valid, the next float above it is."""
    s = [-0.0, 0.0, 0.0, -0.0, float("nan"), INF, INF, -INF, SUB, -SUB, 0.5, float(np.nextafter(F32(0.5), F32(1))),
         NEG_NAN, 1.0, -1.0, 0.25]
    loc = grid_loc(1, 16)
    loc[0, 0, [1, 5, 11]] = TWIN_RIGHT
    return loc, np.array(s, F32)[None]


SCORE_THRESHOLDS = (-INF, 0.0, 0.5)
TABLE_VALID = {-INF: 13, 0.0: 7, 0.5: 4}      # locations with a valid score, by the table's docstring


def _level_case(name, seed):
    """-> dict api ('scale' | 'ops'), level (make_level), B, score_thr, iou_thr."""
    rs = np.random.RandomState(seed)
    if name.startswith("hw"):
        n = int(name[2:])
        H, W = shape_for(n)
        loc, cls, img = random_level(rs, 2, H, W)
        api = "ops" if n % 2 else "scale"
        ops = SIX_OPS[:3] if api == "ops" else scale_ops(0.5, 0.75)
        return {"api": api, "level": make_level(H, W, loc, cls, ops, img=img), "score_thr": -0.5, "iou_thr": 0.3}
    if name == "max_level":
        loc, cls, _ = twin_level(1, LEVEL_MAX_HW)
        return {"api": "scale", "level": make_level(1, LEVEL_MAX_HW, loc, cls), "score_thr": -INF, "iou_thr": 0.3}
    if name == "valid_counts":
        loc, cls, img = random_level(rs, 6, 9, 9, lo=0.01)
        cls[0] = -cls[0]
        cls[0, ::3] = 0.0                       # class 0: everything at or under the threshold of 0
        loc[1, 2 + (np.arange(81) % 2), np.arange(81)] = -10000.0       # class 1: every box has a zero side
        cls[2] = np.nan                         # class 2
        for b, n in ((3, 1), (4, 64), (5, 65)):
            cls[b, rs.permutation(81)[n:]] *= -1
        return {"api": "scale", "level": make_level(9, 9, loc, cls, img=img), "score_thr": 0.0, "iou_thr": 0.3,
                "valid": [0, 0, 0, 1, 64, 65]}
    if name == "kcap_3x3":
        loc = grid_loc(3, 9)
        cls = np.stack([rank_scores(rs.permutation(9)), rank_scores([0, 1, 2, 3, 4, 5, 6, 8, 7]), rank_scores([0, 1, 2, 3, 4, 5, 6, 7, 8])])
        loc[1, 0, 7] = TWIN_RIGHT               # class 1: the twin of location 6, whose kept rank is 6 >= kcap = 4
        loc[2, 0, 1] = TWIN_RIGHT               # class 2: the twin of location 0, kept rank 0
        return {"api": "scale", "level": make_level(3, 3, loc, cls), "score_thr": -INF, "iou_thr": 0.3}
    if name == "level_60x80":
        loc, cls, _ = twin_level(60, 80)
        return {"api": "ops", "level": make_level(60, 80, loc, cls, []), "score_thr": -INF, "iou_thr": 0.3}
    if name.startswith("table"):
        loc, cls = score_table()
        return {"api": "scale", "level": make_level(4, 4, loc, cls), "score_thr": SCORE_THRESHOLDS[int(name[5:])], "iou_thr": 0.3}
    if name in ("chain_6", "chain_0"):
        loc, cls, img = random_level(np.random.RandomState(seed), 3, 6, 7)
        cls[1] -= 0.5
        cls[2] -= 0.9
        return {"api": "ops", "level": make_level(6, 7, loc, cls, SIX_OPS if name == "chain_6" else [], img=img),
                "score_thr": 0.0, "iou_thr": 0.3}
    raise KeyError(name)


LEVEL_CASES = ["hw%d" % n for n in LEVEL_HW] + ["max_level", "valid_counts", "kcap_3x3", "level_60x80", "table0", "table1",
                                                 "table2", "chain_6", "chain_0"]
LEVEL_SEEDED = ["hw%d" % n for n in LEVEL_HW] + ["valid_counts", "chain_6", "chain_0"]


# -------------------------------------------------------------------------------------------------------- os2d_detect_pyramid*
PYRAMID_N = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
CHUNK_M = 20
PASSES = 2                # passes launched by the case "passes"
PASS_GOALS = ((1, None), (2, "nothing removed"), (PASSES, None), (PASSES + 1, None))     # per label: passes needed, how it ended


def merged_twin_views(H, W, seed=2):
    """Two head rows of one label on an HxW grid level: row 1 holds the twin of every box of row 0, GAPS[..] originals behind."""
    HW = H * W
    loc = grid_loc(2, HW)
    loc[1, 0] = TWIN_VIEW
    order = np.random.RandomState(seed).permutation(HW).astype(np.float64)
    times = np.concatenate([order, order + np.array(GAPS)[np.arange(HW) % len(GAPS)] + 0.5])
    return loc, rank_scores(times).reshape(2, HW)


def _corners(rs, B, HW):
    return rs.uniform(0, 300, (B, 8, HW)).astype(F32)


def _pyramid_case(name, seed):
    """-> dict api ('plain' | 'merged' | 'ops'), levels, B (head rows), slot_rows (None: every row its own label), score_thr,
    iou_thr, M (nms_max_batch), passes."""
    rs = np.random.RandomState(seed)
    base = {"api": "plain", "slot_rows": None, "score_thr": -INF, "iou_thr": 0.3, "M": 10000, "passes": 3, "B": 2}

    def rand_levels(B, shapes, ops=None, corners=False, lo=-1.0):
        out = []
        for H, W in shapes:
            loc, cls, img = random_level(rs, B, H, W, lo)
            out.append(make_level(H, W, loc, cls, ops, corners=_corners(rs, B, H * W) if corners else None, img=img))
        return out
    if name.startswith("n"):
        n = int(name[1:])
        return dict(base, levels=rand_levels(2, [shape_for(n)], scale_ops(0.5, 0.75), corners=n % 2 == 1))
    if name == "levels_2":
        return dict(base, levels=rand_levels(2, [(5, 6), (3, 4)]))
    if name == "levels_16":
        return dict(base, levels=rand_levels(2, [(1 + l % 4, 1 + l // 4) for l in range(16)], corners=True))
    if name == "chunks_m":
        lv = rand_levels(3, [(8, 8)], lo=0.01)
        for b, n in enumerate((CHUNK_M, CHUNK_M + 1, 2 * CHUNK_M)):
            lv[0]["cls"][b, rs.permutation(64)[n:]] *= -1
        return dict(base, levels=lv, B=3, score_thr=0.0, M=CHUNK_M, passes=8, valid=[CHUNK_M, CHUNK_M + 1, 2 * CHUNK_M])
    if name == "chunks_64":
        cls = rank_scores(rs.permutation(512))[None]
        return dict(base, levels=[make_level(16, 32, grid_loc(1, 512), cls)], B=1, M=8, passes=2)
    if name == "merged_twins":
        loc, cls = merged_twin_views(48, 64)
        return dict(base, api="merged", levels=[make_level(48, 64, loc, cls)], slot_rows=[[0, 1]], passes=2)
    if name == "single_72x96":
        loc, cls, _ = twin_level(72, 96)
        return dict(base, levels=[make_level(72, 96, loc, cls)], B=1, passes=2)
    if name == "passes":
        levels = []
        loc, cls = np.zeros((4, 4, 64), F32), np.zeros((4, 64), F32)
        for b in range(4):
            l1, c1, img = random_level(np.random.RandomState(SEEDS.get(("passes", b), seed)), 1, 8, 8)
            loc[b], cls[b] = l1[0], c1[0]
        levels.append(make_level(8, 8, loc, cls, img=img))
        return dict(base, levels=levels, B=4, M=16, passes=PASSES)
    if name in ("finalize_16384", "finalize_16512"):
        H = 128 if name == "finalize_16384" else 129
        cls = (1.0 - rs.permutation(H * 128) * 2.0 ** -16).astype(F32)[None]
        return dict(base, levels=[make_level(H, 128, grid_loc(1, H * 128), cls)], B=1, M=8192 + (H == 129), passes=2)
    if name == "merged_ragged":
        lv = rand_levels(6, [(4, 5), (2, 3)], scale_ops(0.75, 0.5), corners=True)
        for l in lv:                                    # row 1 repeats row 0: equal scores in two rows of a label, equal boxes
            l["loc"][1], l["cls"][1] = l["loc"][0], l["cls"][0]
            l["cls"][5] = np.round(l["cls"][4] * 4) / 4  # rows 4 and 5: many equal scores within and across the rows
            l["cls"][4] = l["cls"][5][::-1]
        return dict(base, api="merged", levels=lv, B=6, slot_rows=[[0, 1, 2], [3, -1, -1], [-1, 4, 5]])
    if name.startswith("table"):
        loc, cls = score_table()
        loc2, cls2 = np.concatenate([loc, loc]), np.concatenate([cls, np.roll(cls, 8, 1)])
        lv = [make_level(2, 4, loc2[:, :, :8], cls2[:, :8]), make_level(2, 4, loc2[:, :, 8:], cls2[:, 8:], scale_ops(2.0, 2.0))]
        return dict(base, api="merged", levels=lv, slot_rows=[[0, 1]], score_thr=SCORE_THRESHOLDS[int(name[5:])])
    if name in ("chains", "chains_no_corners", "chains_merged"):
        lv = rand_levels(2, [(4, 6), (3, 3)], corners=name != "chains_no_corners")
        lv[0]["ops"], lv[0]["dops"] = SIX_OPS, [(DM.OP_HFLIP, 256.0, 0.0), (DM.OP_VFLIP, 0.0, 256.0), (DM.OP_SCALE, 1.5, 0.75)]
        lv[1]["ops"] = [(DM.OP_VFLIP, 0.0, 256.0), (DM.OP_HFLIP, 256.0, 0.0), (DM.OP_SCALE, 3.0, 0.9375), (DM.OP_SHIFT, 10.0, -7.0)]
        lv[1]["dops"] = lv[1]["ops"] * 3
        return dict(base, api="ops", levels=lv, slot_rows=[[1, 0]] if name == "chains_merged" else None)
    raise KeyError(name)


PYRAMID_CASES = (["n%d" % n for n in PYRAMID_N] + ["levels_2", "levels_16", "chunks_m", "chunks_64", "merged_twins", "single_72x96",
                                                    "passes", "finalize_16384", "finalize_16512", "merged_ragged", "table0", "table1",
                                                    "table2", "chains", "chains_no_corners", "chains_merged"])
PYRAMID_SEEDED = (["n%d" % n for n in PYRAMID_N] + ["levels_2", "levels_16", "chunks_m", "merged_ragged", "chains", "chains_no_corners",
                                                     "chains_merged"])


# ------------------------------------------------------------------------------------------------------------------ access
def build(kind, name, seed=None):
    seed = SEEDS.get((kind, name), 0) if seed is None else seed
    c = _level_case(name, seed) if kind == "level" else _pyramid_case(name, seed)
    c["name"], c["kind"], c["seed"] = name, kind, seed
    if kind == "level":
        c["B"] = c["level"]["loc"].shape[0]
    return c


def labels_of(c):
    """Rows of every label of a case."""
    if c["kind"] == "level":
        return [[b] for b in range(c["B"])]
    return [list(r) for r in c["slot_rows"]] if c["slot_rows"] is not None else [[b] for b in range(c["B"])]


def run_model(c):
    levels = [c["level"]] if c["kind"] == "level" else c["levels"]
    M = c["level"]["H"] * c["level"]["W"] + 1 if c["kind"] == "level" else c["M"]          # a level is always one chunk
    return [DM.detect_label(levels, rows, c["score_thr"], c["iou_thr"], M) for rows in labels_of(c)]


def clean(results):
    """The two conditions a seed has to meet: an empty band around the IoU threshold, no valid box with a side near zero."""
    for r in results:
        b = r["cand"]["boxes64"][r["cand"]["valid"]]
        sides = np.concatenate([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]])
        if r["band"] < BAND or (sides.size and sides.min() < MIN_SIDE):
            return False
    return True


def first_seed(kind, name, limit=512):
    for seed in range(limit):
        if clean(run_model(build(kind, name, seed))):
            return seed
    raise AssertionError("no seed under {} for {} {}".format(limit, kind, name))


def first_pass_seed(b, limit=4096):
    """First seed from 1000 b on (every label its own range) whose 8x8 random row needs PASS_GOALS[b] passes at nms_max_batch 16
    (and keeps the band)."""
    want, ended = PASS_GOALS[b]
    for seed in range(1000 * b, 1000 * b + limit):
        loc, cls, img = random_level(np.random.RandomState(seed), 1, 8, 8)
        r = DM.detect_label([make_level(8, 8, loc, cls, img=img)], [0], -INF, 0.3, 16)
        if r["passes"] == want and (ended is None or r["ended"] == ended) and clean([r]):
            return seed
    raise AssertionError("no seed for label {} of the case passes".format(b))


@functools.lru_cache(maxsize=None)
def case(kind, name):
    return build(kind, name)


@functools.lru_cache(maxsize=None)
def model(kind, name):
    """The model's result for every label of the case, computed once per process."""
    return run_model(case(kind, name))


def window(c):
    """COVERAGE ONLY: the staging window of pyr_chunk_nms_kernel for the case (a quarter of the sort size it is launched with)."""
    n = sum(l["H"] * l["W"] for l in c["levels"]) * (len(c["slot_rows"][0]) if c["slot_rows"] is not None else 1)
    p = 8
    while p < min(c["M"], n):
        p *= 2
    return max(64, p) // 4


def expect_unfinished(c, r):
    """What os2d_hip.h promises: a label that needs more passes than were launched, or whose multi-chunk result is beyond the
    final sort, comes back with out_count = -1."""
    return r["passes"] > c["passes"] or (r["final_chunks"] > 1 and len(r["order"]) > FINALIZE_SORT)
