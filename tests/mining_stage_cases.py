"""Case tables of the mining stage suite (tests/test_mining_stage_model.py and tests/test_mining_crop_host.py on the CPU,
tests/test_mining_stages_gpu.py on the GPU), each case named after the regime of os2d_train_crop_boxes / os2d_train_mine_select it
exists for; tests/mining_stage_model.py tells whether a case reaches it.  Plain NumPy, nothing of os2d_amd, no torch.

Geometries   GEOMETRIES: one level each - stride and box, feature map, image (a multiple of the stride or not), crop, and the
             level's transform as a list of steps ("resize", w, h) / ("hflip",) / ("vflip",) / ("crop", x0, y0, x1, y1) in the order
             they are applied (chain_ops turns them into the kernel's (kind, ax, ay) chain the way BoxList.resize / transpose / crop
             compute their parameters).
Selection    SELECT_CASES: a pyramid with per-level [A,B,HW] cls_loss / loc_loss / flags / cls_preds (and corners [A,B,8,HW] or
             None), K and the IoU threshold.  The "disjoint" geometry is crop 16x16 on stride 16 with images that are multiples of
             the stride: the window of anchor (y, x) is its own cell, every IoU of two different windows is 0.

Band rule: for every case the smallest |IoU - thr| (float64) over the (kept window, tested window) pairs that the loop model
evaluates is at least BAND.  The only exceptions are the cases of EXACT (an IoU exactly at the threshold, iou_thr 0 and 1): there
every operand of every IoU evaluated is an integer below 2^24, so the float32 quotient is the correctly rounded quotient of two
exact numbers.  A seeded case takes the first seed that keeps the band (SEEDS; the CPU test recomputes them).  Nothing is ever
excluded from a comparison: no candidate, no pair, no role."""
import functools

import numpy as np

import mining_stage_model as SM

F32 = np.float32
BAND = 1e-4                                    # the BAND of tests/detect_stage_cases.py
EXCLUDED = 0                                   # candidates, pairs or roles left out of a comparison: none, ever
SUB = float(np.frombuffer(np.uint32(1).tobytes(), F32)[0])          # smallest subnormal
FLT_MAX = float(np.finfo(F32).max)
INF, NAN = float("inf"), float("nan")
NEG_NAN = float(np.frombuffer(np.uint32(0xFFC00000).tobytes(), F32)[0])
PAD_FLAGS, PAD_SCORE = 7, 1e30                 # what the padding of a strided row holds: a candidate of every role that would win
FILL = 0x7F                                    # byte the output buffers are filled with before a run
MAX_K, MAX_LEVELS, MAX_OPS = 64, 8, 6          # OS2D_MINE_MAX_K, OS2D_MINE_MAX_LEVELS, OS2D_BOX_MAX_OPS


# ------------------------------------------------------------------------------------------------------------------ geometry
def chain_ops(steps, img):
    """Steps on a level whose image is ``img`` (w, h) -> (chain of (kind, ax, ay), (w, h) of the image they end in)."""
    w, h = img
    ops = []
    for s in steps:
        if s[0] == "resize":
            ops.append((SM.OP_SCALE, float(s[1]) / w, float(s[2]) / h))
            w, h = s[1], s[2]
        elif s[0] == "hflip":
            ops.append((SM.OP_HFLIP, float(w), 0.0))
        elif s[0] == "vflip":
            ops.append((SM.OP_VFLIP, 0.0, float(h)))
        elif s[0] == "crop":
            ops.append((SM.OP_SHIFT, float(s[1]), float(s[2])))
            w, h = s[3] - s[1], s[4] - s[2]
        else:
            raise KeyError(s[0])
    return tuple(ops), (w, h)


STRIDE_BOX = ((16, 240), (12, 100), (3, 7), (17, 33))
MAPS = ((1, 1), (3, 5), (7, 13))
STEPS_1 = (("resize", 416, 288),)
STEPS_2 = (("hflip",), ("resize", 416, 288))
STEPS_3 = (("vflip",), ("hflip",), ("resize", 333, 517))
STEPS_6 = (("resize", 300, 200), ("hflip",), ("crop", 10, -7, 250, 150), ("vflip",), ("resize", 480, 196), ("crop", -3, 4, 400, 190))
RECORDED_STEPS = (STEPS_1, STEPS_2, STEPS_3)   # resize and flips: recorded from the reference (tests/golden/mining_geometry.npz)


def ragged(stride):
    """How far an image that is no multiple of the stride ends before its feature map does, per axis."""
    return max(1, stride // 2 - 1), 1


def _geometries():
    out = []

    def add(name, stride, box, H, W, img, crop, steps=()):
        out.append(dict(name=name, stride=stride, box=box, H=H, W=W, img=tuple(img), crop=tuple(crop), steps=tuple(steps)))
    for stride, box in STRIDE_BOX:
        for H, W in MAPS:
            for kind in ("exact", "ragged"):
                kx, ky = (0, 0) if kind == "exact" else ragged(stride)
                img = (W * stride - kx, H * stride - ky)
                for crop in ((80, 64), (81, 63), (96, 48), (1, 1), img, (img[0] + 1, 7), (600, 601)):
                    add("s{}_{}x{}_{}_{}x{}".format(stride, H, W, kind, crop[0], crop[1]), stride, box, H, W, img, crop)
    add("raw0_and_hi_at_img", 16, 240, 3, 5, (80, 48), (16, 16))             # raw == 0 at the first anchor, hi == img at the last
    add("raw0_and_hi_at_img_s12", 12, 100, 4, 6, (72, 48), (36, 12))         # raw == 0 at x = 1; hi == img in the floor branch
    add("wider_than_image_x_only", 16, 240, 3, 5, (80, 48), (96, 32))
    add("taller_than_image_y_only", 16, 240, 3, 5, (80, 48), (32, 64))
    add("wide_level_3600px", 16, 240, 2, 225, (3600, 32), (608, 16))          # the planner's width limit: centres reach 3,600 px
    chained = (("s16_3x5_ragged_81x63", 16, 240, 3, 5, (81, 63)), ("s12_7x13_exact_80x64", 12, 100, 7, 13, (80, 64)),
               ("s3_3x5_ragged_1x1", 3, 7, 3, 5, (1, 1)), ("s17_7x13_ragged_96x48", 17, 33, 7, 13, (96, 48)))
    for name, stride, box, H, W, crop in chained:
        kx, ky = (0, 0) if "exact" in name else ragged(stride)
        for tag, steps in (("chain1", STEPS_1), ("chain2", STEPS_2), ("chain3", STEPS_3), ("chain6", STEPS_6)):
            add(name + "_" + tag, stride, box, H, W, (W * stride - kx, H * stride - ky), crop, steps)
    return out


GEOMETRIES = _geometries()
GEOMETRY = {g["name"]: g for g in GEOMETRIES}
assert len(GEOMETRY) == len(GEOMETRIES) >= 168


@functools.lru_cache(maxsize=None)
def geometry_model(name):
    """The loop model's (crops, anchors, branches on x, branches on y) of a geometry, computed once per process."""
    g = GEOMETRY[name]
    ops, _ = chain_ops(g["steps"], g["img"])
    return SM.crop_table(g["H"], g["W"], g["stride"], g["box"], g["img"][0], g["img"][1], g["crop"][0], g["crop"][1], ops)


# ----------------------------------------------------------------------------------------------------------------- selection
def rank_values(rs, shape, lo=1, scale=2.0 ** -16):
    """Distinct values, exact in float32: a permutation of lo .. lo + n - 1 times ``scale``."""
    n = int(np.prod(shape))
    assert lo + n < 65536
    return ((rs.permutation(n) + lo) * scale).astype(F32).reshape(shape)


def pyramid(name, levels, A=1, B=1, K=4, thr=0.5, stride=16, box=240, crop=(16, 16), imgs=None, chains=None, corners=False, seed=0,
            flags=7):
    """A case whose every element is a candidate of every role (flags 7) with distinct scores in (0, 1); the cases then overwrite
    what their regime needs.  cls_loss and loc_loss are different permutations, cls_preds a third."""
    rs = np.random.RandomState(seed)
    imgs = [(W * stride, H * stride) for H, W in levels] if imgs is None else imgs
    c = dict(name=name, A=A, B=B, K=K, thr=float(F32(thr)), stride=stride, box=box, crop=tuple(crop), levels=list(levels), imgs=list(imgs),
             chains=[()] * len(levels) if chains is None else list(chains), cls_loss=[], loc_loss=[], flags=[], cls_preds=[],
             corners=[] if corners else None, seed=seed, expect={})
    for H, W in levels:
        shape = (A, B, H * W)
        c["cls_loss"].append(rank_values(rs, shape))
        c["loc_loss"].append(rank_values(rs, shape))
        c["cls_preds"].append(rank_values(rs, shape) - F32(0.5))
        c["flags"].append(np.full(shape, flags, np.uint8))
        if corners:
            c["corners"].append(rs.uniform(-50, 300, (A, B, 8, H * W)).astype(F32))
    return c


def offsets(c):
    out = [0]
    for H, W in c["levels"]:
        out.append(out[-1] + c["B"] * H * W)
    return out


def put(c, key, flat, value, image=0):
    """Write ``value`` at a flat (level, label, anchor) candidate index."""
    off = offsets(c)
    l = max(k for k in range(len(c["levels"])) if off[k] <= flat)
    c[key][l][image].reshape(-1)[flat - off[l]] = value


def _tie(levels, B, pair):
    def build(name):
        c = pyramid(name, levels, B=B, K=3, seed=3)
        for flat in pair:
            put(c, "cls_loss", flat, 2.0), put(c, "loc_loss", flat, 2.0)
        c["expect"] = dict(top2=tuple(pair))
        return c
    return build


def _sole(levels):
    def build(name):
        c = pyramid(name, levels, K=2, seed=4)
        n = offsets(c)[-1]
        for key in ("cls_loss", "loc_loss"):
            c[key][0][0, 0, :] = np.resize(np.array([NAN, INF, -INF, NEG_NAN], F32), n)
            put(c, key, n - 1, -3.0)
        c["expect"] = dict(kept=[[[n - 1]] * 3])
        return c
    return build


def _k1(name):
    return pyramid(name, [(9, 13)], B=2, K=1, seed=5)


def _k64(name):
    c = pyramid(name, [(9, 13)], K=MAX_K, seed=6)
    c["expect"] = dict(counts=[[MAX_K] * 3])
    return c


def _partial(name):
    """Role neg has 3 candidates, role pos 24, role pos_loc 5, K = 8: a partial fill, the tail at -1 and 0."""
    c = pyramid(name, [(3, 4)], B=2, K=8, seed=7, flags=1)
    c["flags"][0][0, 1, [2, 5, 11]] |= 2
    c["flags"][0][0, 0, [0, 3, 4, 7, 9]] |= 4
    c["expect"] = dict(counts=[[3, 8, 5]])
    return c


def _crop_covers_image(name):
    """The crop is wider than the image and exactly as high: every window is the same box, one record per role whatever K is."""
    c = pyramid(name, [(3, 4)], B=3, K=5, crop=(80, 48), seed=8)
    c["expect"] = dict(counts=[[1, 1, 1]], one_window=True)
    return c


def _thr1_guard(name):
    """iou_thr 1: nothing is ever killed (no IoU exceeds 1), so only the removal of the kept candidate itself keeps it from being
    kept again.  All 5 labels of anchor 5 carry the top score: kept in label order, then the lone candidate at anchor 7."""
    c = pyramid(name, [(3, 4)], B=5, K=8, thr=1.0, seed=9, flags=0)
    c["flags"][0][0, :, 5] = 7
    c["flags"][0][0, 2, 7] = 7
    for key in ("cls_loss", "loc_loss"):
        c[key][0][0, :, 5] = 1.0
        c[key][0][0, 2, 7] = 0.5
    c["expect"] = dict(kept=[[[5, 17, 29, 41, 53, 31]] * 3], iou_one=5)
    return c


def _thr0_touch(name):
    """iou_thr 0, crop 32x32: columns 0 and 1 share the window [0, 32), column x >= 1 has [16 (x - 1), 16 (x + 1)).  Two columns
    apart the windows touch (IoU 0: survives), one column apart they overlap by one stride (dies)."""
    c = pyramid(name, [(4, 8)], K=3, thr=0.0, crop=(32, 32), seed=10)
    for x, s in ((1, 3.0), (2, 2.9), (3, 2.5)):
        put(c, "cls_loss", 8 + x, s), put(c, "loc_loss", 8 + x, s)
    c["expect"] = dict(first2=(9, 11), killed=10)
    return c


def _exact_half(name):
    """An IoU exactly at the threshold: crop 96x64, identity chain, thr 0.5.  In the floor-branch region of a 256x128 image the
    window of anchor (y, x) is [16 (x - 3), .. + 96) x [16 (y - 2), .. + 64): two columns apart inter = 64 * 64 = 4096 and
    union = 8192 - both survive -, one column apart IoU = 5120 / 7168 - dies."""
    c = pyramid(name, [(8, 16)], K=3, crop=(96, 64), seed=11)
    for x, s in ((5, 3.0), (6, 2.9), (7, 2.8), (8, 2.7), (9, 2.6)):
        put(c, "cls_loss", 4 * 16 + x, s), put(c, "loc_loss", 4 * 16 + x, s)
    c["expect"] = dict(kept=[[[69, 71, 73]] * 3], at_threshold=(4096.0, 8192.0))
    return c


def _exact_quotient(name):
    """An IoU exactly at a threshold that is no dyadic number: crop 61x64, thr = float32(2880 / 4928), the IoU of two windows one
    column apart (inter 45 * 64, union 2 * 3904 - 2880).  The rounded quotient equals the threshold - the neighbour survives -
    while thr * union rounds below inter: a product test alone would kill it."""
    thr = F32(F32(2880) / F32(4928))
    assert F32(2880) > F32(thr * F32(4928))
    c = pyramid(name, [(8, 16)], K=3, thr=thr, crop=(61, 64), seed=12)
    for x, s in ((5, 3.0), (6, 2.9), (7, 2.8)):
        put(c, "cls_loss", 4 * 16 + x, s), put(c, "loc_loss", 4 * 16 + x, s)
    c["expect"] = dict(kept=[[[69, 70, 71]] * 3], at_threshold=(2880.0, 4928.0))
    return c


def _levels8(name):
    c = pyramid(name, [(2, 3)] * MAX_LEVELS, B=2, K=3, seed=13)
    put(c, "cls_loss", 7 * 12 + 9, 2.0), put(c, "loc_loss", 7 * 12 + 4, 2.0)
    c["expect"] = dict(first=[[7 * 12 + 9, 7 * 12 + 9, 7 * 12 + 4]])
    return c


def _rows(name):
    """The case that is also run through [A,B,HW+pad] views (pad 1 and 37) whose padding holds PAD_FLAGS and PAD_SCORE."""
    c = pyramid(name, [(5, 7), (3, 4)], A=2, B=3, K=5, seed=14)
    for t in c["flags"]:
        t[:] = np.random.RandomState(15).randint(0, 8, t.shape).astype(np.uint8)
    return c


def _flag_bits(name):
    """Bytes with the foreign bits 8 .. 128 and no role bit carry the top scores and are never candidates; a byte of 7 is a
    candidate of all three roles, and so is 0xff."""
    c = pyramid(name, [(3, 4)], B=2, K=4, seed=16, flags=0)
    f = c["flags"][0][0]
    f[0, :6] = [8, 16, 32, 64, 128, 0xF8]
    f[1, [1, 6]] = [7, 0xFF]
    f[1, 9] = 8 | 2
    for key in ("cls_loss", "loc_loss"):
        c[key][0][0, 0, :6] = 5.0
    c["expect"] = dict(counts=[[3, 2, 2]])
    return c


def _role_without_candidates(name):
    c = pyramid(name, [(3, 4)], B=2, K=4, seed=17, flags=1 | 4)
    c["expect"] = dict(counts=[[0, 4, 4]])
    return c


SCORE_TABLE = (-0.0, 0.0, SUB, -SUB, FLT_MAX, -FLT_MAX, INF, -INF, NAN, NEG_NAN, 1.0, -1.0, 0.5, -0.5, 0.0, -0.0)
SCORE_ORDER = (4, 10, 12, 2, 0, 1, 14, 15, 3, 13, 11, 5)      # decreasing score, zeros of either sign in index order


def _score_table(name):
    """Negative scores rank below positive ones, the smallest subnormal above 0 and -0 (which tie, by index), FLT_MAX first; inf
    and NaN of either sign are never selected.  loc_loss is the negated table: role pos_loc ranks in the opposite order."""
    c = pyramid(name, [(4, 4)], K=16, seed=18)
    c["cls_loss"][0][0, 0] = np.array(SCORE_TABLE, F32)
    c["loc_loss"][0][0, 0] = -np.array(SCORE_TABLE, F32)
    fwd = list(SCORE_ORDER)
    rev = [5, 11, 13, 3, 0, 1, 14, 15, 2, 12, 10, 4]
    c["expect"] = dict(kept=[[fwd, fwd, rev]])
    return c


def _all_non_finite(name):
    c = pyramid(name, [(3, 4)], B=2, K=4, seed=19)
    for key in ("cls_loss", "loc_loss"):
        c[key][0][:] = np.resize(np.array([NAN, INF, -INF, NEG_NAN], F32), c[key][0].shape)
    c["expect"] = dict(counts=[[0, 0, 0]])
    return c


def _images3(name):
    """N = 585 + 175 = 760 candidates per image (align16(N) = 768 > N); image 1 has no candidate, image 2 holds a permutation of
    image 0's scores.  Crop 80x64 (80 * 64 is not divisible by 3: no IoU of two windows is 0.5): overlapping windows,
    kills in every round."""
    c = pyramid(name, [(9, 13), (5, 7)], A=3, B=5, K=4, crop=(80, 64), seed=20)
    rs = np.random.RandomState(21)
    for l in range(2):
        c["flags"][l][:] = rs.randint(0, 8, c["flags"][l].shape).astype(np.uint8)
        c["flags"][l][1] = 0
        c["flags"][l][2] = c["flags"][l][0]
        for key in ("cls_loss", "loc_loss"):
            c[key][l][2] = rs.permutation(c[key][l][0].reshape(-1)).reshape(c[key][l][0].shape)
    c["expect"] = dict(empty_image=1)
    return c


def _seeded(levels, stride, box, imgs, crop, steps, B=2, K=6, corners=True, thr=0.5):
    def build(name, seed):
        chains = [chain_ops(s, img)[0] for s, img in zip(steps, imgs)]
        c = pyramid(name, levels, B=B, K=K, thr=thr, stride=stride, box=box, crop=crop, imgs=imgs, chains=chains, corners=corners, seed=seed)
        rs = np.random.RandomState(1000 + seed)
        for t in c["flags"]:
            t[:] = rs.randint(0, 8, t.shape).astype(np.uint8)
        return c
    return build


SELECT_BUILDERS = {
    # reduction boundaries: the top score twice, the smaller flat first
    "tie_lanes_62_63": _tie([(25, 41)], 1, (62, 63)),
    "tie_waves_63_64": _tie([(25, 41)], 1, (63, 64)),
    "tie_second_iteration_1023_1024": _tie([(25, 41)], 1, (1023, 1024)),
    "tie_last_two_of_1023": _tie([(31, 33)], 1, (1021, 1022)),
    "tie_last_two_of_1024": _tie([(32, 32)], 1, (1022, 1023)),
    "tie_level_boundary_584_585": _tie([(9, 13), (5, 7)], 5, (584, 585)),
    "sole_finite_last_of_1023": _sole([(31, 33)]),
    "sole_finite_last_of_1024": _sole([(32, 32)]),
    "sole_finite_last_of_1025": _sole([(25, 41)]),
    # K
    "k_1": _k1, "k_64": _k64, "k_above_survivors": _partial, "crop_covers_image": _crop_covers_image,
    # threshold
    "thr_1_guard": _thr1_guard, "thr_0_touch": _thr0_touch, "iou_exactly_half": _exact_half, "iou_exactly_thr_quotient": _exact_quotient,
    # levels, rows, flags, scores, images
    "levels_8": _levels8, "rows": _rows, "flag_bits": _flag_bits, "role_without_candidates": _role_without_candidates,
    "score_table": _score_table, "all_non_finite": _all_non_finite, "images_3": _images3,
}
# seeded cases: odd geometries through the records, six-op chains with corners, the widest level
SEEDED_BUILDERS = {
    "chain_6_s12": _seeded([(7, 13), (3, 5)], 12, 100, [(151, 83), (55, 35)], (81, 63), [STEPS_6, STEPS_6[3:] + STEPS_6[:3]]),
    "chain_2_s3": _seeded([(3, 5), (1, 1)], 3, 7, [(14, 8), (3, 3)], (7, 5), [STEPS_2, STEPS_1], K=5),
    "chain_3_s17": _seeded([(7, 13)], 17, 33, [(214, 118)], (96, 48), [STEPS_3], K=6),
    "wide_level_3600px": _seeded([(2, 225)], 16, 240, [(3600, 32)], (608, 16), [()], B=1, K=6, corners=False),
}
EXACT = ("thr_1_guard", "thr_0_touch", "iou_exactly_half", "iou_exactly_thr_quotient")
# first seeds that keep the band (tests/test_mining_stage_model.py::test_seeds recomputes every one)
SEEDS = {"chain_6_s12": 0, "chain_2_s3": 0, "chain_3_s17": 0, "wide_level_3600px": 0}
SELECT_CASES = sorted(SELECT_BUILDERS) + sorted(SEEDED_BUILDERS)


def build(name, seed=None):
    if name in SEEDED_BUILDERS:
        return SEEDED_BUILDERS[name](name, SEEDS[name] if seed is None else seed)
    return SELECT_BUILDERS[name](name)


def first_seed(name, limit=256):
    for seed in range(limit):
        if SM.mine(build(name, seed))["band_gap"] >= BAND:
            return seed
    raise AssertionError("no seed under {} keeps the band for {}".format(limit, name))


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name)


@functools.lru_cache(maxsize=None)
def model(name):
    """The loop model's result for the case, computed once per process and left unchanged."""
    return SM.mine(case(name))


def same_bits(a, b):
    """Equality of two float32 arrays bit for bit: -0 is not +0 here."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def image_alone(c, a):
    """Image ``a`` of a case as a case of its own (A = 1)."""
    d = dict(c, A=1, name="{}[{}]".format(c["name"], a))
    for key in ("cls_loss", "loc_loss", "flags", "cls_preds"):
        d[key] = [t[a:a + 1] for t in c[key]]
    if c["corners"] is not None:
        d["corners"] = [t[a:a + 1] for t in c["corners"]]
    return d
