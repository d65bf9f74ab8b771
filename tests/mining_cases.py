"""Geometry and input drawing of the hard-patch mining fixtures (tests/golden/mining_*.npz, recorded from the reference by
tests/golden/make_mining_golden.py) and their loader.  The generator redraws the seed until the conditions it asserts on the
reference hold, so the drawn inputs are stored in the fixtures; the tests read them from there.  Test infrastructure only."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIDE, BOX_SIZE = 16, 240
IOU = dict(pos=0.5, neg=0.1, remap_pos=0.8, remap_neg=0.4)
CRITERION = dict(margin=0.5, margin_pos=0.6, class_loss_neg_weight=1.0, remap_classification_targets=True,
                 localization_weight=0.2, neg_to_pos_ratio=3, rll_neg_weight_ratio=0.001)
LOSS = "ContrastiveLoss"
ORIG = (416, 288)                     # (w, h) of the original image
CROP = (80, 64)                       # (w, h): w * h is not divisible by 3, so no IoU of two crops is exactly 0.5
NMS_IOU = 0.5
ROLES = ("neg", "pos", "pos_loc")
OP_SCALE, OP_HFLIP = 1, 2
KEYS = ("pyramid_level", "label_local", "anchor_index", "role", "crop_position_xyxy", "anchor_position_xyxy", "transform_corners",
        "label_global", "loss", "loss_loc", "score", "image_id")

#   levels: feature maps (H, W); the level's image is (W * 16, H * 16); flip: the level's chain ends with a horizontal flip
CASES = {
    "pyr":  dict(A=2, B=5, K=4, levels=[(9, 13), (5, 7), (3, 4)], flip=False, seed=301),
    "flip": dict(A=2, B=5, K=4, levels=[(9, 13)], flip=True, seed=400),
}
CLASS_IDS = [11, 3, 7, 20, 5]         # global ids of the five local labels


def image_size(level):
    return level[1] * STRIDE, level[0] * STRIDE


def chains(name):
    """Per level the box-op chain (kind, ax, ay) of its transform into the original image, as the reference's TransformList
    applies it: [flip inside the level's image, then] resize to ORIG."""
    out = []
    for level in CASES[name]["levels"]:
        w, h = image_size(level)
        ops = [(OP_SCALE, float(ORIG[0]) / w, float(ORIG[1]) / h)]
        if CASES[name]["flip"]:
            ops.insert(0, (OP_HFLIP, float(w), 0.0))
        out.append(tuple(ops))
    return out


def draw(name, seed):
    """-> per image dict(boxes [n,4] in ORIG coordinates, labels (local), difficult), and per level loc [A,B,4,HW],
    cls [A,B,HW], corners [A,B,8,HW].  The second image has no box: no positive at all."""
    c = CASES[name]
    rs = np.random.RandomState(seed)
    images = []
    for a in range(c["A"]):
        n = 0 if a == 1 else 4
        level = rs.randint(0, len(c["levels"]), n)
        size = np.array([BOX_SIZE * float(ORIG[0]) / image_size(c["levels"][l])[0] for l in level]).reshape(n)
        w, h = size * (0.75 + 0.5 * rs.rand(n)), size * (0.75 + 0.5 * rs.rand(n))
        cx, cy = rs.rand(n) * ORIG[0], rs.rand(n) * ORIG[1]
        boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32).reshape(n, 4)
        labels = rs.randint(0, c["B"] - 1, n).astype(np.int64)            # the last label never has a box
        difficult = np.zeros(n, bool)
        if n > 3:
            labels[1] = labels[0]
            difficult[3] = True
        images.append(dict(boxes=boxes, labels=labels, difficult=difficult))
    loc, cls, corners = [], [], []
    for H, W in c["levels"]:
        shape = (c["A"], c["B"], H * W)
        loc.append((rs.randn(shape[0], shape[1], 4, shape[2]) * 0.5).astype(np.float32))
        cls.append((rs.rand(*shape) * 1.4 - 0.4).astype(np.float32))
        corners.append((rs.rand(shape[0], shape[1], 8, shape[2]) * 300 - 50).astype(np.float32))
    return images, loc, cls, corners


def load(name):
    d = np.load(os.path.join(GOLDEN, "mining_{}.npz".format(name)), allow_pickle=False)
    return {k: d[k] for k in d.files}
