"""Inputs of the objective / target-assignment fixtures (tests/golden/objective_*.npz), drawn from numpy RandomState seeds so
that the fixture generator and the tests build the same arrays and only the reference's outputs are stored.  Test
infrastructure only."""
import numpy as np

STRIDE, BOX_SIZE = 16, 240            # anchors: rec_field 16 + 14 * stride
IOU = dict(pos=0.5, neg=0.1, remap_pos=0.8, remap_neg=0.4)
# Os2dObjective arguments of every fixture (the reference's defaults for the two losses)
CRITERION = dict(margin=0.5, margin_pos=0.6, class_loss_neg_weight=1.0, remap_classification_targets=True,
                 localization_weight=0.2, neg_to_pos_ratio=3, rll_neg_weight_ratio=0.001)
LOSSES = ("RLL", "ContrastiveLoss")

#   name: A, B, levels [(H, W)], seed, boxes per image (None = drawn), use remap + cls_preds_for_neg, patch mining
CASES = {
    "small":   dict(A=2, B=5, levels=[(9, 13)], seed=101, remap=True, patch=False),
    "train":   dict(A=4, B=15, levels=[(38, 38)], seed=102, remap=True, patch=False),
    "nopos":   dict(A=2, B=5, levels=[(9, 13)], seed=103, remap=True, patch=False),
    "noremap": dict(A=2, B=5, levels=[(9, 13)], seed=104, remap=False, patch=False),
    "patch":   dict(A=2, B=5, levels=[(9, 13), (5, 7)], seed=105, remap=True, patch=True),
}


def image_size(level):
    H, W = level
    return W * STRIDE, H * STRIDE          # (w, h)


def draw_boxes(name):
    """-> per image (boxes [n,4] float32 xyxy in the coordinates of level 0, labels [n] int64, difficult [n] bool)."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    w_img, h_img = image_size(c["levels"][0])
    out = []
    for a in range(c["A"]):
        if name == "nopos":
            if a == 0:      # an image without any box
                out.append((np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, bool)))
                continue
            n = 2
        elif name == "train":
            n = 12
        else:
            n = 3 + (rs.randint(4) if a else 3)        # 3 to 6, the first image has 6
        if name == "train":
            cx = rs.rand(n) * (w_img - 60) + 30
            cy = rs.rand(n) * (h_img - 60) + 30
        else:               # the 9 x 13 map is smaller than one anchor: centres around the image keep the positives few
            cx = rs.rand(n) * (w_img + 300) - 150
            cy = rs.rand(n) * (h_img + 300) - 150
        w = rs.rand(n) * 140 + 160
        h = rs.rand(n) * 140 + 160
        boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
        if name == "train":
            labels = rs.randint(0, c["B"], n)
            difficult = rs.rand(n) < 0.2
        elif name == "nopos":
            labels = np.array([1, 3])
            difficult = np.ones(n, bool)                 # matched anchors are ignored: no positive anywhere
        else:
            labels = rs.randint(0, c["B"] - 1, n)        # the last label never has a box
            labels[1] = labels[0]                        # a repeated label
            difficult = np.zeros(n, bool)
            difficult[2] = True
        out.append((boxes, labels.astype(np.int64), difficult))
    return out


def draw_predictions(name, loc_targets):
    """loc_targets: the concatenated [A,B,4,HW] encode output.  -> loc_preds, cls_preds, cls_preds_for_neg (float32)."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 1000)
    shape = loc_targets.shape
    # every anchor of a label with a box has a target that decodes to SOME box of the label: predictions near the target on
    # a fraction of the anchors only, or nearly all of them would be remapped to positives
    keep = rs.rand(shape[0], shape[1], 1, shape[3]) < 0.15
    loc = (loc_targets * keep + rs.randn(*shape) * 0.5).astype(np.float32)
    cls = (rs.rand(shape[0], shape[1], shape[3]) * 1.4 - 0.4).astype(np.float32)
    cls_det = (cls + 0.01 * rs.randn(*cls.shape)).astype(np.float32)
    return loc, cls, cls_det
