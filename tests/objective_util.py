"""Shared by the objective tests: fixture loading (tests/golden/objective_*.npz, recorded from the reference by
tests/golden/make_objective_golden.py) and the measured-error pins (tests/golden/objective_pins.json)."""
import json
import os

import numpy as np
import torch

import objective_cases as OC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAND, BAND_CAP = 1e-5, 1.0 / 2000        # remap: anchors whose corrected IoU is this close to a threshold may flip (the issue)
SCALARS = ("loss", "loc", "cls", "cls_pos", "cls_neg")


def pins():
    with open(os.path.join(GOLDEN, "objective_pins.json")) as f:
        return json.load(f)


def load_targets(name):
    d = np.load(os.path.join(GOLDEN, "objective_{}_targets.npz".format(name)))
    fx = {k: d[k] for k in d.files}
    c = OC.CASES[name]
    if "loc_preds" not in fx:             # the training shape: inputs are redrawn from the seed
        fx["loc_preds"], fx["cls_preds"], fx["cls_preds_for_neg"] = OC.draw_predictions(name, fx["loc_targets"])
    check = sum(float(fx[k].astype(np.float64).sum()) for k in ("loc_preds", "cls_preds", "cls_preds_for_neg"))
    assert abs(check - float(fx["input_checksum"])) <= 1e-9 * max(1.0, abs(check)), "regenerated inputs differ"
    fx["boxes"] = [(fx["boxes_{}".format(a)], fx["labels_{}".format(a)], fx["difficult_{}".format(a)]) for a in range(c["A"])]
    return fx


def load_loss(name, loss):
    d = np.load(os.path.join(GOLDEN, "objective_{}_{}.npz".format(name, loss.lower())))
    return {k: d[k] for k in d.files}


def level_boxes(name, level, boxes):
    """The boxes of level 0 scaled to `level` (as the fixture generator does): list of (boxes, labels, difficult) tensors."""
    w0, h0 = OC.image_size(OC.CASES[name]["levels"][0])
    w, h = OC.image_size(level)
    out = []
    for b, labels, difficult in boxes:
        b = torch.from_numpy(b).clone()
        b[:, 0::2] *= float(w) / w0
        b[:, 1::2] *= float(h) / h0
        out.append((b, torch.from_numpy(labels), torch.from_numpy(difficult)))
    return out


def rel_err(ours, ref):
    """max |ours - ref| / max(1e-30, max |ref|): the error figure the pins hold (0 when both are all zero)."""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(ours - ref).max()) if ref.size else 0.0
    return err / scale if scale > 0 else err
