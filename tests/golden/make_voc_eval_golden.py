"""Records tests/golden/voc_eval_*.npz from the reference's ``do_voc_evaluation`` on the CPU, on the inputs of
tests/voc_eval_cases.py, at the IoU thresholds 0.5 and 0.75 and with both AP forms.

    python tests/golden/make_voc_eval_golden.py

The reference is imported as in make_golden.py, with its torchvision stand-in.  Data only is written: inputs (not for the
seed-derived ``medium`` case), and per threshold the match values, tp / fp, prec / rec, n_pos, AP arrays and scalars.  The
reference keeps its match lists local; they are read out through a recording ``defaultdict`` placed in its module while it
runs (the third one it creates).  Before writing, the generator asserts that all scores of a case differ and that no
detection's best IoU lies within 1e-5 of a threshold, so the recorded decisions do not hang on a rounding."""
import collections
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "tests"))

spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
make_golden = importlib.util.module_from_spec(spec)
spec.loader.exec_module(make_golden)
make_golden.install_torchvision_standin()
sys.path.insert(0, make_golden.REFERENCE)

from os2d.data import voc_eval as ref  # noqa: E402
from os2d.structures.bounding_box import BoxList, box_iou  # noqa: E402
from os2d.structures.feature_map import FeatureMapSize  # noqa: E402

import voc_eval_cases as VC  # noqa: E402


class Recorder(object):
    """Stands in for ``defaultdict`` inside the reference module and keeps what it creates."""
    def __init__(self):
        self.made = []

    def __call__(self, factory):
        d = collections.defaultdict(factory)
        self.made.append(d)
        return d


def check_inputs(images, preds, gts):
    scores = np.concatenate([im["scores"] for im in images])
    assert len(np.unique(scores)) == len(scores), "equal scores"
    for pred, gt in zip(preds, gts):
        pred = pred.resize(gt.image_size)
        if len(pred) == 0 or len(gt) == 0:
            continue
        one = torch.tensor([0, 0, 1, 1], dtype=torch.float32)
        iou = box_iou(pred.bbox_xyxy + one, gt.bbox_xyxy + one)
        same = pred.get_field("labels")[:, None] == gt.get_field("labels")[None, :]
        best = torch.where(same, iou, torch.full_like(iou, -1)).max(1).values
        for t in VC.THRESHOLDS:
            assert float((best - t).abs().min()) > 1e-5, "a best IoU within 1e-5 of {}".format(t)


def record(name):
    images = VC.case(name)
    preds, gts = VC.boxlists(images, BoxList, FeatureMapSize)
    check_inputs(images, preds, gts)
    out = {}
    if name != "medium":
        for k in ("pred_boxes", "scores", "labels", "gt_boxes", "gt_labels", "difficult"):
            out["in_" + k] = np.concatenate([im[k].reshape((-1, 4) if k.endswith("boxes") else (-1,)) for im in images])
        out["in_counts"] = np.array([[len(im["scores"]), len(im["gt_labels"])] for im in images])
        out["in_sizes"] = np.array([im["pred_size"] + im["gt_size"] for im in images])
    for t in VC.THRESHOLDS:
        tag = VC.tag(t)
        for use_07 in (False, True):
            rec_dd = Recorder()
            ref.defaultdict = rec_dd
            try:
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    res = ref.do_voc_evaluation(preds, gts, iou_thresh=t, use_07_metric=use_07)
            finally:
                ref.defaultdict = collections.defaultdict
            sfx = tag + ("_07" if use_07 else "")
            out["ap_" + sfx] = np.asarray(res["ap_per_class"], np.float64)
            out["scalars_" + sfx] = np.array([res["map"], res["map_weighted"], res["recall"], res["ap_joint_classes"]], np.float64)
            if use_07:
                continue
            n_pos_d, score_d, match_d = rec_dd.made[0], rec_dd.made[1], rec_dd.made[2]
            L = len(res["prec"])
            out["n_pos"] = np.asarray(res["n_pos"], np.float64)
            out["recall_per_class_" + tag] = np.asarray(res["recall_per_class"], np.float64)
            # match: labels ascending, inside a label the reference's order (images in order, descending score in an image)
            out["match_" + tag] = np.concatenate([np.array(match_d[l], np.int8) for l in range(L) if l in match_d] + [np.zeros(0, np.int8)])
            tp, fp, prec, rec, plen, rlen = [], [], [], [], [], []
            for l in range(L):
                plen.append(-1 if res["prec"][l] is None else len(res["prec"][l]))
                rlen.append(-1 if res["rec"][l] is None else len(res["rec"][l]))
                if res["prec"][l] is None:
                    continue
                order = np.array(score_d[l]).argsort()[::-1]
                m = np.array(match_d[l], np.int8)[order] if len(order) else np.zeros(0, np.int8)
                tp.append(np.cumsum(m == 1))
                fp.append(np.cumsum(m == 0))
                prec.append(res["prec"][l])
                rec.append(res["rec"][l] if res["rec"][l] is not None else np.full(len(m), np.nan))
            cat = lambda xs, dt: np.concatenate(xs + [np.zeros(0)]).astype(dt)   # noqa: E731
            out["tp_" + tag], out["fp_" + tag] = cat(tp, np.int32), cat(fp, np.int32)
            out["prec_" + tag], out["rec_" + tag] = cat(prec, np.float64), cat(rec, np.float64)
            out["prec_len_" + tag], out["rec_len_" + tag] = np.array(plen), np.array(rlen)
    path = os.path.join(HERE, "voc_eval_{}.npz".format(name))
    np.savez_compressed(path, **out)
    print(name, "->", path, os.path.getsize(path), "bytes; mAP@0.5 {:.4f} mAP@0.75 {:.4f}".format(out["scalars_t50"][0], out["scalars_t75"][0]))


if __name__ == "__main__":
    for name in VC.CASES:
        record(name)
