"""Shared by the VOC evaluation tests: fixtures, packing of a case, and the comparison of a computed result with a fixture
under the rules of the issue - match, n_pos, tp, fp, prec, rec exactly, AP and the scalars within 1e-10."""
import os

import numpy as np
import torch

import voc_eval_cases as VC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# AP <= 1 is a sum of fewer than 1e5 non-negative, once-rounded terms added in another order: at most n * 2^-52 ~ 2e-11
AP_ATOL = 1e-10


def fixture(name):
    return dict(np.load(os.path.join(GOLDEN, "voc_eval_{}.npz".format(name))))


def resized_case(name):
    """The images of a case with the prediction boxes already in the ground truth's size (project BoxList.resize)."""
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    images = VC.case(name)
    preds, gts = VC.boxlists(images, BoxList, FeatureMapSize)
    return images, [p.resize(g.image_size) for p, g in zip(preds, gts)], gts


def model_pack(preds, gts, device):
    import voc_eval_model as M
    return M.pack([p.bbox_xyxy for p in preds], [p.get_field("scores") for p in preds], [p.get_field("labels") for p in preds],
                  [g.bbox_xyxy for g in gts], [g.get_field("labels") for g in gts], [g.get_field("difficult") for g in gts], device)


def reference_match_order(labels, image, scores):
    """Packed indices in the order of the fixture's match array: label, then image, then descending score."""
    labels, image, scores = (np.asarray(x) for x in (labels, image, scores))
    return np.lexsort((-scores.astype(np.float64), image, labels))


def check_inputs(name, images, fx):
    if "in_scores" in fx:
        assert np.array_equal(fx["in_scores"], np.concatenate([im["scores"] for im in images]))
        assert np.array_equal(fx["in_pred_boxes"], np.concatenate([im["pred_boxes"].reshape(-1, 4) for im in images]))
        assert np.array_equal(fx["in_gt_boxes"], np.concatenate([im["gt_boxes"].reshape(-1, 4) for im in images]))


def compare(fx, thr, use_07, got):
    """got: numpy arrays - match (packed order), labels / image / scores (packed), tp, fp, prec, rec (class-sorted),
    class_counts, gt_counts, n_pos, ap_per_class, recall_per_class, scalars [map, map_weighted, recall, ap_joint]."""
    tag = VC.tag(thr)
    L = len(fx["n_pos"])
    assert len(got["n_pos"]) == L
    assert np.array_equal(np.asarray(got["n_pos"], np.float64), fx["n_pos"])
    order = reference_match_order(got["labels"], got["image"], got["scores"])
    assert np.array_equal(np.asarray(got["match"])[order], fx["match_" + tag])
    assert np.array_equal(np.asarray(got["tp"], np.int64), fx["tp_" + tag].astype(np.int64))
    assert np.array_equal(np.asarray(got["fp"], np.int64), fx["fp_" + tag].astype(np.int64))
    assert np.array_equal(got["prec"], fx["prec_" + tag], equal_nan=True)
    # which entries the reference has: prec None = label never seen, rec None = no positives
    seen = (np.asarray(got["class_counts"]) > 0) | (np.asarray(got["gt_counts"]) > 0)
    plen = np.where(seen, np.asarray(got["class_counts"]), -1)
    rlen = np.where(seen & (fx["n_pos"] > 0), np.asarray(got["class_counts"]), -1)
    assert np.array_equal(plen, fx["prec_len_" + tag]) and np.array_equal(rlen, fx["rec_len_" + tag])
    has_rec = np.repeat(fx["n_pos"] > 0, np.asarray(got["class_counts"]))
    assert np.array_equal(np.asarray(got["rec"])[has_rec], fx["rec_" + tag][has_rec])
    assert np.isnan(fx["rec_" + tag][~has_rec]).all()
    if not use_07:
        assert np.array_equal(got["recall_per_class"], fx["recall_per_class_" + tag], equal_nan=True)
    sfx = tag + ("_07" if use_07 else "")
    assert np.array_equal(np.isnan(got["ap_per_class"]), np.isnan(fx["ap_" + sfx]))
    assert np.allclose(got["ap_per_class"], fx["ap_" + sfx], rtol=0, atol=AP_ATOL, equal_nan=True)
    assert np.allclose(got["scalars"], fx["scalars_" + sfx], rtol=0, atol=AP_ATOL, equal_nan=True)


def model_bundle(p, r):
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    return dict(match=n(r["match"]), labels=n(p["labels"]), image=n(p["image"]), scores=n(p["scores"]), tp=n(r["tp"]), fp=n(r["fp"]),
                prec=n(r["prec"]), rec=n(r["rec"]), class_counts=n(r["class_counts"]), gt_counts=n(r["gt_counts"]), n_pos=n(r["n_pos"]),
                ap_per_class=n(r["ap_per_class"]), recall_per_class=n(r["recall_per_class"]),
                scalars=np.array([float(r[k]) for k in ("map", "map_weighted", "recall", "ap_joint_classes")]))
