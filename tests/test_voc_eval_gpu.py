"""GPU: the VOC metric of libos2d_eval.so (os2d_amd/engine/voc_eval.py) against the fixtures recorded from the reference and,
at 2,000 images x 1,024 labels x 1,000 detections, against tests/voc_eval_model.py on the same device: match, n_pos, tp, fp,
prec, rec exactly, AP and the scalars within 1e-10 (tests/voc_eval_util.py); equal bits on two runs; no synchronisation
between the first add and the end of compute; the cached sort changes nothing; ``evaluate`` end to end."""
import numpy as np
import pytest
import torch

import voc_eval_cases as VC
import voc_eval_model as M
import voc_eval_util as U

pytestmark = pytest.mark.gpu

SCALARS = ("map", "map_weighted", "recall", "ap_joint_classes")


def _inputs(name, device):
    """Predictions on the device (in their own image sizes), ground truth on the host."""
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    return VC.boxlists(VC.case(name), BoxList, FeatureMapSize, device=device)


def _evaluator(name, device, num_labels=True, inputs=None):
    from os2d_amd.engine.voc_eval import VocEvaluator
    preds, gts = inputs or _inputs(name, device)
    ev = VocEvaluator(num_labels=VC.NUM_LABELS[name] if num_labels else None)
    for p, g in zip(preds, gts):
        ev.add(p, g)
    return ev


def hip_bundle(ev, r):
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    p, last = ev._packed, ev.last
    L = p["L"]
    image = np.repeat(np.arange(p["N"]), np.diff(n(p["det_offsets"])))
    tpfp = n(last["tpfp"])
    return dict(match=n(last["match"]), labels=n(p["det_labels"]), image=image, scores=n(p["det_scores"]), tp=tpfp >> 32, fp=tpfp & 0xffffffff,
                prec=n(last["prec"]), rec=n(last["rec"]), class_counts=np.diff(n(p["class_offsets"])), gt_counts=n(p["gt_count"]),
                n_pos=n(r["n_pos"]), ap_per_class=n(r["ap_per_class"]), recall_per_class=n(r["recall_per_class"]),
                scalars=np.array([float(r[k]) for k in SCALARS]))


@pytest.mark.parametrize("use_07", (False, True))
@pytest.mark.parametrize("thr", VC.THRESHOLDS)
@pytest.mark.parametrize("name", VC.CASES)
def test_hip_reproduces_the_reference(name, thr, use_07, device):
    fx = U.fixture(name)
    ev = _evaluator(name, device)
    r = ev.compute(iou_thresh=thr, use_07_metric=use_07)
    for k in ("ap_per_class", "recall_per_class", "n_pos") + SCALARS:
        assert r[k].is_cuda and r[k].dtype == torch.float64 and r[k].dim() == (1 if k in ("ap_per_class", "recall_per_class", "n_pos") else 0)
    U.compare(fx, thr, use_07, hip_bundle(ev, r))
    tag = VC.tag(thr)
    assert [(-1 if x is None else len(x)) for x in r["prec"]] == fx["prec_len_" + tag].tolist()
    assert [(-1 if x is None else len(x)) for x in r["rec"]] == fx["rec_len_" + tag].tolist()
    assert torch.equal(torch.cat([x for x in r["prec"] if x is not None]).isnan(), ev.last["prec"].isnan())


def test_functions_with_the_reference_signatures(device):
    from os2d_amd.engine import voc_eval as V
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    fx = U.fixture("resize_unequal")
    preds, gts = VC.boxlists(VC.case("resize_unequal"), BoxList, FeatureMapSize, device=device)
    r = V.do_voc_evaluation(preds, gts, iou_thresh=0.75)
    assert np.allclose(r["ap_per_class"].cpu().numpy(), fx["ap_t75"], rtol=0, atol=U.AP_ATOL, equal_nan=True)
    assert np.allclose([float(r[k]) for k in SCALARS], fx["scalars_t75"], rtol=0, atol=U.AP_ATOL, equal_nan=True)
    resized = [p.resize(g.image_size) for p, g in zip(preds, gts)]
    prec, rec, n_pos = V.calc_detection_voc_prec_rec(gts, resized, iou_thresh=0.75)
    assert np.array_equal(n_pos.cpu().numpy(), fx["n_pos"])
    assert np.array_equal(torch.cat([x for x in prec if x is not None]).cpu().numpy(), fx["prec_t75"], equal_nan=True)
    for use_07, key in ((False, "ap_t75"), (True, "ap_t75_07")):
        ap = V.calc_detection_voc_ap(prec, rec, use_07_metric=use_07)
        assert np.allclose(ap.cpu().numpy(), fx[key], rtol=0, atol=U.AP_ATOL, equal_nan=True)
    recall, per_class, n_pos_f = V.calc_detection_recall(rec, n_pos)
    assert np.array_equal(per_class.cpu().numpy(), fx["recall_per_class_t75"], equal_nan=True)
    assert abs(float(recall) - fx["scalars_t75"][2]) <= U.AP_ATOL
    one_p, one_r, one_n = V.calc_detection_voc_prec_rec(gts, resized, iou_thresh=0.75, merge_classes_together=True)
    assert abs(float(V.calc_detection_voc_ap(one_p, one_r)[0]) - fx["scalars_t75"][3]) <= U.AP_ATOL and int(one_n[0]) == fx["n_pos"].sum()


# ------------------------------------------------------------------------------------------------ the large shape
@pytest.fixture(scope="module")
def large(device):
    from os2d_amd.engine.voc_eval import VocEvaluator
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    c = VC.large()
    size = FeatureMapSize(w=c["size"][0], h=c["size"][1])
    dev = {k: c[k].to(device) for k in ("boxes", "scores", "labels")}

    def evaluator():
        ev = VocEvaluator(num_labels=1024)
        for i in range(c["boxes"].shape[0]):
            p = BoxList(dev["boxes"][i], size)
            p.add_field("scores", dev["scores"][i])
            p.add_field("labels", dev["labels"][i])
            g = BoxList(c["gt_boxes"][i], size)
            g.add_field("labels", c["gt_labels"][i])
            g.add_field("difficult", c["difficult"][i])
            ev.add(p, g)
        return ev
    N, n = c["scores"].shape
    m = c["gt_labels"].shape[1]
    packed = dict(boxes=dev["boxes"].reshape(-1, 4), scores=dev["scores"].reshape(-1), labels=dev["labels"].reshape(-1),
                  image=torch.arange(N, device=device).repeat_interleave(n), gt_boxes=c["gt_boxes"].reshape(-1, 4).to(device),
                  gt_labels=c["gt_labels"].reshape(-1).to(device), gt_difficult=c["difficult"].reshape(-1).bool().to(device),
                  gt_image=torch.arange(N, device=device).repeat_interleave(m), N=N)
    return dict(make=evaluator, shared=evaluator(), packed=packed, model={})


@pytest.mark.parametrize("use_07", (False, True))
@pytest.mark.parametrize("thr", VC.THRESHOLDS)
def test_hip_equals_the_model_at_the_large_shape(large, thr, use_07):
    ev, p = large["shared"], large["packed"]
    r = ev.compute(iou_thresh=thr, use_07_metric=use_07, with_curves=False)
    ref = M.evaluate(p, 1024, thr, use_07)
    last = ev.last
    assert torch.equal(last["match"], ref["match"])
    assert torch.equal(last["perm_joint"].long(), ref["order_joint"]) and torch.equal(last["perm_class"].long(), ref["order_class"])
    assert torch.equal(last["tpfp"] >> 32, ref["tp"]) and torch.equal(last["tpfp"] & 0xffffffff, ref["fp"])
    assert torch.equal(last["tpfp_joint"] >> 32, ref["tp_joint"]) and torch.equal(last["tpfp_joint"] & 0xffffffff, ref["fp_joint"])
    for a, b in ((last["prec"], ref["prec"]), (last["rec"], ref["rec"]), (last["prec_joint"], ref["prec_joint"]), (last["rec_joint"], ref["rec_joint"])):
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    assert torch.equal(r["n_pos"], ref["n_pos"].double())
    assert torch.equal(r["ap_per_class"].isnan(), ref["ap_per_class"].isnan())
    assert float((torch.nan_to_num(r["ap_per_class"]) - torch.nan_to_num(ref["ap_per_class"])).abs().max()) <= U.AP_ATOL
    assert torch.equal(torch.nan_to_num(r["recall_per_class"], nan=-1.0), torch.nan_to_num(ref["recall_per_class"], nan=-1.0))
    for k in SCALARS:
        assert abs(float(r[k]) - float(ref[k])) <= U.AP_ATOL, k
    assert 0.0 < float(r["map"]) < 1.0 and 0.0 < float(r["ap_joint_classes"]) < 1.0


def test_two_runs_give_the_same_bits(large):
    outs = []
    for _ in range(2):
        ev = large["make"]()
        r = ev.compute(iou_thresh=0.5, with_curves=False)
        outs.append([r[k].clone() for k in ("ap_per_class", "recall_per_class") + SCALARS] +
                    [ev.last[k].clone() for k in ("match", "perm_class", "perm_joint", "prec", "rec", "mpre", "mpre_joint", "tpfp_joint")])
    for a, b in zip(*outs):
        bits = (lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t)
        assert torch.equal(bits(a.contiguous().reshape(-1)), bits(b.contiguous().reshape(-1)))


# ------------------------------------------------------------------------------------------------ the accumulator
@pytest.mark.parametrize("name", ("medium", "resize_unequal"))
def test_add_and_compute_do_not_synchronise(name, device):
    fx = U.fixture(name)
    inputs = _inputs(name, device)
    _evaluator(name, device, inputs=inputs).compute(with_curves=False)        # library load, first-use allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev = _evaluator(name, device, inputs=inputs)
        results = [ev.compute(iou_thresh=t, use_07_metric=False, with_curves=False) for t in VC.THRESHOLDS]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for t, r in zip(VC.THRESHOLDS, results):
        assert "prec" not in r
        assert np.allclose([float(r[k]) for k in SCALARS], fx["scalars_" + VC.tag(t)], rtol=0, atol=U.AP_ATOL, equal_nan=True)


def test_cached_sort_equals_fresh_objects(device):
    shared = _evaluator("medium", device)
    for thr in VC.THRESHOLDS + (0.5,):
        for use_07 in (False, True):
            a = shared.compute(iou_thresh=thr, use_07_metric=use_07)
            b = _evaluator("medium", device, num_labels=False).compute(iou_thresh=thr, use_07_metric=use_07)
            for k in ("ap_per_class", "recall_per_class", "n_pos") + SCALARS:
                assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), k
            assert all((x is None) == (y is None) and (x is None or torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)))
                       for x, y in zip(a["prec"] + a["rec"], b["prec"] + b["rec"]))


def test_ties_keep_increasing_index(device):
    from os2d_amd.engine.voc_eval import VocEvaluator
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    size = FeatureMapSize(w=100, h=100)
    box = torch.tensor([[10., 10., 50., 50.]])
    ev = VocEvaluator(num_labels=1)
    for k in (2, 1):
        p = BoxList(box.repeat(k, 1).to(device), size)
        p.add_field("scores", torch.full((k,), 0.5, device=device))
        p.add_field("labels", torch.zeros(k, dtype=torch.long, device=device))
        g = BoxList(box, size)
        g.add_field("labels", torch.zeros(1, dtype=torch.long))
        ev.add(p, g)
    r = ev.compute()
    assert ev.last["match"].tolist() == [1, 0, 1] and ev.last["perm_joint"].tolist() == [0, 1, 2]
    assert r["prec"][0].tolist() == [1.0, 0.5, 2.0 / 3.0] and float(r["recall"]) == 1.0


def test_evaluate_equals_detect_then_the_model(device, monkeypatch):
    """``evaluate`` = detect_images + VocEvaluator: its numbers are the CPU model's on the detections it was given (recorded
    on the way: the backbone is not bit-reproducible call to call), and those are per-image ``detect`` results."""
    from os2d_amd.engine import evaluate as E
    from os2d_amd.modeling.model import Os2dModel
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    from os2d_amd.utils import synthetic
    torch.manual_seed(7)
    net = Os2dModel(is_cuda=False, merge_branch_parameters=True, backbone_arch="resnet50", use_inverse_geom_model=True, simplify_affine=False)
    net.os2d_head_creator.aligner.parameter_regressor.load_state_dict(synthetic.make_transform_net_state(6, seed=7))
    net.to(device).eval()
    g = torch.Generator().manual_seed(4)
    class_ids = [0, 1, 2]
    head = E.build_class_head(net, [torch.randn(3, 96, 96, generator=g).to(device) for _ in class_ids])
    coder = net.build_box_coder()
    pyramids = [[torch.randn(1, 3, 96, 128, generator=g), torch.randn(1, 3, 128, 176, generator=g)] for _ in range(3)]
    orig = [FeatureMapSize(w=200 + 10 * i, h=150 + 5 * i) for i in range(3)]
    gt_sizes = [FeatureMapSize(w=2 * o.w, h=3 * o.h) for o in orig]
    # ground truth: the three best detections of a first pass, in the ground truth's (different) image size
    gts = []
    for i, levels in enumerate(pyramids):
        det = E.detect(net, coder, [x.to(device) for x in levels], head, class_ids, orig_size=orig[i], nms_score_threshold=0.0).resize(gt_sizes[i])
        top = det.get_field("scores").argsort(descending=True)[:3].cpu()
        b = BoxList(det.bbox_xyxy.cpu()[top], gt_sizes[i])
        b.add_field("labels", det.get_field("labels").cpu()[top])
        b.add_field("difficult", torch.tensor([0, 0, 1], dtype=torch.uint8)[:len(top)])
        gts.append(b)
    seen = []
    plain_detect = E.detect

    def recording_detect(*args, **kwargs):
        seen.append(plain_detect(*args, **kwargs))
        return seen[-1]
    monkeypatch.setattr(E, "detect", recording_detect)
    out = E.evaluate(net, coder, pyramids, gts, head, class_ids, orig_sizes=orig, mAP_iou_thresholds=(0.5, 0.75), nms_score_threshold=0.0)
    assert len(seen) == 3 and list(out)[-1] == "eval_time" and len(out) == 9 and out["eval_time"] > 0
    resized = [d.resize(s).cpu() for d, s in zip(seen, gt_sizes)]
    p = U.model_pack(resized, gts, torch.device("cpu"))
    for t in (0.5, 0.75):
        ref = M.evaluate(p, 3, t, False)
        for key, name in (("mAP", "map"), ("mAPw", "map_weighted"), ("recall", "recall"), ("AP_joint_classes", "ap_joint_classes")):
            got = out["{}@{:0.2f}".format(key, t)]
            assert isinstance(got, float) and abs(got - float(ref[name])) <= U.AP_ATOL, (key, t)
    assert out["recall@0.50"] > 0
