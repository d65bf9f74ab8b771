"""Times the VOC evaluation at 2,000 images x 1,024 labels x 1,000 detections on the HIP device: the stages of
libos2d_eval.so (pack, sort, match, per-class curves, per-class AP, the joint-class pass on its own, finalise), a whole
``compute`` with the sort cached, and the same computation by tests/voc_eval_model.py run eagerly on the same GPU.  CUDA
events, median of 10 after warm-up.

    python tools/time_voc_eval.py                    # one JSON line
    python tools/time_voc_eval.py --images 200       # a smaller dataset
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import voc_eval_cases as VC  # noqa: E402
import voc_eval_model as M  # noqa: E402
from os2d_amd.engine.voc_eval import VocEvaluator  # noqa: E402
from os2d_amd.structures.bounding_box import BoxList  # noqa: E402
from os2d_amd.structures.feature_map import FeatureMapSize  # noqa: E402


def median_ms(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    if not torch.cuda.is_available():
        raise RuntimeError("needs a HIP device")
    dev = torch.device("cuda:0")
    n_images = int(sys.argv[sys.argv.index("--images") + 1]) if "--images" in sys.argv else 2000
    c = VC.large(n_images=n_images)
    size = FeatureMapSize(w=c["size"][0], h=c["size"][1])
    on_dev = {k: c[k].to(dev) for k in ("boxes", "scores", "labels")}
    ev = VocEvaluator(num_labels=1024)
    for i in range(n_images):
        p = BoxList(on_dev["boxes"][i], size)
        p.add_field("scores", on_dev["scores"][i])
        p.add_field("labels", on_dev["labels"][i])
        g = BoxList(c["gt_boxes"][i], size)
        g.add_field("labels", c["gt_labels"][i])
        g.add_field("difficult", c["difficult"][i])
        ev.add(p, g)
    N, n = c["scores"].shape
    m = c["gt_labels"].shape[1]
    packed = dict(boxes=on_dev["boxes"].reshape(-1, 4), scores=on_dev["scores"].reshape(-1), labels=on_dev["labels"].reshape(-1),
                  image=torch.arange(N, device=dev).repeat_interleave(n), gt_boxes=c["gt_boxes"].reshape(-1, 4).to(dev),
                  gt_labels=c["gt_labels"].reshape(-1).to(dev), gt_difficult=c["difficult"].reshape(-1).bool().to(dev),
                  gt_image=torch.arange(N, device=dev).repeat_interleave(m), N=N)
    result = dict(shape=dict(images=N, labels=1024, detections_per_image=n, ground_truth_per_image=m), unit="ms, median of 10")

    def pack_and_sort():
        ev._packed = None
        ev._pack()
    result["hip_pack_count_sort"] = median_ms(pack_and_sort)
    p = ev._pack()
    L = p["L"]
    rec_last = torch.zeros(L + 1, dtype=torch.float64, device=dev)
    acc = torch.zeros(L + 1, 11, dtype=torch.float64, device=dev)
    result["hip_match"] = median_ms(lambda: ev._match(p, 0.5))
    match = ev._match(p, 0.5)
    result["hip_scans_prec_rec_per_class"] = median_ms(lambda: ev._curves(p, match, False, rec_last))
    _, prec, rec = ev._curves(p, match, False, rec_last)
    result["hip_ap_per_class"] = median_ms(lambda: ev._ap(p, prec, rec, False, False, acc))
    result["hip_ap_per_class_07"] = median_ms(lambda: ev._ap(p, prec, rec, False, True, acc))

    def joint():
        _, pj, rj = ev._curves(p, match, True, rec_last)
        ev._ap(p, pj, rj, True, False, acc)
    result["hip_joint_class_pass"] = median_ms(joint)
    result["hip_compute_sort_cached"] = median_ms(lambda: ev.compute(0.5, with_curves=False))
    result["model_same_gpu"] = median_ms(lambda: M.evaluate(packed, 1024, 0.5, False), warmup=1, reps=10)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
