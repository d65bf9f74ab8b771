"""Times the training objective at the reference's training shape (A = 4 images, B = 15 classes, 38 x 38 maps) on the HIP
device: (i) remap_anchor_targets, (ii) the criterion forward, (iii) its backward - each with the HIP kernels and with
tests/objective_model.py run eagerly on the same GPU (the stand-in for the reference's torch code; it is vectorised over
anchors, so it launches less than the reference's per-(image, label) loops).  CUDA events, median of 10 after warm-up.

    python tools/time_train_objective.py                    # one JSON line
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_train_objective.py --once hip|model
                                                            # one remap + forward + backward, for counting launches
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import objective_cases as OC  # noqa: E402
import objective_model as M  # noqa: E402
import objective_util as U  # noqa: E402
from os2d_amd.engine.objective import Os2dObjective  # noqa: E402
from os2d_amd.modeling.box_coder import Os2dBoxCoder, BoxGridGenerator  # noqa: E402
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
    once = sys.argv[sys.argv.index("--once") + 1] if "--once" in sys.argv else None
    name = "train"
    c = OC.CASES[name]
    H, W = c["levels"][0]
    fx = U.load_targets(name)
    img = FeatureMapSize(w=OC.image_size((H, W))[0], h=OC.image_size((H, W))[1])
    gen = BoxGridGenerator(box_size=FeatureMapSize(w=OC.BOX_SIZE, h=OC.BOX_SIZE), box_stride=FeatureMapSize(w=OC.STRIDE, h=OC.STRIDE))
    coder = Os2dBoxCoder(OC.IOU["pos"], OC.IOU["neg"], OC.IOU["remap_pos"], OC.IOU["remap_neg"], gen, lambda s: FeatureMapSize(w=W, h=H))
    bls = []
    for b, labels, difficult in fx["boxes"]:
        bl = BoxList(torch.from_numpy(b), img)
        bl.add_field("labels", torch.from_numpy(labels))
        bl.add_field("difficult", torch.from_numpy(difficult))
        bls.append(bl)
    dev_boxes = [(torch.from_numpy(b).to(dev), torch.from_numpy(l).to(dev), torch.from_numpy(d).to(dev)) for b, l, d in fx["boxes"]]
    t = lambda a, dt=None: torch.from_numpy(a if dt is None else a.astype(dt)).to(dev)   # noqa: E731
    loc, cls, det = t(fx["loc_preds"]).requires_grad_(), t(fx["cls_preds"]).requires_grad_(), t(fx["cls_preds_for_neg"]).requires_grad_()
    loc_t, cls_t, rem = t(fx["loc_targets"]), t(fx["cls_targets"], np.int64), t(fx["cls_targets_remapped"], np.int64)

    def remap_hip():
        return coder.remap_anchor_targets(loc, [img] * c["A"], None, bls)

    def remap_model():
        return [M.remap_image(loc.detach()[a], b, l, d, c["B"], H, W, OC.STRIDE, OC.BOX_SIZE, OC.IOU["remap_pos"], OC.IOU["remap_neg"])
                for a, (b, l, d) in enumerate(dev_boxes)]

    result = dict(shape=dict(A=c["A"], B=c["B"], H=H, W=W), unit="ms, median of 10")
    for loss in OC.LOSSES:
        crit = Os2dObjective(loss, keep_class_loss_on_cpu=False, **OC.CRITERION)

        def fwd_hip():
            return crit(loc, loc_t, cls, cls_t, cls_targets_remapped=rem, cls_preds_for_neg=det)["loss"]

        def fwd_model():
            return M.objective(loss, loc, loc_t, cls, cls_t, cls_targets_remapped=rem, cls_preds_for_neg=det, **OC.CRITERION)["loss"]
        if once:
            (remap_hip if once == "hip" else remap_model)()
            value = (fwd_hip if once == "hip" else fwd_model)()
            torch.autograd.grad(value, [loc, cls, det])
            torch.cuda.synchronize()
            continue
        for tag, fwd in (("hip", fwd_hip), ("model", fwd_model)):
            held = [fwd()]

            def bwd():
                torch.autograd.grad(held[0], [loc, cls, det], retain_graph=True)
            result["{}_{}_forward".format(loss, tag)] = median_ms(fwd)
            result["{}_{}_backward".format(loss, tag)] = median_ms(bwd)
    if not once:
        result["remap_hip"] = median_ms(remap_hip)
        result["remap_model"] = median_ms(remap_model)
        print(json.dumps(result))


if __name__ == "__main__":
    main()
