"""Records tests/golden/objective_*.npz from the reference implementation on the CPU: Os2dBoxCoder.encode,
remap_anchor_targets and Os2dObjective (forward and autograd backward) on the inputs of tests/objective_cases.py.

    python tests/golden/make_objective_golden.py

The reference is imported as in make_golden.py, with its torchvision stand-in, plus torchvision's Matcher restated from its
published form (torchvision/models/detection/_utils.py; the one in make_golden.py is an empty shell because inference never
reaches it).  Data only is written: boxes, targets, IoUs, loss scalars, per-element losses, masks, gradients.

RLL and (inf * num_pos).long(): the reference sets neg_to_pos_ratio = inf for RLL; on a device the product saturates to the
largest int64 (every negative is used, as objective.py:40-42 intends), on the CPU it gives the smallest (no negative is used).
The project's semantics are the device's, so neg_to_pos_ratio is set to 2**40 on the reference object after construction and
the CPU run records the intended numbers."""
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


class Matcher(object):
    """torchvision.models.detection._utils.Matcher as published, without the low-quality branch (the reference never asks
    for it)."""
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False):
        assert low_threshold <= high_threshold and not allow_low_quality_matches
        self.high_threshold, self.low_threshold = high_threshold, low_threshold

    def __call__(self, match_quality_matrix):
        matched_vals, matches = match_quality_matrix.max(dim=0)
        below = matched_vals < self.low_threshold
        between = (matched_vals >= self.low_threshold) & (matched_vals < self.high_threshold)
        matches[below] = self.BELOW_LOW_THRESHOLD
        matches[between] = self.BETWEEN_THRESHOLDS
        return matches


sys.modules["torchvision.models.detection._utils"].Matcher = Matcher
sys.path.insert(0, make_golden.REFERENCE)

from os2d.modeling.box_coder import Os2dBoxCoder, BoxGridGenerator  # noqa: E402
from os2d.engine.objective import Os2dObjective  # noqa: E402
from os2d.structures.bounding_box import BoxList  # noqa: E402
from os2d.structures.feature_map import FeatureMapSize  # noqa: E402

import objective_cases as OC  # noqa: E402

BAND, BAND_CAP = 1e-5, 1.0 / 2000


def boxlists(name, level):
    w0, h0 = OC.image_size(OC.CASES[name]["levels"][0])
    w, h = OC.image_size(level)
    out = []
    for boxes, labels, difficult in OC.draw_boxes(name):
        b = torch.from_numpy(boxes).clone()
        b[:, 0::2] *= float(w) / w0
        b[:, 1::2] *= float(h) / h0
        bl = BoxList(b, FeatureMapSize(w=w, h=h), mode="xyxy")
        bl.add_field("labels", torch.from_numpy(labels))
        bl.add_field("difficult", torch.from_numpy(difficult))
        out.append(bl)
    return out


def record(name):
    c = OC.CASES[name]
    A, B = c["A"], c["B"]
    sizes = {FeatureMapSize(w=OC.image_size(l)[0], h=OC.image_size(l)[1]): FeatureMapSize(w=l[1], h=l[0]) for l in c["levels"]}
    gen = BoxGridGenerator(box_size=FeatureMapSize(w=OC.BOX_SIZE, h=OC.BOX_SIZE), box_stride=FeatureMapSize(w=OC.STRIDE, h=OC.STRIDE))
    coder = Os2dBoxCoder(OC.IOU["pos"], OC.IOU["neg"], OC.IOU["remap_pos"], OC.IOU["remap_neg"], gen, lambda s: sizes[s])
    loc_t, cls_t, rem, iou_a, iou_c, level_boxes = [], [], [], [], [], []
    for level in c["levels"]:
        img = FeatureMapSize(w=OC.image_size(level)[0], h=OC.image_size(level)[1])
        bls = boxlists(name, level)
        level_boxes.append(bls)
        enc = [coder.encode(b, img, B) for b in bls]
        loc_t.append(torch.stack([e[0] for e in enc]))
        cls_t.append(torch.stack([e[1] for e in enc]))
    loc_np, cls_np, det_np = OC.draw_predictions(name, torch.cat(loc_t, 3).numpy())
    split = [l[0] * l[1] for l in c["levels"]]
    loc_levels = list(torch.from_numpy(loc_np).split(split, 3))
    for level, bls, loc in zip(c["levels"], level_boxes, loc_levels):
        img = FeatureMapSize(w=OC.image_size(level)[0], h=OC.image_size(level)[1])
        r, ia, ic = coder.remap_anchor_targets(loc.contiguous(), [img] * A, None, bls)
        rem.append(r)
        iou_a.append(ia)
        iou_c.append(ic)
    # remap condition: few anchors sit within BAND of a remap threshold (exp differs in the last bit between CPU and device)
    ic = torch.cat(iou_c, 2)
    near = ((ic - OC.IOU["remap_pos"]).abs() < BAND) | ((ic - OC.IOU["remap_neg"]).abs() < BAND)
    assert int(near.sum()) <= BAND_CAP * near.numel(), "{}: {} anchors inside the threshold band".format(name, int(near.sum()))
    targets = dict(loc_targets=torch.cat(loc_t, 3).numpy(), cls_targets=torch.cat(cls_t, 2).numpy().astype(np.int8),
                   cls_targets_remapped=torch.cat(rem, 2).numpy().astype(np.int8), ious_anchor=torch.cat(iou_a, 2).numpy(),
                   ious_anchor_corrected=ic.numpy(), levels=np.array(c["levels"], np.int32))
    for a, (boxes, labels, difficult) in enumerate(OC.draw_boxes(name)):
        targets["boxes_{}".format(a)] = boxes
        targets["labels_{}".format(a)] = labels
        targets["difficult_{}".format(a)] = difficult
    if name != "train":     # the small inputs are stored too; the training-shape ones are redrawn from the seed
        targets.update(loc_preds=loc_np, cls_preds=cls_np, cls_preds_for_neg=det_np)
    targets["input_checksum"] = np.float64(loc_np.astype(np.float64).sum() + cls_np.astype(np.float64).sum() + det_np.astype(np.float64).sum())
    save("objective_{}_targets.npz".format(name), targets)

    for loss_name in OC.LOSSES:
        crit = Os2dObjective(loss_name, **OC.CRITERION)
        if loss_name == "RLL":
            crit.neg_to_pos_ratio = 2 ** 40          # see the module docstring
        loc = [l.clone().contiguous().requires_grad_() for l in loc_levels]
        cls = [t.clone().contiguous().requires_grad_() for t in torch.from_numpy(cls_np).split(split, 2)]
        det = [t.clone().contiguous().requires_grad_() for t in torch.from_numpy(det_np).split(split, 2)]
        one = len(split) == 1
        args = [loc[0] if one else loc, loc_t[0] if one else loc_t, cls[0] if one else cls, cls_t[0] if one else cls_t]
        kw = dict(cls_targets_remapped=(rem[0] if one else rem), cls_preds_for_neg=(det[0] if one else det)) if c["remap"] else {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = crit(*args, patch_mining_mode=c["patch"], **kw)
        losses, per_anchor = res if c["patch"] else (res, None)
        losses["loss"].backward()
        keys = [k.replace("_hardneg{}".format(2 ** 40), "") for k in losses.keys()]     # RLL: the names of neg_to_pos_ratio = inf
        losses = dict(zip(keys, losses.values()))
        out = dict(keys=np.array(keys), scalars=np.array([float(losses[k]) for k in keys if k != "class_loss_per_element_detached_cpu"], np.float32),
                   cls_loss=losses["class_loss_per_element_detached_cpu"].numpy())
        out["dloc"] = torch.cat([t.grad if t.grad is not None else torch.zeros_like(t) for t in loc], 3).numpy()
        out["dcls"] = torch.cat([t.grad if t.grad is not None else torch.zeros_like(t) for t in cls], 2).numpy()
        if c["remap"]:
            out["dcls_for_neg"] = torch.cat([t.grad if t.grad is not None else torch.zeros_like(t) for t in det], 2).numpy()
        # the masks: positives of the class loss, the negatives that entered it, positives of the regression
        tgt = torch.cat(rem, 2) if c["remap"] else torch.cat(cls_t, 2)
        pos = tgt > 0
        cand = ~(pos | (tgt == -1))
        cl = torch.from_numpy(out["cls_loss"])
        num_pos = int(pos.sum())
        if c["patch"]:
            neg = torch.cat(list(per_anchor["neg_mask"]), 2)
            assert torch.equal(torch.cat(list(per_anchor["pos_mask"]), 2), pos)
            out["loc_loss"] = torch.cat(list(per_anchor["loc_loss"]), 2).numpy()
        elif loss_name == "RLL":
            neg = cand & (num_pos > 0)
        else:
            k = OC.CRITERION["neg_to_pos_ratio"] * num_pos
            cand_losses = torch.sort(cl[cand], descending=True)[0]
            if num_pos > 0:
                # mining really cuts, and not at a tie (the reference's sort is unstable)
                assert int((cand_losses > 0).sum()) > k, "{}: {} positive candidate losses, k = {}".format(name, int((cand_losses > 0).sum()), k)
                assert float(cand_losses[k - 1]) > float(cand_losses[k]), "{}: tie at the mining cut".format(name)
                neg = cand & (cl >= cand_losses[k - 1])
            else:
                neg = torch.zeros_like(cand)
        out["pos_mask"], out["neg_mask"], out["pos_reg_mask"] = pos.numpy(), neg.numpy(), (torch.cat(cls_t, 2) > 0).numpy()
        # the recorded masks give the recorded scalars back
        i_pos, i_neg = [i for i, k_ in enumerate(k_ for k_ in keys if k_ != "class_loss_per_element_detached_cpu") if k_.endswith("_pos") or "_neg" in k_]
        n1 = max(num_pos, 1)
        assert abs(float(cl[pos].double().sum()) / n1 - out["scalars"][i_pos]) <= 1e-5 * max(1.0, abs(out["scalars"][i_pos]))
        assert abs(float(cl[neg].double().sum()) / n1 - out["scalars"][i_neg]) <= 1e-5 * max(1.0, abs(out["scalars"][i_neg])), \
            (name, loss_name, float(cl[neg].double().sum()) / n1, out["scalars"][i_neg])
        out["num_pos"] = np.int64(num_pos)
        save("objective_{}_{}.npz".format(name, loss_name.lower()), out)
        print(name, loss_name, dict(zip([k for k in keys if k != "class_loss_per_element_detached_cpu"], out["scalars"])), "num_pos", num_pos,
              "negatives", int(neg.sum()))


def save(fname, arrays):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 1 << 20, "{} is {} bytes".format(fname, size)
    print("wrote", fname, size)


if __name__ == "__main__":
    for case in OC.CASES:
        record(case)
