"""CPU: tests/objective_model.py (our plain torch restatement of target assignment and objective) reproduces every fixture
recorded from the reference: targets exactly, losses and gradients to fp32 rounding.  The model is then the comparator for
shapes too large to store (tests/test_objective_gpu.py)."""
import numpy as np
import pytest
import torch

import objective_cases as OC
import objective_model as M
import objective_util as U

# fp32 rounding: the model and the reference add the same ~1e5 non-negative terms in different orders
RTOL_SCALAR, RTOL_ELEM = 2e-6, 2e-6


def model_targets(name, fx):
    c = OC.CASES[name]
    out = dict(loc=[], cls=[], rem=[], ia=[], ic=[])
    split = [h * w for h, w in c["levels"]]
    loc_levels = torch.from_numpy(fx["loc_preds"]).split(split, 3)
    for level, loc in zip(c["levels"], loc_levels):
        H, W = level
        per_image = [M.encode_image(b, l, d, c["B"], H, W, OC.STRIDE, OC.BOX_SIZE, OC.IOU["pos"], OC.IOU["neg"])
                     for b, l, d in U.level_boxes(name, level, fx["boxes"])]
        out["loc"].append(torch.stack([p[0] for p in per_image]))
        out["cls"].append(torch.stack([p[1] for p in per_image]))
        rem = [M.remap_image(loc[a], b, l, d, c["B"], H, W, OC.STRIDE, OC.BOX_SIZE, OC.IOU["remap_pos"], OC.IOU["remap_neg"])
               for a, (b, l, d) in enumerate(U.level_boxes(name, level, fx["boxes"]))]
        for key, i in (("rem", 0), ("ia", 1), ("ic", 2)):
            out[key].append(torch.stack([r[i] for r in rem]))
    return {k: torch.cat(v, 3 if k == "loc" else 2) for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_model_reproduces_the_reference_targets(name):
    fx = U.load_targets(name)
    t = model_targets(name, fx)
    assert np.array_equal(t["cls"].numpy(), fx["cls_targets"].astype(np.int64))
    assert np.array_equal(t["rem"].numpy(), fx["cls_targets_remapped"].astype(np.int64))
    assert np.array_equal(t["ia"].numpy(), fx["ious_anchor"])
    assert np.array_equal(t["ic"].numpy(), fx["ious_anchor_corrected"])
    assert U.rel_err(t["loc"].numpy(), fx["loc_targets"]) <= 1e-6


@pytest.mark.parametrize("loss", OC.LOSSES)
@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_model_reproduces_the_reference_objective(name, loss):
    c = OC.CASES[name]
    fx, ref = U.load_targets(name), U.load_loss(name, loss)
    loc = torch.from_numpy(fx["loc_preds"]).requires_grad_()
    cls = torch.from_numpy(fx["cls_preds"]).requires_grad_()
    det = torch.from_numpy(fx["cls_preds_for_neg"]).requires_grad_()
    kw = dict(cls_targets_remapped=torch.from_numpy(fx["cls_targets_remapped"].astype(np.int64)), cls_preds_for_neg=det) if c["remap"] else {}
    out = M.objective(loss, loc, torch.from_numpy(fx["loc_targets"]), cls, torch.from_numpy(fx["cls_targets"].astype(np.int64)),
                      patch_mining_mode=c["patch"], **dict(OC.CRITERION, **kw))
    out["loss"].backward()
    for i, key in enumerate(U.SCALARS):
        assert abs(float(out[key]) - float(ref["scalars"][i])) <= RTOL_SCALAR * max(1.0, abs(float(ref["scalars"][i]))), key
    assert np.array_equal(out["pos"].numpy(), ref["pos_mask"]) and np.array_equal(out["neg"].numpy(), ref["neg_mask"])
    assert np.array_equal(out["pos_reg"].numpy(), ref["pos_reg_mask"])
    assert U.rel_err(out["cls_loss"].detach().numpy(), ref["cls_loss"]) <= RTOL_ELEM
    grads = [("dloc", loc), ("dcls", cls)] + ([("dcls_for_neg", det)] if c["remap"] else [])
    for key, t in grads:
        g = t.grad.numpy() if t.grad is not None else np.zeros_like(ref[key])
        assert U.rel_err(g, ref[key]) <= RTOL_ELEM, key
        assert np.array_equal(g != 0, ref[key] != 0), key
