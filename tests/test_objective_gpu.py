"""GPU: target assignment (Os2dBoxCoder.encode / encode_batch / remap_anchor_targets), Os2dObjective and train_one_batch on the
HIP kernels against the fixtures recorded from the reference (tests/golden/objective_*.npz) and, for shapes too large to
store, against tests/objective_model.py.  Tolerances: tests/golden/objective_pins.json = 3x the error measured against the
fixtures on an MI355X; every figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest
import torch

import objective_cases as OC
import objective_model as M
import objective_util as U

pytestmark = pytest.mark.gpu


def make_coder(levels):
    from os2d_amd.modeling.box_coder import Os2dBoxCoder, BoxGridGenerator
    from os2d_amd.structures.feature_map import FeatureMapSize
    sizes = {FeatureMapSize(w=OC.image_size(l)[0], h=OC.image_size(l)[1]): FeatureMapSize(w=l[1], h=l[0]) for l in levels}
    gen = BoxGridGenerator(box_size=FeatureMapSize(w=OC.BOX_SIZE, h=OC.BOX_SIZE), box_stride=FeatureMapSize(w=OC.STRIDE, h=OC.STRIDE))
    return Os2dBoxCoder(OC.IOU["pos"], OC.IOU["neg"], OC.IOU["remap_pos"], OC.IOU["remap_neg"], gen, lambda s: sizes[s])


def boxlists(name, level, fx, device=None):
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    w, h = OC.image_size(level)
    out = []
    for b, labels, difficult in U.level_boxes(name, level, fx["boxes"]):
        bl = BoxList(b if device is None else b.to(device), FeatureMapSize(w=w, h=h))
        bl.add_field("labels", labels)
        bl.add_field("difficult", difficult)
        out.append(bl)
    return out


def make_criterion(loss, **kw):
    from os2d_amd.engine.objective import Os2dObjective
    return Os2dObjective(loss, **dict(OC.CRITERION, **kw))


def run_objective(name, loss, fx, device, lists=False):
    """-> (losses dict, per-anchor dict or None, grads dict, masks) of our criterion on a fixture's inputs."""
    c = OC.CASES[name]
    split = [h * w for h, w in c["levels"]]
    dev = lambda a, dt=None: torch.from_numpy(a if dt is None else a.astype(dt)).to(device)   # noqa: E731
    loc, cls, det = dev(fx["loc_preds"]).requires_grad_(), dev(fx["cls_preds"]).requires_grad_(), dev(fx["cls_preds_for_neg"]).requires_grad_()
    loc_t, cls_t, rem = dev(fx["loc_targets"]), dev(fx["cls_targets"], np.int64), dev(fx["cls_targets_remapped"], np.int64)
    pyr = (lambda t, dim: list(t.split(split, dim))) if lists else (lambda t, dim: t)
    kw = dict(cls_targets_remapped=pyr(rem, 2), cls_preds_for_neg=pyr(det, 2)) if c["remap"] else {}
    crit = make_criterion(loss)
    res = crit(pyr(loc, 3), pyr(loc_t, 3), pyr(cls, 2), pyr(cls_t, 2), patch_mining_mode=c["patch"], **kw)
    losses, per_anchor = res if c["patch"] else (res, None)
    wrt = [loc, cls] + ([det] if c["remap"] else [])
    g = torch.autograd.grad(losses["loss"], wrt, allow_unused=True)
    g = [torch.zeros_like(t) if x is None else x for x, t in zip(g, wrt)]
    grads = dict(zip(("dloc", "dcls", "dcls_for_neg"), g))
    masks = crit.element_masks(pyr(loc.detach(), 3), pyr(loc_t, 3), pyr(cls.detach(), 2), pyr(cls_t, 2), patch_mining_mode=c["patch"],
                               **({k: (v.detach() if isinstance(v, torch.Tensor) else [x.detach() for x in v]) for k, v in kw.items()}))
    torch.cuda.synchronize()
    return crit, losses, per_anchor, grads, masks


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_encode_matches_the_reference(device, name):
    c = OC.CASES[name]
    fx, pins = U.load_targets(name), U.pins()
    coder = make_coder(c["levels"])
    from os2d_amd.structures.feature_map import FeatureMapSize
    locs, clss = [], []
    for level in c["levels"]:
        img = FeatureMapSize(w=OC.image_size(level)[0], h=OC.image_size(level)[1])
        bls = boxlists(name, level, fx)
        loc_t, cls_t = coder.encode_batch(bls, img, c["B"], device)
        assert loc_t.dtype == torch.float32 and cls_t.dtype == torch.int64
        one_loc, one_cls = coder.encode(bls[-1], img, c["B"])         # the reference's per-image call
        assert torch.equal(one_loc, loc_t[-1]) and torch.equal(one_cls, cls_t[-1]) and tuple(one_cls.shape) == (c["B"], level[0] * level[1])
        locs.append(loc_t)
        clss.append(cls_t)
    cls_t, loc_t = torch.cat(clss, 2).cpu().numpy(), torch.cat(locs, 3).cpu().numpy()
    err = U.rel_err(loc_t, fx["loc_targets"])
    print("\n[objective] {} encode: cls_targets mismatches {} loc_targets rel err {:.3e}".format(
        name, int((cls_t != fx["cls_targets"]).sum()), err))
    assert np.array_equal(cls_t, fx["cls_targets"].astype(np.int64))                # exactly: no exp, IoU operation for operation
    assert err <= pins["loc_targets"]                                                # all anchors, dummy-box values included
    if len(c["levels"]) > 1:
        pl, pc = coder.encode_pyramid(boxlists(name, c["levels"][0], fx)[0].to(device), [FeatureMapSize(w=OC.image_size(c["levels"][0])[0], h=OC.image_size(c["levels"][0])[1])], c["B"])
        assert torch.equal(pl[0], locs[0][0]) and torch.equal(pc[0], clss[0][0])
    with pytest.raises(NotImplementedError, match="default_box_transform"):
        coder.encode(boxlists(name, c["levels"][0], fx)[0], FeatureMapSize(w=1, h=1), c["B"], default_box_transform=lambda b: b)


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_remap_matches_the_reference(device, name):
    c = OC.CASES[name]
    fx, pins = U.load_targets(name), U.pins()
    coder = make_coder(c["levels"])
    from os2d_amd.structures.feature_map import FeatureMapSize
    split = [h * w for h, w in c["levels"]]
    rems, ias, ics = [], [], []
    for level, loc in zip(c["levels"], torch.from_numpy(fx["loc_preds"]).split(split, 3)):
        img = FeatureMapSize(w=OC.image_size(level)[0], h=OC.image_size(level)[1])
        rem, ia, ic = coder.remap_anchor_targets(loc.contiguous().to(device), [img] * c["A"], None, boxlists(name, level, fx))
        assert rem.dtype == torch.int64 and ia.dtype == torch.float32
        rems.append(rem), ias.append(ia), ics.append(ic)
    rem, ia, ic = [torch.cat(t, 2).cpu().numpy() for t in (rems, ias, ics)]
    ref_ic = fx["ious_anchor_corrected"]
    band = (np.abs(ref_ic - OC.IOU["remap_pos"]) < U.BAND) | (np.abs(ref_ic - OC.IOU["remap_neg"]) < U.BAND)
    mism = rem != fx["cls_targets_remapped"]
    print("\n[objective] {} remap: mismatches {} (in band {}), anchors in band {} of {}, ious_anchor equal {}, corrected abs err {:.3e}".format(
        name, int(mism.sum()), int((mism & band).sum()), int(band.sum()), band.size, bool(np.array_equal(ia, fx["ious_anchor"])),
        float(np.abs(ic - ref_ic).max())))
    assert band.sum() <= U.BAND_CAP * band.size
    assert not (mism & ~band).any()
    assert np.array_equal(ia, fx["ious_anchor"])                                     # the plain anchor: no exp involved
    assert float(np.abs(ic - ref_ic).max()) <= pins["ious_anchor_corrected_abs"]
    with pytest.raises(NotImplementedError, match="box_reverse_transform"):
        coder.remap_anchor_targets(torch.zeros(1, 1, 4, 1, device=device), [None], None, [None], box_reverse_transform=[None])


@pytest.mark.parametrize("loss", OC.LOSSES)
@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_objective_matches_the_reference(device, name, loss):
    c = OC.CASES[name]
    fx, ref, pins = U.load_targets(name), U.load_loss(name, loss), U.pins()
    crit, losses, per_anchor, grads, masks = run_objective(name, loss, fx, device, lists=len(c["levels"]) > 1)
    keys = [k for k in losses.keys()]
    assert keys == [str(k) for k in ref["keys"]], keys
    if loss == "RLL":
        assert "cls_RLL_neg" in keys and "cls_RLL" in keys
    else:
        assert "cls_ContrastiveLoss_neg_hardneg3" in keys and "cls_ContrastiveLoss_hardneg3" in keys
    scalar_keys = [k for k in keys if k != "class_loss_per_element_detached_cpu"]
    figures = {}
    for k, r in zip(scalar_keys, ref["scalars"]):
        assert losses[k].is_cuda and losses[k].dim() == 0
        figures[k] = abs(float(losses[k]) - float(r)) / max(abs(float(r)), 1e-30) if float(r) != 0 else abs(float(losses[k]))
    host = losses["class_loss_per_element_detached_cpu"]
    assert not host.is_cuda
    figures["cls_loss"] = U.rel_err(host.numpy(), ref["cls_loss"])
    for k, g in grads.items():
        figures[k] = U.rel_err(g.cpu().numpy(), ref[k])
    print("\n[objective] {} {}: {}".format(name, loss, {k: "{:.3e}".format(v) for k, v in figures.items()}))
    for k in scalar_keys:
        assert figures[k] <= pins["scalars"], k
    for k in ["cls_loss"] + list(grads):
        assert figures[k] <= pins[k], k
    for k, g in grads.items():                                                       # non-zero exactly where the fixture's are
        assert np.array_equal(g.cpu().numpy() != 0, ref[k] != 0), k
    cls_loss, pos, neg, pos_reg = masks
    assert np.array_equal(pos.cpu().numpy(), ref["pos_mask"]) and np.array_equal(neg.cpu().numpy(), ref["neg_mask"])
    assert np.array_equal(pos_reg.cpu().numpy(), ref["pos_reg_mask"])
    if c["patch"]:
        split = [h * w for h, w in c["levels"]]
        assert [t.shape[2] for t in per_anchor["cls_loss"]] == split
        assert np.array_equal(torch.cat(per_anchor["neg_mask"], 2).cpu().numpy(), ref["neg_mask"])
        assert np.array_equal(torch.cat(per_anchor["pos_for_regression"], 2).cpu().numpy(), ref["pos_reg_mask"])
        loc_err = U.rel_err(torch.cat(per_anchor["loc_loss"], 2).cpu().numpy(), ref["loc_loss"])
        print("[objective] {} {}: per-anchor loc_loss rel err {:.3e}".format(name, loss, loc_err))
        assert loc_err <= pins["loc_loss"]
    # a second run gives the same bits
    _, losses2, _, grads2, masks2 = run_objective(name, loss, fx, device, lists=len(c["levels"]) > 1)
    for k in scalar_keys:
        assert torch.equal(losses[k], losses2[k]), k
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    assert torch.equal(masks[0], masks2[0]) and torch.equal(masks[2], masks2[2])


def test_objective_options(device):
    """The constructor switch leaves the CPU copy out; inputs may or may not require grad; CPU tensors raise."""
    fx = U.load_targets("small")
    dev = lambda a, dt=None: torch.from_numpy(a if dt is None else a.astype(dt)).to(device)   # noqa: E731
    crit = make_criterion("RLL", keep_class_loss_on_cpu=False)
    loc, cls = dev(fx["loc_preds"]), dev(fx["cls_preds"]).requires_grad_()
    losses = crit(loc, dev(fx["loc_targets"]), cls, dev(fx["cls_targets"], np.int64), cls_preds_for_neg=dev(fx["cls_preds_for_neg"]))
    assert "class_loss_per_element_detached_cpu" not in losses
    losses["loss"].backward()
    assert cls.grad is not None and float(cls.grad.abs().sum()) > 0 and loc.grad is None
    with pytest.raises(RuntimeError, match="HIP device only"):
        crit(loc.cpu(), dev(fx["loc_targets"]).cpu(), cls.detach().cpu(), dev(fx["cls_targets"], np.int64).cpu())
    from os2d_amd.engine.objective import Os2dObjective
    with pytest.raises(RuntimeError, match="Unknown class_loss"):
        Os2dObjective("Focal", **OC.CRITERION)


@pytest.mark.parametrize("loss,ratio", [("RLL", 3), ("ContrastiveLoss", 3), ("ContrastiveLoss", 40)])
def test_large_shape_against_the_model(device, loss, ratio):
    """A x B x HW of about 2 million: beyond one block's reach in every reduction.  ratio 40 makes k larger than the number of
    candidates; with ratio 3 k exceeds the candidates with a positive loss, so the cut falls among equal (zero) losses and
    the increasing-index rule decides the mask."""
    A, B, HW = 4, 16, 181 * 181
    pins = U.pins()
    rs = np.random.RandomState(7)
    dev = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
    cls_t = dev(rs.choice([1, 0, -1], size=(A, B, HW), p=[0.05, 0.85, 0.10]).astype(np.int64))
    rem = dev(rs.choice([1, 0, -1], size=(A, B, HW), p=[0.04, 0.86, 0.10]).astype(np.int64))
    loc_t = dev(rs.randn(A, B, 4, HW).astype(np.float32))
    loc = dev((rs.randn(A, B, 4, HW) * 1.5).astype(np.float32)).requires_grad_()
    cls = dev((rs.rand(A, B, HW) * 1.4 - 0.4).astype(np.float32)).requires_grad_()
    det = dev((rs.rand(A, B, HW) * 1.4 - 0.8).astype(np.float32)).requires_grad_()
    kw = dict(OC.CRITERION, neg_to_pos_ratio=ratio)
    crit = make_criterion(loss, neg_to_pos_ratio=ratio, keep_class_loss_on_cpu=False)
    losses = crit(loc, loc_t, cls, cls_t, cls_targets_remapped=rem, cls_preds_for_neg=det)
    g = torch.autograd.grad(losses["loss"], [loc, cls, det])
    cls_loss, pos, neg, pos_reg = crit.element_masks(loc.detach(), loc_t, cls.detach(), cls_t, cls_targets_remapped=rem, cls_preds_for_neg=det.detach())
    ref = M.objective(loss, loc, loc_t, cls, cls_t, cls_targets_remapped=rem, cls_preds_for_neg=det, **kw)
    rg = torch.autograd.grad(ref["loss"], [loc, cls, det], allow_unused=True)
    rg = [torch.zeros_like(t) if x is None else x for x, t in zip(rg, (loc, cls, det))]
    if loss == "ContrastiveLoss":
        k, cand = ratio * int(ref["pos"].sum()), int((~(ref["pos"] | (rem == -1))).sum())
        assert (k > cand) == (ratio == 40)
    _, cls_name, pos_name, neg_name = crit.loss_names()
    fig = {k: abs(float(losses[n]) - float(ref[k])) / max(abs(float(ref[k])), 1e-30)
           for k, n in (("loss", "loss"), ("loc", "loc_smoothL1"), ("cls", cls_name), ("cls_pos", pos_name), ("cls_neg", neg_name))}
    fig["cls_loss"] = U.rel_err(cls_loss.cpu().numpy(), ref["cls_loss"].detach().cpu().numpy())
    for key, a, b in zip(("dloc", "dcls", "dcls_for_neg"), g, rg):
        fig[key] = U.rel_err(a.cpu().numpy(), b.cpu().numpy())
    print("\n[objective] large {} ratio {}: {}".format(loss, ratio, {k: "{:.3e}".format(v) for k, v in fig.items()}))
    assert torch.equal(pos, ref["pos"]) and torch.equal(neg, ref["neg"]) and torch.equal(pos_reg, ref["pos_reg"])
    # The comparator here is the model on the same device, not the reference.  The scalars keep the pin of the fixtures.  The
    # per-element quantities of RLL carry a per-label fp32 sum of A * HW = 131,044 weights on BOTH sides (ours: 256-wide trees,
    # then 512 partials in sequence, expected error sqrt(520) * 2^-24 = 1.4e-6; torch's pairwise sum 2.5e-7) and exp() of an
    # argument up to 6.9 whose rounding gives 4e-7 on each side: 3e-6 in all - reasoned, not measured.
    for k in ("loss", "loc", "cls", "cls_pos", "cls_neg"):
        assert fig[k] <= pins["scalars"], k
    for k in ("cls_loss", "dloc", "dcls", "dcls_for_neg"):
        assert fig[k] <= pins["large_shape_elementwise"], k


def test_nothing_synchronises_with_the_host(device):
    """remap_anchor_targets, the criterion and the backward of the loss with respect to leaf tensors under
    torch.cuda.set_sync_debug_mode("error")."""
    name = "train"
    c = OC.CASES[name]
    fx = U.load_targets(name)
    coder = make_coder(c["levels"])
    from os2d_amd.structures.feature_map import FeatureMapSize
    img = FeatureMapSize(w=OC.image_size(c["levels"][0])[0], h=OC.image_size(c["levels"][0])[1])
    dev = lambda a, dt=None: torch.from_numpy(a if dt is None else a.astype(dt)).to(device)   # noqa: E731
    loc, cls, det = dev(fx["loc_preds"]).requires_grad_(), dev(fx["cls_preds"]).requires_grad_(), dev(fx["cls_preds_for_neg"]).requires_grad_()
    loc_t, cls_t = dev(fx["loc_targets"]), dev(fx["cls_targets"], np.int64)
    bls = boxlists(name, c["levels"][0], fx)
    crits = [make_criterion(l, keep_class_loss_on_cpu=False) for l in OC.LOSSES]
    for crit in crits:      # warm-up: library loading and first launches
        rem, _, _ = coder.remap_anchor_targets(loc, [img] * c["A"], None, bls)
        torch.autograd.grad(crit(loc, loc_t, cls, cls_t, cls_targets_remapped=rem, cls_preds_for_neg=det)["loss"], [loc, cls, det])
    torch.cuda.synchronize()
    # is the mode effective on this build?  A device-to-host read must raise under it.
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            float(cls_t.sum())
            effective = False
        except RuntimeError:
            effective = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not effective:
        pytest.skip("torch.cuda.set_sync_debug_mode has no effect on this torch-ROCm build")
    torch.cuda.set_sync_debug_mode("error")
    try:
        for crit in crits:
            rem, _, _ = coder.remap_anchor_targets(loc, [img] * c["A"], None, bls)
            losses = crit(loc, loc_t, cls, cls_t, cls_targets_remapped=rem, cls_preds_for_neg=det)
            grads = torch.autograd.grad(losses["loss"], [loc, cls, det])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) for g in grads)


def test_train_one_batch_on_a_synthetic_model(device):
    """Three steps of train_one_batch with boxes placed on anchors: the loss is finite and every trainable parameter moves."""
    from os2d_amd.engine.train import train_one_batch, forward_train, get_trainable_parameters
    from os2d_amd.modeling.model import Os2dModel
    from os2d_amd.modeling.box_coder import Os2dBoxCoder
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    from os2d_amd.utils import synthetic
    net = Os2dModel(is_cuda=False, merge_branch_parameters=True, backbone_arch="resnet50", use_inverse_geom_model=True, simplify_affine=False)
    net.load_state_dict(synthetic.fill_model_state(net.state_dict(), seed=31, P=6))
    net.to(device)
    net.train(freeze_bn_in_extractor=True, freeze_bn_transform=True)
    A, B = 2, 3
    img_size = FeatureMapSize(w=192, h=160)
    images = synthetic.randn_tensor((A, 3, img_size.h, img_size.w), seed=41).to(device)
    class_images = [synthetic.randn_tensor((3, 64 + 16 * b, 80), seed=50 + b).to(device) for b in range(B)]
    coder = Os2dBoxCoder(0.5, 0.1, 0.8, 0.4, net.os2d_head_creator.box_grid_generator_image_level, net.get_feature_map_size)
    anchors = coder._get_default_boxes(img_size).bbox_xyxy
    batch_boxes = []
    for a in range(A):
        idx = torch.tensor([(7 * a + 5 * b + 3) % anchors.shape[0] for b in range(B)])
        bl = BoxList(anchors[idx].clone(), img_size)
        bl.add_field("labels", torch.arange(B))
        bl.add_field("difficult", torch.zeros(B, dtype=torch.bool))
        batch_boxes.append(bl)
    criterion = make_criterion("RLL", keep_class_loss_on_cpu=False)
    params = get_trainable_parameters(net)
    assert params
    # plain SGD; the rate is large enough that one step moves a BatchNorm weight of ~1 by more than its fp32 spacing even where
    # the gradient is ~1e-5 (a smaller rate leaves such parameters bit-identical although their gradient is not zero)
    optimizer = torch.optim.SGD(params, lr=1e-2)
    before = [p.detach().clone() for p in params]
    for step in range(3):
        losses = train_one_batch(net, criterion, optimizer, coder, images, class_images, batch_boxes, img_size, max_grad_norm=100.0)
        value = float(losses["loss"])
        print("\n[objective] train_one_batch step {}: loss {:.6f} grad norm {:.4f}".format(step, value, float(losses["grad_norm"])))
        assert np.isfinite(value)
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    unchanged = [(n, None if p.grad is None else float(p.grad.abs().max())) for n, p, b in zip(names, params, before)
                 if torch.equal(p.detach(), b)]
    print("[objective] train_one_batch: {} trainable tensors, unchanged (name, max |grad|): {}".format(len(params), unchanged))
    assert not unchanged, unchanged
    with pytest.raises(RuntimeError, match="forward_train"):
        net(images=images, class_images=class_images, train_mode=True)
    assert forward_train(net, images, class_images, fine_tune_features=False)[1].requires_grad
