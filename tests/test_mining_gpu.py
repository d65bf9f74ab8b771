"""GPU: hard-patch mining on the HIP kernels against the fixtures recorded from the reference's own mine_hard_patches
(tests/golden/mining_*.npz) and, beyond their sizes, against the plain-torch model (tests/mining_model.py) on the same device."""
import numpy as np
import pytest
import torch

import mining_cases as MC
import mining_model as MM
import objective_util as U

pytestmark = pytest.mark.gpu


def fms(name):
    from os2d_amd.structures.feature_map import FeatureMapSize
    levels = MC.CASES[name]["levels"]
    return ([FeatureMapSize(w=MC.image_size(l)[0], h=MC.image_size(l)[1]) for l in levels], [FeatureMapSize(w=l[1], h=l[0]) for l in levels])


def make_coder(name):
    from os2d_amd.modeling.box_coder import Os2dBoxCoder, BoxGridGenerator
    from os2d_amd.structures.feature_map import FeatureMapSize
    sizes = dict(zip(*fms(name)))
    gen = BoxGridGenerator(box_size=FeatureMapSize(w=MC.BOX_SIZE, h=MC.BOX_SIZE), box_stride=FeatureMapSize(w=MC.STRIDE, h=MC.STRIDE))
    return Os2dBoxCoder(MC.IOU["pos"], MC.IOU["neg"], MC.IOU["remap_pos"], MC.IOU["remap_neg"], gen, lambda s: sizes[s])


def transforms(name):
    """The reference's per-level transforms as closures on BoxLists (traced by the package): applied last to first."""
    from os2d_amd.structures.bounding_box import FLIP_LEFT_RIGHT
    from os2d_amd.structures.feature_map import FeatureMapSize
    orig = FeatureMapSize(w=MC.ORIG[0], h=MC.ORIG[1])
    if MC.CASES[name]["flip"]:
        return [lambda b: b.transpose(FLIP_LEFT_RIGHT).resize(orig) for _ in MC.CASES[name]["levels"]]
    return [lambda b: b.resize(orig) for _ in MC.CASES[name]["levels"]]


def gt_boxes(fx, a, device=None):
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    b = torch.from_numpy(fx["boxes_{}".format(a)])
    bl = BoxList(b if device is None else b.to(device), FeatureMapSize(w=MC.ORIG[0], h=MC.ORIG[1]))
    bl.add_field("labels", torch.from_numpy(fx["labels_{}".format(a)]))
    bl.add_field("difficult", torch.from_numpy(fx["difficult_{}".format(a)]))
    return bl


def per_level(fx, key, a, name, device):
    split = [h * w for h, w in MC.CASES[name]["levels"]]
    return [t.unsqueeze(0).contiguous().to(device) for t in torch.from_numpy(fx["{}_{}".format(key, a)]).split(split, 1)]


def check_records(name, fx, a, count, index, values, exact_losses=True, pins=None):
    K = MC.CASES[name]["K"]
    count, index, values = count.cpu().numpy(), index.cpu().numpy(), values.cpu().numpy()
    for r, role in enumerate(MC.ROLES):
        ref_i, ref_v = fx["rec_{}_{}_index".format(a, role)], fx["rec_{}_{}_values".format(a, role)]
        n = ref_i.shape[0]
        assert count[0, r] == n == fx["counts"][a, r], (a, role, count[0, r], n)
        assert np.array_equal(index[0, r, :n], ref_i), (a, role)                          # triples and order
        assert (index[0, r, n:] == -1).all() and (values[0, r, n:] == 0).all()
        assert np.array_equal(values[0, r, :n, :16], ref_v[:, :16]), (a, role)            # crops, anchors, corners: bit for bit
        if exact_losses:
            assert np.array_equal(values[0, r, :n, 16:], ref_v[:, 16:])
        else:
            assert n == 0 or U.rel_err(values[0, r, :n, 16], ref_v[:, 16]) <= pins["cls_loss"]
            assert n == 0 or U.rel_err(values[0, r, :n, 17], ref_v[:, 17]) <= pins["loc_loss"]
            assert np.array_equal(values[0, r, :n, 18], ref_v[:, 18])
    assert K == index.shape[2]


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_get_box_to_cut_anchor_equals_the_reference(device, name):
    from os2d_amd.structures.feature_map import FeatureMapSize
    fx, coder = MC.load(name), make_coder(name)
    crop = FeatureMapSize(w=MC.CROP[0], h=MC.CROP[1])
    for l, (img, fm, t) in enumerate(zip(*fms(name), transforms(name))):
        for tag, tr in (("t", t), ("p", None)):
            crops, anchors, index = coder.output_box_grid_generator.get_box_to_cut_anchor(img, crop, fm, tr, device=device)
            assert crops.bbox_xyxy.is_cuda and torch.equal(index.cpu(), torch.arange(fm.w * fm.h))
            assert np.array_equal(crops.bbox_xyxy.cpu().numpy(), fx["crop_{}_{}".format(tag, l)])
            assert np.array_equal(anchors.bbox_xyxy.cpu().numpy(), fx["anchor_{}_{}".format(tag, l)])
            assert crops.image_size == (FeatureMapSize(w=MC.ORIG[0], h=MC.ORIG[1]) if tr is not None else img)


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_transformed_encode_and_remap_match_the_reference(device, name):
    c, fx, pins, coder = MC.CASES[name], MC.load(name), U.pins(), make_coder(name)
    imgs, _ = fms(name)
    ts = transforms(name)
    for a in range(c["A"]):
        gt = gt_boxes(fx, a)
        loc_t, cls_t = coder.encode_pyramid_transformed(gt, imgs, c["B"], ts, device=device)
        cls_t, loc_t = torch.cat(cls_t, 1).cpu().numpy(), torch.cat(loc_t, 2).cpu().numpy()
        err = U.rel_err(loc_t, fx["loc_targets_{}".format(a)])
        print("\n[mining] {} image {} encode: loc_targets rel err {:.3e}".format(name, a, err))
        assert np.array_equal(cls_t, fx["cls_targets_{}".format(a)].astype(np.int64))
        assert err <= pins["loc_targets"]
        rems, ias, ics = [], [], []
        for l, (img, t) in enumerate(zip(imgs, ts)):
            loc = torch.from_numpy(fx["loc_{}".format(l)][a:a + 1]).to(device)
            rem, ia, ic = coder.remap_anchor_targets_transformed(loc, [img], None, [gt], box_reverse_transform=[t])
            rems.append(rem[0]), ias.append(ia[0]), ics.append(ic[0])
        rem, ia, ic = [torch.cat(t, 1).cpu().numpy() for t in (rems, ias, ics)]
        ref_ic = fx["ious_anchor_corrected_{}".format(a)]
        band = (np.abs(ref_ic - MC.IOU["remap_pos"]) < U.BAND) | (np.abs(ref_ic - MC.IOU["remap_neg"]) < U.BAND)
        assert not band.any()                                                              # empty by construction
        print("[mining] {} image {} remap: corrected abs err {:.3e}".format(name, a, float(np.abs(ic - ref_ic).max())))
        assert np.array_equal(rem, fx["cls_targets_remapped_{}".format(a)].astype(np.int64))
        assert np.array_equal(ia, fx["ious_anchor_{}".format(a)])
        assert float(np.abs(ic - ref_ic).max()) <= pins["ious_anchor_corrected_abs"]


def test_identity_chain_gives_the_bits_of_the_plain_methods(device):
    name = "pyr"
    c, fx, coder = MC.CASES[name], MC.load(name), make_coder(name)
    imgs, _ = fms(name)
    one = ((MC.OP_SCALE, 1.0, 1.0),)
    from os2d_amd.structures.bounding_box import BoxList
    gt = gt_boxes(fx, 0)
    for l, img in enumerate(imgs):
        scaled = BoxList(gt.bbox_xyxy * (float(img.w) / MC.ORIG[0]), img)      # some boxes in the level's frame
        scaled.add_field("labels", gt.get_field("labels"))
        scaled.add_field("difficult", gt.get_field("difficult"))
        plain = coder.encode(scaled.to(device), img, c["B"])
        ours = coder.encode_transformed(scaled, img, c["B"], one, device=device)
        assert torch.equal(plain[0], ours[0]) and torch.equal(plain[1], ours[1])
        loc = torch.from_numpy(fx["loc_{}".format(l)]).to(device)
        plain = coder.remap_anchor_targets(loc, [img] * c["A"], None, [scaled] * c["A"])
        ours = coder.remap_anchor_targets_transformed(loc, [img] * c["A"], None, [scaled] * c["A"], box_reverse_transform=[one] * c["A"])
        assert all(torch.equal(p, o) for p, o in zip(plain, ours))
        assert int((plain[0] != 0).sum()) > 0


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_mine_select_on_recorded_losses(device, name):
    from os2d_amd.engine import mining
    from os2d_amd.structures.feature_map import FeatureMapSize
    c, fx, coder = MC.CASES[name], MC.load(name), make_coder(name)
    imgs, fm = fms(name)
    for a in range(c["A"]):
        per_anchor = dict(cls_loss=per_level(fx, "cls_loss", a, name, device), loc_loss=per_level(fx, "loc_loss", a, name, device),
                          flags=per_level(fx, "flags", a, name, device))
        cls = [torch.from_numpy(fx["cls_{}".format(l)][a:a + 1]).to(device) for l in range(len(imgs))]
        cor = [torch.from_numpy(fx["corners_{}".format(l)][a:a + 1]).to(device) for l in range(len(imgs))]
        out = mining.mine_select(per_anchor, cls, cor, imgs, fm, transforms(name), FeatureMapSize(w=MC.CROP[0], h=MC.CROP[1]), MC.NMS_IOU,
                                 c["K"], box_grid_generator=coder.output_box_grid_generator)
        check_records(name, fx, a, *out)


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_mine_hard_patches_for_image_end_to_end(device, name):
    from os2d_amd.engine import mining
    from os2d_amd.engine.objective import Os2dObjective
    from os2d_amd.structures.feature_map import FeatureMapSize
    c, fx, coder, pins = MC.CASES[name], MC.load(name), make_coder(name), U.pins()
    imgs, fm = fms(name)
    crit = Os2dObjective(MC.LOSS, **MC.CRITERION)
    items = []
    for a in range(c["A"]):
        L = range(len(imgs))
        scores = ([torch.from_numpy(fx["loc_{}".format(l)][a]).to(device) for l in L], [torch.from_numpy(fx["cls_{}".format(l)][a]).to(device) for l in L],
                  [torch.from_numpy(fx["corners_{}".format(l)][a]).to(device) for l in L], fm)
        items.append(dict(image_levels=imgs, class_head=None, class_ids=MC.CLASS_IDS, gt_boxes=gt_boxes(fx, a),
                          orig_size=FeatureMapSize(w=MC.ORIG[0], h=MC.ORIG[1]), crop_size=FeatureMapSize(w=MC.CROP[0], h=MC.CROP[1]),
                          image_id=a, scores=scores, box_transforms=transforms(name)))
    mined, losses = mining.mine_hard_patches(None, crit, coder, items, nms_iou_threshold=MC.NMS_IOU, num_hard_patches=c["K"])
    assert list(mined.keys()) == list(range(c["A"])) and crit.keep_class_loss_on_cpu
    for a in range(c["A"]):
        recs = mined[a]
        pos = 0
        for role in MC.ROLES:
            ref_i, ref_v = fx["rec_{}_{}_index".format(a, role)], fx["rec_{}_{}_values".format(a, role)]
            mine = recs[pos:pos + ref_i.shape[0]]
            pos += ref_i.shape[0]
            assert [x["role"] for x in mine] == [role] * ref_i.shape[0], (a, role)        # neg, pos, pos_loc, each by decreasing score
            assert [[x["pyramid_level"], x["label_local"], x["anchor_index"]] for x in mine] == ref_i.tolist(), (a, role)
            for x, v in zip(mine, ref_v):
                assert tuple(x.keys()) == MC.KEYS
                assert x["label_global"] == MC.CLASS_IDS[x["label_local"]] and x["image_id"] == a
                assert not x["crop_position_xyxy"].bbox_xyxy.is_cuda and len(x["crop_position_xyxy"]) == 1
                assert np.array_equal(x["crop_position_xyxy"].bbox_xyxy.numpy().reshape(-1), v[0:4])
                assert np.array_equal(x["anchor_position_xyxy"].bbox_xyxy.numpy().reshape(-1), v[4:8])
                assert np.array_equal(x["transform_corners"].numpy(), v[8:16])
                assert x["score"] == v[18]
            if mine:
                e_cls = U.rel_err([x["loss"] for x in mine], ref_v[:, 16])
                e_loc = U.rel_err([x["loss_loc"] for x in mine], ref_v[:, 17])
                print("\n[mining] {} image {} {}: loss rel err {:.3e} loss_loc rel err {:.3e}".format(name, a, role, e_cls, e_loc))
                assert e_cls <= pins["cls_loss"] and e_loc <= pins["loc_loss"]
        assert pos == len(recs)
        ref = dict(zip(fx["loss_names"].tolist(), fx["losses_{}".format(a)]))
        assert set(ref) <= set(losses[a]) and all(isinstance(v, float) for v in losses[a].values())
        for k, v in ref.items():
            assert abs(losses[a][k] - float(v)) <= pins["scalars"] * max(abs(float(v)), 1e-30), (k, losses[a][k], float(v))


@pytest.fixture(scope="module")
def large(device):
    """Two levels (60,80) + (30,40), 12 labels, 2 images: > 10,000 negatives per image, many exact ties (zero losses)."""
    from os2d_amd.structures.feature_map import FeatureMapSize
    levels, A, B = [(60, 80), (30, 40)], 2, 12
    g = torch.Generator().manual_seed(7)
    cls_loss, loc_loss, flags, cls, cor = [], [], [], [], []
    for H, W in levels:
        n = (A, B, H * W)
        u = torch.rand(n, generator=g)
        f = torch.where(u < 0.9, torch.full(n, 2), torch.where(u < 0.95, torch.full(n, 1), torch.zeros(n, dtype=torch.long)))
        f = f + 4 * (torch.rand(n, generator=g) < 0.03).long()
        cl = torch.rand(n, generator=g)
        cl = torch.where(torch.rand(n, generator=g) < 0.5, torch.zeros(n), cl)              # half the class losses are exactly 0
        cl[(f & 1) != 0] = 0.0                                                               # pos: ties only, the index rule decides
        cl[0, 0, :5] = torch.tensor([float("nan"), float("inf"), -float("inf"), 5.0, 5.0])  # never selected / a tie at the top
        f[0, 0, :5] = 2
        cls_loss.append(cl.to(device)), loc_loss.append(torch.rand(n, generator=g).to(device)), flags.append(f.to(torch.uint8).to(device))
        cls.append(torch.rand(n, generator=g).to(device)), cor.append(torch.rand(A, B, 8, H * W, generator=g).to(device) * 100)
    imgs = [FeatureMapSize(w=W * 16, h=H * 16) for H, W in levels]
    chains = [((MC.OP_SCALE, 1280.0 / s.w, 960.0 / s.h),) for s in imgs]
    return dict(levels=levels, A=A, B=B, imgs=imgs, fms=[FeatureMapSize(w=W, h=H) for H, W in levels], chains=chains,
                per_anchor=dict(cls_loss=cls_loss, loc_loss=loc_loss, flags=flags), cls=cls, cor=cor)


def test_large_pyramid_against_the_model(device, large):
    from os2d_amd.engine import mining
    from os2d_amd.structures.feature_map import FeatureMapSize
    d, K = large, 10
    gen = make_coder("pyr").output_box_grid_generator
    assert int(((d["per_anchor"]["flags"][0][0] & 2) != 0).sum()) > 10000
    run = lambda: mining.mine_select(d["per_anchor"], d["cls"], d["cor"], d["imgs"], d["fms"], d["chains"], FeatureMapSize(w=608, h=608),  # noqa: E731
                                     0.5, K, box_grid_generator=gen)
    count, index, values = run()
    again = run()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((count, index, values), again))            # the same bits
    count, index, values = count.cpu(), index.cpu(), values.cpu()
    for a in range(d["A"]):
        ref = MM.mine(d["per_anchor"]["cls_loss"], d["per_anchor"]["loc_loss"], d["per_anchor"]["flags"], d["levels"], MC.STRIDE, MC.BOX_SIZE,
                      [(s.w, s.h) for s in d["imgs"]], (608, 608), d["chains"], 0.5, K, image=a)
        for r in range(3):
            assert int(count[a, r]) == len(ref[r]) > 0
            assert index[a, r, :len(ref[r])].tolist() == [list(x[:3]) for x in ref[r]], (a, r)
            for k, x in enumerate(ref[r]):
                assert torch.equal(values[a, r, k, 0:4], x[3].cpu()) and torch.equal(values[a, r, k, 4:8], x[4].cpu())
                l, b, p = x[:3]
                assert values[a, r, k, 16] == d["per_anchor"]["cls_loss"][l][a, b, p].cpu()
                assert values[a, r, k, 18] == d["cls"][l][a, b, p].cpu()
    assert index[0, 0, 0].tolist() == [0, 0, 3]             # 5.0 twice: the smaller anchor index; nan / inf are skipped
    assert torch.isfinite(values[:, :, :, 16]).all()


def test_mine_select_does_not_synchronise(device, large):
    from os2d_amd.engine import mining
    from os2d_amd.structures.feature_map import FeatureMapSize
    d = large
    gen = make_coder("pyr").output_box_grid_generator
    run = lambda: mining.mine_select(d["per_anchor"], d["cls"], d["cor"], d["imgs"], d["fms"], d["chains"], FeatureMapSize(w=608, h=608),  # noqa: E731
                                     0.5, 10, box_grid_generator=gen)
    run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            float(d["cls"][0].sum())
            effective = False
        except RuntimeError:
            effective = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not effective:
        pytest.skip("torch.cuda.set_sync_debug_mode has no effect on this torch-ROCm build")
    torch.cuda.set_sync_debug_mode("error")
    try:
        count, _, _ = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(count.min()) > 0


def test_bad_arguments_raise(device):
    from os2d_amd.engine import mining
    from os2d_amd.structures.feature_map import FeatureMapSize
    coder = make_coder("pyr")
    imgs, fm = fms("pyr")
    z = lambda hw, dt=torch.float32, dev=device: torch.zeros(1, 5, hw, dtype=dt, device=dev)   # noqa: E731
    per_anchor = dict(cls_loss=[z(117)], loc_loss=[z(117)], flags=[z(117, torch.uint8)])
    crop = FeatureMapSize(w=80, h=64)
    kw = dict(box_grid_generator=coder.output_box_grid_generator)
    with pytest.raises(ValueError, match="chain"):
        mining.mine_select(per_anchor, [z(117)], None, imgs[:1], fm[:1], [[(1, 1.0, 1.0)] * 7], crop, 0.5, 4, **kw)
    with pytest.raises(ValueError, match="num_hard_patches"):
        mining.mine_select(per_anchor, [z(117)], None, imgs[:1], fm[:1], None, crop, 0.5, 65, **kw)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mining.mine_select(per_anchor, [z(117, dev="cpu")], None, imgs[:1], fm[:1], None, crop, 0.5, 4, **kw)
    with pytest.raises(ValueError, match="chain"):
        coder.encode_transformed(gt_boxes(MC.load("pyr"), 0), imgs[0], 5, lambda b: b.bbox_xyxy, device=device)
    with pytest.raises(RuntimeError, match="HIP device only"):
        coder.remap_anchor_targets_transformed(torch.zeros(1, 5, 4, 117), imgs[:1], None, [None])
    count, index, _ = mining.mine_select(per_anchor, [z(117)], None, imgs[:1], fm[:1], None, crop, 0.5, 4, **kw)
    assert int(count.sum()) == 0 and bool((index == -1).all())                # nothing flagged: nothing mined
