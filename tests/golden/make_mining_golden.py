"""Records tests/golden/mining_*.npz from the reference implementation on the CPU: the reference's own mine_hard_patches
(os2d/engine/train.py:142-370) on the drawn inputs of tests/mining_cases.py, with get_box_to_cut_anchor, the transformed encode
and remap outputs and the per-anchor losses recorded on the way.

    python tests/golden/make_mining_golden.py             every fixture
    python tests/golden/make_mining_golden.py geometry    mining_geometry.npz only

How the reference is driven: its train module's ``make_iterator_extract_scores_from_images_batched`` is replaced by a generator
that yields the drawn scores and corners; a stub dataloader supplies ``box_coder``, ``get_image_annotation_for_imageid``,
``update_box_labels_to_local``, ``data_augmentation.random_crop_size`` and ``__len__``; a plain namespace serves as ``cfg``.
The reference imports ``yacs`` for its config module, which is not needed here: an attribute-dictionary stand-in is installed
for it, next to the torchvision stand-in of make_golden.py / make_objective_golden.py.  Data only is written.

Conditions asserted on the reference alone (the seed is redrawn until they hold): no corrected IoU within BAND of a remap
threshold; per role the scores of the records and of the best candidate surviving after them differ pairwise by more than 1e-4
relative; some role returns K records, some fewer than K but more than 0, and the image without a box returns none for pos and
pos_loc; every candidate list has at most 10,000 entries (where the reference's chunked NMS is global greedy NMS); every branch
of the crop placement is hit (case "pyr").

mining_geometry.npz: the reference's get_box_to_cut_anchor on every geometry of tests/mining_stage_cases.py (strides that are no
power of two, odd crops, images that are no multiple of the stride, crops larger than the image on one axis, a 3,600 px level),
without a transform and, for a handful, through a TransformList of resize / flip / crop closures.  Asserted on the reference alone:
the loop model (tests/mining_stage_model.py) and the torch model equal it bit for bit, and every branch is hit on each axis."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


class _CfgNode(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__

    def clone(self):
        return self


yacs, yacs_config = types.ModuleType("yacs"), types.ModuleType("yacs.config")
yacs_config.CfgNode = _CfgNode
yacs.config = yacs_config
sys.modules.setdefault("yacs", yacs)
sys.modules.setdefault("yacs.config", yacs_config)

spec = importlib.util.spec_from_file_location("make_objective_golden", os.path.join(HERE, "make_objective_golden.py"))
mog = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mog)        # installs the torchvision stand-in and the Matcher, puts the reference on the path

import os2d.engine.train as ref_train  # noqa: E402
from os2d.modeling.box_coder import Os2dBoxCoder, BoxGridGenerator  # noqa: E402
from os2d.engine.objective import Os2dObjective  # noqa: E402
from os2d.structures.bounding_box import BoxList, FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM  # noqa: E402
from os2d.structures.feature_map import FeatureMapSize  # noqa: E402
from os2d.structures.transforms import TransformList  # noqa: E402

import mining_cases as MC  # noqa: E402
import mining_model as MM  # noqa: E402
import mining_stage_cases as SC  # noqa: E402
import mining_stage_model as SM  # noqa: E402
from objective_util import BAND  # noqa: E402


class Unfit(Exception):
    pass


def need(cond, why):
    if not cond:
        raise Unfit(why)


def transforms(name):
    out = []
    orig = FeatureMapSize(w=MC.ORIG[0], h=MC.ORIG[1])
    for _ in MC.CASES[name]["levels"]:
        t = TransformList()                        # applied last to first
        t.append(lambda b: b.resize(orig))
        if MC.CASES[name]["flip"]:
            t.append(lambda b: b.transpose(FLIP_LEFT_RIGHT))
        out.append(t)
    return out


def record(name, seed):
    c = MC.CASES[name]
    A, B, K, levels = c["A"], c["B"], c["K"], c["levels"]
    images, loc, cls, corners = MC.draw(name, seed)
    fm_of = {FeatureMapSize(w=MC.image_size(l)[0], h=MC.image_size(l)[1]): FeatureMapSize(w=l[1], h=l[0]) for l in levels}
    gen = BoxGridGenerator(box_size=FeatureMapSize(w=MC.BOX_SIZE, h=MC.BOX_SIZE), box_stride=FeatureMapSize(w=MC.STRIDE, h=MC.STRIDE))
    coder = Os2dBoxCoder(MC.IOU["pos"], MC.IOU["neg"], MC.IOU["remap_pos"], MC.IOU["remap_neg"], gen,
                         lambda s: fm_of.get(s, FeatureMapSize(w=1, h=1)))
    crit = Os2dObjective(MC.LOSS, **MC.CRITERION)
    tls = transforms(name)
    orig = FeatureMapSize(w=MC.ORIG[0], h=MC.ORIG[1])
    crop = FeatureMapSize(w=MC.CROP[0], h=MC.CROP[1])
    img_sizes = [FeatureMapSize(w=MC.image_size(l)[0], h=MC.image_size(l)[1]) for l in levels]
    fm_sizes = [FeatureMapSize(w=l[1], h=l[0]) for l in levels]
    out = dict(seed=np.int64(seed))

    def annotation(a):
        bl = BoxList(torch.from_numpy(images[a]["boxes"]).clone(), orig, mode="xyxy")
        bl.add_field("labels", torch.tensor([MC.CLASS_IDS[i] for i in images[a]["labels"]], dtype=torch.long))
        bl.add_field("difficult", torch.from_numpy(images[a]["difficult"]).clone())
        return bl

    # ---- the pieces on their own: crop placement (with and without the chain), transformed encode and remap
    hit = set()
    for l, (lv, s, fm, t, ops) in enumerate(zip(levels, img_sizes, fm_sizes, tls, MC.chains(name))):
        for tag, tr, chain in (("t", t, ops), ("p", None, ())):
            cb, ab, index = gen.get_box_to_cut_anchor(s, crop, fm, tr)
            assert torch.equal(index, torch.arange(lv[0] * lv[1]))
            out["crop_{}_{}".format(tag, l)], out["anchor_{}_{}".format(tag, l)] = cb.bbox_xyxy.numpy(), ab.bbox_xyxy.numpy()
            mc, ma, h = MM.crop_boxes(lv[0], lv[1], MC.STRIDE, MC.BOX_SIZE, s.w, s.h, crop.w, crop.h, chain)
            assert torch.equal(mc, cb.bbox_xyxy) and torch.equal(ma, ab.bbox_xyxy), "the model's crop placement differs from the reference"
            hit |= h
    if name == "pyr":
        assert hit == set(MM.BRANCHES), hit
    for a in range(A):
        gt = annotation(a)
        gt.add_field("labels", torch.from_numpy(images[a]["labels"]).clone())
        lt, ct = coder.encode_pyramid(gt, img_sizes, B, default_box_transform_pyramid=tls)
        out["loc_targets_{}".format(a)] = torch.cat(lt, 2).numpy()
        out["cls_targets_{}".format(a)] = torch.cat(ct, 1).numpy().astype(np.int8)
        rem, ia, ic = [], [], []
        for l in range(len(levels)):
            r = coder.remap_anchor_targets(torch.from_numpy(loc[l][a:a + 1]), [img_sizes[l]], None, [gt], box_reverse_transform=[tls[l]])
            rem.append(r[0][0]), ia.append(r[1][0]), ic.append(r[2][0])
        icc = torch.cat(ic, 1)
        near = ((icc - MC.IOU["remap_pos"]).abs() < BAND) | ((icc - MC.IOU["remap_neg"]).abs() < BAND)
        need(not bool(near.any()), "an anchor inside the threshold band")
        out["cls_targets_remapped_{}".format(a)] = torch.cat(rem, 1).numpy().astype(np.int8)
        out["ious_anchor_{}".format(a)], out["ious_anchor_corrected_{}".format(a)] = torch.cat(ia, 1).numpy(), icc.numpy()
        for k in ("boxes", "labels", "difficult"):
            out["{}_{}".format(k, a)] = images[a][k]
    for l in range(len(levels)):
        out["loc_{}".format(l)], out["cls_{}".format(l)], out["corners_{}".format(l)] = loc[l], cls[l], corners[l]

    # ---- the reference's mine_hard_patches, driven as the module docstring says
    captured = []

    def criterion(*args, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = crit(*args, **kw)
        captured.append(res)
        return res

    def iterator(dataloader, net, logger, **kw):
        for a in range(A):
            yield (a, [torch.from_numpy(t[a]) for t in loc], [torch.from_numpy(t[a]) for t in cls],
                   [torch.zeros(1, 3, s.h, s.w) for s in img_sizes], [FeatureMapSize(w=64, h=64)] * B, list(MC.CLASS_IDS), tls, fm_sizes,
                   [torch.from_numpy(t[a]) for t in corners])

    class Loader(object):
        box_coder = coder
        data_augmentation = types.SimpleNamespace(random_crop_size=crop)

        def __len__(self):
            return A

        def get_image_annotation_for_imageid(self, image_id):
            return annotation(image_id)

        def update_box_labels_to_local(self, boxes, class_ids):
            boxes.add_field("labels", torch.tensor([class_ids.index(int(g)) for g in boxes.get_field("labels")], dtype=torch.long))

    off = types.SimpleNamespace(show_gt_boxes=False, show_class_heatmaps=False, show_mined_patches=False)
    cfg = types.SimpleNamespace(is_cuda=False, eval=types.SimpleNamespace(batch_size=1), visualization=types.SimpleNamespace(mining=off),
                                train=types.SimpleNamespace(mining=types.SimpleNamespace(
                                    num_random_pyramid_scales=0, num_random_negative_classes=0,
                                    nms_iou_threshold_in_mining=MC.NMS_IOU, num_hard_patches_per_image=K)))
    ref_train.make_iterator_extract_scores_from_images_batched = iterator
    mined = ref_train.mine_hard_patches(Loader(), types.SimpleNamespace(eval=lambda: None), cfg, criterion)

    counts = np.zeros((A, 3), np.int64)
    for a in range(A):
        losses, per_anchor = captured[a]
        names = [k for k in losses if k != "class_loss_per_element_detached_cpu"]
        out["loss_names"] = np.array(names)
        out["losses_{}".format(a)] = np.array([float(losses[k]) for k in names], np.float32)
        cat = lambda k: torch.cat([t[0] for t in per_anchor[k]], 1)   # noqa: E731
        cl, ll = cat("cls_loss").float(), cat("loc_loss").float()
        flags = cat("pos_mask").to(torch.uint8) + 2 * cat("neg_mask").to(torch.uint8) + 4 * cat("pos_for_regression").to(torch.uint8)
        out["cls_loss_{}".format(a)], out["loc_loss_{}".format(a)], out["flags_{}".format(a)] = cl.numpy(), ll.numpy(), flags.numpy()
        need(int((flags & 2).ne(0).sum()) <= 10000, "more than 10,000 candidates")
        recs = mined[a]
        if recs:
            assert tuple(recs[0].keys()) == MC.KEYS, tuple(recs[0].keys())
        split = [h * w for h, w in levels]
        lv = lambda t: [x.unsqueeze(0) for x in t.split(split, 1)]    # noqa: E731
        model = MM.mine(lv(cl), lv(ll), lv(flags), levels, MC.STRIDE, MC.BOX_SIZE, [(s.w, s.h) for s in img_sizes], MC.CROP,
                        MC.chains(name), MC.NMS_IOU, K + 1)
        for r, role in enumerate(MC.ROLES):
            mine_r = [x for x in recs if x["role"] == role]
            counts[a, r] = len(mine_r)
            src = "loss_loc" if role == "pos_loc" else "loss"
            sc = [float(x[src]) for x in mine_r]
            if len(model[r]) > len(mine_r):           # the best candidate that survives after the records
                l_, b_, p_ = model[r][len(mine_r)][:3]
                off_ = sum(split[:l_]) + p_
                sc.append(float((ll if role == "pos_loc" else cl)[b_, off_]))
            for i in range(len(sc)):
                for j in range(i + 1, len(sc)):
                    need(abs(sc[i] - sc[j]) > 1e-4 * max(abs(sc[i]), abs(sc[j])), "scores of role {} closer than 1e-4 relative".format(role))
            out["rec_{}_{}_index".format(a, role)] = np.array([[x["pyramid_level"], x["label_local"], x["anchor_index"]] for x in mine_r],
                                                              np.int32).reshape(-1, 3)
            vals = [torch.cat([x["crop_position_xyxy"].bbox_xyxy.view(-1), x["anchor_position_xyxy"].bbox_xyxy.view(-1),
                               x["transform_corners"].view(-1).float(),
                               torch.tensor([x["loss"], x["loss_loc"], x["score"]], dtype=torch.float32)]) for x in mine_r]
            out["rec_{}_{}_values".format(a, role)] = (torch.stack(vals) if vals else torch.zeros(0, 19)).numpy()
            assert all(x["label_global"] == MC.CLASS_IDS[x["label_local"]] and x["image_id"] == a for x in mine_r)
    need((counts == K).any(), "no role returns K records")
    need(((counts > 0) & (counts < K)).any(), "no role returns fewer than K but more than 0 records")
    need(counts[1, 1] == 0 and counts[1, 2] == 0 and images[1]["boxes"].shape[0] == 0, "the image without a box has positives")
    out["counts"] = counts
    return out


def steps_transform(steps):
    """The steps of a geometry (applied first to last) as the reference's TransformList (which runs its closures last to first)."""
    def closure(s):
        if s[0] == "resize":
            return lambda b: b.resize(FeatureMapSize(w=s[1], h=s[2]))
        if s[0] == "hflip":
            return lambda b: b.transpose(FLIP_LEFT_RIGHT)
        if s[0] == "vflip":
            return lambda b: b.transpose(FLIP_TOP_BOTTOM)
        return lambda b: b.crop(s[1:])
    t = TransformList()
    for s in reversed(steps):
        t.append(closure(s))
    return t


def record_geometry():
    out = {}
    hit_x, hit_y = set(), set()
    for g in SC.GEOMETRIES:
        gen = BoxGridGenerator(box_size=FeatureMapSize(w=g["box"], h=g["box"]), box_stride=FeatureMapSize(w=g["stride"], h=g["stride"]))
        img, crop = FeatureMapSize(w=g["img"][0], h=g["img"][1]), FeatureMapSize(w=g["crop"][0], h=g["crop"][1])
        cb, ab, index = gen.get_box_to_cut_anchor(img, crop, FeatureMapSize(w=g["W"], h=g["H"]), steps_transform(g["steps"]) if g["steps"] else None)
        assert torch.equal(index, torch.arange(g["H"] * g["W"]))
        ops, size = SC.chain_ops(g["steps"], g["img"])
        assert (cb.image_size.w, cb.image_size.h) == tuple(size), g["name"]
        crops, anchors, bx, by = SC.geometry_model(g["name"])
        assert np.array_equal(crops, cb.bbox_xyxy.numpy()) and np.array_equal(anchors, ab.bbox_xyxy.numpy()), \
            "the loop model's crop placement differs from the reference: " + g["name"]
        mc, ma, _ = MM.crop_boxes(g["H"], g["W"], g["stride"], g["box"], img.w, img.h, crop.w, crop.h, ops)
        assert torch.equal(mc, cb.bbox_xyxy) and torch.equal(ma, ab.bbox_xyxy), "the torch model differs from the reference: " + g["name"]
        hit_x |= set(bx)
        hit_y |= set(by)
        out["crop_" + g["name"]], out["anchor_" + g["name"]] = cb.bbox_xyxy.numpy(), ab.bbox_xyxy.numpy()
    assert hit_x == hit_y == set(SM.BRANCHES), (hit_x, hit_y)
    out["names"] = np.array([g["name"] for g in SC.GEOMETRIES])
    return out


def save(fname, arrays):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 1 << 20, "{} is {} bytes".format(fname, size)
    print("wrote", fname, size)


if __name__ == "__main__":
    import logging
    logging.disable(logging.CRITICAL)
    save("mining_geometry.npz", record_geometry())
    for case, c in ({} if sys.argv[1:] == ["geometry"] else MC.CASES).items():
        for seed in range(c["seed"], c["seed"] + 200):
            try:
                arrays = record(case, seed)
            except Unfit as e:
                print(case, "seed", seed, "redrawn:", e)
                continue
            print(case, "seed", seed, "counts", arrays["counts"].tolist())
            save("mining_{}.npz".format(case), arrays)
            break
        else:
            raise SystemExit("no seed fits case " + case)
