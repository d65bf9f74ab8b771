"""CPU: the plain-torch restatement of hard-patch mining (tests/mining_model.py) against the fixtures recorded from the
reference's own mine_hard_patches, exactly; the new entry points of libos2d_train.so exist, refuse bad arguments before anything
is launched and use no scratch memory; os2d_amd.engine.mining imports without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import mining_cases as MC
import mining_model as MM

SYMBOLS = ("os2d_train_assign_targets_ops", "os2d_train_crop_boxes", "os2d_train_mine_select")


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_crop_placement_equals_the_reference(name):
    fx = MC.load(name)
    hit = set()
    for l, ((H, W), ops) in enumerate(zip(MC.CASES[name]["levels"], MC.chains(name))):
        w, h = MC.image_size((H, W))
        for tag, chain in (("t", ops), ("p", ())):
            crops, anchors, branches = MM.crop_boxes(H, W, MC.STRIDE, MC.BOX_SIZE, w, h, MC.CROP[0], MC.CROP[1], chain)
            assert np.array_equal(crops.numpy(), fx["crop_{}_{}".format(tag, l)])            # bit for bit
            assert np.array_equal(anchors.numpy(), fx["anchor_{}_{}".format(tag, l)])
            hit |= branches
    if name == "pyr":
        assert hit == set(MM.BRANCHES)


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_selection_equals_the_reference(name):
    c, fx = MC.CASES[name], MC.load(name)
    split = [h * w for h, w in c["levels"]]
    counts = fx["counts"]
    assert (counts == c["K"]).any() and ((counts > 0) & (counts < c["K"])).any() and counts[1, 1] == 0 and counts[1, 2] == 0
    for a in range(c["A"]):
        lv = lambda k: [t.unsqueeze(0) for t in torch.from_numpy(fx["{}_{}".format(k, a)]).split(split, 1)]   # noqa: E731
        recs = MM.mine(lv("cls_loss"), lv("loc_loss"), lv("flags"), c["levels"], MC.STRIDE, MC.BOX_SIZE,
                       [MC.image_size(l) for l in c["levels"]], MC.CROP, MC.chains(name), MC.NMS_IOU, c["K"])
        for r, role in enumerate(MC.ROLES):
            index, values = fx["rec_{}_{}_index".format(a, role)], fx["rec_{}_{}_values".format(a, role)]
            assert [list(x[:3]) for x in recs[r]] == index.tolist(), (a, role)               # triples and order
            assert len(recs[r]) == counts[a, r]
            for x, v in zip(recs[r], values):
                assert np.array_equal(x[3].numpy(), v[0:4]) and np.array_equal(x[4].numpy(), v[4:8])   # bit for bit


def test_selection_tie_rule_and_non_finite_scores():
    crops = torch.tensor([[0., 0, 10, 10], [100, 0, 110, 10], [200, 0, 210, 10], [300, 0, 310, 10], [0, 0, 10, 10]])
    scores = torch.tensor([1.0, float("nan"), 1.0, float("inf"), 2.0])
    assert MM.select(scores, torch.ones(5, dtype=torch.bool), crops, 0.5, 4) == [4, 2]     # 0 dies under 4; equal scores by index
    assert MM.select(torch.zeros(5), torch.ones(5, dtype=torch.bool), crops, 0.5, 2) == [0, 1]


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import build, _train_lib
    build.build_train(verbose=False)
    assert "mining.hip" in build.TRAIN_SOURCES
    return _train_lib.load()


def test_library_exports_the_mining_entry_points(lib):
    raw = ctypes.CDLL(lib._name)
    for s in SYMBOLS + ("os2d_train_mine_select_workspace_bytes",):
        assert getattr(raw, s) is not None
    import os2d_amd.engine.mining as mining               # no GPU needed to import
    assert mining.ROLES == MC.ROLES and callable(mining.mine_select) and callable(mining.mine_hard_patches)
    from os2d_amd.modeling.box_coder import BoxGridGenerator, Os2dBoxCoder
    assert hasattr(BoxGridGenerator, "get_box_to_cut_anchor")
    for m in ("encode_transformed", "encode_pyramid_transformed", "remap_anchor_targets_transformed", "apply_transform_to_corners"):
        assert hasattr(Os2dBoxCoder, m)


def test_mining_entry_points_refuse_bad_arguments(lib):
    fake = ctypes.c_void_p(256)      # never dereferenced: every call below is refused by its argument checks
    f = ctypes.c_float
    err = lib.os2d_train_last_error
    kinds = (ctypes.c_int * 8)(*([1] * 8))
    args = (ctypes.c_float * 16)(*([1.0] * 16))

    def assign(nops=1, k=kinds, mode=0):
        return lib.os2d_train_assign_targets_ops(mode, fake, fake, fake, fake, 3, fake, 2, 5, 9, 13, 16, 16, f(0.5), f(0.1), nops, k, args,
                                                 fake, fake, fake, fake, None)
    assert assign(nops=7) == -1 and b"chain" in err()
    assert assign(nops=-1) == -1 and b"chain" in err()
    assert assign(k=(ctypes.c_int * 8)(*([5] * 8))) == -1 and b"chain" in err()
    assert assign(mode=3) == -1 and b"mode" in err()

    def crop(H=9, nops=0, out=fake, crop_w=80):
        return lib.os2d_train_crop_boxes(H, 13, 16, 240, 208, 144, crop_w, 64, nops, kinds, args, out, fake, None)
    assert crop(H=0) == -1 and b"geometry" in err()
    assert crop(crop_w=0) == -1 and b"geometry" in err()
    assert crop(nops=7) == -1 and b"chain" in err()
    assert crop(out=None) == -1 and b"null" in err()

    hw = (ctypes.c_int * 2)(9, 13)
    img = (ctypes.c_int * 2)(208, 144)
    rows = (ctypes.c_int * 1)(117)
    cnt = (ctypes.c_int * 1)(0)
    ptr = (ctypes.c_void_p * 1)(256)
    need = lib.os2d_train_mine_select_workspace_bytes(2, 5, 1, hw)
    assert need == 2 * 3 * (592 + 117 * 16) and lib.os2d_train_mine_select_workspace_bytes(2, 5, 9, hw) == 0

    def select(L=1, K=4, counts=cnt, ws_bytes=need, cls=ptr, r=rows):
        return lib.os2d_train_mine_select(2, 5, L, hw, img, r, 16, 240, counts, kinds, args, cls, ptr, ptr, ptr, None, 80, 64, f(0.5), K,
                                          fake, fake, fake, fake, ws_bytes, None)
    assert select(K=65) == -1 and b"K=65" in err()
    assert select(K=0) == -1
    assert select(L=9) == -1 and b"levels" in err()
    assert select(counts=(ctypes.c_int * 1)(7)) == -1 and b"chain" in err()
    assert select(cls=None) == -1 and b"null" in err()
    assert select(r=(ctypes.c_int * 1)(100)) == -1 and b"stride" in err()
    assert select(ws_bytes=need - 1) == -2 and b"workspace" in err()


def test_mining_kernels_use_no_scratch(lib):
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    ks = codeobj.kernels(build.TRAIN_LIB_PATH)
    for name in ("mine_select_kernel", "crop_boxes_kernel", "assign_targets_kernel"):
        mine = {n: k for n, k in ks.items() if name in n}
        assert mine, name
        assert not {n: k for n, k in mine.items() if k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]}
    assert len([n for n in ks if "assign_targets_kernel" in n]) == 2        # one body, two instantiations


def test_python_layer_refuses_what_it_cannot_run():
    from os2d_amd.engine import mining
    from os2d_amd.modeling.box_coder import Os2dBoxCoder, BoxGridGenerator, traced_box_ops
    from os2d_amd.structures.feature_map import FeatureMapSize
    size = FeatureMapSize(w=208, h=144)
    with pytest.raises(ValueError, match="chain"):
        Os2dBoxCoder._chain([(1, 1.0, 1.0)] * 7, size)                                        # over-long
    with pytest.raises(ValueError, match="chain"):
        traced_box_ops(lambda b: b.bbox_xyxy, size)                                           # not resize / transpose / crop
    gen = BoxGridGenerator(FeatureMapSize(w=240, h=240), FeatureMapSize(w=16, h=16))
    z = torch.zeros(1, 5, 117)
    per_anchor = dict(cls_loss=[z], loc_loss=[z], flags=[z.to(torch.uint8)])
    kw = dict(box_grid_generator=gen)
    with pytest.raises(ValueError, match="num_hard_patches"):
        mining.mine_select(per_anchor, [z], None, [size], [FeatureMapSize(w=13, h=9)], None, FeatureMapSize(w=80, h=64), 0.5, 65, **kw)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mining.mine_select(per_anchor, [z], None, [size], [FeatureMapSize(w=13, h=9)], None, FeatureMapSize(w=80, h=64), 0.5, 4, **kw)
    with pytest.raises(RuntimeError, match="HIP device only"):
        gen.get_box_to_cut_anchor(size, FeatureMapSize(w=80, h=64), FeatureMapSize(w=13, h=9), device="cpu")
