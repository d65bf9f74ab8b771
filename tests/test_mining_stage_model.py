"""CPU: the loop model of the mining stage suite (tests/mining_stage_model.py) against the fixtures recorded from the reference
(mining_pyr / mining_flip: placement, selection and records; mining_geometry: placement on odd geometries) and against the torch
model (tests/mining_model.py), exactly; and the conditions every case of tests/mining_stage_cases.py has to meet, from the loop
model alone: the band around the IoU threshold is empty (or, for the designated cases, every IoU operand is an integer below
2^24), the recorded seeds are the first that keep it, and every case reaches the regime it is named after."""
import os

import numpy as np
import pytest
import torch

import mining_cases as MC
import mining_model as MM
import mining_stage_cases as SC
import mining_stage_model as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_case(name, fx, a):
    """Image ``a`` of a recorded fixture as a case of the loop model."""
    c = MC.CASES[name]
    split = np.cumsum([h * w for h, w in c["levels"]])[:-1]
    lv = lambda key: [t[None] for t in np.split(fx["{}_{}".format(key, a)], split, axis=1)]   # noqa: E731
    L = range(len(c["levels"]))
    return dict(name=name, A=1, B=c["B"], K=c["K"], thr=MC.NMS_IOU, stride=MC.STRIDE, box=MC.BOX_SIZE, crop=MC.CROP, levels=c["levels"],
                imgs=[MC.image_size(l) for l in c["levels"]], chains=MC.chains(name), cls_loss=lv("cls_loss"), loc_loss=lv("loc_loss"),
                flags=lv("flags"), cls_preds=[fx["cls_{}".format(l)][a:a + 1] for l in L], corners=[fx["corners_{}".format(l)][a:a + 1] for l in L])


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_loop_model_equals_the_recorded_fixtures_and_the_torch_model(name):
    c, fx = MC.CASES[name], MC.load(name)
    for l, ((H, W), ops) in enumerate(zip(c["levels"], MC.chains(name))):
        w, h = MC.image_size((H, W))
        for tag, chain in (("t", ops), ("p", ())):
            crops, anchors, _, _ = SM.crop_table(H, W, MC.STRIDE, MC.BOX_SIZE, w, h, MC.CROP[0], MC.CROP[1], chain)
            assert np.array_equal(crops, fx["crop_{}_{}".format(tag, l)]) and np.array_equal(anchors, fx["anchor_{}_{}".format(tag, l)])
            mc, ma, _ = MM.crop_boxes(H, W, MC.STRIDE, MC.BOX_SIZE, w, h, MC.CROP[0], MC.CROP[1], chain)
            assert np.array_equal(crops, mc.numpy()) and np.array_equal(anchors, ma.numpy())
    for a in range(c["A"]):
        case = fixture_case(name, fx, a)
        m = SM.mine(case)
        assert m["band_gap"] >= SC.BAND
        torch_model = MM.mine([torch.from_numpy(t) for t in case["cls_loss"]], [torch.from_numpy(t) for t in case["loc_loss"]],
                              [torch.from_numpy(t) for t in case["flags"]], c["levels"], MC.STRIDE, MC.BOX_SIZE, case["imgs"], MC.CROP,
                              case["chains"], MC.NMS_IOU, c["K"])
        for r, role in enumerate(MC.ROLES):
            index, values = fx["rec_{}_{}_index".format(a, role)], fx["rec_{}_{}_values".format(a, role)]
            n = index.shape[0]
            assert m["count"][0, r] == n == fx["counts"][a, r]
            assert np.array_equal(m["index"][0, r, :n], index) and (m["index"][0, r, n:] == -1).all()     # triples and order
            assert np.array_equal(m["values"][0, r, :n], values) and (m["values"][0, r, n:] == 0).all()   # all 19 values, bit for bit
            assert [list(x[:3]) for x in torch_model[r]] == index.tolist()


def test_loop_model_crops_equal_the_geometry_fixture():
    fx = np.load(os.path.join(GOLDEN, "mining_geometry.npz"), allow_pickle=False)
    assert fx["names"].tolist() == [g["name"] for g in SC.GEOMETRIES] and len(SC.GEOMETRIES) >= 168
    hit_x, hit_y = set(), set()
    for g in SC.GEOMETRIES:
        crops, anchors, bx, by = SC.geometry_model(g["name"])
        assert SC.same_bits(crops, fx["crop_" + g["name"]]), g["name"]                                # bit for bit
        assert SC.same_bits(anchors, fx["anchor_" + g["name"]]), g["name"]
        hit_x |= set(bx)
        hit_y |= set(by)
    assert hit_x == set(SM.BRANCHES) and hit_y == set(SM.BRANCHES)                                     # every branch on each axis
    assert {len(g["steps"]) for g in SC.GEOMETRIES} >= {0, 1, 2, SC.MAX_OPS}


def test_geometries_reach_their_edges():
    g = SC.GEOMETRY["raw0_and_hi_at_img"]
    crops, _, bx, by = SC.geometry_model(g["name"])
    # anchor 0: the raw corner 8 - 16 / 2 is exactly 0 -> the "zero" branch, not floor_to_stride of 0; the last anchor's window ends
    # exactly at the image -> not shifted
    assert (bx[0], by[0]) == ("zero", "zero") and crops[0].tolist() == [0, 0, 16, 16]
    assert (bx[-1], by[-1]) == ("floor", "floor") and crops[-1].tolist() == [64, 32, 80, 48] and g["img"] == (80, 48)
    g = SC.GEOMETRY["raw0_and_hi_at_img_s12"]
    crops, _, bx, by = SC.geometry_model(g["name"])
    assert bx[1] == "zero" and bx[2] == "floor" and crops[4].tolist()[::2] == [36, 72] and bx[4] == "floor" and bx[5] == "shift"
    _, _, bx, by = SC.geometry_model("wider_than_image_x_only")
    assert set(bx) == {"full"} and "full" not in by
    _, _, bx, by = SC.geometry_model("taller_than_image_y_only")
    assert set(by) == {"full"} and "full" not in bx
    g = SC.GEOMETRY["wide_level_3600px"]
    _, anchors, bx, _ = SC.geometry_model(g["name"])
    assert g["W"] >= 3600 // 16 and float(anchors[:, 0].max() + anchors[:, 2].max()) / 2 > 3590 and set(bx) >= {"zero", "floor", "shift"}
    assert any(g["H"] * g["W"] == 1 for g in SC.GEOMETRIES)


@pytest.mark.parametrize("name", SC.SELECT_CASES)
def test_band_or_exactness(name):
    m = SC.model(name)
    if name in SC.EXACT:
        assert m["exact"] and m["band_gap"] < SC.BAND            # at the threshold on purpose: every operand an integer below 2^24
    else:
        assert m["band_gap"] >= SC.BAND, m["band_gap"]
    assert SC.EXCLUDED == 0


@pytest.mark.parametrize("name", sorted(SC.SEEDED_BUILDERS))
def test_seeds(name):
    assert SC.first_seed(name) == SC.SEEDS[name] == SC.case(name)["seed"]


@pytest.mark.parametrize("name", SC.SELECT_CASES)
def test_loop_model_equals_the_torch_model(name):
    c, m = SC.case(name), SC.model(name)
    t = lambda key: [torch.from_numpy(np.ascontiguousarray(x)) for x in c[key]]   # noqa: E731
    for a in range(c["A"]):
        ref = MM.mine(t("cls_loss"), t("loc_loss"), t("flags"), c["levels"], c["stride"], c["box"], c["imgs"], c["crop"], c["chains"],
                      c["thr"], c["K"], image=a)
        for r in range(3):
            n = len(ref[r])
            assert m["count"][a, r] == n and m["index"][a, r, :n].tolist() == [list(x[:3]) for x in ref[r]], (a, r)
            for k, x in enumerate(ref[r]):
                assert np.array_equal(m["values"][a, r, k, 0:4], x[3].numpy()) and np.array_equal(m["values"][a, r, k, 4:8], x[4].numpy())


@pytest.mark.parametrize("name", SC.SELECT_CASES)
def test_cases_reach_their_regime(name):
    c, m, e = SC.case(name), SC.model(name), SC.case(name)["expect"]
    N = SC.offsets(c)[-1]
    if "top2" in e:                  # the tie pair was the top two, the smaller flat first
        i, j = e["top2"]
        assert i < j
        for r, key in enumerate(("cls_loss", "cls_loss", "loc_loss")):
            s = np.concatenate([x[0].reshape(-1) for x in c[key]])
            assert s[i] == s[j] and (np.delete(s, [i, j]) < s[i]).all()
            assert m["kept"][0][r][:2] == [i, j]
    if "first2" in e:
        assert all(k[:2] == list(e["first2"]) for k in m["kept"][0])
    if "kept" in e:
        assert m["kept"] == e["kept"]
    if "counts" in e:
        assert m["count"].tolist() == e["counts"]
    if "first" in e:
        assert [[k[0] for k in img] for img in m["kept"]] == e["first"]
    if name.startswith("tie_"):
        assert {"tie_lanes_62_63": 1025, "tie_waves_63_64": 1025, "tie_second_iteration_1023_1024": 1025, "tie_last_two_of_1023": 1023,
                "tie_last_two_of_1024": 1024, "tie_level_boundary_584_585": 760}[name] == N
        if name == "tie_level_boundary_584_585":
            assert SC.offsets(c)[1] == 585 and 585 % 1024 != 0 and m["where"][584][0] == 0 and m["where"][585] == (1, 0, 0)
        if "last_two" in name:
            assert e["top2"] == (N - 2, N - 1)
    if name.startswith("sole_finite"):
        s = c["cls_loss"][0][0].reshape(-1)
        assert int(np.isfinite(s).sum()) == 1 and np.isfinite(s[N - 1]) and N in (1023, 1024, 1025) and m["candidates"] == [[1, 1, 1]]
    if name == "k_1":
        assert c["K"] == 1 and m["count"].tolist() == [[1, 1, 1]]
    if name == "k_64":
        assert c["K"] == SC.MAX_K == 64 and m["candidates"][0] == [117] * 3 and all(len(set(k)) == 64 for k in m["kept"][0])
    if name == "k_above_survivors":
        assert all(0 < n < c["K"] for n in (m["count"][0, 0], m["count"][0, 2])) and (m["index"][0, 0, 3:] == -1).all()
    if e.get("one_window"):
        w = np.unique(np.concatenate([SM.crop_table(H, W, c["stride"], c["box"], iw, ih, *c["crop"])[0]
                                      for (H, W), (iw, ih) in zip(c["levels"], c["imgs"])]), axis=0)
        assert len(w) == 1 and c["crop"][0] > c["imgs"][0][0] and c["crop"][1] >= c["imgs"][0][1] and min(m["candidates"][0]) > c["K"]
    if name == "thr_1_guard":
        # the guard case really has IoU exactly 1 (and nothing is killed): all B labels of one anchor in label order, no triple twice
        ones = [p for p in m["pairs"][0][0] if float(p[4]) == 1.0 and p[5] == 1.0]
        assert c["thr"] == 1.0 and len(ones) >= c["B"] - 1 and not any(p[3] for p in m["pairs"][0][0])
        triples = [tuple(t) for t in m["index"][0, 0, :6].tolist()]
        assert len(set(triples)) == 6 and [t[1] for t in triples[:5]] == [0, 1, 2, 3, 4] and {t[2] for t in triples[:5]} == {5}
    if name == "thr_0_touch":
        first = [p for p in m["pairs"][0][0] if p[0] == 0]
        assert any(float(p[6][2]) == 0 and not p[3] for p in first)                              # windows that touch: inter 0, survives
        assert any(float(p[6][0]) == c["stride"] and p[3] for p in first) and e["killed"] not in m["kept"][0][0]
    if "at_threshold" in e:
        inter, union = e["at_threshold"]
        at = [p for p in m["pairs"][0][0] if float(p[6][2]) == inter and float(p[6][6]) == union]
        assert at and not any(p[3] for p in at) and all(p[4] == np.float32(c["thr"]) for p in at)   # IoU == thr: survives
        assert any(p[3] for p in m["pairs"][0][0])                                               # and closer windows die
        for k in m["kept"][0][0]:                                                                # in the floor-branch region
            l, _, p = m["where"][k]
            assert (m["branches_x"][l][p], m["branches_y"][l][p]) == ("floor", "floor")
    if name == "iou_exactly_thr_quotient":
        inter, union, thr = np.float32(2880), np.float32(4928), np.float32(c["thr"])
        assert not (np.float32(inter / union) > thr) and inter > np.float32(thr * union)           # quotient keeps it, a product test would not
    if name == "levels_8":
        assert len(c["levels"]) == SC.MAX_LEVELS == 8 and all(m["where"][k[0]][0] == 7 for k in m["kept"][0])
    if name == "rows":
        top = max(float(np.max(x)) for key in ("cls_loss", "loc_loss") for x in c[key])
        assert SC.PAD_SCORE > top and SC.PAD_FLAGS == 7                                          # the padding really would have won
    if name == "flag_bits":
        f, kept = c["flags"][0][0].reshape(-1), m["kept"][0]
        foreign = [i for i in range(N) if f[i] != 0 and f[i] & 7 == 0]
        assert len(foreign) == 6 and all(c["cls_loss"][0][0].reshape(-1)[i] == 5.0 for i in foreign)          # they would have won
        assert not set(foreign) & set(kept[0] + kept[1] + kept[2]) and all(12 + 1 in k and 12 + 6 in k for k in kept)
    if name == "score_table":
        s = c["cls_loss"][0][0, 0]
        assert [float(s[i]) for i in m["kept"][0][0]] == sorted((float(v) for v in s if np.isfinite(v)), reverse=True)
        assert m["kept"][0][0][0] == 4 and m["kept"][0][2][-1] == 4                               # opposite orders in one case
        assert np.isfinite(m["values"][0, :, :12, 16:18]).all() and float(s[4]) == SC.FLT_MAX
    if name == "images_3":
        assert N == 585 + 175 and N % 16 != 0 and m["count"][1].tolist() == [0, 0, 0] and m["count"][0].min() > 0
        assert sorted(c["cls_loss"][0][2].reshape(-1)) == sorted(c["cls_loss"][0][0].reshape(-1))
        assert any(p[3] for p in m["pairs"][0][0])                                               # kills happen
    if name == "chain_6_s12":
        assert all(len(ch) == SC.MAX_OPS for ch in c["chains"]) and c["corners"] is not None
        assert {k for ch in c["chains"] for k, _, _ in ch} == {1, 2, 3, 4} and np.abs(m["values"][0, :, 0, 8:16]).min() > 0
    if name == "wide_level_3600px":
        assert c["levels"][0][1] * c["stride"] >= 3600
