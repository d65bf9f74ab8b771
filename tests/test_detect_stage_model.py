"""CPU: the plain model of the detection stage (tests/detect_stage_model.py) against independent results, and every condition
the case tables (tests/detect_stage_cases.py) exist for, asserted from the model alone - a case that does not reach its regime
of the kernels fails here, before anyone runs a GPU."""
import os

import numpy as np
import pytest
import torch

import detect_stage_cases as C
import detect_stage_model as DM
import util
from oracle import decode_oracle as D

SMALL = 1500          # cases of at most this many candidates also go through the oracle's N x N greedy NMS
CACHE = 2048          # COVERAGE ONLY: KEPT_LDS of nms.hip, KCAP of detect_pyramid.hip, kcap of detect.hip at 8192 sort keys
ALL = [("level", n) for n in C.LEVEL_CASES] + [("pyramid", n) for n in C.PYRAMID_CASES]
ids = lambda p: "-".join(p)        # noqa: E731


def oracle_order(r, M):
    """decode_oracle.nms_chunked on the model's float32 boxes -> surviving candidates by decreasing score (stable)."""
    cand = r["cand"]
    scores = torch.from_numpy(np.where(cand["valid"], cand["scores"], -np.inf).astype(np.float32))
    boxes = torch.from_numpy(np.nan_to_num(cand["boxes32"]))
    got = D.nms_chunked(boxes, scores, 0.3, M)
    return got[torch.argsort(scores[got], descending=True, stable=True)].numpy(), boxes, scores


@pytest.mark.parametrize("case", ALL, ids=ids)
def test_model_matches_the_decode_oracle(case):
    c = C.case(*case)
    for r in C.model(*case):
        if len(r["cand"]["scores"]) > SMALL:
            continue
        M = c.get("M", len(r["cand"]["scores"]) + 1)
        ref, boxes, scores = oracle_order(r, M)
        assert np.array_equal(ref, r["order"])
        if r["passes"] == 1 and len(r["runs"][0]) <= 1:          # one chunk: a plain greedy NMS
            v = np.nonzero(r["cand"]["valid"])[0]
            assert np.array_equal(v[D.greedy_nms(boxes[v], scores[v], 0.3).numpy()], r["order"])


def test_decode_matches_the_decode_oracle():
    for case in (("level", "hw65"), ("pyramid", "levels_16"), ("level", "valid_counts")):
        c = C.case(*case)
        for lv in ([c["level"]] if case[0] == "level" else c["levels"]):
            ref = D.decode_level(torch.from_numpy(lv["loc"]).double(), lv["H"], lv["W"], lv["img_w"], lv["img_h"]).numpy()
            for b in range(lv["loc"].shape[0]):
                assert np.array_equal(DM.decode_level(lv["loc"][b], lv["H"], lv["W"], lv["img_w"], lv["img_h"]), ref[b])


def test_nms_model_matches_the_oracle_and_its_conditions():
    for name, c in C.NMS_CASES.items():
        for (keep, run), boxes, n in zip(C.nms_model(name), c["boxes"], c["counts"]):
            n = min(n, len(boxes))
            assert keep[n:].sum() == 0
            if n <= SMALL:
                ref = D.greedy_nms(torch.from_numpy(boxes[:n]), torch.arange(n, 0, -1).float(), c["iou_thr"])
                assert np.array_equal(np.sort(ref.numpy()), np.nonzero(keep)[0]), name
    N = C.NMS_CASES["counts"]["boxes"].shape[1]
    assert C.NMS_CASES["counts"]["counts"][:7] == [0, 1, 63, 64, 65, N, N + 1] and C.NMS_CASES["counts"]["counts"][7] > N
    # the kept count goes over the cache inside one step of 64 candidates, all 64 of them disjoint
    run = C.nms_model("across_2048")[0][1]
    assert run.kept_before(2048) == 2040 and run.kept_before(2112) == 2104 and not ((run.victim_pos >= 2048) & (run.victim_pos < 2112)).any()
    sup_pos = run.kept_pos[run.sup_rank]
    same_step = run.victim_pos // 64 == sup_pos // 64
    for far in (False, True):
        for same in (False, True):
            assert int((((run.sup_rank >= CACHE) == far) & (same_step == same)).sum()) >= 2, (far, same)
    assert [r.kept_count for _, r in C.nms_model("across_2048")] == [2300, 2104, 2039]
    # thresholds 0 and 1, zero-area boxes
    assert C.nms_model("iou_thr_0")[0][0].tolist() == [1, 1, 1, 1, 0, 1, 0, 1]       # touching boxes (inter == 0) survive
    assert C.nms_model("iou_thr_1")[0][0].tolist() == [1, 1, 1, 1, 1]                # identical boxes: IoU 1 is not > 1
    assert C.nms_model("zero_area")[0][0].tolist() == [1, 1, 1, 1, 1, 0]             # 0/0 compares false: both kept
    assert C.nms_model("zero_area")[1][0].tolist() == [1, 1, 0, 0, 0, 0]


def test_model_matches_the_reference_chunked_nms():
    d = np.load(os.path.join(util.GOLDEN, "nms_chunked.npz"))
    for name in d["cases"]:
        boxes, scores = d["boxes_" + name].astype(np.float32), d["scores_" + name].astype(np.float32)
        for thr_name, thr in (("tinf", -np.inf), ("t0", 0.0)):
            r = DM.nms_chunked(boxes, scores, scores > thr, 0.3, int(d["max_batch_" + name]))
            ref = d["ref_{}_{}".format(name, thr_name)]
            assert np.array_equal(ref[DM.stable_descending(scores[ref])], r["order"]), (name, thr_name)
            assert sorted(ref.tolist()) == sorted(r["order"].tolist())


def test_model_matches_the_reference_decode_pyramid():
    d = np.load(util.GOLDEN + "/decode_pyramid.npz")
    L, B = int(d["n_levels"]), int(d["n_classes"])
    orig = [float(v) for v in d["orig_size"]]
    levels = []
    for i in range(L):
        w, h = (int(v) for v in d["img_sizes"][i])
        H, W = d["ref_boxes_%d" % i].shape[1] // ((w + 15) // 16), (w + 15) // 16
        assert H * W == d["cls_%d" % i].shape[1]
        levels.append(C.make_level(H, W, d["loc_%d" % i], d["cls_%d" % i], C.scale_ops(orig[0] / w, orig[1] / h), img=(w, h)))
    for name, thr in (("t0", 0.0), ("tinf", -np.inf), ("t06", 0.6)):
        res = [DM.detect_label(levels, [b], thr, 0.3, 10000) for b in range(B)]
        assert np.array_equal(np.concatenate([r["cand"]["scores"][r["order"]] for r in res]), d["ref_%s_scores" % name])
        assert np.array_equal(np.concatenate([np.full(len(r["order"]), b) for b, r in enumerate(res)]), d["ref_%s_labels" % name])
        boxes = np.concatenate([r["cand"]["boxes64"][r["order"]] for r in res])
        assert np.abs(boxes - d["ref_%s_boxes" % name]).max() < 1e-3


# ------------------------------------------------------------------------------------------------------------ conditions
def test_band_is_empty_and_nothing_is_excluded():
    assert C.EXCLUDED == 0 and C.BAND == 1e-4
    for case in ALL:
        assert C.clean(C.model(*case)), case
        for r in C.model(*case):
            assert r["band"] >= C.BAND


def test_seeds():
    for kind, names in (("level", C.LEVEL_SEEDED), ("pyramid", C.PYRAMID_SEEDED)):
        for n in names:
            assert C.first_seed(kind, n) == C.SEEDS.get((kind, n), 0) == C.case(kind, n)["seed"], (kind, n)
    for b in range(4):
        assert C.first_pass_seed(b) == C.SEEDS[("passes", b)]


def crosses_inside(run, limit, step):
    """The kept count is under ``limit`` before some step of ``step`` candidates and over it after."""
    edges = list(range(0, run.n, step)) + [run.n]
    return any(run.kept_before(a) < limit < run.kept_before(b) for a, b in zip(edges, edges[1:]))


def test_level_conditions():
    assert [C.case("level", "hw%d" % n)["level"]["H"] * C.case("level", "hw%d" % n)["level"]["W"] for n in C.LEVEL_HW] == list(C.LEVEL_HW)
    assert C.LEVEL_HW == (1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025)
    lds = lambda hw: 6 * 8192 + ((2 * hw + 15) & ~15) + 16 * hw + 4608       # noqa: E731  (include/os2d_hip.h)
    assert lds(C.LEVEL_MAX_HW) <= 160 * 1024 < lds(C.LEVEL_MAX_HW + 1)
    lv = C.case("level", "max_level")["level"]
    assert (lv["H"], lv["W"]) == (1, C.LEVEL_MAX_HW)
    # valid candidates: 0 for three reasons, 1, 64, 65
    c, m = C.case("level", "valid_counts"), C.model("level", "valid_counts")
    assert [int(r["cand"]["valid"].sum()) for r in m] == c["valid"] == [0, 0, 0, 1, 64, 65]
    s = c["level"]["cls"]
    assert (s[0] <= 0).all() and (s[0] == 0).any() and (s[1] > 0).all() and np.isnan(s[2]).all()
    b1 = m[1]["cand"]["boxes64"]
    assert ((b1[:, 2] <= b1[:, 0]) | (b1[:, 3] <= b1[:, 1])).all()
    # kept list past kcap = 4 at 9 locations
    runs = [r["runs"][0][0] for r in C.model("level", "kcap_3x3")]
    assert [r.kept_count for r in runs] == [9, 8, 8]
    assert runs[1].sup_rank.tolist() == [6] and runs[2].sup_rank.tolist() == [0]
    # 60x80 and the largest level: past 2048 kept boxes
    for name in ("level_60x80", "max_level"):
        run = C.model("level", name)[0]["runs"][0][0]
        assert run.kept_count > CACHE and int((run.sup_rank >= CACHE).sum()) >= 10 and int((run.sup_rank < CACHE).sum()) >= 10
        assert crosses_inside(run, CACHE, 64), name
        sup_pos = run.kept_pos[run.sup_rank]
        assert int((run.victim_pos // 64 == sup_pos // 64).sum()) >= 10 and int((run.victim_pos // 64 > sup_pos // 64).sum()) >= 10
    # the score table
    for k, thr in enumerate(C.SCORE_THRESHOLDS):
        r = C.model("level", "table%d" % k)[0]
        assert int(r["cand"]["valid"].sum()) == C.TABLE_VALID[thr]
    assert C.model("level", "table0")[0]["order"].tolist() == [5, 6, 13, 11, 15, 8, 0, 2, 3, 9, 14]
    assert C.model("level", "table1")[0]["order"].tolist() == [5, 6, 13, 11, 15, 8]
    assert C.model("level", "table2")[0]["order"].tolist() == [5, 6, 13, 11]
    # chains
    ops = C.case("level", "chain_6")["level"]["ops"]
    kinds = [k for k, _, _ in ops]
    assert len(ops) == 6 and {DM.OP_HFLIP, DM.OP_VFLIP, DM.OP_SHIFT} <= set(kinds) and any(k == DM.OP_SCALE and ax != ay for k, ax, ay in ops)
    assert C.case("level", "chain_0")["level"]["ops"] == []
    assert len({int(r["cand"]["valid"].sum()) for r in C.model("level", "chain_6")}) == 3
    assert {C.case("level", n)["api"] for n in C.LEVEL_CASES} == {"scale", "ops"}


def test_pyramid_conditions():
    assert C.PYRAMID_N == (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
    for n in C.PYRAMID_N:
        assert all(len(r["cand"]["scores"]) == n for r in C.model("pyramid", "n%d" % n))
    assert {len(C.case("pyramid", n)["levels"]) for n in ("n1", "levels_2", "levels_16")} == {1, 2, 16}
    # chunking
    c, m = C.case("pyramid", "chunks_m"), C.model("pyramid", "chunks_m")
    M = C.CHUNK_M
    assert [int(r["cand"]["valid"].sum()) for r in m] == [M, M + 1, 2 * M] and [len(r["runs"][0]) for r in m] == [1, 2, 2] and c["M"] == M
    r = C.model("pyramid", "chunks_64")[0]
    assert len(r["runs"][0]) == 64 and r["passes"] == 1 and r["final_chunks"] == 64 and len(r["order"]) == 512
    assert all(C.expect_unfinished(C.case("pyramid", n), r) is False for n in ("chunks_m", "chunks_64") for r in C.model("pyramid", n))
    # one chunk keeping more than 2048: the four ways a suppressed candidate meets its suppressor, at least 10 of each
    for name in ("merged_twins", "single_72x96"):
        c, r = C.case("pyramid", name), C.model("pyramid", name)[0]
        assert r["passes"] == 1 and len(r["runs"][0]) == 1
        run, win = r["runs"][0][0], C.window(c)
        assert run.kept_count > CACHE and win == 2048
        k = run.classify(win)
        far = run.sup_rank >= CACHE
        assert int((far & k["earlier"]).sum()) >= 10
        assert int((far & ~k["earlier"] & (k["between"] >= 64)).sum()) >= 10          # the vote path
        assert int((~far).sum()) >= 10
        assert int((k["same_group"] & (k["between"] == 0)).sum()) >= 10              # the resolve path
        if name == "single_72x96":
            assert crosses_inside(run, CACHE, 1024)
            assert int((k["sup_pos"] // win < run.victim_pos // win).sum()) >= 10
    assert C.case("pyramid", "merged_twins")["slot_rows"] == [[0, 1]]
    # passes
    c, m = C.case("pyramid", "passes"), C.model("pyramid", "passes")
    P = c["passes"]
    assert [r["passes"] for r in m] == [1, 2, P, P + 1] and m[1]["ended"] == "nothing removed" and len(m[0]["runs"][0]) > 1
    assert [C.expect_unfinished(c, r) for r in m] == [False, False, False, True]
    # the boundary of the final sort
    c, r = C.case("pyramid", "finalize_16384"), C.model("pyramid", "finalize_16384")[0]
    assert (c["M"], len(r["order"]), r["final_chunks"], r["passes"]) == (8192, 16384, 2, 1) and not C.expect_unfinished(c, r)
    c, r = C.case("pyramid", "finalize_16512"), C.model("pyramid", "finalize_16512")[0]
    assert (c["M"], len(r["order"]), r["passes"]) == (8193, 16512, 1) and r["final_chunks"] > 1 and C.expect_unfinished(c, r)
    # merged labels
    c = C.case("pyramid", "merged_ragged")
    assert [sum(1 for x in rows if x >= 0) for rows in c["slot_rows"]] == [3, 1, 2] and any(x < 0 for rows in c["slot_rows"] for x in rows)
    for g, r in enumerate(C.model("pyramid", "merged_ragged")):
        s, N1 = r["cand"]["scores"], r["cand"]["N1"]
        if g == 0:        # row 1 repeats row 0, score for score and box for box: the tie goes to row 0, whose box kills the copy
            assert r["cand"]["valid"][N1:2 * N1].any() and not ((r["order"] >= N1) & (r["order"] < 2 * N1)).any()
        if g == 2:        # rows 4 and 5 share a handful of score values
            kept = s[r["order"]]
            tied = [(a, b) for a, b in zip(r["order"][:-1], r["order"][1:]) if s[a] == s[b]]
            assert any(a // N1 != b // N1 for a, b in tied), "survivors of two rows of the label with one score"
            assert all(a < b for a, b in tied) and (np.diff(kept) <= 0).all()
    # the score table over two levels and two rows
    for k, thr in enumerate(C.SCORE_THRESHOLDS):
        c, r = C.case("pyramid", "table%d" % k), C.model("pyramid", "table%d" % k)[0]
        assert len(c["levels"]) == 2 and c["slot_rows"] == [[0, 1]] and int(r["cand"]["valid"].sum()) == 2 * C.TABLE_VALID[thr]
    assert C.model("pyramid", "table0")[0]["order"].tolist()[:2] == [5, 6]
    # chains
    for name in ("chains", "chains_no_corners", "chains_merged"):
        c = C.case("pyramid", name)
        for lv in c["levels"]:
            assert lv["ops"] != lv["dops"] and {DM.OP_HFLIP, DM.OP_VFLIP} <= {k for k, _, _ in lv["ops"]}
            assert (lv["corners"] is None) == (name == "chains_no_corners")
        assert max(len(lv["dops"]) for lv in c["levels"]) == 12
    assert {C.case("pyramid", n)["api"] for n in C.PYRAMID_CASES} == {"plain", "merged", "ops"}
