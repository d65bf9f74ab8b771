"""CPU: tests/voc_eval_stage_model.py (one plain function per entry point of libos2d_eval.so, written as loops) against the
recorded fixtures, against tests/voc_eval_model.py (the parallel formulation in vectorised torch) on the fixtures and on every
case of tests/voc_eval_stage_cases.py where the latter is defined, and against values written out by hand where it is not: an
IoU exactly on the threshold, ties, labels outside [0, L), the 11-point levels.  The two models share no code; the GPU tests
(tests/test_voc_eval_stages_gpu.py) compare the kernels with the stage model only."""
import math

import numpy as np
import pytest
import torch

import voc_eval_cases as VC
import voc_eval_model as M
import voc_eval_stage_cases as C
import voc_eval_stage_model as S
import voc_eval_util as U

EPS = 2.0 ** -52
NAN = float("nan")


def numpy_case(p):
    """The packed tensors of voc_eval_model.pack as the arrays of the entry points."""
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    N = p["N"]
    offsets = lambda image: np.concatenate([[0], np.cumsum(np.bincount(n(image), minlength=N))]).astype(np.int32)   # noqa: E731
    return dict(det_boxes=n(p["boxes"]), det_scores=n(p["scores"]), det_labels=n(p["labels"]).astype(np.int32), det_offsets=offsets(p["image"]),
                gt_boxes=n(p["gt_boxes"]), gt_labels=n(p["gt_labels"]).astype(np.int32), gt_difficult=n(p["gt_difficult"]).astype(np.uint8),
                gt_offsets=offsets(p["gt_image"]))


def torch_case(c):
    """The arrays of a match case as the packed dictionary of voc_eval_model."""
    t = torch.from_numpy
    image = lambda o: torch.repeat_interleave(torch.arange(len(o) - 1), t(np.diff(o).astype(np.int64)))   # noqa: E731
    return dict(boxes=t(c["det_boxes"]), scores=t(c["det_scores"]), labels=t(c["det_labels"].astype(np.int64)), image=image(c["det_offsets"]),
                gt_boxes=t(c["gt_boxes"]), gt_labels=t(c["gt_labels"].astype(np.int64)), gt_difficult=t(c["gt_difficult"] != 0),
                gt_image=image(c["gt_offsets"]), N=len(c["det_offsets"]) - 1)


# ------------------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("use_07", (False, True))
@pytest.mark.parametrize("thr", VC.THRESHOLDS)
@pytest.mark.parametrize("name", VC.CASES)
def test_chained_stages_reproduce_the_reference_and_the_other_model(name, thr, use_07):
    fx = U.fixture(name)
    images, preds, gts = U.resized_case(name)
    U.check_inputs(name, images, fx)
    p = U.model_pack(preds, gts, torch.device("cpu"))
    L = VC.NUM_LABELS[name]
    c = numpy_case(p)
    r = S.evaluate(c, L, thr, use_07)
    image = np.repeat(np.arange(p["N"]), np.diff(c["det_offsets"]))
    U.compare(fx, thr, use_07, dict(match=r["match"], labels=c["det_labels"], image=image, scores=c["det_scores"], tp=r["tp"], fp=r["fp"],
                                    prec=r["prec"], rec=r["rec"], class_counts=np.diff(r["class_offsets"]), gt_counts=r["gt_count"], n_pos=r["n_pos"][:L],
                                    ap_per_class=r["ap_per_class"], recall_per_class=r["recall_per_class"], scalars=r["scalars"]))
    ref = M.evaluate(p, L, thr, use_07)
    n = lambda k: ref[k].numpy()   # noqa: E731
    assert np.array_equal(r["match"], n("match")) and np.array_equal(r["perm_joint"], n("order_joint")) and np.array_equal(r["perm_class"], n("order_class"))
    assert np.array_equal(r["n_pos"][:L], n("n_pos")) and np.array_equal(r["gt_count"], n("gt_counts"))
    for a, b in (("tp", "tp"), ("fp", "fp"), ("tp_joint", "tp_joint"), ("fp_joint", "fp_joint")):
        assert np.array_equal(r[a], n(b)), a
    for a in ("prec", "rec", "prec_joint", "rec_joint"):
        assert S.same_bits(r[a], n(a)), a
    assert S.same_bits(r["recall_per_class"], n("recall_per_class"))
    # the same terms in another order: |difference| <= n * 2^-52 * sum, n <= the detections of the class, sum <= 1
    assert np.array_equal(np.isnan(r["ap_per_class"]), np.isnan(n("ap_per_class")))
    bound = (np.diff(r["class_offsets"]) + 11) * EPS
    assert (np.abs(np.nan_to_num(r["ap_per_class"]) - np.nan_to_num(n("ap_per_class"))) <= bound).all()
    D = len(c["det_scores"])
    for k, key in enumerate(("map", "map_weighted", "recall", "ap_joint_classes")):
        assert abs(r["scalars"][k] - float(ref[key])) <= (D + L + 2) * EPS, key


# -------------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("c", C.count_cases(), ids=lambda c: c["name"])
def test_count_gt(c):
    n_pos, gt_count = S.count_gt(c["gt_labels"], c["gt_difficult"], c["L"])
    labels, plain = c["gt_labels"].astype(np.int64), c["gt_difficult"] == 0
    ok = (labels >= 0) & (labels < c["L"])
    assert np.array_equal(gt_count, np.bincount(labels[ok], minlength=c["L"]))
    assert np.array_equal(n_pos[:-1], np.bincount(labels[ok & plain], minlength=c["L"])) and n_pos[-1] == (ok & plain).sum()
    if len(labels) >= 2:
        assert (~ok).sum() >= 2 or c["name"].endswith("one_label")


MATCH = C.match_cases()


@pytest.mark.parametrize("c", MATCH, ids=lambda c: c["name"])
def test_match(c):
    m, index = S.match(c["det_boxes"], c["det_scores"], c["det_labels"], c["det_offsets"], c["gt_boxes"], c["gt_labels"], c["gt_difficult"],
                       c["gt_offsets"], c["thr"])
    if c["expect_match"] is not None:       # written out by hand
        assert m.tolist() == list(c["expect_match"]) and index.tolist() == list(c["expect_index"])
    ref, _ = M.match(torch_case(c), c["thr"])
    assert np.array_equal(m, ref.numpy())
    assert ((index >= 0) | (m == 0)).all()


def test_match_table_holds_what_it_names():
    by = {c["name"]: c for c in MATCH}
    assert S.iou_f32(C.TALL, C.HALF) == np.float32(0.5) and S.iou_f32(C.TALL, C.THREEQ) == np.float32(0.75)
    assert np.float32(by["iou_one_ulp_below_thr_0.5"]["thr"]) == np.nextafter(np.float32(0.5), np.float32(1))
    assert np.signbit(by["tie_zero_minus_plus"]["det_scores"][1]) and not np.signbit(by["tie_zero_minus_plus"]["det_scores"][2])
    sub = by["tie_subnormal"]["det_scores"]
    assert 0 < sub[1] < np.finfo(np.float32).tiny and sub[3] < 0
    assert len(by["tie_crowd"]["det_scores"]) > 256 and len(by["no_ground_truth_D257"]["gt_labels"]) == 0
    assert sorted(len(c["det_scores"]) for c in MATCH if c["name"].startswith("drawn_N1")) == [1, 255, 256, 257]


SORT = C.sort_cases() + C.pass_count_cases()


@pytest.mark.parametrize("c", SORT, ids=lambda c: c["name"])
def test_sort(c):
    joint, by_class, keys, offsets = S.sort(c["scores"], c["labels"], c["L"])
    scores, labels = torch.from_numpy(c["scores"]), torch.from_numpy(c["labels"].astype(np.int64))
    order = torch.sort(scores, descending=True, stable=True).indices
    assert np.array_equal(joint, order.numpy())
    assert np.array_equal(by_class, order[torch.sort(labels[order], stable=True).indices].numpy())
    assert np.array_equal(keys, c["labels"][by_class.astype(np.int64)])
    assert np.array_equal(np.diff(offsets), np.bincount(c["labels"], minlength=c["L"])) and offsets[0] == 0
    assert (c["L"] - 1) >> c["label_bits"] == 0


def test_sort_table_holds_what_it_names():
    by = {c["name"]: c for c in SORT}
    assert sorted(set(len(c["scores"]) for c in SORT if c["name"].endswith("all_equal"))) == sorted(set(C.SORT_D + (C.WAVE + 1, C.TILE + 1)))
    assert 256 * -(-C.SORT_SECOND_ROUND // C.TILE) > C.RADIX_ROUND
    low = by["D513_lowest_byte"]["scores"].view(np.uint32)
    assert len(set(low >> 8)) == 1 and len(set(low & 255)) > 100
    high = by["D513_highest_byte"]["scores"].view(np.uint32)
    assert len(set(high & 0xFFFFFF)) == 1 and len(set(high >> 24)) > 100 and np.isfinite(by["D513_highest_byte"]["scores"]).all()
    runs = by["D{}_runs_on_edges".format(C.TILE + C.WAVE + 1)]["scores"]
    for edge in (C.WAVE, C.TILE):
        assert len(set(runs[edge - 32:edge + 32])) == 1 and runs[edge - 33] != runs[edge - 32] != runs[edge + 32]
    assert np.signbit(by["D513_zeros"]["scores"]).any() and not np.signbit(by["D513_zeros"]["scores"]).all()
    assert [c["label_bits"] for c in C.pass_count_cases()] == [3, 9, 17, 25]
    assert by["L65537_bits17"]["labels"].max() == 65536


def test_sort_with_labels_outside_by_hand():
    """L = 5 too small for the labels 256, 261, 65536 + 2 and -1: those rows follow the classes, in descending score, and
    everything of the classes 0 .. 4 is what the same call gives without them.  voc_eval_model.py is not defined here."""
    c = C.out_of_range_case()
    scores, labels = c["scores"], c["labels"]
    joint, by_class, keys, offsets = S.sort(scores, labels, 5)
    r2 = lambda rows: [round(float(scores[i]), 2) for i in rows]   # noqa: E731
    assert r2(joint) == [round(0.90 - 0.05 * k, 2) for k in range(18)]
    assert r2(by_class) == [0.90, 0.80, 0.50, 0.25, 0.60, 0.75, 0.65, 0.15, 0.40, 0.35, 0.10, 0.85, 0.70, 0.55, 0.45, 0.30, 0.20, 0.05]
    assert keys.tolist() == [0, 0, 0, 0, 1, 2, 2, 2, 3, 4, 4] + [5] * 7 and offsets.tolist() == [0, 4, 5, 8, 9, 11]
    inside = np.flatnonzero((labels >= 0) & (labels < 5))
    j2, c2, k2, o2 = S.sort(scores[inside], labels[inside], 5)
    assert np.array_equal(inside[c2.astype(np.int64)], by_class[:11]) and np.array_equal(k2, keys[:11]) and np.array_equal(o2, offsets)
    # the curves of the classes: by hand for class 0 (hit, miss, hit, miss of 3 positives) and class 2 (miss, hit, difficult of 2)
    tp, fp, prec, rec, last = S.prec_rec(c["match"], by_class, keys, c["n_pos"], 5)
    assert tp[:4].tolist() == [1, 1, 2, 2] and fp[:4].tolist() == [0, 1, 1, 2] and prec[:4].tolist() == [1.0, 0.5, 2 / 3, 0.5]
    assert rec[:4].tolist() == [1 / 3, 1 / 3, 2 / 3, 2 / 3] and prec[5:8].tolist() == [0.0, 0.5, 0.5] and rec[5:8].tolist() == [0.0, 0.5, 0.5]
    assert last == {0: 2 / 3, 1: 1.0, 2: 0.5, 4: 1.0}          # class 3 has no positives; the rows outside have no n_pos
    assert tp[11:].tolist() == [0] * 7 and fp[11:].tolist() == [1, 2, 3, 4, 5, 6, 7] and np.isnan(rec[11:]).all()
    mpre, terms = S.ap(prec, rec, keys, 5, False)
    assert sorted(terms) == [0, 1, 2, 3, 4] and math.fsum(terms[0]) == (1 / 3) * 1.0 + (2 / 3 - 1 / 3) * (2 / 3) and terms[2] == [0.5 * 0.5]
    t2, f2, p2, r2_, l2 = S.prec_rec(c["match"][inside], c2, k2, c["n_pos"], 5)
    assert np.array_equal(tp[:11], t2) and np.array_equal(fp[:11], f2) and S.same_bits(prec[:11], p2) and S.same_bits(rec[:11], r2_) and last == l2
    m2, terms2 = S.ap(p2, r2_, k2, 5, False)
    assert S.same_bits(mpre[:11], m2) and {k: v for k, v in terms.items() if not np.isnan(v).any()} == {k: v for k, v in terms2.items() if not np.isnan(v).any()}


scan_table, curves = C.scan_table, C.scan_reference


@pytest.mark.parametrize("c", scan_table(), ids=lambda c: c["name"])
def test_prec_rec_and_ap(c):
    """Against voc_eval_model.curves / average_precision on the segments whose label lies in [0, L) (it indexes n_pos by the
    label and is not defined outside); outside, by the rule: no n_pos, so rec = tp / 0."""
    r = curves(c)
    D, L = c["D"], c["L"]
    seg = np.zeros(D, np.int64) if c["seg"] is None else c["seg"].astype(np.int64)
    inside = (seg >= 0) & (seg < L)
    m_sorted = torch.from_numpy(c["match"][c["perm"].astype(np.int64)][inside])
    tseg = torch.from_numpy(seg[inside])
    tp, fp, prec, rec, mpre = M.curves(m_sorted, tseg, torch.from_numpy(c["n_pos"].astype(np.int64)), L)
    assert np.array_equal(r["tp"][inside], tp.numpy()) and np.array_equal(r["fp"][inside], fp.numpy())
    assert S.same_bits(r["prec"][inside], prec.numpy()) and S.same_bits(r["rec"][inside], rec.numpy())
    assert S.same_bits(r["ap"][0][inside], mpre.numpy()) and S.same_bits(r["ap07"][0], r["ap"][0])
    out = ~inside
    assert (r["rec"][out][r["tp"][out] == 0] != r["rec"][out][r["tp"][out] == 0]).all() and np.isinf(r["rec"][out][r["tp"][out] > 0]).all()
    assert set(r["last"]) == set(int(s) for s in np.unique(seg[inside]) if c["n_pos"][s] > 0)
    ap = M.average_precision(rec, mpre, tseg, L, False).numpy()
    ap07 = M.average_precision(rec, mpre, tseg, L, True).numpy()
    for s in np.unique(seg[inside]):
        terms, row = r["ap"][1][int(s)], r["ap07"][1][int(s)]
        if c["n_pos"][s] > 0:
            assert all(t >= 0 for t in terms) and abs(ap[s] - math.fsum(terms)) <= len(terms) * EPS * math.fsum(terms)
            assert S.class_ap(row, True) == ap07[s]
        else:
            assert not np.isfinite(ap[s]) and not np.isfinite(terms).all()      # rec = tp / 0: NaN, then inf


def test_scan_table_holds_what_it_names():
    names = [c["name"] for c in scan_table()]
    assert len(set(names)) == len(names)
    assert C.SCAN_D == (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 526339) and C.SEGMENT_LENGTHS == (7, 8, 9, 511, 512, 513, 2047, 2048, 2049)
    assert -(-C.SCAN_SECOND_ROUND // C.TILE) > C.CARRY_ROUND
    span = C.span_case()
    starts = np.flatnonzero(np.diff(span["seg"])) + 1
    assert starts[0] == 3 * C.TILE and not ((starts >= C.TILE) & (starts < 3 * C.TILE)).any() and len(starts) > C.ITEMS
    c = [c for c in scan_table() if c["name"] == "D4097_segments_of_8"][0]
    assert c["seg"][0] == -1 and c["seg"][-1] > c["L"] and (c["n_pos"] == 0).any()
    r = curves(c)
    assert np.isnan(r["prec"]).any() and np.isinf(r["rec"]).any() and np.isnan(r["rec"]).any()


def test_ap07_levels_by_hand():
    c = C.ap07_levels_case()
    r = curves(c)
    assert r["rec"][:5].tolist() == [0.1, 0.1, 0.2, 3 / 10.0, 3 / 10.0] and not 3 / 10.0 >= 0.1 * 3 and 1 / 2.0 == 0.1 * 5
    row = r["ap07"][1]
    assert row[0] == [1.0, 1.0, 0.75, 0, 0, 0, 0, 0, 0, 0, 0]       # level 0.2 first reached at position 2: max(2/3, 3/4)
    assert row[1] == [0.5] * 6 + [0.0] * 5 and row[2] == [0.0] * 11
    assert r["last"] == {0: 0.3, 1: 0.5, 2: 0.0}


@pytest.mark.parametrize("use_07", (False, True))
@pytest.mark.parametrize("c", C.finalise_cases(), ids=lambda c: c["name"])
def test_finalise(c, use_07):
    """Against numpy's nanmean / nansum, the reference's own words (voc_eval.py:65, 232-253)."""
    L, n_pos = c["L"], c["n_pos"].astype(np.float64)
    ap, rc, n_out, scalars = S.finalise(c["acc"], c["rec_last"], c["n_pos"], L, use_07)
    seen = n_pos[:L] > 0
    assert np.array_equal(np.isnan(ap), ~seen) and np.array_equal(np.isnan(rc), ~seen) and np.array_equal(n_out, n_pos[:L])
    ref_ap = np.array([S.class_ap(c["acc"][l], use_07) for l in range(L)])
    assert np.array_equal(ap[seen], ref_ap[seen]) and np.array_equal(rc[seen], c["rec_last"][:L][seen])
    if not seen.any():
        # no class with positives: nanmean, the recall and the joint AP are NaN, the reference's nansum is 0.0
        assert np.isnan(scalars[[0, 2, 3]]).all() and scalars[1] == 0.0
        return
    bound = (L + 2) * EPS
    ref = [ap[seen].mean(), (ap[seen] * n_pos[:L][seen] / n_pos[L]).sum(), (n_pos[:L][seen] * rc[seen]).sum() / n_pos[L], S.class_ap(c["acc"][L], use_07)]
    for got, want in zip(scalars, ref):
        assert abs(got - want) <= bound * abs(want)
    if c["name"].endswith("mixed"):
        assert ((ap == 0.0) & (rc == 0.0)).any()
