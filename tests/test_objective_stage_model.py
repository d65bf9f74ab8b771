"""CPU: the conditions the cases of tests/objective_stage_model.py must meet, asserted on the models alone (the kernels are
judged in tests/test_objective_stages_gpu.py): the model reproduces the fixtures recorded from the reference; the float64 and the
fp32 evaluation decide every element alike; every threshold that is not a deliberate boundary case keeps a margin, with NO
element excluded; the mining cases have the k, plateau and low-byte properties they claim.  The last test prints the fp32 CPU
evaluation's own error against float64 per quantity - the scale the kernels are expected to sit near (run with -s)."""
import numpy as np
import pytest
import torch

import objective_cases as OC
import objective_stage_model as S
import objective_util as U

RTOL = 2e-6          # fixtures: as tests/test_objective_model.py


def fixture_case(name, level, fx):
    c = OC.CASES[name]
    gt = [(b, l.to(torch.int32), d.to(torch.uint8)) for b, l, d in U.level_boxes(name, level, fx["boxes"])]
    return dict(name=name, A=c["A"], B=c["B"], H=level[0], W=level[1], stride=OC.STRIDE, rec_field=OC.BOX_SIZE - 14 * OC.STRIDE,
                high=OC.IOU["pos"], low=OC.IOU["neg"], ops=None, gt=gt, loc_scores=None, special=None)


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_assignment_model_reproduces_the_fixtures(name):
    c, fx = OC.CASES[name], U.load_targets(name)
    split = [h * w for h, w in c["levels"]]
    got = dict(cls=[], loc=[], rem=[], ia=[], ic=[])
    for level, loc in zip(c["levels"], torch.from_numpy(fx["loc_preds"]).split(split, 3)):
        case = fixture_case(name, level, fx)
        enc = S.assign(case, 0, S.F32)
        rem = S.assign(dict(case, high=OC.IOU["remap_pos"], low=OC.IOU["remap_neg"], loc_scores=loc.contiguous()), 1, S.F32)
        for k, v in (("cls", enc["cls"]), ("loc", enc["loc"]), ("rem", rem["cls"]), ("ia", rem["ia"]), ("ic", rem["ic"])):
            got[k].append(v)
    got = {k: torch.cat(v, 3 if k == "loc" else 2).numpy() for k, v in got.items()}
    assert np.array_equal(got["cls"], fx["cls_targets"].astype(np.int64))
    assert np.array_equal(got["rem"], fx["cls_targets_remapped"].astype(np.int64))
    assert np.array_equal(got["ia"], fx["ious_anchor"]) and np.array_equal(got["ic"], fx["ious_anchor_corrected"])
    assert U.rel_err(got["loc"], fx["loc_targets"]) <= 1e-6


@pytest.mark.parametrize("loss", OC.LOSSES)
@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_objective_model_reproduces_the_fixtures(name, loss):
    c, fx, ref = OC.CASES[name], U.load_targets(name), U.load_loss(name, loss)
    t = lambda k, dt=None: torch.from_numpy(fx[k] if dt is None else fx[k].astype(dt))   # noqa: E731
    inp = dict(loc_preds=t("loc_preds"), loc_targets=t("loc_targets"), cls_preds=t("cls_preds"), cls_targets=t("cls_targets", np.int64),
               cls_targets_remapped=t("cls_targets_remapped", np.int64) if c["remap"] else None,
               cls_preds_for_neg=t("cls_preds_for_neg") if c["remap"] else None)
    par = dict(loss=loss, patch=c["patch"], ratio=float("inf") if loss == "RLL" else OC.CRITERION["neg_to_pos_ratio"],
               rll_ratio=OC.CRITERION["rll_neg_weight_ratio"], **{k: OC.CRITERION[k] for k in S.CRITERION})
    for dtype in (S.F32, S.F64):
        out = S.objective_outputs(inp, par, dtype)
        for i, key in enumerate(S.SCALARS):
            assert abs(out[key] - float(ref["scalars"][i])) <= RTOL * max(1.0, abs(float(ref["scalars"][i]))), (key, dtype)
        flags = out["flags"].numpy()
        assert np.array_equal((flags & S.F_POS) != 0, ref["pos_mask"]) and np.array_equal((flags & S.F_NEG) != 0, ref["neg_mask"])
        assert np.array_equal((flags & S.F_POSREG) != 0, ref["pos_reg_mask"])
        assert U.rel_err(out["cls_loss"].numpy(), ref["cls_loss"]) <= RTOL
        for key in ("dloc", "dcls") + (("dcls_for_neg",) if c["remap"] else ()):
            assert U.rel_err(out[key].numpy(), ref[key]) <= RTOL, (key, dtype)
            assert np.array_equal(out[key].numpy() != 0, ref[key] != 0), (key, dtype)


ASSIGN_TABLES = [("encode", S.encode_cases, 0), ("encode ops", S.ops_cases, 0), ("remap", S.remap_cases, 1), ("remap ops", S.remap_ops_cases, 1)]


@pytest.mark.parametrize("table,cases,mode", ASSIGN_TABLES, ids=[t[0] for t in ASSIGN_TABLES])
def test_assignment_float64_and_fp32_decide_alike(table, cases, mode):
    for case in cases():
        lo, hi = S.assigned(case, mode, S.F32), S.assigned(case, mode, S.F64)
        assert torch.equal(lo["cls"], hi["cls"]), case["name"]
        assert all(bool(torch.isfinite(v).all()) for m in (lo, hi) for k, v in m.items() if k in ("loc", "ia", "ic")), case["name"]


def test_encode_cases_sit_where_they_claim():
    for case in S.encode_cases():
        m = S.assigned(case, 0, S.F32)
        if case["boundary"]:
            got = [int(m["cls"][a, b, p]) for a, b, p, _ in case["boundary"]]
            # IoU == threshold: `best < high` / `best < low` are false, the anchor is matched / ignored; one step below: ignored / negative
            assert got == ([-1, 0] if "below" in case["name"] else [1, -1]), (case["name"], got)
            HW = case["H"] * case["W"]
            assert int(m["cls"][0, 1, HW // 2]) == 1, "the first of two identical boxes is not difficult: positive"
            assert int(m["cls"][0, 2, HW - 1]) == -1, "a matched difficult box: ignored"
            assert m["has"].tolist() == [[True] * 4, [False] * 4, [True, True, False, True]]
            assert int((m["cls"][2, 0] != 0).sum()) == 0 and bool(torch.isfinite(m["loc"][2, 0]).all()), "the box far outside"
            thin = case["gt"][0][0][4]
            assert float(thin[2] - thin[0]) < 1
    empty = [c for c in S.encode_cases() if "no boxes" in c["name"]][0]
    assert all(g[0].shape[0] == 0 for g in empty["gt"]) and not S.assigned(empty, 0, S.F32)["has"].any()
    plain, nops0 = S.assigned(S.encode_cases()[2], 0, S.F32), S.assigned(S.ops_cases()[0], 0, S.F32)
    assert S.ops_cases()[0]["ops"] == [] and plain["cls"].shape == nops0["cls"].shape
    assert [len(c["ops"]) for c in S.ops_cases()] == [0, 1, 1, 1, 1, 6] and {o[0] for o in S.OPS_CHAIN} == {1, 2, 3, 4}


def test_remap_cases_keep_their_margins_with_no_element_excluded():
    for case in S.remap_cases() + S.remap_ops_cases():
        iou_margin, clamp_margin, _ = S._remap_margin(case)
        assert iou_margin > S.REL_MARGIN and clamp_margin > S.REL_MARGIN, (case["name"], iou_margin, clamp_margin)
        if case["special"].any():
            assert int(case["special"].sum()) == 8
            loc, m = case["loc_scores"], S.assigned(case, 1, S.F32)
            at = case["special"][:, :, 2].nonzero().tolist()
            values = sorted(float(loc[a, b, 2, p]) for a, b, p in at)
            assert values == [-1e4, -600.0, S.next_up(S.CLIP_SCORE), 1e4]
            a, b, p = [x for x in at if float(loc[x[0], x[1], 2, x[2]]) == -600.0][0]
            assert float(m["ic"][a, b, p]) == 0.0, "expf underflows: a decoded box of zero area has IoU 0"
            assert np.float32(S.next_up(S.CLIP_SCORE)) / np.float32(5) >= np.float32(S.XFORM_CLIP) > np.float32(S.next_down(S.CLIP_SCORE)) / np.float32(5)


ALL_SCENARIOS = [(shape, remap) for shape in S.OBJ_SHAPES for remap in (False, True)]
scenario_ids = [S.shape_id(s) + ("_remap" if r else "") for s, r in ALL_SCENARIOS]


@pytest.mark.parametrize("shape,remap", ALL_SCENARIOS, ids=scenario_ids)
def test_objective_float64_and_fp32_decide_alike(shape, remap):
    for name, inp, par, _ in S.scenarios(shape, remap):
        lo, hi = S.objective_outputs(inp, par, S.F32), S.objective_outputs(inp, par, S.F64)
        assert torch.equal(lo["flags"], hi["flags"]), name
        for k in ("dloc", "dcls", "dcls_for_neg", "coef"):
            if lo[k] is not None:
                assert torch.equal(lo[k] != 0, hi[k] != 0), (name, k)
        if par["loss"] == "RLL":
            assert S.rll_margin(inp, par) > S.REL_MARGIN, name


@pytest.mark.parametrize("shape,remap", ALL_SCENARIOS, ids=scenario_ids)
def test_scenarios_have_the_properties_they_claim(shape, remap):
    A, B, HW = shape
    seen = set()
    for name, inp, par, facts in S.scenarios(shape, remap):
        out = S.objective_outputs(inp, par, S.F32)
        pos, cand, pos_reg = S.masks(inp)
        neg, loss_bits = out["neg"].view(-1), S.bits(out["cls_loss"]).view(-1)
        cand_idx = cand.view(-1).nonzero().view(-1).tolist()
        seen.add(name)
        if "k" in facts and "total" in facts:
            assert facts["total"] == len(cand_idx) and int(neg.sum()) == min(facts["k"], facts["total"]), name
        if "plateau" in facts:
            pl, krem, above = facts["plateau"], facts["krem"], facts["above"]
            assert len(pl) >= 3 and len({int(loss_bits[i]) for i in pl}) == 1, name
            assert len({i // HW for i in pl}) >= 2, "the plateau spans two (image, label) rows"
            if HW == 257:
                assert any(i % HW < S.OBJ_THREADS for i in pl) and any(i % HW >= S.OBJ_THREADS for i in pl if i // HW == pl[0] // HW)
            others = [i for i in cand_idx if i not in pl and i not in above]
            assert all(int(loss_bits[i]) > int(loss_bits[pl[0]]) for i in above) and all(int(loss_bits[i]) < int(loss_bits[pl[0]]) for i in others)
            assert neg.nonzero().view(-1).tolist() == sorted(above + pl[:krem]), name
        if "pair" in facts:
            hi, lo = facts["pair"]
            x = int(loss_bits[hi]) ^ int(loss_bits[lo])
            assert 0 < x < 256 and int(loss_bits[hi]) > int(loss_bits[lo]) and hi > lo, name
            assert neg.nonzero().view(-1).tolist() == sorted(facts["above"] + [hi]), name
        if facts.get("all_zero"):
            assert all(int(loss_bits[i]) == 0 for i in cand_idx) and neg.nonzero().view(-1).tolist() == cand_idx[:facts["k"]], name
        if par["loss"] == "RLL" and not par["patch"]:
            max_l, norm, weights = S.rll_threshold_quantities(inp, par)
            if facts.get("dead_label"):
                assert 0 < float(max_l[0]) < S.RLL_LIVE and bool((max_l[1:] > S.RLL_LIVE).any()), name
            if facts.get("one_image_label"):
                assert bool(cand[0, 1].any()) and not bool(cand[1:, 1].any()), name
            if facts.get("both_sides"):
                assert bool((weights < S.RLL_WEIGHT_CUT).any()) and bool((weights > S.RLL_WEIGHT_CUT).any()), name
            if facts.get("trivial"):
                assert int(pos.sum()) > 0 and out["cls_pos"] == 0.0 and not bool((out["dcls"][pos] != 0).any()), name
            if facts.get("no_pos"):
                assert int(pos.sum()) == 0 and int(neg.sum()) == 0 and int(cand.sum()) > 0, name
        # the fixed elements of base_inputs
        if A * B * HW > 1 and not facts.get("no_pos"):
            x, xn = inp["cls_preds"].view(-1), S._neg_scores(inp).view(-1)
            assert bool(pos.view(-1)[0]) and float(x[0]) == S.MARGIN_POS and bool(cand.view(-1)[1]) and float(xn[1]) == S.MARGIN
            flags = out["flags"].view(-1)
            assert int(flags[0]) & S.F_HINGE and int(flags[1]) & S.F_HINGE
            if par["loss"] == "RLL" and not facts.get("trivial"):      # torch's clamp passes the gradient at the kink
                assert float(out["dcls"].view(-1)[0]) < 0, name
                if par["patch"]:
                    assert float((out["dcls"] if out["dcls_for_neg"] is None else out["dcls_for_neg"]).view(-1)[1]) > 0, name
            d = (inp["loc_preds"] - inp["loc_targets"]).view(A * B, 4, HW)
            assert d[0, :, 0].tolist() == [1.0, S.next_up(1.0), S.next_down(1.0), -1.0] and bool(pos_reg.view(-1)[0])
            assert bool((S._effective(inp)[A - 1, B - 1] == -1).all())
            assert bool(cand.view(-1)[2]) and bool(pos_reg.view(-1)[2]) == remap, "a regression positive that is a class negative"
    if A * B * HW > 16:
        for want in ("k=0", "k=1", "plateau krem=1", "low byte", "all zero", "patch"):
            assert "ContrastiveLoss " + want in seen, want
        for want in ("live", "patch", "1e-12", "trivial", "no pos"):
            assert "RLL " + want in seen, want
        ks = sorted(f["k"] for n, _, _, f in S.scenarios(shape, remap) if n.startswith("ContrastiveLoss k="))
        total = int(S.masks(S.scenarios(shape, remap)[0][1])[1].sum())
        assert ks == [0, 1, total - 1, total, total + 1]


def test_shapes_reach_the_paths_they_claim():
    assert [h * w for h, w in S.GRIDS] == [1, 255, 256, 257]
    nblk = lambda s: s[0] * s[1] * ((s[2] + S.OBJ_THREADS - 1) // S.OBJ_THREADS)   # noqa: E731
    assert nblk((3, 100, 1)) == 300 > S.OBJ_THREADS, "mining_scan_kernel: two blocks per thread"
    assert all(B > S.OBJ_THREADS for _, B, _ in [(1, 257, 3), (1, 300, 5)]), "rll_normalise_kernel: strided label loops"
    assert nblk((2, 3, 257)) == 12
    hi, lo = S.low_byte_pair()
    assert 0 < S.contrastive_loss_bits(hi) ^ S.contrastive_loss_bits(lo) < 256


def test_fp32_model_error_against_float64():
    """Prints the largest error of the fp32 CPU evaluation against float64 per quantity; asserts only that it is of fp32 size."""
    worst = {}

    def note(k, e, case):
        if e >= worst.get(k, (-1.0, ""))[0]:
            worst[k] = (e, case)
    for _, cases, mode in ASSIGN_TABLES:
        for case in cases():
            lo, hi = S.assigned(case, mode, S.F32), S.assigned(case, mode, S.F64)
            if mode == 0:
                note("loc_targets", S.rel_err(lo["loc"], hi["loc"]), case["name"])
            else:
                note("ious_anchor", float((lo["ia"].double() - hi["ia"]).abs().max()), case["name"])
                note("ious_anchor_corrected", float((lo["ic"].double() - hi["ic"]).abs().max()), case["name"])
    for shape, remap in ALL_SCENARIOS:
        for name, inp, par, _ in S.scenarios(shape, remap):
            lo, hi = S.objective_outputs(inp, par, S.F32), S.objective_outputs(inp, par, S.F64)
            case = "{} {}{}".format(S.shape_id(shape), name, " remap" if remap else "")
            note("scalars", max(S.scalar_err(lo[k], hi[k]) for k in S.SCALARS), case)
            for k in ("cls_loss", "loc_loss", "coef", "dloc", "dcls", "dcls_for_neg"):
                if lo[k] is not None:
                    note(k, S.rel_err(lo[k], hi[k]), case)
    for k, (e, case) in sorted(worst.items()):
        print("\nFP32-CPU {:<24s} {:.3e}  {}".format(k, e, case))
        assert e < 3e-6, k
