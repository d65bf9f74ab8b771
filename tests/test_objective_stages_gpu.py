"""GPU: the entry points of os2d_amd/csrc_train/objective.hip on their own - os2d_train_assign_targets, os2d_train_assign_targets_ops,
os2d_train_objective_forward, os2d_train_objective_backward, os2d_train_objective_workspace_floats - called through
os2d_amd/_train_lib.py on operands built on the host, against the models of tests/objective_stage_model.py at the edge shapes of
its case tables.  The other objective tests reach these kernels through Os2dBoxCoder / Os2dObjective, on random inputs that
never sit on a decision boundary.  Counterpart of tests/test_forward_matrix_gpu.py, with its rules:

  * every written output and the whole workspace start as 0xFF bytes (NaN as float, -1 as int64) with GUARD elements behind each
    buffer that must come back untouched; every element of a written output must come back finite / valid; an output the mode
    does not write (loc_targets in mode 1, the IoUs in mode 0) stays untouched;
  * integer outputs and masks are ``torch.equal`` to the fp32 evaluation of the model: cls_targets, flags, the zero pattern of the
    gradients - and the contrastive cls_loss / coef, which are chains of single IEEE operations;
  * values are compared with the float64 evaluation, never with another kernel run;
  * bit-exact claims (a second call, a batch against its images, nops = 0 against the plain entry point, the gradient sum without
    dcls_preds_for_neg) are ``torch.equal`` on integer views.
"""
import ctypes

import numpy as np
import pytest
import torch

import objective_stage_model as S

pytestmark = pytest.mark.gpu

F32 = torch.float32
GUARD = 64
FLOOR = 3 * 2.0 ** -24
# The ceiling no pin may exceed: the bound DESIGN.md section 11 reasons for an fp32 sum plus expf / logf.
CEILING = 3e-6
# Pins: 3x the largest error measured on the MI355X over the cases of this file, never below 3 * 2^-24 (measured value and its
# case in the comment; the table is in DESIGN.md section 11).  Arrays: max |got - ref| / max |ref|; IoUs: max |got - ref|;
# scalars: |got - ref| / |ref|, the largest of the five.
PIN = {
    "loc_targets": FLOOR,               # measured 3.91e-8 (15x17 6-op chain): the floor
    "ious_anchor": FLOOR,               # measured 2.97e-8 (15x17 stride 8 rec_field 8): the floor; the bits of the fp32 evaluation
    "ious_anchor_corrected": 2.4e-6,    # measured 7.88e-7 (1x257): decoded boxes 62 anchors wide; the fp32 CPU evaluation has 7.88e-7 too
    "scalars": 5.3e-7,                  # measured 1.74e-7 (A2_B3_HW256 RLL trivial remap)
    "cls_loss": 5.2e-7,                 # measured 1.71e-7 (A1_B300_HW5 RLL trivial)
    "loc_loss": 3.3e-7,                 # measured 1.08e-7 (A3_B100_HW1 ContrastiveLoss all zero remap)
    "coef": 5.1e-7,                     # measured 1.68e-7 (A1_B300_HW5 RLL trivial)
    "dloc": 3.7e-7,                     # measured 1.23e-7 (A2_B3_HW256 RLL trivial)
    "dcls": 7.1e-7,                     # measured 2.35e-7 (A1_B300_HW5 RLL trivial)
    "dcls_for_neg": 4.6e-7,             # measured 1.52e-7 (A1_B300_HW5 RLL 1e-12 remap)
}


def _T():
    from os2d_amd import _train_lib
    return _train_lib


def _ptr(t):
    from os2d_amd import _lib
    return _lib.ptr(t)


def _stream(device):
    from os2d_amd import _lib
    return _lib.current_stream(device)


def _error_text():
    return _T().load().os2d_train_last_error() or b""


class Buf(object):
    """n elements of ``dtype`` plus GUARD more, every byte 0xFF."""

    def __init__(self, device, n, dtype=F32):
        self.n, self.item = int(n), torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((self.n + GUARD) * self.item,), 0xFF, dtype=torch.uint8, device=device)
        self.t = self.raw.view(dtype)

    @property
    def ptr(self):
        return _ptr(self.t)

    def untouched(self):
        return bool((self.raw == 0xFF).all())

    def guard_intact(self):
        return bool((self.raw[self.n * self.item:] == 0xFF).all())

    def get(self):
        return self.t[:self.n].cpu()


def written(bufs, valid):
    """Every buffer's guard is intact; ``valid``: name -> what its n elements must be ("finite", or a set of values / a bound)."""
    out = {}
    for k, b in bufs.items():
        assert b.guard_intact(), "written past the end of " + k
        if k not in valid:
            continue
        out[k] = v = b.get()
        if valid[k] == "finite":
            assert bool(torch.isfinite(v).all()), "not every element of {} was written".format(k)
        else:
            assert bool(((v >= valid[k][0]) & (v <= valid[k][1])).all()), "not every element of {} was written".format(k)
    return out


def bits(t):
    return S.bits(t)


def report(stage, case, err):
    print("\nSTAGE {:<22s} {:<60s} {:.3e}".format(stage, case, err))


def check_pins(errors):
    """errors: quantity -> {case: error}.  Every line is printed before anything is asserted."""
    for q, errs in errors.items():
        for case, e in errs.items():
            report(q, case, e)
    for q, errs in errors.items():
        assert FLOOR <= PIN[q] <= CEILING, q
        bad = {k: e for k, e in errs.items() if not e < PIN[q]}
        assert not bad, (q, bad)


def dev(t, device):
    return None if t is None else t.contiguous().to(device)


# ------------------------------------------------------------------------------------------------------ target assignment
def run_assign(case, mode, device, entry):
    """One call of os2d_train_assign_targets (entry "plain") or os2d_train_assign_targets_ops ("ops") with all four outputs
    given: -> the outputs the mode writes, checked for guards, validity and for leaving the others alone."""
    tl = _T().load()
    A, B, H, W = case["A"], case["B"], case["H"], case["W"]
    N = A * B * H * W
    boxes, labels, difficult = [torch.cat([g[i] for g in case["gt"]]) for i in range(3)]
    n = int(boxes.shape[0])
    offsets = torch.tensor(np.cumsum([0] + [g[0].shape[0] for g in case["gt"]]), dtype=torch.int32)
    gt = [dev(boxes, device), dev(labels, device), dev(difficult, device)] if n else [None, None, None]   # n = 0: NULL pointers
    offsets_d, loc_scores = dev(offsets, device), dev(case["loc_scores"], device) if mode == 1 else None
    bufs = dict(cls=Buf(device, N, torch.int64), loc=Buf(device, 4 * N), ia=Buf(device, N), ic=Buf(device, N))
    head = (mode, _ptr(gt[0]), _ptr(gt[1]), _ptr(gt[2]), _ptr(offsets_d), n, _ptr(loc_scores), A, B, H, W, case["stride"], case["rec_field"],
            ctypes.c_float(case["high"]), ctypes.c_float(case["low"]))
    tail = (bufs["loc"].ptr, bufs["cls"].ptr, bufs["ia"].ptr, bufs["ic"].ptr, _stream(device))
    if entry == "plain":
        rc = tl.os2d_train_assign_targets(*(head + tail))
    else:
        ops = case["ops"] or []
        kinds = (ctypes.c_int * max(len(ops), 1))(*[o[0] for o in ops])
        args = (ctypes.c_float * (2 * max(len(ops), 1)))(*[v for o in ops for v in o[1:]])
        rc = tl.os2d_train_assign_targets_ops(*(head + (len(ops), kinds, args) + tail))
    torch.cuda.synchronize()
    _T().check(rc, "os2d_train_assign_targets ({})".format(entry))
    valid = dict(cls=(-1, 1), loc="finite") if mode == 0 else dict(cls=(-1, 1), ia="finite", ic="finite")
    out = written(bufs, valid)
    for k in bufs:
        assert k in valid or bufs[k].untouched(), "mode {} wrote {}".format(mode, k)
    return out


ASSIGN = [(0, "plain", c) for c in S.encode_cases()] + [(0, "ops", c) for c in S.ops_cases()] + \
         [(1, "plain", c) for c in S.remap_cases()] + [(1, "ops", c) for c in S.remap_ops_cases()]


@pytest.mark.parametrize("mode,entry,case", ASSIGN, ids=["mode{}-{}-{}".format(m, e, c["name"].replace(" ", "_")) for m, e, c in ASSIGN])
def test_assign_targets(device, mode, entry, case):
    """Class targets equal the fp32 evaluation (IoUs on a threshold and one step below it, the first maximum, difficult boxes);
    loc_targets and the IoUs against float64; a second call, every image alone and - for an empty chain - the plain entry point
    give the same bits."""
    got = run_assign(case, mode, device, entry)
    want, ref = S.assigned(case, mode, S.F32), S.assigned(case, mode, S.F64)
    A, B, HW = case["A"], case["B"], case["H"] * case["W"]
    mism = got["cls"].view(A, B, HW) != want["cls"]
    print("\n{}: class targets that differ from the fp32 evaluation: {}".format(case["name"], mism.nonzero().tolist()[:8]))
    errors = {}
    if mode == 0:
        errors["loc_targets"] = {case["name"]: S.rel_err(got["loc"], ref["loc"])}
    else:
        errors["ious_anchor"] = {case["name"]: float((got["ia"].double() - ref["ia"].view(-1)).abs().max())}
        errors["ious_anchor_corrected"] = {case["name"]: float((got["ic"].double() - ref["ic"].view(-1)).abs().max())}
    for q, errs in errors.items():
        report(q, *list(errs.items())[0])
    assert not bool(mism.any())
    if mode == 1:     # the plain anchor's IoU has no expf in it: the fp32 evaluation's bits
        assert torch.equal(bits(got["ia"]), bits(want["ia"].view(-1))), "ious_anchor"
    check_pins(errors)
    again = run_assign(case, mode, device, entry)
    assert all(torch.equal(bits(again[k]), bits(got[k])) for k in got), "a second call gives other bits"
    if entry == "ops" and not case["ops"]:
        plain = run_assign(case, mode, device, "plain")
        assert all(torch.equal(bits(plain[k]), bits(got[k])) for k in got), "nops = 0 differs from the plain entry point"
    for a in range(A if A > 1 else 0):
        one = run_assign(S.one_image(case, a), mode, device, entry)
        for k in got:
            assert torch.equal(bits(one[k]), bits(got[k].view(A, -1)[a])), "image {} alone gives other bits of {}".format(a, k)


def test_assign_targets_refuses_a_bad_chain(device):
    tl, case = _T().load(), S.ops_cases()[1]
    N = case["A"] * case["B"] * case["H"] * case["W"]
    boxes, labels, difficult = [dev(torch.cat([g[i] for g in case["gt"]]), device) for i in range(3)]
    offsets = dev(torch.tensor(np.cumsum([0] + [g[0].shape[0] for g in case["gt"]]), dtype=torch.int32), device)
    kinds, args = (ctypes.c_int * 8)(*([1] * 8)), (ctypes.c_float * 16)(*([1.0] * 16))
    for what, nops, k in (("nops = 7", 7, kinds), ("nops = -1", -1, kinds), ("kind 5", 1, (ctypes.c_int * 8)(*([5] * 8)))):
        bufs = dict(cls=Buf(device, N, torch.int64), loc=Buf(device, 4 * N))
        rc = tl.os2d_train_assign_targets_ops(0, _ptr(boxes), _ptr(labels), _ptr(difficult), _ptr(offsets), int(boxes.shape[0]), None,
                                              case["A"], case["B"], case["H"], case["W"], 16, 16, ctypes.c_float(0.5), ctypes.c_float(0.25), nops,
                                              k, args, bufs["loc"].ptr, bufs["cls"].ptr, None, None, _stream(device))
        torch.cuda.synchronize()
        assert rc != 0, what + ": accepted"
        assert b"chain" in _error_text(), what
        assert all(b.untouched() for b in bufs.values()), what + ": an output was touched"


# ------------------------------------------------------------------------------------------------------ objective
def run_forward(inp, par, device, loc_loss=True, ws_short=0, check=True):
    """One os2d_train_objective_forward into 0xFF buffers: -> dict(rc, bufs, inputs on the device, outputs on the host)."""
    tl = _T().load()
    A, B, HW = inp["cls_preds"].shape
    N = A * B * HW
    need = int(tl.os2d_train_objective_workspace_floats(A, B, HW))
    assert need > 0
    d = {k: dev(v, device) for k, v in inp.items()}
    bufs = dict(losses=Buf(device, 5), cls_loss=Buf(device, N), loc_loss=Buf(device, N), flags=Buf(device, N, torch.uint8), coef=Buf(device, N),
                ws=Buf(device, need - ws_short))
    rc = tl.os2d_train_objective_forward(
        0 if par["loss"] == "ContrastiveLoss" else 1, 1 if par["patch"] else 0, _ptr(d["loc_preds"]), _ptr(d["loc_targets"]), _ptr(d["cls_preds"]),
        _ptr(d["cls_targets"]), _ptr(d["cls_targets_remapped"]), _ptr(d["cls_preds_for_neg"]), A, B, HW, ctypes.c_float(par["margin"]),
        ctypes.c_float(par["margin_pos"]), ctypes.c_float(par["class_loss_neg_weight"]), ctypes.c_float(par["localization_weight"]),
        ctypes.c_float(par["ratio"]), ctypes.c_double(par["rll_ratio"]), bufs["losses"].ptr, bufs["cls_loss"].ptr,
        bufs["loc_loss"].ptr if loc_loss else None, bufs["flags"].ptr, bufs["coef"].ptr, bufs["ws"].ptr, bufs["ws"].n, _stream(device))
    torch.cuda.synchronize()
    fw = dict(rc=rc, bufs=bufs, dev=d, shape=(A, B, HW))
    if check:
        _T().check(rc, "os2d_train_objective_forward")
        valid = dict(losses="finite", cls_loss="finite", flags=(0, 31), coef="finite")
        if loc_loss:
            valid["loc_loss"] = "finite"
        fw["out"] = written(bufs, valid)
        assert loc_loss or bufs["loc_loss"].untouched(), "loc_loss = NULL, yet its buffer was written"
    return fw


WANT_ALL = (True, True, True)
GRADS = ("dloc", "dcls", "dcls_for_neg")


def run_backward(fw, par, grad_loss, device, want=WANT_ALL, check=True):
    """os2d_train_objective_backward on what ``run_forward`` left; ``want``: which of dloc / dcls / dcls_for_neg are not NULL."""
    tl = _T().load()
    A, B, HW = fw["shape"]
    N = A * B * HW
    g = torch.tensor([grad_loss], dtype=F32, device=device)
    bufs = {k: Buf(device, 4 * N if k == "dloc" else N) for k, w in zip(GRADS, want) if w}
    p = lambda k: bufs[k].ptr if k in bufs else None   # noqa: E731
    rc = tl.os2d_train_objective_backward(_ptr(g), _ptr(fw["dev"]["loc_preds"]), _ptr(fw["dev"]["loc_targets"]), fw["bufs"]["flags"].ptr,
                                          fw["bufs"]["coef"].ptr, fw["bufs"]["ws"].ptr, A, B, HW, ctypes.c_float(par["class_loss_neg_weight"]),
                                          ctypes.c_float(par["localization_weight"]), p("dloc"), p("dcls"), p("dcls_for_neg"), _stream(device))
    torch.cuda.synchronize()
    if not check:
        return rc, bufs
    _T().check(rc, "os2d_train_objective_backward")
    return written(bufs, {k: "finite" for k in bufs})


def check_scenario(device, shape, remap, name, inp, par, grad_loss, errors):
    A, B, HW = shape
    case = "{} {}{}".format(S.shape_id(shape), name, " remap" if remap else "")
    want, ref = S.objective_outputs(inp, par, S.F32, grad_loss), S.objective_outputs(inp, par, S.F64, grad_loss)
    fw = run_forward(inp, par, device)
    out = fw["out"]
    flag_mism = (out["flags"].view(shape) != want["flags"]).nonzero().tolist()
    if flag_mism:
        print("\n{}: flags differ from the fp32 evaluation at {} (got {}, want {})".format(
            case, flag_mism[:6], [int(out["flags"].view(shape)[tuple(i)]) for i in flag_mism[:6]], [int(want["flags"][tuple(i)]) for i in flag_mism[:6]]))
    errs = dict(scalars=max(S.scalar_err(float(out["losses"][i]), ref[k]) for i, k in enumerate(S.SCALARS)),
                cls_loss=S.rel_err(out["cls_loss"], ref["cls_loss"]), loc_loss=S.rel_err(out["loc_loss"], ref["loc_loss"]),
                coef=S.rel_err(out["coef"], ref["coef"]))
    # backward: with cls_preds_for_neg the two class terms go to their own outputs, without it both land in dcls
    grads = run_backward(fw, par, grad_loss, device, want=(True, True, remap))
    for k in grads:
        errs[k] = S.rel_err(grads[k], ref[k])
    for q, e in errs.items():
        errors.setdefault(q, {})[case] = e
        report(q, case, e)
    assert not flag_mism, case
    if par["loss"] == "ContrastiveLoss":       # single IEEE operations: the bits of the fp32 evaluation (the sign of a zero aside)
        assert torch.equal(bits(out["cls_loss"]), bits(want["cls_loss"]).view(-1)), case + ": cls_loss bits"
        assert torch.equal(out["coef"], want["coef"].view(-1)), case + ": coef"
    for k in grads:
        assert torch.equal(grads[k] != 0, want[k].reshape(-1) != 0), "{}: zero pattern of {}".format(case, k)
    # d loc is exactly +-scale where |diff| >= 1 (the clamp), scale = grad_loss * localization_weight / num_pos_for_regression
    pos_reg = (inp["cls_targets"] > 0)[:, :, None, :].expand(A, B, 4, HW)
    diff = inp["loc_preds"] - inp["loc_targets"]
    scale = np.float32(grad_loss) * np.float32(par["localization_weight"]) / np.float32(max(int((inp["cls_targets"] > 0).sum()), 1))
    for sign, sel in ((1.0, pos_reg & (diff >= 1)), (-1.0, pos_reg & (diff <= -1))):
        exact = torch.full((int(sel.sum()),), float(np.float32(sign) * scale), dtype=F32)
        assert torch.equal(bits(grads["dloc"].view(A, B, 4, HW)[sel]), bits(exact)), case + ": d loc at the clamp"
    # a second call into fresh buffers, this one without loc_loss: the same bits
    again = run_forward(inp, par, device, loc_loss=False)["out"]
    assert all(torch.equal(bits(again[k]), bits(out[k])) for k in again), case + ": a second call gives other bits"


SCENARIOS = [(shape, remap) for shape in S.OBJ_SHAPES for remap in (False, True)]


@pytest.mark.parametrize("shape,remap", SCENARIOS, ids=[S.shape_id(s) + ("_remap" if r else "") for s, r in SCENARIOS])
def test_objective_forward_backward(device, shape, remap):
    """Every scenario of the shape (objective_stage_model.scenarios): mining counts, plateaus, the low-byte pair, all-zero losses,
    the RLL cuts, patch mode, the kinks of both hinges and of smooth-L1, with grad_loss 1, 0.37 and -2 in turn."""
    errors = {}
    for i, (name, inp, par, _) in enumerate(S.scenarios(shape, remap)):
        check_scenario(device, shape, remap, name, inp, par, (1.0, 0.37, -2.0)[i % 3], errors)
    check_pins(errors)


KINK_SHAPE = (2, 3, 256)


@pytest.mark.parametrize("remap", [False, True], ids=["plain", "remap"])
@pytest.mark.parametrize("which", ["RLL live", "RLL patch"])
def test_hinge_kinks_follow_autograd(device, which, remap):
    """torch's clamp(min=0) passes the gradient where its argument is exactly 0.  Element 0 is an RLL positive with cls_preds ==
    margin_pos: its gradient is -0.5 * num_pos / num_nontrivial_pos / num_pos (patch mode: -0.5 / num_pos), not 0, although it does
    not count as non-trivial.  Element 1 is a candidate with its score == margin: +0.5 * neg_weight / num_pos in patch mode."""
    name, inp, par, _ = [s for s in S.scenarios(KINK_SHAPE, remap) if s[0] == which][0]
    ref = S.objective_outputs(inp, par, S.F64, 1.0)
    fw = run_forward(inp, par, device)
    grads = run_backward(fw, par, 1.0, device, want=(False, True, True))
    assert float(inp["cls_preds"].view(-1)[0]) == S.MARGIN_POS and float(S._neg_scores(inp).view(-1)[1]) == S.MARGIN
    got_pos, want_pos = float(grads["dcls"][0]), float(ref["dcls"].view(-1)[0])
    got_neg = float(grads["dcls_for_neg"][1])
    want_neg = float((ref["dcls_for_neg"] if remap else ref["dcls"]).view(-1)[1])
    print("\nKINK {} {}: positive at margin_pos {:.9g} (model {:.9g}), candidate at margin {:.9g} (model {:.9g})".format(
        which, "remap" if remap else "plain", got_pos, want_pos, got_neg, want_neg))
    flags = fw["out"]["flags"]
    assert int(flags[0]) & S.F_HINGE and int(flags[1]) & S.F_HINGE
    assert want_pos < 0 and abs(got_pos - want_pos) <= PIN["dcls"] * abs(want_pos)
    assert (want_neg > 0) == par["patch"] and abs(got_neg - want_neg) <= PIN["dcls_for_neg"] * abs(want_neg)


NULL_CASES = [("ContrastiveLoss plateau krem=1", False), ("ContrastiveLoss plateau krem=1", True), ("RLL live", True), ("RLL patch", False)]


@pytest.mark.parametrize("grad_loss", [1.0, 0.37, -2.0])
@pytest.mark.parametrize("which,remap", NULL_CASES)
def test_backward_null_combinations(device, which, remap, grad_loss):
    """Each of the seven non-empty NULL combinations of dloc / dcls / dcls_for_neg writes what the full call writes, bit for bit;
    without dcls_for_neg both class terms land in dcls and equal the sum of the split call bit for bit."""
    shape = (2, 3, 257)
    name, inp, par, _ = [s for s in S.scenarios(shape, remap) if s[0] == which][0]
    fw = run_forward(inp, par, device)
    full = run_backward(fw, par, grad_loss, device)
    assert not bool(((full["dcls"] != 0) & (full["dcls_for_neg"] != 0)).any()), "an element is never both"
    total = full["dcls"] + full["dcls_for_neg"]
    ref = S.objective_outputs(inp, par, S.F64, grad_loss)
    errors = {"dcls": {name: S.rel_err(total, ref["dcls"] + (ref["dcls_for_neg"] if remap else 0))}, "dloc": {name: S.rel_err(full["dloc"], ref["dloc"])}}
    check_pins(errors)
    for n in range(1, 8):
        want = tuple(bool(n >> i & 1) for i in range(3))
        if want == WANT_ALL:
            continue
        got = run_backward(fw, par, grad_loss, device, want=want)
        assert sorted(got) == sorted(k for k, w in zip(GRADS, want) if w)
        for k in got:
            expect = total if (k == "dcls" and not want[2]) else full[k]
            assert torch.equal(bits(got[k]), bits(expect)), (want, k)


def test_objective_refusals(device):
    """A workspace one float short: -2; every gradient NULL: refused; each with the error text set and every buffer untouched."""
    name, inp, par, _ = S.scenarios((2, 3, 257), True)[1]
    short = run_forward(inp, par, device, ws_short=1, check=False)
    assert short["rc"] == -2 and b"workspace" in _error_text()
    assert all(b.untouched() for b in short["bufs"].values()), "a refused forward touched a buffer"
    fw = run_forward(inp, par, device)
    rc, _ = run_backward(fw, par, 1.0, device, want=(False, False, False), check=False)
    assert rc != 0 and b"gradient" in _error_text()
    tl = _T().load()
    assert int(tl.os2d_train_objective_workspace_floats(0, 3, 257)) == 0 and int(tl.os2d_train_objective_workspace_floats(2, 3, 257)) == fw["bufs"]["ws"].n
