"""GPU: the entry points of libos2d_eval.so (include/os2d_eval.h) on their own - os2d_eval_count_gt, os2d_eval_match, os2d_eval_sort,
os2d_eval_prec_rec, os2d_eval_ap, os2d_eval_finalise - called through os2d_amd/_eval_lib.py on operands built on the host,
against the plain functions of tests/voc_eval_stage_model.py at the cases of tests/voc_eval_stage_cases.py: ties, an IoU exactly
on the threshold, segment boundaries on every thread / wave / tile / round edge, labels outside [0, L).  The other evaluation
tests reach these kernels through VocEvaluator, on inputs without ties.  The rules of tests/test_objective_stages_gpu.py:

  * every output and workspace starts as 0xFF bytes with GUARD elements behind it that must come back untouched (match and
    gt_index start as 0x7F bytes: 0xFF is -1 there, a value they may hold); every element the header says is written must come
    back valid; what the header says is left alone still holds the sentinel;
  * every call is made twice on fresh buffers and must give equal bits;
  * comparisons go against the stage model, never against another kernel run.

Tolerances: integer outputs and every float that is one IEEE fp64 division or a selection - prec, rec,
rec_last, mpre, the 11-point acc, ap_per_class - have the model's bits (NaN where the model has NaN).  The area under the curve
is a sum of the model's terms in another order: within n * 2^-52 * sum of math.fsum for n nonzero terms; the four scalars
within (L + 2) * 2^-52 * |model|."""
import ctypes
import math

import numpy as np
import pytest
import torch

import voc_eval_stage_cases as C
import voc_eval_stage_model as S

pytestmark = pytest.mark.gpu

GUARD = 64
EPS = 2.0 ** -52
TORCH = {np.dtype(np.int8): torch.int8, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32,
         np.dtype(np.int64): torch.int64, np.dtype(np.uint64): torch.int64, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def _E():
    from os2d_amd import _eval_lib
    return _eval_lib


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def dev(a, device):
    """A host array on the device (unsigned as the signed type of its width); None and empty arrays become NULL pointers."""
    if a is None or a.size == 0:
        return None
    a = np.array(a, order="C")         # a writable copy: the shared references are read-only
    return torch.from_numpy(a.view(np.dtype("i{}".format(a.dtype.itemsize))) if a.dtype.kind == "u" and a.dtype.itemsize > 1 else a).to(device)


class Buf(object):
    """n elements of a numpy ``dtype`` plus GUARD more, every byte ``fill``."""

    def __init__(self, device, n, dtype, fill=0xFF):
        self.n, self.dtype, self.fill = int(n), np.dtype(dtype), fill
        self.item = self.dtype.itemsize
        self.raw = torch.full(((self.n + GUARD) * self.item,), fill, dtype=torch.uint8, device=device)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr())

    def zero(self):
        self.raw[:self.n * self.item] = 0
        return self

    def guard_intact(self):
        return bool((self.raw[self.n * self.item:] == self.fill).all())

    def untouched(self):
        return bool((self.raw == self.fill).all())

    def get(self):
        return self.raw[:self.n * self.item].cpu().numpy().view(self.dtype).copy()

    def left(self):
        """Which elements still hold the sentinel."""
        return (self.raw[:self.n * self.item].cpu().numpy().reshape(self.n, self.item) == self.fill).all(1)


def finish(what, rc, bufs, written):
    """Synchronise, check the return code and the guards -> name: array; the buffers named in ``written`` hold no sentinel."""
    torch.cuda.synchronize()
    _E().check(rc, what)
    out = {}
    for k, b in bufs.items():
        assert b.guard_intact(), "{} wrote past the end of {}".format(what, k)
        if k in written:
            assert not b.left().any(), "{} did not write every element of {}".format(what, k)
        out[k] = b.get()
    return out


def twice(run):
    """Two calls on fresh buffers give equal bits; -> the first."""
    a, b = run(), run()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "two calls differ in " + k
    return a


# ----------------------------------------------------------------------------------------------------------------- count_gt
def run_count(c, device):
    G, L = len(c["gt_labels"]), c["L"]
    labels, difficult = dev(c["gt_labels"], device), dev(c["gt_difficult"], device)       # G = 0: NULL
    bufs = dict(n_pos=Buf(device, L + 1, np.int32), gt_count=Buf(device, L, np.int32))
    rc = _E().load().os2d_eval_count_gt(ptr(labels), ptr(difficult), G, L, bufs["n_pos"].ptr, bufs["gt_count"].ptr, _stream(device))
    return finish("os2d_eval_count_gt", rc, bufs, ("n_pos", "gt_count"))


@pytest.mark.parametrize("c", C.count_cases(), ids=lambda c: c["name"])
def test_count_gt(c, device):
    got = twice(lambda: run_count(c, device))
    n_pos, gt_count = S.count_gt(c["gt_labels"], c["gt_difficult"], c["L"])
    assert np.array_equal(got["n_pos"], n_pos) and np.array_equal(got["gt_count"], gt_count)


# -------------------------------------------------------------------------------------------------------------------- match
def run_match(c, device):
    D, G, N = len(c["det_scores"]), len(c["gt_labels"]), len(c["det_offsets"]) - 1
    ins = [dev(c[k], device) for k in ("det_boxes", "det_scores", "det_labels", "det_offsets", "gt_boxes", "gt_labels", "gt_difficult", "gt_offsets")]
    bufs = dict(gt_index=Buf(device, D, np.int32, 0x7F), match=Buf(device, D, np.int8, 0x7F))
    winner = Buf(device, G, np.uint64)
    rc = _E().load().os2d_eval_match(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), D, N, ptr(ins[4]), ptr(ins[5]), ptr(ins[6]), ptr(ins[7]), G,
                                     ctypes.c_float(c["thr"]), bufs["gt_index"].ptr, winner.ptr if G else None, bufs["match"].ptr, _stream(device))
    out = finish("os2d_eval_match", rc, bufs, ("gt_index", "match"))
    assert winner.guard_intact()
    return out


MATCH = C.match_cases()


@pytest.mark.parametrize("c", MATCH, ids=lambda c: c["name"])
def test_match(c, device):
    got = twice(lambda: run_match(c, device))
    m, index = S.match(c["det_boxes"], c["det_scores"], c["det_labels"], c["det_offsets"], c["gt_boxes"], c["gt_labels"], c["gt_difficult"],
                       c["gt_offsets"], c["thr"])
    assert np.array_equal(got["match"], m), (got["match"].tolist()[:16], m.tolist()[:16])
    assert np.array_equal(got["gt_index"], index), (got["gt_index"].tolist()[:16], index.tolist()[:16])
    if c["expect_match"] is not None:
        assert got["match"].tolist() == list(c["expect_match"]) and got["gt_index"].tolist() == list(c["expect_index"])


# --------------------------------------------------------------------------------------------------------------------- sort
def run_sort(c, device, label_bits=None):
    lib = _E().load()
    D, L = len(c["scores"]), c["L"]
    scores, labels = dev(c["scores"], device), dev(c["labels"], device)
    need = lib.os2d_eval_sort_workspace_bytes(D)
    bufs = dict(perm_joint=Buf(device, D, np.uint32), perm_class=Buf(device, D, np.uint32), sorted_labels=Buf(device, D, np.int32),
                class_offsets=Buf(device, L + 1, np.int32), workspace=Buf(device, need, np.uint8))          # exactly the bytes asked for
    rc = lib.os2d_eval_sort(ptr(scores), ptr(labels), D, L, c["label_bits"] if label_bits is None else label_bits, bufs["perm_joint"].ptr,
                            bufs["perm_class"].ptr, bufs["sorted_labels"].ptr, bufs["class_offsets"].ptr, bufs["workspace"].ptr, need, _stream(device))
    out = finish("os2d_eval_sort", rc, bufs, ("perm_joint", "perm_class", "sorted_labels", "class_offsets") if D else ("class_offsets",))
    out.pop("workspace")
    return out


def check_sort(got, c):
    joint, by_class, keys, offsets = S.sort(c["scores"], c["labels"], c["L"])
    for k, want in (("perm_joint", joint), ("perm_class", by_class), ("sorted_labels", keys), ("class_offsets", offsets)):
        bad = np.flatnonzero(got[k] != want)
        assert bad.size == 0, "{}: {} differ, first at {}: {} for {}".format(k, bad.size, bad[0], got[k][bad[0]], want[bad[0]])


SORT = C.sort_cases() + C.pass_count_cases()


@pytest.mark.parametrize("c", SORT, ids=lambda c: c["name"])
def test_sort(c, device):
    check_sort(twice(lambda: run_sort(c, device)), c)


def test_sort_of_nothing_zeroes_the_offsets_only(device):
    lib = _E().load()
    assert lib.os2d_eval_sort_workspace_bytes(0) == 0
    bufs = dict(perm_joint=Buf(device, 4, np.uint32), perm_class=Buf(device, 4, np.uint32), sorted_labels=Buf(device, 4, np.int32),
                class_offsets=Buf(device, 6, np.int32), workspace=Buf(device, 256, np.uint8))
    rc = lib.os2d_eval_sort(None, None, 0, 5, 3, bufs["perm_joint"].ptr, bufs["perm_class"].ptr, bufs["sorted_labels"].ptr, bufs["class_offsets"].ptr,
                            bufs["workspace"].ptr, 256, _stream(device))
    out = finish("os2d_eval_sort", rc, bufs, ("class_offsets",))
    assert out["class_offsets"].tolist() == [0] * 6
    assert all(bufs[k].untouched() for k in ("perm_joint", "perm_class", "sorted_labels", "workspace"))


def test_sort_with_nan_scores_permutes_and_keeps_the_others_in_order(device):
    c = C.nan_case()
    got = twice(lambda: run_sort(c, device))
    D = len(c["scores"])
    real = np.flatnonzero(~np.isnan(c["scores"]))
    assert 0 < real.size < D
    joint, by_class, _, _ = S.sort(c["scores"][real], c["labels"][real], c["L"])
    for k, want in (("perm_joint", joint), ("perm_class", by_class)):
        assert np.array_equal(np.sort(got[k]), np.arange(D)), k
        kept = got[k][~np.isnan(c["scores"][got[k].astype(np.int64)])]
        assert np.array_equal(kept, real[want.astype(np.int64)]), k


def test_sort_over_more_tiles_than_are_resident(device):
    """Three label passes at C.MANY_TILES_D rows: equal scores, label MANY_LABELS[i % 6]; the orders are closed forms."""
    lib = _E().load()
    D, L = C.MANY_TILES_D, C.MANY_L
    rows = torch.arange(D, dtype=torch.int32, device=device)
    labels = torch.tensor(C.MANY_LABELS, dtype=torch.int32, device=device)[(rows % 6).long()]
    scores = torch.full((D,), 0.25, device=device)
    need = lib.os2d_eval_sort_workspace_bytes(D)
    out = [torch.full((D + GUARD,), -1, dtype=torch.int32, device=device) for _ in range(3)]
    offsets = torch.full((L + 1 + GUARD,), -1, dtype=torch.int32, device=device)
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=device)
    rc = lib.os2d_eval_sort(ptr(scores), ptr(labels), D, L, 17, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(offsets), ptr(ws), need, _stream(device))
    torch.cuda.synchronize()
    _E().check(rc, "os2d_eval_sort")
    assert all(bool((t[D:] == -1).all()) for t in out) and bool((offsets[L + 1:] == -1).all()) and bool((ws[need:] == 0xFF).all())
    assert torch.equal(out[0][:D], rows)
    order = C.many_tiles_order(D)
    assert torch.equal(out[1][:D], torch.cat([torch.arange(r, D, 6, dtype=torch.int32, device=device) for r, _ in order]))
    counts = [len(range(r, D, 6)) for r, _ in order]
    assert torch.equal(out[2][:D], torch.repeat_interleave(torch.tensor([l for _, l in order], dtype=torch.int32, device=device),
                                                           torch.tensor(counts, device=device)))
    want = np.searchsorted(np.repeat([l for _, l in order], counts), np.arange(L + 1)).astype(np.int32)
    assert np.array_equal(offsets[:L + 1].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------ prec_rec and ap
def run_prec_rec(c, device, with_tpfp=True):
    lib = _E().load()
    D, L = c["D"], c["L"]
    ins = [dev(c[k], device) for k in ("match", "perm", "seg", "n_pos")]
    need = lib.os2d_eval_scan_workspace_bytes(D)
    bufs = dict(prec=Buf(device, D, np.float64), rec=Buf(device, D, np.float64), rec_last=Buf(device, L, np.float64), workspace=Buf(device, need, np.uint8))
    if with_tpfp:
        bufs["tpfp"] = Buf(device, D, np.uint64)
    rc = lib.os2d_eval_prec_rec(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), L, D, bufs["tpfp"].ptr if with_tpfp else None, bufs["prec"].ptr,
                                bufs["rec"].ptr, bufs["rec_last"].ptr, bufs["workspace"].ptr, need, _stream(device))
    out = finish("os2d_eval_prec_rec", rc, bufs, ("prec", "rec", "tpfp"))
    out["rec_last_left"] = bufs["rec_last"].left()
    out.pop("workspace")
    return out


def first_difference(got, want):
    bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))))
    return "none" if not bad.size else "{} differ, first at {}: {!r} for {!r}".format(bad.size, bad[0], got[bad[0]], want[bad[0]])


SCANS = C.scan_table()


@pytest.mark.parametrize("c", SCANS, ids=lambda c: c["name"])
def test_prec_rec(c, device):
    got = twice(lambda: run_prec_rec(c, device))
    ref = C.scan_reference(c)
    assert np.array_equal(got["tpfp"] >> np.uint64(32), ref["tp"].astype(np.uint64)), first_difference(got["tpfp"] >> np.uint64(32), ref["tp"])
    assert np.array_equal(got["tpfp"] & np.uint64(0xFFFFFFFF), ref["fp"].astype(np.uint64))
    assert S.same_bits(got["prec"], ref["prec"]), first_difference(got["prec"], ref["prec"])
    assert S.same_bits(got["rec"], ref["rec"]), first_difference(got["rec"], ref["rec"])
    last = np.array([s in ref["last"] for s in range(c["L"])])
    assert np.array_equal(got["rec_last_left"], ~last)                      # left where the header says so
    assert np.array_equal(S.bits(got["rec_last"][last]), S.bits(np.array([ref["last"][s] for s in range(c["L"]) if s in ref["last"]])))
    bare = run_prec_rec(c, device, with_tpfp=False)                          # tpfp = NULL
    for k in ("prec", "rec", "rec_last"):
        assert np.array_equal(bare[k].view(np.uint8), got[k].view(np.uint8)), k


def run_ap(c, device, use_07):
    lib = _E().load()
    D, L = c["D"], c["L"]
    ref = C.scan_reference(c)
    prec, rec, seg = dev(ref["prec"], device), dev(ref["rec"], device), dev(c["seg"], device)      # the model's curves
    need = lib.os2d_eval_scan_workspace_bytes(D)
    bufs = dict(mpre=Buf(device, D, np.float64), acc=Buf(device, L * 11, np.float64).zero(), workspace=Buf(device, need, np.uint8))
    rc = lib.os2d_eval_ap(ptr(prec), ptr(rec), ptr(seg), L, D, int(use_07), bufs["mpre"].ptr, bufs["acc"].ptr, bufs["workspace"].ptr, need, _stream(device))
    out = finish("os2d_eval_ap", rc, bufs, ("mpre", "acc"))
    out.pop("workspace")
    return out


def check_area(got, terms, where):
    """got: the kernel's sum of the model's ``terms`` in its own order."""
    if not np.isfinite(terms).all():                    # a segment without n_pos: rec = tp / 0
        assert np.isnan(got) if np.isnan(terms).any() else got == float("inf"), where
        return
    nonzero = [t for t in terms if t != 0.0]
    total = math.fsum(nonzero)
    assert all(t > 0 for t in nonzero), where
    if not nonzero:
        assert got == 0.0 and not np.signbit(got), where
    assert abs(got - total) <= len(nonzero) * EPS * total, (where, got, total, len(nonzero))


@pytest.mark.parametrize("use_07", (False, True), ids=("area", "11_point"))
@pytest.mark.parametrize("c", SCANS, ids=lambda c: c["name"])
def test_ap(c, use_07, device):
    got = twice(lambda: run_ap(c, device, use_07))
    mpre, per_segment = C.scan_reference(c)["ap07" if use_07 else "ap"]
    assert S.same_bits(got["mpre"], mpre), first_difference(got["mpre"], mpre)
    acc = got["acc"].reshape(c["L"], 11)
    want = np.zeros((c["L"], 11))
    if use_07:
        for s, row in per_segment.items():
            want[s] = row
        assert S.same_bits(acc, want), first_difference(acc.reshape(-1), want.reshape(-1))
        return
    assert (acc[:, 1:].view(np.int64) == 0).all()                            # only t = 0 is written
    for s in range(c["L"]):
        if s in per_segment:
            check_area(acc[s, 0], per_segment[s], (c["name"], s))
        else:
            assert acc[s, 0].view(np.int64) == 0, s                          # no positions: the caller's zero


# ----------------------------------------------------------------------------------------------------------------- finalise
def run_finalise(c, device, use_07):
    L = c["L"]
    acc, rec_last, n_pos = dev(c["acc"], device), dev(c["rec_last"], device), dev(c["n_pos"], device)
    bufs = dict(ap=Buf(device, L, np.float64), recall=Buf(device, L, np.float64), n_pos=Buf(device, L, np.float64), scalars=Buf(device, 4, np.float64))
    rc = _E().load().os2d_eval_finalise(ptr(acc), ptr(rec_last), ptr(n_pos), L, int(use_07), bufs["ap"].ptr, bufs["recall"].ptr, bufs["n_pos"].ptr,
                                        bufs["scalars"].ptr, _stream(device))
    return finish("os2d_eval_finalise", rc, bufs, ("ap", "recall", "n_pos", "scalars"))


@pytest.mark.parametrize("use_07", (False, True), ids=("area", "11_point"))
@pytest.mark.parametrize("c", C.finalise_cases(), ids=lambda c: c["name"])
def test_finalise(c, use_07, device):
    got = twice(lambda: run_finalise(c, device, use_07))
    ap, recall, n_pos, scalars = S.finalise(c["acc"], c["rec_last"], c["n_pos"], c["L"], use_07)
    assert S.same_bits(got["ap"], ap), first_difference(got["ap"], ap)
    assert S.same_bits(got["recall"], recall) and S.same_bits(got["n_pos"], n_pos)
    for k, (g, w) in enumerate(zip(got["scalars"], scalars)):
        assert np.isnan(g) == np.isnan(w), k
        assert np.isnan(w) or abs(g - w) <= (c["L"] + 2) * EPS * abs(w), (k, g, w)
    if c["name"].endswith("no_positives"):
        # nanmean, recall and the joint AP are NaN; map_weighted is the reference's nansum over nothing, 0.0
        assert np.isnan(got["ap"]).all() and np.isnan(got["scalars"][[0, 2, 3]]).all() and got["scalars"][1] == 0.0


# --------------------------------------------------------------------------------------------------- labels outside [0, L)
def run_chain(c, device):
    """os2d_eval_sort -> prec_rec -> ap (area) on the match and n_pos of the case."""
    s = run_sort(c, device)
    scan = dict(name=c["name"], D=len(c["scores"]), L=c["L"], match=c["match"], perm=s["perm_class"], seg=s["sorted_labels"], n_pos=c["n_pos"][:c["L"]])
    pr = run_prec_rec(scan, device)
    lib = _E().load()
    D, L = scan["D"], scan["L"]
    prec, rec, seg = dev(pr["prec"], device), dev(pr["rec"], device), dev(s["sorted_labels"], device)
    need = lib.os2d_eval_scan_workspace_bytes(D)
    bufs = dict(mpre=Buf(device, D, np.float64), acc=Buf(device, L * 11, np.float64).zero(), workspace=Buf(device, need, np.uint8))
    rc = lib.os2d_eval_ap(ptr(prec), ptr(rec), ptr(seg), L, D, 0, bufs["mpre"].ptr, bufs["acc"].ptr, bufs["workspace"].ptr, need, _stream(device))
    a = finish("os2d_eval_ap", rc, bufs, ("mpre", "acc"))
    return dict(s, tpfp=pr["tpfp"], prec=pr["prec"], rec=pr["rec"], rec_last=pr["rec_last"], rec_last_left=pr["rec_last_left"], mpre=a["mpre"], acc=a["acc"])


def test_labels_outside_follow_the_classes_and_change_none_of_them(device):
    """L = 5 with detections of the labels 256, 261, 65536 + 2 and -1 (low bytes 0, 5, 2, 255) between those of the classes
    0 and 2: the per-class outputs are those of the same calls without them (CPU twin with the values written out:
    tests/test_voc_eval_stage_model.py::test_sort_with_labels_outside_by_hand)."""
    c = C.out_of_range_case()
    L = c["L"]
    inside = np.flatnonzero((c["labels"] >= 0) & (c["labels"] < L))
    n = inside.size
    trimmed = dict(c, scores=c["scores"][inside], labels=c["labels"][inside], match=c["match"][inside])
    full, cut = run_chain(c, device), run_chain(trimmed, device)
    check_sort(full, c)                                          # the joint ordering holds every detection, the rows outside are last
    check_sort(cut, trimmed)
    assert np.array_equal(full["class_offsets"], cut["class_offsets"]) and full["class_offsets"][L] == n
    assert np.array_equal(full["perm_class"][:n], inside[cut["perm_class"].astype(np.int64)].astype(np.uint32))
    assert np.array_equal(full["sorted_labels"][:n], cut["sorted_labels"]) and (full["sorted_labels"][n:] == L).all()
    joint, by_class, keys, offsets = S.sort(c["scores"], c["labels"], L)
    tp, fp, prec, rec, last = S.prec_rec(c["match"], by_class, keys, c["n_pos"][:L], L)
    mpre, terms = S.ap(prec, rec, keys, L, False)
    for got, m in ((full, n), (cut, n)):
        assert np.array_equal(got["tpfp"][:m] >> np.uint64(32), tp[:m].astype(np.uint64)) and np.array_equal(got["tpfp"][:m] & np.uint64(0xFFFFFFFF), fp[:m].astype(np.uint64))
        assert S.same_bits(got["prec"][:m], prec[:m]) and S.same_bits(got["rec"][:m], rec[:m]) and S.same_bits(got["mpre"][:m], mpre[:m])
        assert np.array_equal(got["rec_last_left"], np.array([s not in last for s in range(L)]))
        assert all(got["rec_last"][s] == last[s] for s in last)
        acc = got["acc"].reshape(L, 11)
        for s in range(L):
            check_area(acc[s, 0], terms[s], s)
    for k in ("prec", "rec", "mpre", "tpfp"):
        assert np.array_equal(full[k][:n].view(np.uint8), cut[k].view(np.uint8)), k
    assert np.array_equal(full["acc"].view(np.uint8), cut["acc"].view(np.uint8)) and np.array_equal(full["rec_last"].view(np.uint8), cut["rec_last"].view(np.uint8))
