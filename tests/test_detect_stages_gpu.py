"""GPU: the detection entry points of libos2d_hip.so (os2d_nms, os2d_detect_level*, os2d_detect_pyramid* of include/os2d_hip.h)
on their own, called through os2d_amd/_lib.py with inputs built on the host, against the plain model of the stage
(tests/detect_stage_model.py) at the regime edges of the kernels (tests/detect_stage_cases.py; that every case reaches its
regime is asserted on the CPU by tests/test_detect_stage_model.py).  The rules of tests/test_forward_stages_gpu.py:

  * every output, workspace and guard is pre-filled with 0xFF bytes (NaN as a float, -1 as an int); a workspace has exactly the
    size its *_workspace_bytes entry point reports; guards and everything past a count must come back untouched;
  * counts, indices, keep masks and ``unfinished`` are exact, scores and the anchors / corners (float32 chains) bit-equal,
    boxes are compared with the float64 decode; nothing is compared with another kernel;
  * a second call gives the same bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import detect_stage_cases as C
import detect_stage_model as DM

pytestmark = pytest.mark.gpu

GUARD = 256
# Box error in px over the largest scale factor of the case's chain.  CEILING: the project's 1e-3 px on decoded boxes.  PIN: 3x the
# largest error measured on the MI355X over the cases of this file, against the model
CEILING = {"boxes": 1e-3}
PIN = {
    "boxes": 1.2e-4,      # measured 3.87e-5 px (level hw1025: 25x41 locations, random boxes, the 3-op chain whose scale is 1.5);
}                         # grid and twin cases 2.1e-7 px (their corners are integers up to a rounding of exp)


def _L():
    from os2d_amd import _lib
    return _lib


def _call(name, *args):
    L = _L()
    L.check(getattr(L.load(), name)(*args), name)


def _refused(name, *args):
    """The call returns non-zero and leaves an error text."""
    lib = _L().load()
    rc = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert rc != 0, name + " accepted what it has to refuse"
    msg = lib.os2d_last_error()
    assert msg and len(msg.decode("utf-8", "replace").strip()) > 8
    return rc


class Buf:
    """A device buffer of ``nbytes`` bytes followed by a guard, all 0xFF."""

    def __init__(self, device, nbytes):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + GUARD,), 0xFF, dtype=torch.uint8, device=device)

    def ptr(self):
        return _L().ptr(self.raw)

    def host(self, dtype, *shape):
        return self.raw[:self.n].cpu().numpy().view(dtype).reshape(*shape)

    def guard_ok(self):
        return bool((self.raw[self.n:] == 0xFF).all())

    def untouched(self):
        return bool((self.raw == 0xFF).all())


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def all_ff(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


ERRORS = {}


def check_pin(case, err):
    print("\nSTAGE boxes {:<32s} {:.3e}".format(case, err))
    ERRORS[case] = err
    assert PIN["boxes"] <= CEILING["boxes"]
    assert err < PIN["boxes"], (case, err)


def check_label(c, r, what, count, index, scores, boxes, default=None, corners=None):
    """One label's outputs (arrays over its N candidates) against the model's result ``r``.  Returns the box error."""
    cand, order = r["cand"], r["order"]
    if c["kind"] == "pyramid" and C.expect_unfinished(c, r):
        assert count == -1, what
        assert all(all_ff(a) for a in (index, scores, boxes, default, corners) if a is not None), what + ": written although unfinished"
        return 0.0
    n = len(order)
    assert count == n, (what, count, n)
    assert np.array_equal(index[:n], order), what + ": out_index"
    assert same_bits(scores[:n], cand["scores"][order]), what + ": out_scores are not the source scores"
    for name, got, ref in (("out_default", default, cand["default32"]), ("out_corners", corners, cand["corners32"])):
        if got is not None:
            assert same_bits(got[:n], ref[order]), what + ": " + name
            assert all_ff(got[n:]), what + ": " + name + " past out_count"
    assert all_ff(index[n:]) and all_ff(scores[n:]) and all_ff(boxes[n:]), what + ": written past out_count"
    if n == 0:
        return 0.0
    assert np.isfinite(boxes[:n]).all(), what
    return float((np.abs(boxes[:n].astype(np.float64) - cand["boxes64"][order]).max(1) / cand["scale"][order]).max())


def op_tables(chains, width):
    """HOST arrays counts [L], kinds [L][width], args [L][width][2] of the ABI."""
    L = len(chains)
    counts = (ctypes.c_int * L)(*[len(ch) for ch in chains])
    kinds, args = (ctypes.c_int * (L * width))(), (ctypes.c_float * (L * width * 2))()
    for l, ch in enumerate(chains):
        for k, (kind, ax, ay) in enumerate(ch[:width]):
            kinds[l * width + k], args[(l * width + k) * 2], args[(l * width + k) * 2 + 1] = kind, ax, ay
    return counts, kinds, args


# ------------------------------------------------------------------------------------------------------------------ os2d_nms
@pytest.mark.parametrize("name", list(C.NMS_CASES))
def test_nms(device, name):
    """Counts 0 .. N and beyond; the kept list beyond the 2048 boxes held in LDS (suppressors on either side of the cache, in the
    victim's step of 64 and before it, the kept count going over 2048 inside a step); thresholds 0 and 1; 0/0."""
    c = C.NMS_CASES[name]
    NC, N = c["boxes"].shape[:2]
    boxes, counts = dev(c["boxes"], device), dev(np.array(c["counts"], np.int32), device)
    nbytes = ctypes.c_size_t()
    _call("os2d_nms_workspace_bytes", NC, N, ctypes.byref(nbytes))
    assert nbytes.value >= NC * N * 16
    runs = []
    for _ in range(2):
        keep, num, ws = Buf(device, NC * N), Buf(device, NC * 4), Buf(device, nbytes.value)
        _call("os2d_nms", _L().ptr(boxes), _L().ptr(counts), NC, N, c["iou_thr"], keep.ptr(), num.ptr(), ws.ptr(), nbytes.value,
              _L().current_stream(device))
        torch.cuda.synchronize()
        assert keep.guard_ok() and num.guard_ok() and ws.guard_ok()
        runs.append((keep.host(np.uint8, NC, N), num.host(np.int32, NC)))
    (keep, num), again = runs
    assert np.array_equal(keep, again[0]) and np.array_equal(num, again[1])
    for k, (ref, run) in enumerate(C.nms_model(name)):
        assert num[k] == run.kept_count, (name, k)
        assert np.array_equal(keep[k], ref), (name, k, np.nonzero(keep[k] != ref)[0][:8])
        assert keep[k, min(c["counts"][k], N):].sum() == 0


# ------------------------------------------------------------------------------------------------- os2d_detect_level[_ops]
def call_level(device, c, H=None, W=None, ops=None, refuse=False):
    lv = c["level"]
    B = c["B"]
    H, W = H or lv["H"], W or lv["W"]
    HW = H * W
    ops = lv["ops"] if ops is None else ops
    loc, cls = dev(lv["loc"], device), dev(lv["cls"], device)
    o = {"boxes": Buf(device, B * HW * 16), "scores": Buf(device, B * HW * 4), "index": Buf(device, B * HW * 4), "count": Buf(device, B * 4)}
    head = (_L().ptr(loc), _L().ptr(cls), B, H, W, 16, 16, lv["img_w"], lv["img_h"])
    tail = (c["score_thr"], c["iou_thr"], o["boxes"].ptr(), o["scores"].ptr(), o["index"].ptr(), o["count"].ptr(), _L().current_stream(device))
    if c["api"] == "scale":
        (_, sx, sy), = ops
        args = ("os2d_detect_level",) + head + (sx, sy) + tail
    else:
        _, kinds, fargs = op_tables([ops], max(len(ops), 1))
        args = ("os2d_detect_level_ops",) + head + (len(ops), kinds, fargs) + tail
    if refuse:
        _refused(*args)
        assert all(b.untouched() for b in o.values())
        return None
    _call(*args)
    torch.cuda.synchronize()
    assert all(b.guard_ok() for b in o.values())
    return (o["count"].host(np.int32, B), o["index"].host(np.int32, B, HW), o["scores"].host(np.float32, B, HW),
            o["boxes"].host(np.float32, B, HW, 4))


@pytest.mark.parametrize("name", C.LEVEL_CASES)
def test_detect_level(device, name):
    """H*W around the steps of 64 and the sort sizes, up to the largest level the kernel takes; 0 / 1 / 64 / 65 valid candidates;
    the kept list past the boxes cached in LDS (kcap = 4 at 9 locations, 2048 at 60x80 and the largest level); the score table;
    chains of 0 and 6 ops."""
    c = C.case("level", name)
    if name == "max_level":
        lib = _L().load()
        assert lib.os2d_detect_level_supported(1, C.LEVEL_MAX_HW) == 1 and lib.os2d_detect_level_supported(1, C.LEVEL_MAX_HW + 1) == 0
    got = call_level(device, c)
    again = call_level(device, c)
    assert all(same_bits(a, b) for a, b in zip(got, again)), "a second call gives other bits"
    errs = [check_label(c, r, "{} class {}".format(name, b), got[0][b], got[1][b], got[2][b], got[3][b])
            for b, r in enumerate(C.model("level", name))]
    check_pin("level " + name, max(errs))


# -------------------------------------------------------------------------------------------------------- os2d_detect_pyramid*
def call_pyramid(device, c, refuse=False, **over):
    """``over``: arguments replaced for a refusal (L, M, passes, chains)."""
    levels = c["levels"]
    L, B = over.get("L", len(levels)), c["B"]
    levels = (levels * L)[:L]
    rows = C.labels_of(c)
    G, V = len(rows), len(rows[0])
    N1 = sum(lv["H"] * lv["W"] for lv in levels)
    N = N1 * V
    M, passes = over.get("M", c["M"]), over.get("passes", c["passes"])
    keep = [[dev(lv[k], device) for lv in levels] for k in ("loc", "cls")]
    has_corners = levels[0]["corners"] is not None
    keep.append([dev(lv["corners"], device) for lv in levels] if has_corners else None)
    c_loc, c_cls, c_cor = [(ctypes.c_void_p * L)(*[t.data_ptr() for t in ts]) if ts is not None else None for ts in keep]
    c_hw = (ctypes.c_int * (2 * L))(*[v for lv in levels for v in (lv["H"], lv["W"])])
    c_img = (ctypes.c_float * (2 * L))(*[v for lv in levels for v in (lv["img_w"], lv["img_h"])])
    slot_rows = dev(np.array(rows, np.int32), device) if c["slot_rows"] is not None else None
    nbytes = ctypes.c_size_t()
    _call("os2d_detect_pyramid_workspace_bytes", G, N, min(passes, 16), ctypes.byref(nbytes))
    ws = Buf(device, nbytes.value)
    assert ws.raw.data_ptr() % 256 == 0
    o = {"boxes": Buf(device, G * N * 16), "scores": Buf(device, G * N * 4), "index": Buf(device, G * N * 4),
         "default": Buf(device, G * N * 16), "corners": Buf(device, G * N * 32) if has_corners else None,
         "count": Buf(device, G * 4), "unfinished": Buf(device, 4)}
    outs = tuple(o[k].ptr() if o[k] is not None else None for k in ("boxes", "scores", "index", "default", "corners", "count", "unfinished"))
    head = (c_loc, c_cls, c_cor, B, L, c_hw, 16, 16, c_img)
    tail = outs + (ws.ptr(), nbytes.value, _L().current_stream(device))
    nms = (c["score_thr"], c["iou_thr"], M, passes)
    if c["api"] == "ops":
        t = op_tables(over.get("chains", [lv["ops"] for lv in levels]), 6) + op_tables([lv["dops"] for lv in levels], 12)
        args = ("os2d_detect_pyramid_ops",) + head + t + nms + (G, V, _L().ptr(slot_rows)) + tail
    else:
        for lv in levels:
            assert len(lv["ops"]) == 1 and lv["ops"][0][0] == DM.OP_SCALE and lv["dops"] == lv["ops"]
        scale = (ctypes.c_float * (2 * L))(*[v for lv in levels for v in lv["ops"][0][1:]])
        if c["api"] == "merged":
            args = ("os2d_detect_pyramid_merged",) + head + (scale,) + nms + (G, V, _L().ptr(slot_rows)) + tail
        else:
            args = ("os2d_detect_pyramid",) + head + (scale,) + nms + tail
    if refuse:
        _refused(*args)
        assert all(b.untouched() for b in o.values() if b is not None) and ws.untouched()
        return None
    _call(*args)
    torch.cuda.synchronize()
    assert all(b.guard_ok() for b in o.values() if b is not None) and ws.guard_ok()
    return {"count": o["count"].host(np.int32, G), "unfinished": int(o["unfinished"].host(np.int32, 1)[0]),
            "index": o["index"].host(np.int32, G, N), "scores": o["scores"].host(np.float32, G, N),
            "boxes": o["boxes"].host(np.float32, G, N, 4), "default": o["default"].host(np.float32, G, N, 4),
            "corners": o["corners"].host(np.float32, G, N, 8) if has_corners else None}


@pytest.mark.parametrize("name", C.PYRAMID_CASES)
def test_detect_pyramid(device, name):
    """The three entry points (tests/detect_stage_cases.py says which case takes which).  The workspace is dirty (0xFF) in every
    case: with 32 candidates or fewer per label a read of uninitialised workspace shows up as a wrong result."""
    c = C.case("pyramid", name)
    got = call_pyramid(device, c)
    again = call_pyramid(device, c)
    assert all(a is b or same_bits(a, b) for a, b in ((got[k], again[k]) for k in got if k != "unfinished")), "a second call gives other bits"
    assert got["unfinished"] == again["unfinished"]
    model = C.model("pyramid", name)
    assert got["unfinished"] == sum(C.expect_unfinished(c, r) for r in model)
    errs = []
    for g, r in enumerate(model):
        errs.append(check_label(c, r, "{} label {}".format(name, g), got["count"][g], got["index"][g], got["scores"][g], got["boxes"][g],
                                got["default"][g], None if got["corners"] is None else got["corners"][g]))
    check_pin("pyramid " + name, max(errs))


def test_generic_fallback_equals_the_model_beyond_the_final_sort(device):
    """16512 survivors in three chunks: os2d_detect_pyramid reports the label unfinished (test_detect_pyramid[finalize_16512]) and
    Os2dBoxCoder.decode_pyramid falls back to os2d_decode_boxes + os2d_nms, whose result is the model's."""
    from os2d_amd.modeling.box_coder import BoxGridGenerator, Os2dBoxCoder
    from os2d_amd.structures.feature_map import FeatureMapSize
    c, r = C.case("pyramid", "finalize_16512"), C.model("pyramid", "finalize_16512")[0]
    lv = c["levels"][0]
    coder = Os2dBoxCoder(output_box_grid_generator=BoxGridGenerator(box_size=FeatureMapSize(w=240, h=240), box_stride=FeatureMapSize(w=16, h=16)))
    coder.nms_max_batch = c["M"]
    size = FeatureMapSize(w=int(lv["img_w"]), h=int(lv["img_h"]))
    fm = coder.get_feature_map_size(size)
    assert (fm.h, fm.w) == (lv["H"], lv["W"])
    res = coder.decode_pyramid([dev(lv["loc"], device)], [dev(lv["cls"], device)], [size], class_ids=[0],
                               nms_score_threshold=c["score_thr"], nms_iou_threshold=c["iou_thr"])
    order = r["order"]
    assert len(res) == len(order) == 16512
    assert same_bits(res.get_field("scores").cpu().numpy(), r["cand"]["scores"][order])
    assert same_bits(res.get_field("default_boxes").bbox_xyxy.cpu().numpy(), r["cand"]["default32"][order])
    check_pin("fallback finalize_16512", float(np.abs(res.bbox_xyxy.cpu().numpy().astype(np.float64) - r["cand"]["boxes64"][order]).max()))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(device):
    """Non-zero, an error text, and no output, workspace or guard byte touched."""
    lib = _L().load()
    base = C.case("pyramid", "levels_2")
    call_pyramid(device, base, refuse=True, L=17)
    call_pyramid(device, base, refuse=True, M=12289)
    call_pyramid(device, base, refuse=True, passes=17)
    nbytes = ctypes.c_size_t()
    assert lib.os2d_detect_pyramid_workspace_bytes(2, 32, 17, ctypes.byref(nbytes)) != 0
    # 65 chunks: 513 candidates at nms_max_batch 8
    assert lib.os2d_detect_pyramid_supported(1, 512, 8) == 1 and lib.os2d_detect_pyramid_supported(1, 513, 8) == 0
    wide = dict(C.case("pyramid", "chunks_64"))
    wide["levels"] = [C.make_level(1, 513, C.grid_loc(1, 513), np.zeros((1, 513), np.float32))]
    call_pyramid(device, wide, refuse=True)
    chains = C.case("pyramid", "chains")
    seven = [chains["levels"][0]["ops"] + [(DM.OP_SHIFT, 1.0, 1.0)], chains["levels"][1]["ops"]]
    call_pyramid(device, chains, refuse=True, chains=seven)
    # a level one location above the largest, a chain of 7 ops
    big = dict(C.case("level", "max_level"))
    big["level"] = C.make_level(1, C.LEVEL_MAX_HW + 1, C.grid_loc(1, C.LEVEL_MAX_HW + 1), np.zeros((1, C.LEVEL_MAX_HW + 1), np.float32))
    call_level(device, big, refuse=True)
    call_level(device, C.case("level", "chain_6"), ops=C.SIX_OPS + [(DM.OP_SHIFT, 1.0, 1.0)], refuse=True)
