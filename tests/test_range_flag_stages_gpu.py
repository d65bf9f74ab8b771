"""GPU: the range-flag protocol of the split-fp16 forward kernels (Os2dRangeFlag, os2d_amd/csrc/os2d_common.h).

a. The RAISERS through their stage entry points, on the cases of tests/range_flag_cases.py (each held to a float64 model by
   tests/test_range_flag_model.py): os2d_transform_conv_f16x3 (layers 1 and 2; terms 3 and 2 for layer 1), os2d_fft_inverse (both
   spectra layouts), os2d_dft_inverse, os2d_dft_inverse_planes.  Per case
     * the status word, pre-set to 0 and read once after a synchronise, equals OS2D_STATUS_F16_RANGE exactly when the case says so;
     * a word pre-set to 1 stays 1 after a clean call (never cleared);
     * in a raised call every cell the case marks clean has the bits of the same call with the offending value made finite;
     * the NaN-prefilled output comes back fully written (every data cell finite outside the offending cells, every border 0).
   Layer 3 writes fp32 and has no check: a NaN in its input reaches the parameters as NaN.
b. / c. The CALL protocol of os2d_head_forward_ex2 - per-image words, whole-call word, epoch, chunked workspaces - and the
   non-finite class operand.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import range_flag_cases as RC
import train_forward_f16x3_model as SHB

pytestmark = pytest.mark.gpu

RAISED = RC.STATUS_F16_RANGE


def _L():
    from os2d_amd import _lib
    return _lib


def _ptr(t):
    return _L().ptr(t)


def _call(name, *args):
    L = _L()
    L.check(getattr(L.load(), name)(*args), name)


def _stream(device):
    return _L().current_stream(device)


def _status(device, value):
    return torch.full((1,), value, dtype=torch.int32, device=device)


def _read(status):
    torch.cuda.synchronize()
    return int(status.item())


# =================================================================================================== a. convolutions
_packed = {}


def _pack(case, device):
    """os2d_pack_conv_f16x3 of the case's layer with the case's own exponents and eps; cached by content."""
    key = (case.layer, case.w.tobytes(), case.b.tobytes())
    if key not in _packed:
        lib = _L().load()
        w, b = torch.from_numpy(case.w).to(device), torch.from_numpy(case.b).to(device)
        bn = [torch.from_numpy(t).to(device) for t in case.bn]
        exps = [torch.from_numpy(e).to(device) for e in case.exps]
        pw = torch.full((int(lib.os2d_packed_conv_bytes(case.layer, 1)),), 0xFF, dtype=torch.uint8, device=device)
        pb = torch.full((int(lib.os2d_packed_bias_floats(case.layer)),), float("nan"), device=device)
        _call("os2d_pack_conv_f16x3", case.layer, 6, _ptr(w), _ptr(b), *[_ptr(t) for t in bn], ctypes.c_float(case.eps),
              *[_ptr(e) for e in exps], _ptr(pw), _ptr(pb), _stream(device))
        torch.cuda.synchronize()
        _packed[key] = (pw, pb)
    return _packed[key]


def _run_conv(case, device, preset=0):
    """One os2d_transform_conv_f16x3 call into a 0xFF-prefilled buffer: (status word after the call, output halves
    [NB, G, 2, PLANE, 8] float16)."""
    H, W = case.shape
    cout = RC.LAYERS[case.layer][1]
    pw, pb = _pack(case, device)
    xin = RC.conv_shb_input(case).to(device)
    out = torch.full((RC.CONV_NB * int(_L().load().os2d_shb_bytes(cout, H, W)),), 0xFF, dtype=torch.uint8, device=device)
    status = _status(device, preset)
    _call("os2d_transform_conv_f16x3", case.layer, _ptr(xin), _ptr(pw), _ptr(pb), _ptr(out), RC.CONV_NB, 6, H, W, case.terms, _ptr(status),
          _stream(device))
    word = _read(status)
    return word, out.cpu().numpy().view(np.float16).reshape(RC.CONV_NB, SHB.groups(cout), 2, SHB.plane(H, W), 8)


def _shb_cells(halves, channels, H, W):
    """[NB, G, 2, PLANE, 8] -> the data cells as [NB, channels, 2 (hi | lo), H, W] uint16 bit patterns."""
    NB = halves.shape[0]
    cells = halves.view(np.uint16)[:, :, :, SHB.plane_index(H, W), :]                       # [NB, G, 2, H*W, 8]
    return cells.transpose(0, 1, 4, 2, 3).reshape(NB, -1, 2, H, W)[:, :channels]


def _check_written(halves, channels, H, W, clean, what):
    """Borders exactly 0 (both halves, every channel slot), and every clean data cell finite: nothing of the 0xFF prefill left."""
    assert not halves[:, :, :, ~SHB.interior_mask(H, W)].view(np.uint16).any(), what + ": non-zero border unit"
    cells = _shb_cells(halves, channels, H, W).view(np.float16).astype(np.float32)
    mask = np.broadcast_to(clean[:, :, None], cells.shape)
    assert np.isfinite(cells[mask]).all(), what + ": a clean cell was not written"


@pytest.mark.parametrize("layer,terms,shape", RC.CONV_GROUPS, ids=["L{}-terms{}-{}x{}".format(l, t, *s) for l, t, s in RC.CONV_GROUPS])
def test_conv_f16x3_raises_exactly_when_a_stored_cell_leaves_the_range(device, layer, terms, shape):
    H, W = shape
    cout = RC.LAYERS[layer][1]
    everything = np.ones((RC.CONV_NB, cout, H, W), dtype=bool)
    fixed_runs, lines, wrong = {}, [], []
    for case in RC.conv_cases(layer, terms, shape):
        word, halves = _run_conv(case, device)
        lines.append("RANGE conv L{} terms {} {}x{} {:<28s} word {} (want {})".format(layer, terms, H, W, case.name, word, RAISED if case.raises else 0))
        if word != (RAISED if case.raises else 0):
            wrong.append(case.name)
            continue
        if not case.raises:
            _check_written(halves, cout, H, W, everything, case.name)
            fixed_runs[case.name] = halves
            again, halves1 = _run_conv(case, device, preset=1)
            assert again == 1, case.name + ": a clean call cleared the status word"
            assert np.array_equal(halves1.view(np.uint16), halves.view(np.uint16)), case.name
        else:
            _check_written(halves, cout, H, W, case.clean, case.name)
            twin = fixed_runs.get(case.fixed.name)
            if twin is None:
                w0, twin = _run_conv(case.fixed, device)
                assert w0 == 0, case.fixed.name
                fixed_runs[case.fixed.name] = twin
            a, b = _shb_cells(halves, cout, H, W), _shb_cells(twin, cout, H, W)
            mask = np.broadcast_to(case.clean[:, :, None], a.shape)
            assert np.array_equal(a[mask], b[mask]), case.name + ": a clean cell differs from the call with the offending value made finite"
    print("\n" + "\n".join(lines))
    assert not wrong, wrong


def test_layer_3_has_no_check_and_passes_a_nan_on(device):
    """Layer 3 writes fp32 parameters: no range word to raise (the entry point takes one and leaves it alone), a NaN in its
    input arrives in the parameters of that cell's 5x5 neighbourhood as NaN, everything else stays finite."""
    lib = _L().load()
    H, W, NB, P = 9, 14, 2, 6
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(P, 64, 5, 5, generator=g) * 0.05, torch.randn(P, generator=g)
    x = torch.rand(NB, 64, H, W, generator=g).numpy()
    exps = [torch.zeros(P, dtype=torch.int32, device=device), torch.zeros(64, dtype=torch.int32, device=device)]
    pw = torch.full((int(lib.os2d_packed_conv_bytes(3, 1)),), 0xFF, dtype=torch.uint8, device=device)
    pb = torch.full((int(lib.os2d_packed_bias_floats(3)),), float("nan"), device=device)
    wd, bd = w.to(device), b.to(device)
    _call("os2d_pack_conv_f16x3", 3, P, _ptr(wd), _ptr(bd), *[_ptr(None)] * 4, ctypes.c_float(0.0), _ptr(exps[0]), _ptr(exps[1]), _ptr(None),
          _ptr(pw), _ptr(pb), _stream(device))
    halves = SHB.pack(x, np.zeros(64, dtype=np.int32))
    halves[1, 2, 0, SHB.base(W) + 4 * SHB.ws(W) + 6, 3] = np.float16(np.nan)           # pair 1, channel 19, cell (4, 6)
    xin = torch.from_numpy(halves.view(np.uint8).reshape(-1)).to(device)
    out = torch.full((NB * P * H * W,), float("nan"), device=device)
    for preset in (0, 1):
        status = _status(device, preset)
        _call("os2d_transform_conv_f16x3", 3, _ptr(xin), _ptr(pw), _ptr(pb), _ptr(out), NB, P, H, W, 3, _ptr(status), _stream(device))
        assert _read(status) == preset
    got = out.cpu().view(NB, P, H, W)
    want = torch.zeros(NB, P, H, W, dtype=torch.bool)
    want[1, :, 2:7, 4:9] = True
    assert torch.equal(torch.isnan(got), want)


# =================================================================================================== a. inverse transforms
def _plan(entry, shape):
    import freq_util
    if entry.startswith("fft"):
        P, Q, nbins = freq_util.fft_sizes(*shape)
        return RC.Plan(P, Q, nbins, *freq_util.fft_tiles(*shape), False)
    P, Q, nbins, t = freq_util.dft_sizes(*shape)
    return RC.Plan(P, Q, nbins, *t[:4], True)


_tables = {}


def _operands(entry, plan, device):
    import freq_util
    key = (entry.startswith("fft"), plan.P, plan.Q)
    if key not in _tables:
        _tables[key] = (freq_util.twiddles(plan.Q, device), freq_util.twiddles(plan.P, device)) if key[0] else (freq_util.matrices(plan.P, plan.Q, device),)
    return _tables[key]


def _lay_out(entry, plan, Y):
    """complex64 [NB, T, Cout, P, V] -> the float buffer of the entry point: rows [NBT, Cout, nbins] with bin = u V + v, or
    quads [nbins / 4, NBT, Cout, 4] (bin = u V + v for the FFTs, v P + u for the matrix-product transforms)."""
    NB, T, C, P, V = Y.shape
    if plan.u_fastest:
        Y = Y.transpose(3, 4)
    rows = torch.zeros(NB * T, C, plan.nbins, 2)
    rows[:, :, :P * V] = torch.view_as_real(Y.reshape(NB * T, C, P * V))
    if entry == "fft_rows":
        return rows.contiguous()
    return rows.view(NB * T, C, plan.nbins // 4, 4, 2).permute(2, 0, 1, 3, 4).contiguous()


def _run_transform(case, device, preset=0):
    """(status word, stored values [NB, Cout, 2, H, W]: uint16 halves of the SHB buffer, or one int32 plane for dft_planes)."""
    H, W = case.shape
    lib, plan, NB, C = _L().load(), case.plan, RC.T_NB, RC.T_COUT
    Y = _lay_out(case.entry, plan, RC.transform_spectra(case)).to(device)
    bp = torch.zeros(3 * 128)
    bp[:C] = torch.from_numpy(case.bias)
    bp[256:256 + C] = torch.exp2(torch.from_numpy(RC.t_out_exp()).float())
    bp = bp.to(device)
    ops = _operands(case.entry, plan, device)
    status = _status(device, preset)
    st = _stream(device)
    if case.entry == "dft_planes":
        out = torch.full((NB, C, H, W), float("nan"), device=device)
        _call("os2d_dft_inverse_planes", _ptr(Y), _ptr(bp), _ptr(out), _ptr(ops[0]), NB, C, H, W, _ptr(status), st)
        word = _read(status)
        return word, out.cpu().numpy().view(np.int32).reshape(NB, C, 1, H, W), None
    out = torch.full((NB * int(lib.os2d_shb_bytes(C, H, W)),), 0xFF, dtype=torch.uint8, device=device)
    if case.entry == "dft":
        _call("os2d_dft_inverse", _ptr(Y), _ptr(bp), _ptr(out), _ptr(ops[0]), NB, C, H, W, _ptr(status), st)
    elif case.entry == "fft_rows":
        _call("os2d_fft_inverse", _ptr(Y), _ptr(bp), _ptr(out), _ptr(ops[0]), _ptr(ops[1]), NB, C, H, W, _ptr(status), st)
    else:
        _call("os2d_fft_inverse_ex", _ptr(Y), _ptr(bp), _ptr(out), _ptr(ops[0]), _ptr(ops[1]), NB, C, H, W, _ptr(status), 1, st)
    word = _read(status)
    halves = out.cpu().numpy().view(np.float16).reshape(NB, SHB.groups(C), 2, SHB.plane(H, W), 8)
    return word, _shb_cells(halves, C, H, W), halves


def _values(entry, cells):
    return cells.view(np.float32) if entry == "dft_planes" else cells.view(np.float16).astype(np.float32)


@pytest.mark.parametrize("shape", RC.TRANSFORM_SHAPES, ids=["{}x{}".format(*s) for s in RC.TRANSFORM_SHAPES])
@pytest.mark.parametrize("entry", RC.ENTRIES)
def test_inverse_transforms_raise_exactly_when_a_stored_cell_leaves_the_range(device, entry, shape):
    H, W = shape
    everything = np.ones((RC.T_NB, RC.T_COUT, H, W), dtype=bool)
    runs, lines, wrong = {}, [], []
    for case in RC.transform_cases(entry, shape, _plan(entry, shape)):
        word, cells, halves = _run_transform(case, device)
        lines.append("RANGE {} {}x{} {:<24s} word {} (want {})".format(entry, H, W, case.name, word, RAISED if case.raises else 0))
        if word != (RAISED if case.raises else 0):
            wrong.append(case.name)
            continue
        clean = case.clean if case.raises else everything
        vals = _values(entry, cells)
        assert np.isfinite(vals[np.broadcast_to(clean[:, :, None], vals.shape)]).all(), case.name + ": a clean cell was not written"
        if halves is not None:
            assert not halves[:, :, :, ~SHB.interior_mask(H, W)].view(np.uint16).any(), case.name + ": non-zero border unit"
        if not case.raises:
            runs[case.name] = cells
            again, cells1, _ = _run_transform(case, device, preset=1)
            assert again == 1, case.name + ": a clean call cleared the status word"
            assert np.array_equal(cells1, cells), case.name
        else:
            twin = runs.get(case.fixed.name)
            if twin is None:
                w0, twin, _ = _run_transform(case.fixed, device)
                assert w0 == 0, case.fixed.name
                runs[case.fixed.name] = twin
            mask = np.broadcast_to(case.clean[:, :, None], cells.shape)
            assert np.array_equal(cells[mask], twin[mask]), case.name + ": a clean cell differs from the call with the offending value made finite"
    print("\n" + "\n".join(lines))
    assert not wrong, wrong


# =================================================================================================== b. the call protocol
# os2d_head_forward_ex2 driven directly (tests/util.py: head_forward_ex2) at ROUTE_SHAPES["9x14"] of tests/test_head_gpu.py: A = 2,
# B = 5, C = 32.  The test owns the workspace and reads its first (A + 1) * 4 bytes - the range words - back as int32.
A_, B_, C_, H_, W_ = 2, 5, 32, 9, 14
ROUTES = [("f16x3", True), ("fft", True), ("fftx3", True), ("fftx3", False)]          # (precision, wspec2 for the 5x5 layer)
ROUTE_IDS = ["f16x3", "fft", "fftx3", "fftx3-direct-conv2"]
NONFINITE = [float("nan"), float("inf"), float("-inf")]
_heads = {}


def _util():
    import util
    return util


def _head(kind, device):
    """Heads on the network and class maps of test_head_gpu._route_head("9x14") (tests/util.py: route_head_inputs), built once:
      clean           as there
      overflow1 / 2   a bias of 3e38 under a BatchNorm weight of 1e3 in layer 1 / layer 2: the activation overflows whatever the
                      range plan chooses (the bias case of part a, through the head)
      (value, cell)   class 3 of 5 poisoned at channel 4 of template cell ``cell`` of its 15 x 15 map."""
    if kind not in _heads:
        state, class_fms, _ = _util().route_head_inputs(A_, B_, H_, W_, C_)
        if kind == "overflow1":
            state["conv.0.bias"][5], state["conv.1.weight"][5] = 3e38, 1e3
        elif kind == "overflow2":
            state["conv.3.bias"][5], state["conv.4.weight"][5] = 3e38, 1e3
        elif kind != "clean":
            value, (ty, tx) = kind
            assert tuple(class_fms[3].shape[-2:]) == (15, 15)
            class_fms = [c.clone() for c in class_fms]
            class_fms[3].view(C_, 15, 15)[4, ty, tx] = value
        creator = _util().make_head_creator(6, True, state, device)
        with torch.no_grad():
            head = creator.create_os2d_head([c.to(device) for c in class_fms])
        _heads[kind] = head, state, class_fms
    return _heads[kind][0]


def _clean_fm():
    return _util().route_head_inputs(A_, B_, H_, W_, C_)[2]


def _words(ws):
    return ws[:(A_ + 1) * 4].cpu().view(torch.int32).tolist()


def _bits(outs):
    return [t.cpu().view(torch.int32) for t in outs]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _protocol(device, precision, conv2_freq):
    """Every outcome of part b for one route, for workspaces of 5, 2 and 1 classes per chunk; returns the report lines."""
    U = _util()
    lines = []
    fm = _clean_fm().to(device)
    single = {}                                       # outcome name -> bits of the single-chunk call
    for Bc in (B_, 2, 1):
        size = U.head_workspace_bytes(A_, Bc, C_, H_, W_, precision)

        def run(kind, x, ws, status):
            chunk, outs = U.head_forward_ex2(_head(kind, device), x, precision, ws, status, conv2_freq)
            assert chunk == Bc, (chunk, Bc)
            return _bits(outs)

        def same_as_single(name, outs):
            if Bc == B_:
                single[name] = outs
            else:
                assert _same(outs, single[name]), "{}: {} classes per chunk differ from the single-chunk call".format(name, Bc)

        # ---- clean call
        ws, status = torch.zeros(size, dtype=torch.uint8, device=device), _status(device, 0)
        clean = run("clean", fm, ws, status)
        assert _words(ws) == [0] * (A_ + 1) and int(status.item()) == 0
        assert all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in clean)
        same_as_single("clean", clean)

        # ---- a non-finite feature of image 1, first and last location
        for value in NONFINITE:
            for where, (c, h, w) in (("first", (0, 0, 0)), ("last", (C_ - 1, H_ - 1, W_ - 1))):
                name = "feature {} {}".format(value, where)
                bad = fm.clone()
                bad[1, c, h, w] = value
                ws, status = torch.zeros(size, dtype=torch.uint8, device=device), _status(device, 0)
                outs = run("clean", bad, ws, status)
                words = _words(ws)
                lines.append("PROTOCOL {} conv2_freq={} Bc={} {:<22s} words {} status {}".format(precision, conv2_freq, Bc, name, words, int(status.item())))
                assert words[0] == 0 and words[A_] == 0 and words[1] not in (0, RAISED), (name, words)
                assert int(status.item()) == 1, name
                for t, t0 in zip(outs, clean):
                    assert bool(torch.isnan(t[1].view(torch.float32)).all()), name + ": image 1 is not all-NaN"
                    assert torch.equal(t[0], t0[0]), name + ": image 0 differs from the clean call"
                same_as_single(name, outs)
                if value != value and where == "last":
                    # a second, CLEAN call on the same workspace, not re-zeroed: the clean bits, the stale words untouched, no status
                    status.zero_()
                    again = run("clean", fm, ws, status)
                    assert _same(again, clean), "a clean call after a flagged one on the same workspace differs"
                    assert _words(ws) == words and int(status.item()) == 0
                    # a second FLAGGED call on the same workspace: another epoch
                    outs2 = run("clean", bad, ws, status)
                    words2 = _words(ws)
                    assert words2[1] not in (0, RAISED, words[1]) and words2[0] == 0 and words2[A_] == 0, (words, words2)
                    assert _same(outs2, outs) and int(status.item()) == 1

        # ---- an activation beyond the range, layer 1 and layer 2: the word of the whole call, every output NaN
        for kind in ("overflow1", "overflow2"):
            ws, status = torch.zeros(size, dtype=torch.uint8, device=device), _status(device, 0)
            outs = run(kind, fm, ws, status)
            words = _words(ws)
            lines.append("PROTOCOL {} conv2_freq={} Bc={} {:<22s} words {} status {}".format(precision, conv2_freq, Bc, kind, words, int(status.item())))
            assert words[:A_] == [0] * A_ and words[A_] not in (0, RAISED), (kind, words)
            assert int(status.item()) == 1
            assert all(bool(torch.isnan(t.view(torch.float32)).all()) for t in outs), kind + ": an output is not NaN"
            same_as_single(kind, outs)
            # a CLEAN call on the same workspace, not re-zeroed, with the stale epoch in the word of the whole call: a consumer
            # that tested the word against 0 instead of against its own epoch would poison this one
            status.zero_()
            again = run("clean", fm, ws, status)
            assert _same(again, clean), kind + ": a clean call after an overflowing one on the same workspace differs"
            assert _words(ws) == words and int(status.item()) == 0, kind

        # ---- finite features whose sum of squares overflows float32 (2e19 in all 32 channels of one location of image 1): the
        # reference stays finite; either the device does what its fp32 route does, bit for bit, or it flags the image
        big = fm.clone()
        big[1, :, 4, 7] = 2e19
        ws, status = torch.zeros(size, dtype=torch.uint8, device=device), _status(device, 0)
        outs = run("clean", big, ws, status)
        ws32 = torch.zeros(U.head_workspace_bytes(A_, B_, C_, H_, W_, "f32"), dtype=torch.uint8, device=device)
        ref32 = _bits(U.head_forward_ex2(_head("clean", device), big, "f32", ws32, None)[1])
        flagged = all(bool(torch.isnan(t[1].view(torch.float32)).all()) for t in outs) and int(status.item()) == 1
        lines.append("PROTOCOL {} conv2_freq={} Bc={} sum-of-squares overflow: {} (words {}, fp32 route finite: {})".format(
            precision, conv2_freq, Bc, "image flagged, all-NaN" if flagged else "as the fp32 route", _words(ws),
            all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in ref32)))
        assert _same(outs, ref32) or (flagged and all(torch.equal(t[0], t0[0]) for t, t0 in zip(outs, clean)))
        same_as_single("sumsq", outs)
    return lines


@pytest.mark.parametrize("precision,conv2_freq", ROUTES, ids=ROUTE_IDS)
def test_call_protocol_fused_tail(device, precision, conv2_freq):
    assert not os.environ.get("OS2D_FUSED_TAIL", "1").startswith("0"), "this test is for the fused tail (the default)"
    with torch.no_grad():
        print("\n" + "\n".join(_protocol(device, precision, conv2_freq)))


def test_call_protocol_and_class_operand_with_the_tail_as_two_launches():
    """OS2D_FUSED_TAIL=0 - layer 3 and sample_decode_kernel as two launches, the other consumer of the range words - is read once
    per process: parts b and c again in a fresh child process (this file as a script)."""
    env = dict(os.environ, OS2D_FUSED_TAIL="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]


# =================================================================================================== c. non-finite class operand
POISONS = [(v, cell) for v in (float("nan"), float("inf")) for cell in ((0, 0), (7, 7))]       # (0, 0): outside the pooled 11 x 11 interior
_oracles = {}


def _class_oracle(kind):
    """The CPU oracle (tests/test_head_gpu.py: _oracle) on the poisoned class maps: computed once per poison."""
    if kind not in _oracles:
        from test_head_gpu import _oracle
        _, state, class_fms = _heads[kind]
        ref = _oracle(_clean_fm(), class_fms, state, True)
        _oracles[kind] = ref[0], ref[3]                      # loc, corners
    return _oracles[kind]


def _class_operand(device, precision, conv2_freq):
    U = _util()
    lines = []
    fm = _clean_fm().to(device)
    for kind in POISONS:
        head = _head(kind, device)
        ref_loc, ref_corners = _class_oracle(kind)
        assert bool(torch.isnan(ref_loc[:, 3]).all()) and bool(torch.isnan(ref_corners[:, 3]).all()), "the reference poisons the class on every image"
        for Bc in (B_, 2, 1):
            size = U.head_workspace_bytes(A_, Bc, C_, H_, W_, precision)
            ws, status = torch.zeros(size, dtype=torch.uint8, device=device), _status(device, 0)
            chunk, clean = U.head_forward_ex2(_head("clean", device), fm, precision, ws, status, conv2_freq)
            ws, status = torch.zeros(size, dtype=torch.uint8, device=device), _status(device, 0)
            chunk, outs = U.head_forward_ex2(head, fm, precision, ws, status, conv2_freq)
            assert chunk == Bc
            loc, cls, corners = [t.cpu() for t in outs]
            missing = [int((torch.isnan(r) & ~torch.isnan(g)).sum()) for r, g in ((ref_loc, loc), (ref_corners, corners))]
            nan_classes = [sorted(set(torch.isnan(t).any(dim=4).any(dim=3).any(dim=2).nonzero()[:, 1].tolist())) for t in (loc, cls, corners)]
            lines.append("CLASS {} conv2_freq={} Bc={} poison {} at {}: reference NaNs the device leaves finite: loc {} corners {}; status {}; "
                         "words {}; classes with NaN (loc, cls, corners): {}".format(precision, conv2_freq, Bc, kind[0], kind[1], missing[0], missing[1],
                                                                                  int(status.item()), _words(ws), nan_classes))
            print(lines[-1])
            assert missing == [0, 0], lines[-1]
            assert int(status.item()) == 1, lines[-1]
            for t, t0 in zip(outs, clean):
                t, t0 = t.cpu(), t0.cpu()
                keep = ~torch.isnan(t)
                assert torch.equal(t.view(torch.int32)[keep], t0.view(torch.int32)[keep]), "a finite output differs from the clean call"
    return lines


@pytest.mark.parametrize("precision,conv2_freq", ROUTES, ids=ROUTE_IDS)
def test_non_finite_class_operand_poisons_its_class(device, precision, conv2_freq):
    """A NaN or an Inf in a CLASS feature map (through os2d_class_prepare_batch and os2d_class_split, which the head's constructor
    runs): the reference gives all-NaN loc and corners for that class on every image.  The correlation epilogue's fmaxf dropped a
    NaN row from the norm (only an Inf row was flagged) and the 7x7 layer saw a zero channel: finite loc and corners, no status."""
    with torch.no_grad():
        _class_operand(device, precision, conv2_freq)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dev_ = torch.device("cuda")
    with torch.no_grad():
        for (p_, c2_) in ROUTES:
            for line_ in _protocol(dev_, p_, c2_):
                print(line_)
            _class_operand(dev_, p_, c2_)
    print("ok")
