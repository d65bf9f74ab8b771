"""CPU: the range-flag cases of tests/range_flag_cases.py held to their own statements by a float64 model of each stage - the
intended cells land where the case says, exactly (threshold cases: in the float32 arithmetic of the packing kernel) or with the
stated margin (single cells) - and the workspace zero-fill of os2d_amd/modeling/device_buffers.py.  No kernel runs here;
tests/test_range_flag_stages_gpu.py runs them on the same cases."""
import numpy as np
import pytest
import torch

import freq_util
import range_flag_cases as RC

FP16_MAX = RC.FP16_MAX


def model_raises(pre, stored):
    """The kernels' predicate over the cells they store: a NaN pre-activation, or a stored value not within the fp16 range."""
    return bool((torch.isnan(pre) | ~(stored.abs() <= FP16_MAX)).any())


def test_margin_comes_from_the_pins():
    import test_forward_matrix_gpu as G
    m = RC.margin()
    worst = max(G.PIN["conv1_f16x3"], G.PIN["conv2_f16x3"])
    assert m == 2.0 ** -10 and 100.0 * worst < m <= 200.0 * worst
    # the transforms are held to 2e-6 of the largest sample (tests/test_dft_gpu.py, tests/test_spectral_gpu.py): further still
    assert m > 200 * 2e-6
    # the values the single-cell cases rest on are exact: fp32, fp16 hi + lo, and doubled
    for x in (np.float32(32752.0 * (1 + m)), np.float32(32752.0 * (1 - m))):
        hi, lo = RC.SHB.split(x)
        assert float(hi) + float(lo) == float(x) and float(x) in (32752.0 * (1 + m), 32752.0 * (1 - m))
    assert 2 * 32752.0 * (1 + m) == FP16_MAX * (1 + m) > FP16_MAX > FP16_MAX * (1 - m)


@pytest.mark.parametrize("layer,terms,shape", RC.CONV_GROUPS, ids=["L{}-terms{}-{}x{}".format(l, t, *s) for l, t, s in RC.CONV_GROUPS])
def test_conv_cases(layer, terms, shape):
    H, W = shape
    m = RC.margin()
    cases = RC.conv_cases(layer, terms, shape)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for want in ("first", "last", "row_end"):
        assert "cell_hi_" + want in names and "cell_lo_" + want in names
    assert any("seam" in n for n in names) and {"at_max", "nan_pre", "pad_cell"} <= set(names)
    for case in cases:
        pre, stored = RC.conv_stored_model(case)
        assert model_raises(pre, stored) == case.raises, case.name
        assert (case.fixed is not None) == case.raises and (case.clean is not None) == case.raises
        if case.raises:
            assert not case.fixed.raises
            fpre, fstored = RC.conv_stored_model(case.fixed)
            clean = torch.from_numpy(case.clean)
            # every offending cell is outside ``clean``, the clean cells are finite, in range and the same in the twin
            bad = torch.isnan(pre) | ~(stored.abs() <= FP16_MAX)
            assert not bool((bad & clean).any()), case.name
            assert torch.equal(stored[clean], fstored[clean]), case.name
            assert bool(clean[0].any()) and bool(clean[1].any())
        if case.name in ("at_max",) or case.name.startswith("next_above"):
            # exact in the float32 arithmetic of the fold (prep.hip) and of the epilogue, for every channel
            bias, unscale, oscale, st32 = RC.conv_fold_f32(case)
            assert np.array_equal(bias, case.b) and np.all(unscale == 1.0)
            over = st32 > np.float32(FP16_MAX)
            if case.name == "at_max":
                assert np.all(st32 == np.float32(FP16_MAX))
            else:
                o = int(case.name.split("_o")[1])
                assert over[o] and over.sum() == 1 and float(st32[o]) == RC.next_above(FP16_MAX) and np.all(st32[~over] == np.float32(FP16_MAX))
            assert float(stored.min()) == float(st32.min()) and float(stored.max()) == float(st32.max())       # float64 agrees
        if case.name.startswith("cell_"):
            label = case.name[len("cell_hi_"):]
            h, w = RC.conv_positions(layer, H, W)[label]
            x1 = case.x[1, :, h, w]
            o = int(np.argmax(np.abs(x1 - case.fixed.x[1, :, h, w]))) if case.raises else None
            top = float(stored.max())
            if case.raises:
                assert float(stored[1, o, h, w]) == FP16_MAX * (1 + m) == top
                rest = stored.clone()
                rest[1, o, h, w] = 0
                assert float(rest.max()) <= FP16_MAX * (1 - m)
            else:
                assert top == FP16_MAX * (1 - m)
        if case.name == "nan_pre":
            nb, c, h, w = case.nan_at
            assert bool(torch.isnan(pre[nb, :, h, w]).all()) and float(case.b.max()) < 0
            assert not bool(torch.isnan(RC.conv_stored_model(case.fixed)[0]).any())
        if case.name.startswith("neg_inf"):
            o = int(case.name.split("_o")[1])
            assert bool((pre[:, o] == -np.inf).all()) and bool((stored[:, o] == 0).all())
        if case.name.startswith("pos_inf"):
            o = int(case.name.split("_o")[1])
            assert bool((pre[:, o] == np.inf).all())
        if case.name == "pad_cell":
            nb, c, h, w, v = case.pad_at
            _, full = RC.conv_stored_model(case, with_pads=True)
            assert float(full[nb, c, h, w]) == FP16_MAX * (1 + m) and float(full[..., :W].max()) <= FP16_MAX * (1 - m)


def test_conv_positions_cover_the_tile_geometry():
    """The position tables against the kernels' geometry, stated on its own.  Linear maps: plane cells from the first data cell in
    tiles of 128 - the shape that runs at NB = 2 - and the cells where the 256-cell shape WOULD cut (it takes 384 work-groups: not
    run here).  Strips (W = 317: two strips of 160 output columns, strip-plane pitch 164, the 256-cell shape): 1 x 317 is one
    partial tile per strip, strip-plane index 128 a wave boundary inside it; 2 x 317 has 328 cells per strip, two tiles, the seam
    at strip-plane index 256 = row 1, strip column 92."""
    p = RC.conv_positions(1, 9, 14)                      # Ws = 17: cell 127 = (7, 8), 128 = (7, 9); 153 cells: one seam, a partial tile
    assert p["tile128_seam1_l"] == (7, 8) and p["tile128_seam1_r"] == (7, 9) and not any(k.startswith("tile256") for k in p)
    p = RC.conv_positions(2, 17, 13)                     # Ws = 16: cells 127 / 128 are (7, 15) - a pad cell - and (8, 0)
    assert p["tile128_seam1_l"] == (7, 12) and p["tile128_seam1_r"] == (8, 0)
    assert p["tile256_seam1_l"] == (15, 12) and p["tile256_seam1_r"] == (16, 0) and p["tile128_seam2_r"] == (16, 0)
    p = RC.conv_positions(2, 1, 317)
    assert p["strip_seam_l"] == (0, 159) and p["strip_seam_r"] == (0, 160) and p["last"] == (0, 316)
    assert p["strip0_wave_r"] == (0, 126) and p["strip1_wave_r"] == (0, 286) and not any("tile_seam" in k for k in p)
    p = RC.conv_positions(2, 2, 317)
    assert p["strip0_tile_seam_l"] == (1, 89) and p["strip0_tile_seam_r"] == (1, 90)
    assert p["strip1_tile_seam_l"] == (1, 249) and p["strip1_tile_seam_r"] == (1, 250) and p["last"] == (1, 316)


def _plans(shape):
    """The plans of the library's own host functions (no GPU needed; a library that does not load or a refused plan FAILS)."""
    P, Q, nbins = freq_util.fft_sizes(*shape)
    TY, TX, TH, TW = freq_util.fft_tiles(*shape)
    dP, dQ, dn, (dTY, dTX, dTH, dTW, _, _) = freq_util.dft_sizes(*shape)
    return {"fft": RC.Plan(P, Q, nbins, TY, TX, TH, TW, False), "dft": RC.Plan(dP, dQ, dn, dTY, dTX, dTH, dTW, True)}


@pytest.mark.parametrize("shape", RC.TRANSFORM_SHAPES, ids=["{}x{}".format(*s) for s in RC.TRANSFORM_SHAPES])
@pytest.mark.parametrize("kind", ["fft", "dft"])
def test_transform_cases(kind, shape):
    """(The transform plans are the library's own host functions: no GPU needed.)"""
    H, W = shape
    m = RC.margin()
    plan = _plans(shape)[kind]
    if shape == (5, 212) and kind == "dft":        # (the in-LDS FFT takes 5 x 212 whole: one long Stockham transform)
        assert plan.TX > 1, "5 x 212 is there for the tiled route"
    cases = RC.transform_cases("dft" if kind == "dft" else "fft_rows", shape, plan)
    names = [c.name for c in cases]
    assert {"over_first", "over_last", "over_row_end", "nan_pre", "overhang"} <= set(names)
    assert (plan.TX == 1) or {"over_tile_x1_l", "over_tile_x1_r", "over_last_tile_first"} <= set(names)
    tol = 1e-5                                     # float64 transforms of complex64 spectra: 1e-7; far inside the margin
    for case in cases:
        pre, stored, outside = RC.transform_stored_model(case)
        assert model_raises(pre, stored) == case.raises, case.name
        if case.raises:
            assert not case.fixed.raises
            bad = torch.isnan(pre) | ~(stored.abs() <= FP16_MAX)
            assert not bool((bad & torch.from_numpy(case.clean)).any()), case.name
        finite = torch.nan_to_num(stored, nan=0.0, posinf=0.0)
        if case.name.startswith("over_") or case.name.startswith("under_"):
            nb, t, o, hwin, wwin, a = case.special
            label = case.name.split("_", 1)[1]
            h, w = RC.transform_positions(plan, H, W)[label]
            assert abs(float(stored[nb, o, h, w]) / a - 1) < tol and a == FP16_MAX * (1 + m if case.raises else 1 - m)
            rest = finite.clone()
            rest[nb, o, h, w] = 0
            assert float(rest.max()) <= FP16_MAX * (1 - m) * (1 + tol)
        elif case.name == "overhang":
            assert outside >= FP16_MAX * (1 + m) * (1 - tol) and float(finite.max()) <= FP16_MAX * (1 - m) * (1 + tol)
        else:
            assert outside <= FP16_MAX * (1 - m) * (1 + tol)
        if case.name == "nan_pre":
            nb, t, o, b = case.nan_bin
            assert bool(torch.isnan(pre[nb, o]).any()) and case.bias[o] < 0 and not bool(torch.isnan(pre[:, :o]).any())


# ------------------------------------------------------------------------------------------------ the workspace zero-fill
def test_new_workspace_is_zero_filled_over_the_range_words_of_any_batch(monkeypatch):
    """A head call keeps A + 1 range words at the start of its workspace and a NEW workspace must hold zeros there
    (include/os2d_hip.h).  The fixed 4096 bytes covered A <= 1023: the fill now follows the call's A."""
    from os2d_amd.modeling import device_buffers as DB
    assert DB.range_words_bytes(0) == 4096 == DB.range_words_bytes(1023) and DB.range_words_bytes(1024) == 4100
    assert DB.range_words_bytes(5000) == 20004
    monkeypatch.setattr(DB.torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 7})())
    monkeypatch.setattr(DB.torch.cuda, "current_device", lambda: 0)
    real_empty = torch.empty
    monkeypatch.setattr(DB.torch, "empty", lambda n, dtype, device: real_empty(n, dtype=dtype).fill_(0xFF))
    monkeypatch.setattr(DB, "_WORKSPACES", {})
    dev = torch.device("cpu")
    for A, size in ((2, 1 << 16), (1023, 1 << 17), (1024, 1 << 18), (5000, 1 << 19)):
        buf = DB.get_workspace(dev, size, 4 * (A + 1), A)
        n = 4 * (A + 1)
        assert buf.numel() == size and int(buf[:max(n, 4096)].max()) == 0 and int(buf[max(n, 4096):].min()) == 0xFF, A
    # a buffer made for a small batch and REUSED (not grown) for a larger one: the words it was never filled for are zeroed
    # once, and only once (a later call's fill must not wipe what a call in flight may have raised - nor cost a launch per call)
    monkeypatch.setattr(DB, "_WORKSPACES", {})
    buf = DB.get_workspace(dev, 1 << 16, 64, 2)
    buf[4096:] = 0xAA
    same = DB.get_workspace(dev, 1 << 16, 64, 3000)
    assert same is buf and int(buf[:12004].max()) == 0 and int(buf[12004:].min()) == 0xAA
    buf[:12004] = 0x55
    assert DB.get_workspace(dev, 1 << 16, 64, 3000) is buf and DB.get_workspace(dev, 1 << 16, 64, 7) is buf
    assert int(buf[:12004].min()) == 0x55
    # a minimum smaller than the fill (a tiny workspace) is filled whole, not past its end
    monkeypatch.setattr(DB, "_WORKSPACES", {})
    assert int(DB.get_workspace(dev, 64, 64, 3).max()) == 0
