"""CPU: the order-independent d corr scatter of the decode backward (os2d_train_decode_backward_det, include/os2d_train.h) -
the exponent rule against its Python restatement, the float64 / integer model of the rule against the exact model, the refusals
before any launch, and the resources of the new kernels.  (The kernels themselves: tests/test_backward_det_gpu.py.)"""
import ctypes

import pytest
import torch

import backward_det_model as D
import backward_model as M
from test_backward_stages_gpu import PIN

LARGEST = (2048, 1024)        # H W = 2^21: L = 23, the largest admitted
REFUSED = (2049, 1024)


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import _train_lib, build
    build.build(verbose=False)
    return _train_lib.load()


# ---------------------------------------------------------------------------------------------------------- the exponent
WORDS = {"zero": 0, "smallest subnormal": 1, "largest subnormal": 0x007FFFFF, "smallest normal": 0x00800000, "1.0": 0x3F800000,
         "1.5": 0x3FC00000, "just below 2": 0x3FFFFFFF, "2^126": 0x7E800000, "largest finite": 0x7F7FFFFF, "+inf": 0x7F800000,
         "a NaN": 0x7FC00001}
SIZES = [(1, 1), (2, 2), (1, 4), (38, 38), (3, 3), LARGEST, REFUSED, (0, 5)]


def test_exponent_helper_matches_its_restatement_and_keeps_the_headroom(lib):
    """m 2^e lies in [2^(60-L), 2^(61-L)); with floor(log2 m) + 1 for log2 m the sum of 4 H W such values stays at or below
    2^62 (in fact 2^61) for every admitted row."""
    assert [hw[0] * hw[1] for hw in SIZES[:4]] == [1, 4, 4, 1444]
    for H, W in SIZES:
        L = D.log2_addends(H, W)
        for name, bits in WORDS.items():
            e = lib.os2d_train_decode_det_exponent(bits, H, W)
            assert e == D.exponent(bits, H, W), (name, H, W)
            if (H, W) in (REFUSED, (0, 5)):
                assert e == D.DET_REFUSED
            elif bits == 0:
                assert e == D.DET_ZERO
            elif bits >= 0x7F800000:
                assert e == D.DET_NONFINITE
            else:
                fl = D.floor_log2_of_word(bits)
                m = bits * 2.0 ** -149 if bits < 0x00800000 else (1 + (bits & 0x7FFFFF) * 2.0 ** -23) * 2.0 ** ((bits >> 23) - 127)
                assert 2.0 ** fl <= m < 2.0 ** (fl + 1)
                assert 2 ** (fl + 1 + e) * 4 * H * W <= 2 ** 62                # integers: fl + 1 + e = 61 - L >= 38
                assert 60 - L <= fl + e < 61 - L and -90 <= e <= 207
                # one rounding step 2^-e against the largest possible addend m / 121: at most 2^-30
                assert 121 * 2.0 ** -e / m <= 2.0 ** -30
    assert D.log2_addends(*LARGEST) == D.MAX_LOG2 and D.log2_addends(38, 38) == 13 and D.log2_addends(1, 1) == 2
    assert lib.os2d_train_decode_det_exponent(0x3F800000, 38, 38) == 47
    assert lib.os2d_train_decode_det_exponent(1, 1, 1) == 207 and lib.os2d_train_decode_det_exponent(0x7F7FFFFF, *LARGEST) == -90


def test_workspace_size(lib):
    size = lib.os2d_train_decode_backward_det_workspace_bytes
    assert size(2, 38, 38) == D.workspace_bytes(2, 38, 38) == 5198592
    assert size(3, 2, 2) == D.workspace_bytes(3, 2, 2) == (3 * 225 * 4 * 8 + 3 * 4 + 255) // 256 * 256
    assert size(1, *LARGEST) == D.workspace_bytes(1, *LARGEST) and size(1, *LARGEST) % 256 == 0
    assert size(0, 9, 13) == 0 and size(65536, 9, 13) == 0 and size(1, *REFUSED) == 0 and size(1, 0, 13) == 0


# ---------------------------------------------------------------------------------------------------------- the model of the rule
def _check_model(tag, inp, dc, inverse, stride, rec_field):
    NB, _, H, W = inp["corr"].shape
    det = D.decode_det_model(inp["corr"], inp["params"], inp["dcls"], inp["dcls_det"], inverse, stride, rec_field)
    assert all(-90 <= e <= 207 for e in det["e"])
    peak = int(det["acc"].abs().max())
    assert 0 < peak < 2 ** 62
    assert int(det["count"].max()) <= 4 * H * W
    for nb, e in enumerate(det["e"]):
        count = det["count"][nb].double()
        # (1) the grid, with no allowance: quantised against unquantised sums of the SAME float64 addends.  In grid steps the
        # difference is resid, at most half a step per addend (a rule that truncated would reach a whole one) ...
        assert bool((det["resid"][nb].abs() <= 0.5 * count).all()), (tag, nb)
        # ... and the convert pass adds one fp32 rounding of the (exactly represented, < 2^53) integer sum
        quantised = det["acc"][nb].double() * 2.0 ** -e
        assert bool(((det["added"][nb] - quantised).abs() <= quantised.abs() * 2.0 ** -24).all()), (tag, nb)
        # (2) the tap restatement: the plain float64 sum of the unquantised addends against the exact model.  The allowance is
        # the exact model's own float64 error: it samples ONE tall [225 H, W] image (oracle resample_and_pool), normalising
        # y + channel * H (magnitude up to 225 H) to [-1, 1] and grid_sample undoes it: four roundings at that magnitude, so
        # the y coordinate - hence each bilinear weight, hence each addend - is off by up to 4 * 225 H 2^-53 of the largest
        # addend m / 121; one addend more covers the float64 summation of both sides
        m = float((inp["dcls"].float() + inp["dcls_det"].float())[nb].abs().max())
        own = (count + 1) * (m / 121) * 4 * M.K * H * 2.0 ** -53
        diff = (det["taps"][nb] - dc[nb]).abs()
        assert bool((diff <= own).all()), (tag, nb, float((diff - own).max()))
    err = M.rel_err(det["added"], dc)
    print("MODEL decode_dcorr (fixed point) {:<24s} rel_err {:.3e}  largest |sum| 2^{:.1f}  most addends in a cell {}".format(
        tag, err, torch.log2(torch.tensor(float(peak))).item(), int(det["count"].max())))
    # the wide margin below the pin (7.5e-6): one fp32 rounding, 2^-24; the grid adds at most 4 H W half steps of
    # 2^-30 / 121 of the largest addend each (L <= 13 here: 2^-25 of ONE largest addend at the very most)
    assert err < 2.0 ** -23 < PIN["decode_dcorr"] / 50
    return det


@pytest.mark.parametrize("name", sorted(M.DECODE_CASES))
def test_model_of_the_rule_against_the_exact_model(name):
    P, inverse, stride, rec_field = M.DECODE_CASES[name][:4]
    inp, dc, _ = D.case_reference(name)
    _check_model(name, inp, dc, inverse, stride, rec_field)


@pytest.mark.parametrize("inverse", [True, False], ids=["inv", "fwd"])
def test_model_of_the_rule_on_the_hand_placed_locations(inverse):
    """Location 4 has all 121 points clamped: each of the 121 pooled channels piles its whole weight onto one border cell."""
    inp, dc, _ = D.hand_reference(inverse)
    det = _check_model("hand inverse={}".format(inverse), inp, dc, inverse, 16, 16)
    only = {k: v.clone() for k, v in inp.items()}
    keep = torch.zeros(1, 3, 3)
    keep.view(-1)[4] = 1
    only["dcls"], only["dcls_det"] = inp["dcls"] * keep, inp["dcls_det"] * keep
    alone = D.decode_det_model(only["corr"], only["params"], only["dcls"], only["dcls_det"], inverse, 16, 16)
    # x clamped at W - 1 (x0 = x1, ax = 0), y at 0 (ay = 0, y1 = 1): the whole of a channel's weight lands on cell (0, W - 1),
    # the two taps of row 1 carry weight 0
    assert int((alone["acc"] != 0).sum()) == 121 and int((alone["count"] > 0).sum()) == 242 and int(alone["count"].max()) == 2
    assert int((alone["acc"].view(1, M.K, 3, 3)[0, :, 0, 2] != 0).sum()) == 121
    assert 2 ** 47 < int(alone["acc"].abs().max()) < 2 ** 62 and int(det["acc"].abs().max()) < 2 ** 62


# ---------------------------------------------------------------------------------------------------------- refusals, resources
def test_bad_arguments_fail_before_launch(lib):
    fake = ctypes.c_void_p(256)      # never dereferenced: every call below is refused by its argument checks
    f = lib.os2d_train_decode_backward_det
    big = 1 << 40

    def err():
        return lib.os2d_train_last_error()

    for k in (0, 1, 12, 13, 14):     # corr, params, dcorr, dparams, workspace
        args = [fake, fake, None, None, None, 4, 9, 13, 6, 1, 16, 16, fake, fake, fake, big, None]
        args[k] = None
        assert f(*args) == -1 and b"os2d_train_decode_backward_det: null pointer" in err(), k
    assert f(fake, fake, None, None, None, 4, 9, 13, 5, 1, 16, 16, fake, fake, fake, big, None) == -1
    assert b"os2d_train_decode_backward_det" in err() and b"P=5" in err()
    assert f(fake, fake, None, None, None, 65536, 9, 13, 6, 1, 16, 16, fake, fake, fake, big, None) == -3
    assert b"os2d_train_decode_backward_det: NB=65536" in err()
    need = lib.os2d_train_decode_backward_det_workspace_bytes(4, 9, 13)
    assert f(fake, fake, None, None, None, 4, 9, 13, 6, 1, 16, 16, fake, fake, fake, need - 1, None) == -2
    assert b"os2d_train_decode_backward_det: workspace" in err() and str(need).encode() in err()
    assert f(fake, fake, None, None, None, 1, REFUSED[0], REFUSED[1], 6, 1, 16, 16, fake, fake, fake, 1 << 62, None) == -3
    assert b"os2d_train_decode_backward_det" in err() and b"2^-30" in err()
    assert f(fake, fake, None, None, None, 4, 9, 13, 6, 1, 16, 16, fake, fake, ctypes.c_void_p(260), big, None) == -1
    assert b"os2d_train_decode_backward_det" in err() and b"aligned" in err()
    # the float entry point refuses as before, under its own name
    assert lib.os2d_train_decode_backward(fake, fake, None, None, None, 4, 9, 13, 5, 1, 16, 16, fake, fake, None) == -1
    assert err().startswith(b"os2d_train_decode_backward: bad shape")


def test_new_kernels_do_not_spill():
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    build.build(verbose=False)
    ks = codeobj.kernels(build.TRAIN_LIB_PATH)
    mine = {n: k for n, k in ks.items() if "decode_det_max_kernel" in n or "decode_det_convert_kernel" in n or "decode_backward_kernel" in n}
    assert len(mine) == 4, sorted(mine)                      # maxima, convert, and the two instantiations of the shared body
    assert sum("decode_backward_kernelILb1" in n for n in mine) == 1 and sum("decode_backward_kernelILb0" in n for n in mine) == 1
    bad = {n: k for n, k in mine.items() if k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------- the switch (no device)
def test_resolve_deterministic(monkeypatch):
    from os2d_amd.modeling.head_train import resolve_deterministic
    monkeypatch.delenv("OS2D_DETERMINISTIC", raising=False)
    assert not torch.are_deterministic_algorithms_enabled()
    assert resolve_deterministic(None) is False and resolve_deterministic(True) is True and resolve_deterministic(False) is False
    for text, want in (("1", True), ("0", False), ("", False), ("yes", True)):
        monkeypatch.setenv("OS2D_DETERMINISTIC", text)
        assert resolve_deterministic(None) is want and resolve_deterministic(not want) is (not want)
    monkeypatch.delenv("OS2D_DETERMINISTIC")
    torch.use_deterministic_algorithms(True)
    try:
        assert resolve_deterministic(None) is True and resolve_deterministic(False) is False
        monkeypatch.setenv("OS2D_DETERMINISTIC", "0")          # the environment is asked before torch
        assert resolve_deterministic(None) is False
    finally:
        torch.use_deterministic_algorithms(False)
    for bad in ("on", 1, 0.0):
        with pytest.raises(ValueError, match="deterministic"):
            resolve_deterministic(bad)
