"""CPU: the model of the split-half blocked layout (tests/train_forward_f16x3_model.py) is consistent with itself and with the
plane geometry the library reports, the switch of the split-fp16 training forward resolves as documented, and
os2d_train_planes_from_shb refuses bad arguments before anything is launched and has a kernel without spills."""
import ctypes

import numpy as np
import pytest

import train_forward_f16x3_model as M

SHAPES = [(2, 2), (3, 5), (17, 19), (2, 209), (38, 38), (10, 12), (9, 13)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_plane_indexing_restates_the_library(H, W):
    """os2d_plane_floats comes from the built library (a host function: no device needed); os2d_interior is restated operation
    for operation in the model and must select exactly the H x W cells BASE + h * WS + w."""
    from os2d_amd import _lib
    PL = M.plane(H, W)
    assert PL == int(_lib.load().os2d_plane_floats(H, W)) and PL % 64 == 0
    by_predicate = np.array([M.interior(n, H, W) for n in range(PL)])
    assert np.array_equal(by_predicate, M.interior_mask(H, W)) and int(by_predicate.sum()) == H * W
    idx = M.plane_index(H, W)
    assert idx[0] == M.base(W) and idx[-1] == M.base(W) + (H - 1) * M.ws(W) + W - 1 < PL
    assert M.base(W) % 4 == 0 and M.base(W) >= 3 * M.ws(W) + 3 and PL >= M.base(W) + (H + 3) * M.ws(W) + 3


def _split_values(rs, shape, exp):
    """fp32 values that ARE hi + lo of a split at the channel's exponent: random magnitudes over the fp16 range, some zeros,
    some so small that the lo half is subnormal or vanishes."""
    C = shape[1]
    v = (rs.standard_normal(shape) * 10.0 ** rs.uniform(-7, 4, size=shape)).astype(np.float32)
    v[rs.uniform(size=shape) < 0.05] = 0.0
    hi, lo = M.split(v)
    return np.ldexp(hi.astype(np.float64) + lo.astype(np.float64), -np.asarray(exp).reshape(1, C, 1, 1))


@pytest.mark.parametrize("NB,C,H,W", [(1, 1, 2, 2), (2, 9, 3, 5), (2, 17, 9, 13)])
def test_pack_then_unpack_is_the_identity_for_split_values(NB, C, H, W):
    rs = np.random.RandomState(C * 100 + H)
    exp = rs.randint(-20, 31, size=C)
    exp[0] = 0
    x = _split_values(rs, (NB, C, H, W), exp)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)          # 24 bits: an fp32 value
    shb = M.pack(x.astype(np.float32), exp)
    assert shb.shape == (NB, M.groups(C), 2, M.plane(H, W), 8)
    assert np.array_equal(M.unpack_interior(shb, exp, C, H, W, np.float64), x)
    # the fp32 arithmetic of the kernel gives the same values, and zeros everywhere else
    p32 = M.unpack(shb, exp, C, C + 1, H, W, np.float32)
    assert np.array_equal(p32[:, :C, M.plane_index(H, W)].reshape(NB, C, H, W).astype(np.float64), x)
    assert not p32[:, :, ~M.interior_mask(H, W)].any() and not p32[:, C].any()


def test_unpack_ignores_what_pad_cells_and_padded_channels_hold():
    NB, C, H, W = 2, 9, 3, 5
    rs = np.random.RandomState(5)
    exp = rs.randint(-20, 31, size=C)
    shb = M.pack(_split_values(rs, (NB, C, H, W), exp).astype(np.float32), exp)
    dirty = shb.copy()
    dirty.view(np.uint16)[:, :, :, ~M.interior_mask(H, W), :] = 0xFFFF
    dirty.view(np.uint16)[:, 1, :, :, 1:] = 0xFFFF                              # channels 9 .. 15 of the last group
    a, b = M.unpack(shb, exp, C, C + 2, H, W), M.unpack(dirty, exp, C, C + 2, H, W)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_resolve_train_forward_precision(monkeypatch):
    from os2d_amd.modeling import head_train as T
    monkeypatch.delenv("OS2D_TRAIN_FORWARD_PRECISION", raising=False)
    monkeypatch.delenv("OS2D_TRAIN_PRECISION", raising=False)
    assert T.resolve_train_forward_precision() == T.resolve_train_forward_precision(None) == "f32" == T.DEFAULT_TRAIN_FORWARD_PRECISION
    assert T.resolve_train_forward_precision("f16x3") == "f16x3"
    monkeypatch.setenv("OS2D_TRAIN_FORWARD_PRECISION", "f16x3")
    assert T.resolve_train_forward_precision() == "f16x3"                     # the environment beats the default
    assert T.resolve_train_forward_precision("f32") == "f32"                  # the attribute beats the environment
    assert T.resolve_train_precision() == "f32"                               # ... and does not reach the backward's switch
    monkeypatch.setenv("OS2D_TRAIN_FORWARD_PRECISION", "fp8")
    with pytest.raises(ValueError, match="train_forward_precision"):
        T.resolve_train_forward_precision()
    assert T.resolve_train_forward_precision("f32") == "f32"
    with pytest.raises(ValueError, match="fftx3"):
        T.resolve_train_forward_precision("fftx3")
    # independent of train_precision, both ways
    monkeypatch.delenv("OS2D_TRAIN_FORWARD_PRECISION")
    monkeypatch.setenv("OS2D_TRAIN_PRECISION", "f16x3")
    assert T.resolve_train_forward_precision() == "f32" and T.resolve_train_precision() == "f16x3"


def test_planes_from_shb_refuses_bad_arguments_before_launch():
    from os2d_amd import _train_lib
    lib = _train_lib.load()
    fake = ctypes.c_void_p(256)      # never dereferenced: every call below is refused by its argument checks

    def call(shb=fake, exp=fake, NB=2, channels=9, out_channels=9, H=3, W=5, planes=fake):
        return lib.os2d_train_planes_from_shb(shb, exp, NB, channels, out_channels, H, W, planes, None)

    for kw in (dict(shb=None), dict(exp=None), dict(planes=None)):
        assert call(**kw) == -1 and b"os2d_train_planes_from_shb: null pointer" in lib.os2d_train_last_error()
    for kw, text in ((dict(out_channels=8), b"out_channels=8"), (dict(H=0), b"H=0"), (dict(W=0), b"W=0"), (dict(NB=0), b"NB=0"),
                     (dict(channels=0, out_channels=0), b"channels=0"), (dict(W=3601), b"W=3601")):
        assert call(**kw) == -1 and text in lib.os2d_train_last_error(), kw
    assert call(NB=2260, channels=225, out_channels=226) == -1 and b"65535" in lib.os2d_train_last_error()   # 2260 * 29 = 65540 rows
    assert call(shb=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.os2d_train_last_error()
    assert call(planes=ctypes.c_void_p(260)) == -1 and b"aligned" in lib.os2d_train_last_error()


def test_bridge_kernel_has_no_spills_scratch_or_lds():
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    build.build(verbose=False)
    ks = {n: k for n, k in codeobj.kernels(build.TRAIN_LIB_PATH).items() if "planes_from_shb_kernel" in n}
    assert len(ks) == 1
    (k,) = ks.values()
    assert not (k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"] or k["lds_bytes"]), k
