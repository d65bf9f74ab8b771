"""CPU: libos2d_image.so has ABI version 1, refuses bad arguments before anything is launched, and its kernels are a listed
set without scratch or spills, atomics or inline assembly.  (Header, binding, exports, flags and sources: test_native_libs.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KERNELS = ("resample_kernel",)


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import build, _image_lib
    build.build_image(verbose=False)
    return _image_lib.load()


def test_header_and_binding_agree_on_the_argument_count_of_resample():
    """(the one entry point with many)"""
    from os2d_amd import _image_lib
    header = open(os.path.join(REPO, "include", "os2d_image.h")).read()
    decl = re.search(r"int os2d_image_resample\((.*?)\);", header, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_image_lib.SIGNATURES["os2d_image_resample"][1]) == 26


def test_abi_version_is_1(lib):
    from os2d_amd import _image_lib
    assert lib.os2d_image_abi_version() == _image_lib.ABI_VERSION == 1
    assert "#define OS2D_IMAGE_ABI_VERSION 1" in open(os.path.join(REPO, "include", "os2d_image.h")).read()



def _call(lib, fake, **over):
    """os2d_image_resample on a 64x48 image resized to 32x24 with every pointer `fake`, one argument replaced at a time"""
    a = dict(src=fake, A=1, img_w=64, img_h=48, row_pitch=192, image_stride=192 * 48, x0=0, y0=0, w=64, h=48, hflip=0, vflip=0,
             xcoef=fake, xbounds=fake, xbounds_host=fake, kx=5, ycoef=fake, ybounds=fake, ybounds_host=fake, ky=5, ow=32, oh=24,
             lut=fake, out=fake, out_u8=0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.os2d_image_resample(*a.values())


def test_entry_point_refuses_bad_arguments(lib):
    fake = ctypes.c_void_p(256)         # never dereferenced: every call below is refused by the checks before the tables are read
    err = lib.os2d_image_last_error
    for name in ("src", "xcoef", "xbounds", "xbounds_host", "ycoef", "ybounds", "ybounds_host", "out", "lut"):
        assert _call(lib, fake, **{name: None}) == -1 and b"null" in err(), name
    assert _call(lib, fake, out=ctypes.c_void_p(264)) == -1 and b"aligned" in err()         # float rows are stored as 16-byte units
    assert _call(lib, fake, ycoef=ctypes.c_void_p(258)) == -1 and b"aligned" in err()
    assert _call(lib, fake, lut=ctypes.c_void_p(257)) == -1 and b"aligned" in err()
    for bad in (dict(A=0), dict(ow=0), dict(oh=-1), dict(kx=0), dict(w=0), dict(row_pitch=191), dict(A=2, image_stride=192 * 48 - 1)):
        assert _call(lib, fake, **bad) == -1 and b"shape" in err(), bad
    for bad in (dict(x0=-1), dict(x0=1), dict(y0=1), dict(w=65), dict(x0=60, w=5), dict(y0=40, h=9), dict(img_w=63, row_pitch=192)):
        assert _call(lib, fake, **bad) == -1 and b"window" in err(), bad
    for bad in (dict(ow=3), dict(oh=2), dict(w=2, ow=33), dict(h=1, oh=17)):
        assert _call(lib, fake, **bad) == -1 and b"ratio" in err(), bad
    # tables whose taps leave the window are refused from the host copy (read only now; nothing is launched)
    ok = np.stack([np.arange(32) * 2, np.full(32, 2)], 1).astype(np.int32)
    yok = np.ascontiguousarray(ok[:24])
    for xb in (ok + np.array([1, 0], np.int32), ok - np.array([1, 0], np.int32), ok * np.array([1, 0], np.int32), ok + np.array([0, 4], np.int32)):
        xb = np.ascontiguousarray(xb)
        assert _call(lib, fake, xbounds_host=ctypes.c_void_p(xb.ctypes.data), ybounds_host=ctypes.c_void_p(yok.ctypes.data)) == -1
        assert b"bounds" in err()
    # a tile's staged rows must fit in LDS: 200 taps per output row never do
    wide = np.stack([np.zeros(24), np.full(24, 200)], 1).astype(np.int32)
    assert _call(lib, fake, img_h=240, image_stride=192 * 240, h=240, ky=200, xbounds_host=ctypes.c_void_p(ok.ctypes.data),
                 ybounds_host=ctypes.c_void_p(wide.ctypes.data)) == -1 and b"LDS" in err()


def test_kernels_are_the_listed_set_and_do_not_spill(lib):
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    ks = codeobj.kernels(build.IMAGE_LIB_PATH)
    assert len(ks) == 2                     # float planes and uint8 HWC
    for n, k in ks.items():
        assert any(name in n for name in KERNELS), n
        assert not (k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]), (n, k)
    for name in KERNELS:
        assert any(name in n for n in ks), name


def test_no_atomics_and_no_inline_assembly_in_the_sources():
    from os2d_amd import build
    for s in build.IMAGE_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(os.path.join(build.IMAGE_CSRC, s)).read())
        assert not re.search(r"atomic\w*\s*\(", code) and "asm" not in code
