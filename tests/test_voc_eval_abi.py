"""CPU: libos2d_eval.so has ABI version 1, refuses bad arguments before anything is launched, its kernels are a listed set
without scratch or spills, and its source holds no floating-point atomic.  (Header, binding, exports, flags and sources:
test_native_libs.py.)"""
import ctypes
import os
import re

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KERNELS = ("count_gt_kernel", "match_kernel", "resolve_kernel", "sort_init_kernel", "gather_labels_kernel", "radix_hist_kernel",
           "radix_scan_kernel", "radix_scatter_kernel", "class_offsets_kernel", "scan_partials_kernel", "scan_carries_kernel",
           "scan_apply_kernel", "ap11_kernel", "finalise_kernel")


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import build, _eval_lib
    build.build_eval(verbose=False)
    return _eval_lib.load()



def test_abi_version_is_1(lib):
    from os2d_amd import _eval_lib
    assert lib.os2d_eval_abi_version() == _eval_lib.ABI_VERSION == 1
    assert "#define OS2D_EVAL_ABI_VERSION 1" in open(os.path.join(REPO, "include", "os2d_eval.h")).read()



def test_entry_points_refuse_bad_arguments(lib):
    fake = ctypes.c_void_p(256)         # never dereferenced: every call below is refused by its argument checks
    err = lib.os2d_eval_last_error
    f = ctypes.c_float
    assert lib.os2d_eval_count_gt(fake, fake, 3, 0, fake, fake, None) == -1 and b"shape" in err()
    assert lib.os2d_eval_count_gt(None, fake, 3, 4, fake, fake, None) == -1 and b"null" in err()
    assert lib.os2d_eval_match(fake, fake, fake, fake, 5, 0, fake, fake, fake, fake, 2, f(0.5), fake, fake, fake, None) == -1 and b"shape" in err()
    assert lib.os2d_eval_match(fake, fake, fake, None, 5, 1, fake, fake, fake, fake, 2, f(0.5), fake, fake, fake, None) == -1 and b"null" in err()
    assert lib.os2d_eval_match(None, fake, fake, fake, 5, 1, fake, fake, fake, fake, 2, f(0.5), fake, fake, fake, None) == -1 and b"null" in err()
    assert lib.os2d_eval_match(ctypes.c_void_p(260), fake, fake, fake, 5, 1, fake, fake, fake, fake, 2, f(0.5), fake, fake, fake, None) == -1 \
        and b"aligned" in err()
    need = lib.os2d_eval_sort_workspace_bytes(5000)
    assert need > 0 and lib.os2d_eval_sort_workspace_bytes(0) == 0
    assert lib.os2d_eval_sort(fake, fake, 5000, 1024, 8, fake, fake, fake, fake, fake, need, None) == -1 and b"label_bits" in err()
    assert lib.os2d_eval_sort(fake, fake, 5000, 1024, 10, fake, None, fake, fake, fake, need, None) == -1 and b"null" in err()
    assert lib.os2d_eval_sort(fake, fake, 5000, 1024, 10, fake, fake, fake, fake, fake, need - 1, None) == -2 and b"workspace" in err()
    scan = lib.os2d_eval_scan_workspace_bytes(5000)
    assert scan > 0
    assert lib.os2d_eval_prec_rec(fake, fake, None, fake, 0, 5000, None, fake, fake, fake, fake, scan, None) == -1 and b"shape" in err()
    assert lib.os2d_eval_prec_rec(fake, None, None, fake, 4, 5000, None, fake, fake, fake, fake, scan, None) == -1 and b"null" in err()
    assert lib.os2d_eval_prec_rec(fake, fake, None, fake, 4, 5000, None, fake, fake, fake, fake, scan - 1, None) == -2 and b"workspace" in err()
    assert lib.os2d_eval_ap(fake, fake, None, 4, 5000, 0, None, fake, fake, scan, None) == -1 and b"null" in err()
    assert lib.os2d_eval_ap(fake, fake, None, 4, 5000, 0, fake, fake, fake, 0, None) == -2 and b"workspace" in err()
    assert lib.os2d_eval_finalise(fake, fake, fake, 0, 0, fake, fake, fake, fake, None) == -1 and b"shape" in err()
    assert lib.os2d_eval_finalise(fake, fake, None, 4, 0, fake, fake, fake, fake, None) == -1 and b"null" in err()


def test_kernels_are_the_listed_set_and_do_not_spill(lib):
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    ks = codeobj.kernels(build.EVAL_LIB_PATH)
    assert ks
    for n, k in ks.items():
        assert any(name in n for name in KERNELS), n
        assert not (k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]), (n, k)
    for name in KERNELS:
        assert any(name in n for n in ks), name


def test_no_float_atomic_in_the_sources():
    from os2d_amd import build
    for s in build.EVAL_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(os.path.join(build.EVAL_CSRC, s)).read())
        for m in re.finditer(r"atomic(Add|Min)\s*\(([^;]*);", code):
            args = m.group(2)
            assert ("1u" in args or ", 1)" in args) if m.group(1) == "Add" else "winner" in args, args
        assert not re.search(r"atomic(Max|Exch|CAS|Sub|Or|And)\s*\(", code)
        assert "unsafeAtomicAdd" not in code and "atomicAdd_system" not in code
        assert not re.search(r"atomicAdd\s*\(\s*(reinterpret_cast<(float|double)|\((float|double))", code)
