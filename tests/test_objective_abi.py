"""CPU: the target-assignment and objective entry points of libos2d_train.so refuse bad arguments before anything is
launched, none of their kernels spills or uses scratch memory, and objective.hip holds no float atomicAdd (its sums are
reduced in a fixed order)."""
import ctypes
import os
import re

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SOURCE = os.path.join(REPO, "os2d_amd", "csrc_train", "objective.hip")
KERNELS = ("assign_targets_kernel", "objective_elements_kernel", "mining_histogram_kernel", "mining_ties_kernel", "mining_scan_kernel",
           "mining_select_kernel", "rll_weight_sums_kernel", "rll_normalise_kernel", "rll_elements_kernel", "objective_finalise_kernel",
           "objective_backward_kernel")


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import build, _train_lib
    build.build_train(verbose=False)
    assert "objective.hip" in build.TRAIN_SOURCES and "objective.hip" not in build.SOURCES
    return _train_lib.load()


def err(lib):
    return lib.os2d_train_last_error()


def test_abi_version_is_2(lib):
    from os2d_amd import _train_lib
    assert lib.os2d_train_abi_version() == _train_lib.ABI_VERSION == 2
    assert "#define OS2D_TRAIN_ABI_VERSION 2" in open(os.path.join(REPO, "include", "os2d_train.h")).read()


def test_assign_targets_refuses_bad_arguments(lib):
    fake = ctypes.c_void_p(256)         # never dereferenced: every call below is refused by its argument checks
    f = ctypes.c_float

    def call(mode=0, gt=fake, offsets=fake, n=3, loc_scores=fake, A=2, B=5, H=9, W=13, stride=16, loc_t=fake, cls_t=fake, ia=fake, ic=fake):
        return lib.os2d_train_assign_targets(mode, gt, gt, gt, offsets, n, loc_scores, A, B, H, W, stride, 16, f(0.5), f(0.1), loc_t, cls_t,
                                             ia, ic, None)
    assert call(mode=2) == -1 and b"mode" in err(lib)
    assert call(A=0) == -1 and b"shape" in err(lib)
    assert call(H=0) == -1 and b"shape" in err(lib)
    assert call(stride=0) == -1 and b"stride" in err(lib)
    assert call(n=-1) == -1
    assert call(gt=None) == -1 and b"null" in err(lib)
    assert call(offsets=None) == -1 and b"null" in err(lib)
    assert call(cls_t=None) == -1 and b"null" in err(lib)
    assert call(mode=0, loc_t=None) == -1 and b"null" in err(lib)
    assert call(mode=1, loc_scores=None) == -1 and b"null" in err(lib)
    assert call(mode=1, ic=None) == -1 and b"null" in err(lib)


def test_objective_refuses_bad_arguments(lib):
    fake = ctypes.c_void_p(256)
    f, d = ctypes.c_float, ctypes.c_double
    need = lib.os2d_train_objective_workspace_floats(2, 5, 117)
    assert need > 0 and lib.os2d_train_objective_workspace_floats(0, 5, 117) == 0

    def fwd(kind=0, loc=fake, cls_t=fake, A=2, B=5, HW=117, losses=fake, flags=fake, ws=fake, ws_floats=need, ratio=3.0, rll=0.001):
        return lib.os2d_train_objective_forward(kind, 0, loc, fake, fake, cls_t, None, None, A, B, HW, f(0.5), f(0.6), f(1.0), f(0.2), f(ratio),
                                                d(rll), losses, fake, None, flags, fake, ws, ws_floats, None)
    assert fwd(kind=2) == -1 and b"class loss" in err(lib)
    assert fwd(HW=0) == -1 and b"shape" in err(lib)
    assert fwd(B=0) == -1 and b"shape" in err(lib)
    assert fwd(loc=None) == -1 and b"null" in err(lib)
    assert fwd(cls_t=None) == -1 and b"null" in err(lib)
    assert fwd(losses=None) == -1 and b"null" in err(lib)
    assert fwd(flags=None) == -1 and b"null" in err(lib)
    assert fwd(ws=None) == -1 and b"null" in err(lib)
    assert fwd(ws_floats=need - 1) == -2 and b"workspace" in err(lib)
    assert fwd(ratio=-1.0) == -1 and b"neg_to_pos_ratio" in err(lib)
    assert fwd(kind=1, rll=0.0) == -1 and b"rll_neg_weight_ratio" in err(lib)

    def bwd(g=fake, flags=fake, loc=fake, A=2, HW=117, dloc=fake, dcls=fake):
        return lib.os2d_train_objective_backward(g, loc, fake, flags, fake, fake, A, 5, HW, f(1.0), f(0.2), dloc, dcls, None, None)
    assert bwd(g=None) == -1 and b"null" in err(lib)
    assert bwd(flags=None) == -1 and b"null" in err(lib)
    assert bwd(loc=None) == -1 and b"null" in err(lib)
    assert bwd(A=0) == -1 and b"shape" in err(lib)
    assert bwd(dloc=None, dcls=None) == -1 and b"gradient" in err(lib)


def test_objective_kernels_do_not_spill(lib):
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    ks = codeobj.kernels(build.TRAIN_LIB_PATH)
    for name in KERNELS:
        mine = {n: k for n, k in ks.items() if name in n}
        assert mine, name
        bad = {n: k for n, k in mine.items() if k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]}
        assert not bad, bad


def test_no_float_atomic_add_in_the_objective_source():
    text = open(SOURCE).read()
    code = re.sub(r"//[^\n]*", "", text)
    # the only atomicAdd targets are the unsigned counters and histograms; atomicMax works on float BIT PATTERNS (order-free)
    for m in re.finditer(r"atomicAdd\s*\(([^;]*);", code):
        args = m.group(1)
        assert "1u" in args or "hist[tid]" in args or re.search(r"&ws\[W_CNT \+ \d\], n", args), args
    assert not re.search(r"atomicAdd\s*\(\s*(reinterpret_cast<float|\(float)", code)
    assert "unsafeAtomicAdd" not in code and "atomicAdd_system" not in code
    from os2d_amd import build
    assert "-ffp-contract=off" in build.unit_flags(build.TRAIN, "objective.hip")
