"""CPU: libos2d_train.so (the head's backward pass) is built by build(), bad arguments are refused before anything is
launched, and no backward kernel spills or uses scratch memory.  (Header, binding and exports: test_native_libs.py.)"""
import ctypes
import subprocess

import pytest


@pytest.fixture(scope="module")
def lib_path():
    from os2d_amd import build
    build.build(verbose=False)
    assert build.train_up_to_date()
    return build.TRAIN_LIB_PATH




def test_forward_library_is_unchanged_by_the_training_build(lib_path):
    """The backward kernels live in their own library: libos2d_hip.so's sources do not include them."""
    from os2d_amd import build
    assert "train.hip" not in build.SOURCES
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB_PATH]).decode()
    assert "os2d_train_" not in out


def test_bad_arguments_fail_before_launch(lib_path):
    from os2d_amd import _train_lib
    lib = _train_lib.load()
    assert lib.os2d_train_abi_version() == _train_lib.ABI_VERSION
    fake = ctypes.c_void_p(256)      # never dereferenced: every call below is refused by its argument checks
    assert lib.os2d_train_conv_data_workspace_floats(1, 6) == 128 * 225 * 49
    assert lib.os2d_train_conv_data_workspace_floats(3, 4) == 4 * 64 * 25
    assert lib.os2d_train_conv_data_workspace_floats(3, 5) == 0
    assert lib.os2d_train_corr_workspace_floats(2, 64, 9, 13) == 2 * 2 * 117 + 2 * 64 * 117
    rc = lib.os2d_train_decode_backward(None, fake, None, None, None, 4, 9, 13, 6, 1, 16, 16, fake, fake, None)
    assert rc == -1 and b"null" in lib.os2d_train_last_error()
    rc = lib.os2d_train_decode_backward(fake, fake, None, None, None, 4, 9, 13, 5, 1, 16, 16, fake, fake, None)
    assert rc == -1 and b"P=5" in lib.os2d_train_last_error()
    rc = lib.os2d_train_conv_backward_data(4, 6, fake, fake, 4, 9, 13, fake, fake, 10 ** 6, None)
    assert rc == -1 and b"layer" in lib.os2d_train_last_error()
    rc = lib.os2d_train_conv_backward_data(1, 6, fake, fake, 4, 9, 210, fake, fake, 10 ** 7, None)
    assert rc == -1 and b"209" in lib.os2d_train_last_error()
    rc = lib.os2d_train_conv_backward_data(1, 6, fake, fake, 4, 9, 13, fake, fake, 100, None)
    assert rc == -2 and b"workspace" in lib.os2d_train_last_error()
    rc = lib.os2d_train_conv_backward_weight(2, 6, fake, fake, 4, 9, 13, fake, fake, 100, None)
    assert rc == -2 and b"slice" in lib.os2d_train_last_error()
    rc = lib.os2d_train_bn_relu_backward(3, fake, fake, fake, fake, fake, 1e-5, 4, 9, 13, fake, None, None, None, None)
    assert rc == -1 and b"BatchNorm" in lib.os2d_train_last_error()
    rc = lib.os2d_train_params_backward(fake, 4, 5, 9, 13, fake, None, None)
    assert rc == -1
    rc = lib.os2d_train_norm225_backward(fake, fake, 0, 9, 13, fake, None)
    assert rc == -1
    rc = lib.os2d_train_corr_backward(fake, fake, fake, 2, 3, 64, 9, 13, fake, fake, fake, 10, None)
    assert rc == -2
    rc = lib.os2d_train_class_backward(fake, fake, 3, 0, fake, fake, fake, 10 ** 6, None)
    assert rc == -1
    assert lib.os2d_train_last_error() != b""


def test_pair_counts_beyond_the_grid_limits_fail_before_launch(lib_path):
    """One grid row per plane (pair x channel): at most 65535 of them (include/os2d_train.h)."""
    from os2d_amd import _train_lib
    lib = _train_lib.load()
    fake = ctypes.c_void_p(256)      # never dereferenced
    rc = lib.os2d_train_bn_relu_backward(1, fake, fake, fake, fake, fake, 1e-5, 512, 9, 13, fake, None, None, None, None)   # 512 * 128
    assert rc == -1 and b"NB=512" in lib.os2d_train_last_error()
    rc = lib.os2d_train_bn_relu_backward(2, fake, fake, fake, fake, fake, 1e-5, 1024, 9, 13, fake, None, None, None, None)  # 1024 * 64
    assert rc == -1
    rc = lib.os2d_train_params_backward(fake, 10923, 6, 9, 13, fake, None, None)                                            # 65538 planes
    assert rc == -1 and b"NB=10923" in lib.os2d_train_last_error()
    rc = lib.os2d_train_params_backward(fake, 16384, 4, 9, 13, fake, None, None)                                            # 65536 planes
    assert rc == -1
    rc = lib.os2d_train_conv_backward_data(1, 6, fake, fake, 65536, 9, 13, fake, fake, 10 ** 7, None)
    assert rc == -1 and b"NB=65536" in lib.os2d_train_last_error()


def test_backward_kernels_do_not_spill(lib_path):
    pytest.importorskip("msgpack")
    from os2d_amd import codeobj
    ks = codeobj.kernels(lib_path)
    assert len(ks) >= 10
    bad = {n: k for n, k in ks.items() if k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]}
    assert not bad, bad
    assert sum("gemm16_kernel" in n for n in ks) == 4      # conv data / forward (one), conv weight, correlation image, class
