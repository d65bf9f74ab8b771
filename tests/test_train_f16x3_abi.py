"""CPU: the *_ex entry points of libos2d_train.so (include/os2d_train.h: the backward GEMMs with a choice of arithmetic) refuse
bad arguments before anything is launched, and their size functions return the old sizes at arith = 0."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import _train_lib, build
    build.build(verbose=False)
    return _train_lib.load()


fake = ctypes.c_void_p(256)      # never dereferenced: every call below is refused by its argument checks


def test_size_functions_at_arith_0_return_the_old_sizes(lib):
    for layer, P in ((1, 6), (2, 6), (3, 6), (3, 4), (3, 5), (4, 6)):
        assert lib.os2d_train_conv_data_workspace_floats_ex(0, layer, P, 7) == lib.os2d_train_conv_data_workspace_floats(layer, P)
        assert lib.os2d_train_conv_weight_slice_floats_ex(0, layer, P) == lib.os2d_train_conv_weight_slice_floats(layer, P)
    for shape in ((2, 64, 9, 13), (1, 1, 2, 2), (0, 64, 9, 13)):
        A, C, H, W = shape
        assert lib.os2d_train_corr_workspace_floats_ex(0, A, 3, C, H, W) == lib.os2d_train_corr_workspace_floats(A, C, H, W)


def test_size_functions_at_arith_1(lib):
    """The f16x3 route keeps its maxima words behind / in front of what the fp32 route keeps there."""
    assert lib.os2d_train_conv_data_workspace_floats_ex(1, 1, 6, 7) == 128 * 225 * 49 + 1 + 7
    assert lib.os2d_train_conv_weight_slice_floats_ex(1, 3, 4) == 4 * 64 * 25 + 16
    assert lib.os2d_train_corr_workspace_floats_ex(1, 2, 3, 64, 9, 13) == 2 * 2 * 117 + 2 * 64 * 117 + 2 + 2 + 3
    # a bad argument: 0
    assert lib.os2d_train_conv_data_workspace_floats_ex(2, 1, 6, 7) == 0 and lib.os2d_train_conv_data_workspace_floats_ex(1, 3, 5, 7) == 0
    assert lib.os2d_train_conv_data_workspace_floats_ex(1, 1, 6, 0) == 0
    assert lib.os2d_train_conv_weight_slice_floats_ex(2, 1, 6) == 0 and lib.os2d_train_conv_weight_slice_floats_ex(1, 4, 6) == 0
    assert lib.os2d_train_corr_workspace_floats_ex(2, 2, 3, 64, 9, 13) == 0 and lib.os2d_train_corr_workspace_floats_ex(1, 2, 0, 64, 9, 13) == 0


@pytest.mark.parametrize("arith", [0, 1])
def test_bad_arguments_fail_before_launch(lib, arith):
    err = lib.os2d_train_last_error
    big = 10 ** 8
    # a bad arithmetic
    assert lib.os2d_train_conv_backward_data_ex(2, 1, 6, fake, fake, 4, 9, 13, fake, fake, big, None) == -1 and b"arith 2" in err()
    assert lib.os2d_train_conv_backward_weight_ex(2, 1, 6, fake, fake, 4, 9, 13, fake, fake, big, None) == -1 and b"arith 2" in err()
    assert lib.os2d_train_corr_backward_ex(2, fake, fake, fake, 2, 3, 64, 9, 13, fake, fake, fake, big, None) == -1 and b"arith 2" in err()
    assert lib.os2d_train_conv_backward_data_ex(-1, 1, 6, fake, fake, 4, 9, 13, fake, fake, big, None) == -1
    # a bad layer
    assert lib.os2d_train_conv_backward_data_ex(arith, 4, 6, fake, fake, 4, 9, 13, fake, fake, big, None) == -1 and b"layer" in err()
    assert lib.os2d_train_conv_backward_weight_ex(arith, 3, 5, fake, fake, 4, 9, 13, fake, fake, big, None) == -1 and b"layer" in err()
    # W = 210
    assert lib.os2d_train_conv_backward_data_ex(arith, 1, 6, fake, fake, 4, 9, 210, fake, fake, big, None) == -1 and b"209" in err()
    assert lib.os2d_train_conv_backward_weight_ex(arith, 1, 6, fake, fake, 4, 9, 210, fake, fake, big, None) == -1 and b"209" in err()
    assert lib.os2d_train_corr_backward_ex(arith, fake, fake, fake, 2, 0, 64, 9, 13, fake, fake, fake, big, None) == -1
    # null pointers, too many pairs
    assert lib.os2d_train_conv_backward_data_ex(arith, 1, 6, None, fake, 4, 9, 13, fake, fake, big, None) == -1 and b"null" in err()
    assert lib.os2d_train_conv_backward_data_ex(arith, 1, 6, fake, fake, 65536, 9, 13, fake, fake, big, None) == -1 and b"NB=65536" in err()
    # a short workspace: one float less than the size function asks for
    n = lib.os2d_train_conv_data_workspace_floats_ex(arith, 1, 6, 4)
    assert lib.os2d_train_conv_backward_data_ex(arith, 1, 6, fake, fake, 4, 9, 13, fake, fake, n - 1, None) == -2 and b"workspace" in err()
    n = lib.os2d_train_conv_weight_slice_floats_ex(arith, 2, 6)
    assert lib.os2d_train_conv_backward_weight_ex(arith, 2, 6, fake, fake, 4, 9, 13, fake, fake, n - 1, None) == -2 and b"slice" in err()
    n = lib.os2d_train_corr_workspace_floats_ex(arith, 2, 3, 64, 9, 13)
    assert lib.os2d_train_corr_backward_ex(arith, fake, fake, fake, 2, 3, 64, 9, 13, fake, fake, fake, n - 1, None) == -2 and b"workspace" in err()


def test_the_f16x3_kernels_are_in_the_library(lib):
    pytest.importorskip("msgpack")
    from os2d_amd import build, codeobj
    ks = codeobj.kernels(build.TRAIN_LIB_PATH)
    mine = {n: k for n, k in ks.items() if "gemm_f16x3_kernel" in n or "absmax_" in n}
    # two tile shapes for the convolution gradients, the 64-row one for the correlation; the maxima pass and its two loaders
    assert sum("gemm_f16x3_kernel" in n for n in mine) == 6 and sum("absmax_kernel" in n for n in mine) == 2
    assert not {n: k for n, k in mine.items() if k["vgpr_spills"] or k["sgpr_spills"] or k["scratch_bytes"]}
