"""ctypes binding of libos2d_backbone_conv_bf16.so: the backbone's 1x1 convolutions in split-bf16 arithmetic - three bf16 parts per fp32
operand, six products on the bf16 MFMA, fp32 accumulation - with the folded BatchNorm, the residual add and the ReLU as the epilogue
(C ABI declared in include/os2d_backbone_conv_bf16.h).

Same rules as ``_lib``: no fallback (os2d_amd/_native.py)."""
import ctypes

from . import build
from ._native import NativeLibrary

ABI_VERSION = 1
TILE_M, TILE_N, TILE_K = 128, 128, 32       # OS2D_BACKBONE_CONV_BF16_TILE_M / _N / _K: output channels, pixels, input channels
SMALL_TILE_M, SMALL_TILE_N = 64, 256        # OS2D_BACKBONE_CONV_BF16_SMALL_TILE_M / _N: the shape of layers of at most 64 outputs
MAX_GROUPS = 2048                           # OS2D_BACKBONE_CONV_BF16_MAX_GROUPS
PARTS = 3

_p = ctypes.c_void_p
_i = ctypes.c_int

SIGNATURES = {
    "os2d_backbone_conv_bf16_abi_version": (_i, []),
    "os2d_backbone_conv_bf16_last_error": (ctypes.c_char_p, []),
    "os2d_backbone_conv_bf16_packed_elems": (ctypes.c_size_t, [_i, _i]),
    "os2d_backbone_conv_bf16_pack_weights": (_i, [_p, _p, _i, _i, _p]),
    "os2d_backbone_conv1x1_bf16x3": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
}

LIBRARY = NativeLibrary(build.BACKBONE_CONV_BF16, SIGNATURES, ABI_VERSION, "os2d_backbone_conv_bf16_abi_version",
                        "os2d_backbone_conv_bf16_last_error", "the bf16x3 precision of the backbone's fused_conv1x1 inference route", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call


def packed_elems(cout, cin):
    """The size of a layer's packed weights in 16-bit elements (os2d_backbone_conv_bf16_packed_elems); ValueError for a size the library
    refuses."""
    n = load().os2d_backbone_conv_bf16_packed_elems(int(cout), int(cin))
    if n == 0:
        raise ValueError("no packed weights for Cout {} and Cin {} (both 1 ... 2^20)".format(cout, cin))
    return n
