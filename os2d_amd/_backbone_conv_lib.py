"""ctypes binding of libos2d_backbone_conv.so: the backbone's 1x1 convolutions as fp32 MFMA GEMMs with the folded BatchNorm, the
residual add and the ReLU as the epilogue (C ABI declared in include/os2d_backbone_conv.h).

Same rules as ``_lib``: no fallback (os2d_amd/_native.py)."""
import ctypes

from . import build
from ._native import NativeLibrary

ABI_VERSION = 1
TILE_M, TILE_N, TILE_K = 128, 128, 16       # OS2D_BACKBONE_CONV_TILE_M / _N / _K: output channels, pixels, input channels
SMALL_TILE_M, SMALL_TILE_N = 64, 256        # OS2D_BACKBONE_CONV_SMALL_TILE_M / _N: the shape of layers of at most 64 outputs
MAX_GROUPS = 2048                           # OS2D_BACKBONE_CONV_MAX_GROUPS

_p = ctypes.c_void_p
_i = ctypes.c_int

SIGNATURES = {
    "os2d_backbone_conv_abi_version": (_i, []),
    "os2d_backbone_conv_last_error": (ctypes.c_char_p, []),
    "os2d_backbone_conv1x1": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
}

LIBRARY = NativeLibrary(build.BACKBONE_CONV, SIGNATURES, ABI_VERSION, "os2d_backbone_conv_abi_version", "os2d_backbone_conv_last_error",
                        "the backbone's fused_conv1x1 inference route", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call
