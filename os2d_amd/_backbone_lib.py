"""ctypes binding of libos2d_backbone.so: the folded-BatchNorm epilogues and the stem's pooling of the backbone's inference route
(C ABI declared in include/os2d_backbone.h).

Same rules as ``_lib``: no fallback (os2d_amd/_native.py)."""
import ctypes

from . import build
from ._native import NativeLibrary

ABI_VERSION = 1
MAX_GROUPS = 2048      # OS2D_BACKBONE_MAX_GROUPS

_p = ctypes.c_void_p
_i = ctypes.c_int

SIGNATURES = {
    "os2d_backbone_abi_version": (_i, []),
    "os2d_backbone_last_error": (ctypes.c_char_p, []),
    "os2d_backbone_bn_relu": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "os2d_backbone_bn_add_relu": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "os2d_backbone_bn_relu_maxpool": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
}

LIBRARY = NativeLibrary(build.BACKBONE, SIGNATURES, ABI_VERSION, "os2d_backbone_abi_version", "os2d_backbone_last_error",
                        "the backbone's fused inference route", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call
