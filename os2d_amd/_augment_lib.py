"""ctypes binding of libos2d_augment.so: padded crops and colour distortion of uint8 images on the device (C ABI declared in
include/os2d_augment.h).

Same rules as ``_lib``: no fallback (os2d_amd/_native.py)."""
import ctypes

from . import build
from ._native import NativeLibrary

ABI_VERSION = 1

_p = ctypes.c_void_p
_i = ctypes.c_int
_ll = ctypes.c_longlong

COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION, COLOR_HUE, COLOR_TO_HSV, COLOR_FROM_HSV = 1, 2, 3, 4, 5, 6   # OS2D_AUGMENT_COLOR_*
COLOR_MAX_OPS, COLOR_SLOTS = 4, 256

SIGNATURES = {
    "os2d_augment_abi_version": (_i, []),
    "os2d_augment_last_error": (ctypes.c_char_p, []),
    "os2d_augment_resample_padded": (_i, [_p, _i, _i, _i, _ll, _ll, _i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _i, _i, _i, _p, _p, _i, _p]),
    "os2d_augment_color": (_i, [_p, _i, _i, _ll, _i, _p, _p, _p, _p, _i, _p, _p]),
}

LIBRARY = NativeLibrary(build.AUGMENT, SIGNATURES, ABI_VERSION, "os2d_augment_abi_version", "os2d_augment_last_error", "the device training images", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call
