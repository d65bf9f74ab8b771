"""ctypes binding of libos2d_image.so: the image pyramid from uint8 images on the device (C ABI declared in include/os2d_image.h).

Same rules as ``_lib``: no fallback (os2d_amd/_native.py)."""
import ctypes

from . import build
from ._native import NativeLibrary

ABI_VERSION = 1

_p = ctypes.c_void_p
_i = ctypes.c_int
_ll = ctypes.c_longlong

SIGNATURES = {
    "os2d_image_abi_version": (_i, []),
    "os2d_image_last_error": (ctypes.c_char_p, []),
    "os2d_image_resample": (_i, [_p, _i, _i, _i, _ll, _ll, _i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _i, _i, _i, _p, _p, _i, _p]),
}

LIBRARY = NativeLibrary(build.IMAGE, SIGNATURES, ABI_VERSION, "os2d_image_abi_version", "os2d_image_last_error", "the device image pyramid", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call
