"""ctypes binding of libos2d_eval.so: the VOC detection metric on the device (C ABI declared in include/os2d_eval.h).

Same rules as ``_lib``: no fallback (os2d_amd/_native.py)."""
import ctypes

from . import build
from ._native import NativeLibrary

ABI_VERSION = 1

_p = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_d = ctypes.c_double

SIGNATURES = {
    "os2d_eval_abi_version": (_i, []),
    "os2d_eval_last_error": (ctypes.c_char_p, []),
    "os2d_eval_count_gt": (_i, [_p, _p, _i, _i, _p, _p, _p]),
    "os2d_eval_match": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _i, _f, _p, _p, _p, _p]),
    "os2d_eval_sort_workspace_bytes": (_sz, [_i]),
    "os2d_eval_sort": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "os2d_eval_scan_workspace_bytes": (_sz, [_i]),
    "os2d_eval_prec_rec": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "os2d_eval_ap": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "os2d_eval_finalise": (_i, [_p, _p, _p, _i, _i, _p, _p, _p, _p, _p]),
}

LIBRARY = NativeLibrary(build.EVAL, SIGNATURES, ABI_VERSION, "os2d_eval_abi_version", "os2d_eval_last_error", "the device evaluation", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call
