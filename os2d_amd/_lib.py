"""ctypes binding of libos2d_hip.so (C ABI declared in include/os2d_hip.h).

There is deliberately NO fallback: if the shared library is missing or does not export the declared ABI, loading it fails
loudly (``Os2dLibraryError``, os2d_amd/_native.py).  Build it with ``python -m os2d_amd.build`` (or ``__graft_entry__.build()``).
"""
import ctypes

from . import build
from ._native import NativeLibrary, Os2dLibraryError, ptr, host_ptr, current_stream  # noqa: F401  (re-exported: tests and tools use them from here)

ABI_VERSION = 9

_c_float_p = ctypes.c_void_p   # device pointers travel as raw addresses (tensor.data_ptr())
_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t

# name -> (restype, argtypes): must list EVERY symbol of include/os2d_hip.h (tests/test_native_libs.py checks the header)
SIGNATURES = {
    "os2d_abi_version": (_i, []),
    "os2d_last_error": (ctypes.c_char_p, []),
    "os2d_packed_conv_floats": (_sz, [_i]),
    "os2d_packed_bias_floats": (_sz, [_i]),
    "os2d_pack_conv": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    "os2d_class_prepare": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "os2d_head_workspace_bytes": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(_sz)]),
    "os2d_head_forward": (_i, [_vp] * 8 + [_i] * 9 + [_vp, _vp, _vp, _vp, _sz, _vp]),
    "os2d_packed_conv_bytes": (_sz, [_i, _i]),
    "os2d_pack_conv_f16x3": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "os2d_rnorm_exp": (_i, []),
    "os2d_class_prepare_batch": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "os2d_class_prepare_workspace_floats": (_sz, [_i, _i]),
    "os2d_shb_bytes": (_sz, [_i, _i, _i]),
    "os2d_corr_normalize_f16x3": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "os2d_transform_conv_f16x3": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "os2d_alignment_grids": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "os2d_spectral_weight_bytes": (_sz, [_i, _i, _i]),
    "os2d_spectral_gemm": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "os2d_spectral_weight16_bytes": (_sz, [_i, _i]),
    "os2d_spectral_xscale": (_f, [_i, _i]),
    "os2d_spectral_weights_build": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "os2d_spectral_gemm_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "os2d_debug_set_dump": (None, [_vp, _i, _vp, _sz]),
    "os2d_fft_sizes": (_i, [_i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "os2d_fft_tiles": (_i, [_i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "os2d_fft_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "os2d_fft_inverse": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "os2d_fft_inverse_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "os2d_dft_sizes": (_i, [_i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "os2d_dft_channel_stride": (_i, [_i]),
    "os2d_dft_matrices_bytes": (_sz, [_i, _i]),
    "os2d_dft_matrices_build": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "os2d_dft_forward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "os2d_dft_inverse": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "os2d_spectral_weights_build_dft": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "os2d_spectral_gemm_f16_quads": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "os2d_dft_xscale": (_f, [_i, _i]),
    "os2d_class_split": (_i, [_vp, _vp, _i, _i, _vp]),
    "os2d_class_split_bytes": (_sz, [_i, _i]),
    "os2d_head_forward_ex": (_i, [_vp] * 8 + [_i] * 9 + [_vp, _vp, _vp, _vp, _sz, _vp, _i, _vp,
                                  ctypes.POINTER(_vp), ctypes.POINTER(_i), _vp, _vp, _vp, _vp]),
    "os2d_head_forward_ex2": (_i, [_vp] * 8 + [_i] * 9 + [_vp, _vp, _vp, _vp, _sz, _vp, _i, _vp,
                                   ctypes.POINTER(_vp), ctypes.POINTER(_i), _vp, _vp, _vp, _vp, _vp]),
    "os2d_dft_inverse_planes": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "os2d_head_workspace_bytes_ex": (_i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_sz)]),
    "os2d_prof_event_create": (_i, [ctypes.POINTER(_vp)]),
    "os2d_prof_event_destroy": (_i, [_vp]),
    "os2d_prof_event_elapsed_ms": (_i, [_vp, _vp, ctypes.POINTER(_f)]),
    "os2d_fm_sumsq": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "os2d_plane_floats": (_sz, [_i, _i]),
    "os2d_corr": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "os2d_corr_normalize": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "os2d_corr_f16x3_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "os2d_corr_f16x3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "os2d_corr_f16x3_packed_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "os2d_corr_f16x3_packed": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "os2d_transform_conv": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "os2d_sample_decode": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "os2d_decode_boxes": (_i, [_vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp]),
    "os2d_nms_workspace_bytes": (_i, [_i, _i, ctypes.POINTER(_sz)]),
    "os2d_nms": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "os2d_detect_level_supported": (_i, [_i, _i]),
    "os2d_detect_level": (_i, [_vp, _vp] + [_i] * 5 + [_f] * 6 + [_vp] * 5),
    "os2d_detect_level_ops": (_i, [_vp, _vp] + [_i] * 5 + [_f, _f, _i, _vp, _vp, _f, _f] + [_vp] * 5),
    "os2d_detect_pyramid_supported": (_i, [_i, _i, _i]),
    "os2d_detect_pyramid_workspace_bytes": (_i, [_i, _i, _i, ctypes.POINTER(_sz)]),
    "os2d_detect_pyramid": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _vp, _sz, _vp]),
    "os2d_detect_pyramid_merged": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _f, _f, _i, _i, _i, _i, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "os2d_detect_pyramid_ops": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _i, _i, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


LIBRARY = NativeLibrary(build.HIP, SIGNATURES, ABI_VERSION, "os2d_abi_version", "os2d_last_error", "the OS2D head", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call
