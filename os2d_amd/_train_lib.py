"""ctypes binding of libos2d_train.so: the backward pass of the head, the target assignment and the training objective
(C ABI declared in include/os2d_train.h).

Same rules as ``_lib``: no fallback (os2d_amd/_native.py)."""
import ctypes

from . import build
from ._native import NativeLibrary

ABI_VERSION = 2

_p = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_d = ctypes.c_double


class OptimTensor(ctypes.Structure):
    """os2d_train_optim_tensor of include/os2d_train.h: one tensor of a multi-tensor optimiser launch (64 bytes)."""
    _fields_ = [("param", _p), ("grad", _p), ("state1", _p), ("state2", _p), ("step", _p), ("numel", ctypes.c_longlong),
                ("lr", _f), ("weight_decay", _f), ("first_chunk", _i), ("aligned", _i)]


OPTIM_MAX_TENSORS, OPTIM_CHUNK = 60, 4096      # OS2D_TRAIN_OPTIM_MAX_TENSORS, OS2D_TRAIN_OPTIM_CHUNK
OPTIM_SGD, OPTIM_ADAM = 0, 1
OPTIM_ADAGRAD, OPTIM_ADADELTA, OPTIM_ADAMAX, OPTIM_ASGD, OPTIM_RMSPROP, OPTIM_RPROP = 2, 3, 4, 5, 6, 7
OPTIM_MAX_HYPER, OPTIM_FACTORS = 8, 4          # OS2D_TRAIN_OPTIM_MAX_HYPER, OS2D_TRAIN_OPTIM_FACTORS

SIGNATURES = {
    "os2d_train_abi_version": (_i, []),
    "os2d_train_last_error": (ctypes.c_char_p, []),
    "os2d_train_decode_backward": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "os2d_train_decode_backward_det_workspace_bytes": (_sz, [_i, _i, _i]),
    "os2d_train_decode_backward_det": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "os2d_train_decode_det_exponent": (_i, [ctypes.c_uint, _i, _i]),
    "os2d_train_params_backward": (_i, [_p, _i, _i, _i, _i, _p, _p, _p]),
    "os2d_train_bn_relu_backward": (_i, [_i, _p, _p, _p, _p, _p, _f, _i, _i, _i, _p, _p, _p, _p, _p]),
    "os2d_train_conv_data_workspace_floats": (_sz, [_i, _i]),
    "os2d_train_conv_backward_data": (_i, [_i, _i, _p, _p, _i, _i, _i, _p, _p, _sz, _p]),
    "os2d_train_conv_weight_slice_floats": (_sz, [_i, _i]),
    "os2d_train_conv_backward_weight": (_i, [_i, _i, _p, _p, _i, _i, _i, _p, _p, _sz, _p]),
    "os2d_train_norm225_backward": (_i, [_p, _p, _i, _i, _i, _p, _p]),
    "os2d_train_corr_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "os2d_train_corr_backward": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "os2d_train_conv_data_workspace_floats_ex": (_sz, [_i, _i, _i, _i]),
    "os2d_train_conv_backward_data_ex": (_i, [_i, _i, _i, _p, _p, _i, _i, _i, _p, _p, _sz, _p]),
    "os2d_train_conv_weight_slice_floats_ex": (_sz, [_i, _i, _i]),
    "os2d_train_conv_backward_weight_ex": (_i, [_i, _i, _i, _p, _p, _i, _i, _i, _p, _p, _sz, _p]),
    "os2d_train_corr_workspace_floats_ex": (_sz, [_i, _i, _i, _i, _i, _i]),
    "os2d_train_corr_backward_ex": (_i, [_i, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "os2d_train_conv_forward_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "os2d_train_conv_forward": (_i, [_i, _i, _i, _p, _p, _p, _i, _i, _i, _p, _p, _sz, _p]),
    "os2d_train_bn_workspace_bytes": (_sz, [_i, _i]),
    "os2d_train_bn_stats": (_i, [_i, _p, _i, _i, _i, _f, _p, _p, _p, _p, _sz, _p]),
    "os2d_train_bn_relu_forward": (_i, [_i, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "os2d_train_bn_relu_backward_batch": (_i, [_i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "os2d_train_class_backward": (_i, [_p, _p, _i, _i, _p, _p, _p, _sz, _p]),
    "os2d_train_planes_from_shb": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "os2d_train_assign_targets": (_i, [_i, _p, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _f, _f, _p, _p, _p, _p, _p]),
    "os2d_train_assign_targets_ops": (_i, [_i, _p, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _f, _f, _i, _p, _p, _p, _p, _p, _p, _p]),
    "os2d_train_crop_boxes": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "os2d_train_mine_select_workspace_bytes": (_sz, [_i, _i, _i, _p]),
    "os2d_train_mine_select": (_i, [_i, _i, _i, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _i, _p, _p, _p, _p, _sz, _p]),
    "os2d_train_objective_workspace_floats": (_sz, [_i, _i, _i]),
    "os2d_train_objective_forward": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _f, _f, _f, _d, _p, _p, _p, _p, _p,
                                          _p, _sz, _p]),
    "os2d_train_objective_backward": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _p, _p, _p, _p]),
    "os2d_train_optim_max_tensors": (_i, []),
    "os2d_train_optim_chunks": (_sz, [ctypes.c_longlong]),
    "os2d_train_optim_sumsq": (_i, [_p, _i, _p, _sz, _p]),
    "os2d_train_optim_finalize": (_i, [_p, _sz, _f, _p, _p]),
    "os2d_train_optim_prepare": (_i, [_p, _i, _p, _d, _d, _p, _p]),
    "os2d_train_optim_update": (_i, [_i, _p, _i, _p, _p, _d, _d, _d, _p]),
    "os2d_train_optim_prepare_ex": (_i, [_i, _p, _i, _p, _p, _i, _p, _p]),
    "os2d_train_optim_update_ex": (_i, [_i, _p, _i, _p, _p, _p, _i, _p]),
    "os2d_train_range_plan_ints": (_sz, []),
    "os2d_train_range_plan_doubles": (_sz, []),
    "os2d_train_range_plan": (_i, [_i] + [_p] * 6 + [_d] + [_p] * 6 + [_d] + [_p] * 4),
}

LIBRARY = NativeLibrary(build.TRAIN, SIGNATURES, ABI_VERSION, "os2d_train_abi_version", "os2d_train_last_error", "the head's backward pass", __name__)
lib_path, load, check, call = LIBRARY.lib_path, LIBRARY.load, LIBRARY.check, LIBRARY.call
