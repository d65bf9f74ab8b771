"""ctypes binding of libos2d_image.so: the image pyramid from uint8 images on the device (C ABI declared in include/os2d_image.h).

Same rules as ``_lib``: no fallback.  A missing or stale library is built in-tree (os2d_amd/build.py) and an export that is
not there, or an ABI version that does not match, raises ``Os2dLibraryError``."""
import ctypes
import os

from ._lib import Os2dLibraryError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libos2d_image.so")
ABI_VERSION = 1

_p = ctypes.c_void_p
_i = ctypes.c_int
_ll = ctypes.c_longlong

SIGNATURES = {
    "os2d_image_abi_version": (_i, []),
    "os2d_image_last_error": (ctypes.c_char_p, []),
    "os2d_image_resample": (_i, [_p, _i, _i, _i, _ll, _ll, _i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _i, _i, _i, _p, _p, _i, _p]),
}

_LIB = None


def lib_path():
    return os.environ.get("OS2D_IMAGE_LIB", LIB_PATH)


def load():
    """Load (once) and return the ctypes handle of libos2d_image.so."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if "OS2D_IMAGE_LIB" not in os.environ:
        from . import build as _build
        if not _build.image_up_to_date():
            try:
                import fcntl
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path + ".lock", "w") as lock:
                    fcntl.flock(lock, fcntl.LOCK_EX)
                    if not _build.image_up_to_date():
                        _build.build_image(verbose=False)
            except Exception as e:  # noqa: BLE001
                raise Os2dLibraryError("libos2d_image.so is missing or stale and building it failed ({}); the device "
                                       "image pyramid has no CPU or PyTorch fallback".format(e))
    if not os.path.exists(path):
        raise Os2dLibraryError("libos2d_image.so not found at {}: python -m os2d_amd.build --image".format(path))
    import torch  # noqa: F401  (the HIP runtime of torch first: one runtime, shared streams)
    try:
        handle = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    except OSError as e:
        raise Os2dLibraryError("cannot load {}: {}".format(path, e))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise Os2dLibraryError("{} does not export {} (stale build? python -m os2d_amd.build --image --force)".format(path, name))
        fn.restype = res
        fn.argtypes = args
    if handle.os2d_image_abi_version() != ABI_VERSION:
        raise Os2dLibraryError("ABI version mismatch: libos2d_image.so {} vs binding {}".format(handle.os2d_image_abi_version(), ABI_VERSION))
    _LIB = handle
    return _LIB


def check(rc, what):
    if rc != 0:
        msg = load().os2d_image_last_error()
        raise RuntimeError("{} failed (code {}): {}".format(what, rc, msg.decode("utf-8", "replace") if msg else "?"))
