"""The one loader of the HIP libraries: a ``NativeLibrary`` ties a build record (os2d_amd/build.py) to its ctypes signatures.

There is deliberately NO fallback: a library that is missing, does not export its declared ABI or reports another ABI version
fails loudly (``Os2dLibraryError``).  Build with ``python -m os2d_amd.build`` (or ``__graft_entry__.build()``)."""
import ctypes
import os
import sys

from . import build as _build


class Os2dLibraryError(RuntimeError):
    pass


STREAM = object()      # argument of NativeLibrary.call: the current stream of the call's device


def _device_tensor(t, contiguous):
    import torch
    return isinstance(t, torch.Tensor) and t.is_cuda and (t.is_contiguous() or not contiguous)


def ptr(t):
    """Device address of a contiguous CUDA/HIP tensor of any dtype (None -> NULL)."""
    if t is None:
        return None
    if not _device_tensor(t, True):
        raise ValueError("expected a contiguous device tensor, got {}".format(
            (type(t).__name__, getattr(t, "device", None), getattr(t, "dtype", None))))
    return ctypes.c_void_p(t.data_ptr())


def raw_ptr(t):
    """Device address of a CUDA/HIP tensor that need NOT be contiguous: only for entry points that take the strides themselves."""
    if not _device_tensor(t, False):
        raise ValueError("expected a device tensor, got {}".format((type(t).__name__, getattr(t, "device", None))))
    return ctypes.c_void_p(t.data_ptr())


def host_ptr(t):
    """Address of a PINNED host tensor (hipHostMalloc memory is mapped into the device address space under the same
    address: kernels may store to it); None -> NULL."""
    if t is None:
        return None
    if not t.is_pinned():
        raise ValueError("expected a pinned host tensor")
    return ctypes.c_void_p(t.data_ptr())


def current_stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class NativeLibrary:
    def __init__(self, record, signatures, abi_version, version_fn, error_fn, what, binding):
        """record: build.Library; signatures: name -> (restype, argtypes), EVERY symbol of the public header; version_fn /
        error_fn: names of the ABI-version and last-error entry points; what: the part of the project it serves, for messages;
        binding: name of the module that exports this instance's ``load`` and ``call`` (its ``__name__``)."""
        self.record, self.signatures, self.abi_version = record, signatures, abi_version
        self.version_fn, self.error_fn, self.what, self.binding = version_fn, error_fn, what, binding
        self._handle = None

    def lib_path(self):
        return os.environ.get(self.record.env, _build.lib_path(self.record))

    def load(self):
        """Load (once) and return the ctypes handle; raises Os2dLibraryError if it is not there."""
        if self._handle is not None:
            return self._handle
        name, path = self.record.name, self.lib_path()
        if self.record.env not in os.environ and not _build.up_to_date(self.record):
            # The .so is a build artefact (not tracked): compile it in-tree when it is missing OR was built from other sources
            # than the ones in the tree (content hash - an edited kernel never runs stale).  This is the same HIP library, not
            # a fallback implementation; if hipcc is missing the error below fires.
            try:
                import fcntl
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path + ".lock", "w") as lock:      # one builder at a time (torchrun starts N ranks at once);
                    fcntl.flock(lock, fcntl.LOCK_EX)         # the check is repeated under the lock
                    _build.build_library(self.record, verbose=False)
            except Exception as e:  # noqa: BLE001
                raise Os2dLibraryError("{} is missing or stale and building it failed ({}); {} has no CPU or PyTorch "
                                       "fallback".format(name, e, self.what))
        if not os.path.exists(path):
            raise Os2dLibraryError("{} not found at {} - {} has no CPU or PyTorch fallback; build the HIP libraries first: "
                                   "python -m os2d_amd.build".format(name, path, self.what))
        # torch must be imported first so that the HIP runtime already mapped in the process (same soname,
        # libamdhip64.so.7) is the one our library binds to: one runtime, shared streams and allocations.
        import torch  # noqa: F401
        try:
            handle = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        except OSError as e:
            raise Os2dLibraryError("cannot load {}: {}".format(path, e))
        for fn_name, (res, args) in self.signatures.items():
            try:
                fn = getattr(handle, fn_name)
            except AttributeError:
                raise Os2dLibraryError("{} does not export {} (stale build? run python -m os2d_amd.build --force)".format(path, fn_name))
            fn.restype = res
            fn.argtypes = args
        version = getattr(handle, self.version_fn)()
        if version != self.abi_version:
            raise Os2dLibraryError("ABI version mismatch: {} {} vs binding {}".format(name, version, self.abi_version))
        self._handle = handle
        return handle

    def check(self, rc, what):
        """Raise RuntimeError with the library's message if a call returned an error code."""
        if rc != 0:
            msg = getattr(self.load(), self.error_fn)()
            raise RuntimeError("{} failed (code {}): {}".format(what, rc, msg.decode("utf-8", "replace") if msg else "?"))

    def call(self, name, *args, device=None):
        """Call the status-returning entry point ``name`` and raise what ``check`` raises if it does not return 0.

        A tensor argument must be a contiguous device tensor and travels as its address; all tensors of one call are on one
        device, which is the call's device (without tensors: ``device``).  ``STREAM`` is that device's current stream and the
        entry point runs with that device current.  None is NULL; anything else goes to ctypes as it is (the declared
        argtypes convert).  A violation raises ValueError with the argument's position (0-based) BEFORE the entry point runs."""
        import torch
        try:
            restype = self.signatures[name][0]
        except KeyError:
            raise AttributeError("{} declares no entry point {}".format(self.record.name, name))
        if restype is not ctypes.c_int:
            raise TypeError("{} does not return a status code: call it on load()".format(name))
        # the handle is what the binding module's ``load`` returns at this moment, as for a site that writes ``_x_lib.load()``: a
        # test that puts a recording handle there (tests/test_backward_det_gpu.py) sees the calls made through here as well
        fn = getattr(sys.modules[self.binding].load(), name)
        args, dev, streams = list(args), None, []
        for k, a in enumerate(args):
            if isinstance(a, torch.Tensor):
                if not (a.is_cuda and a.is_contiguous()):
                    raise ValueError("{}: argument {} must be a contiguous device tensor, got {} on {}{}".format(
                        name, k, a.dtype, a.device, "" if a.is_contiguous() else " (not contiguous)"))
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise ValueError("{}: argument {} is on {}, earlier tensors are on {}".format(name, k, a.device, dev))
                args[k] = a.data_ptr()
            elif a is STREAM:
                streams.append(k)
        if dev is None:
            dev = device
        if dev is None:
            if streams:
                raise ValueError("{}: argument {} is STREAM, but the call has neither a tensor nor device=".format(name, streams[0]))
            return self.check(fn(*args), name)
        with torch.cuda.device(dev):
            for k in streams:
                args[k] = torch.cuda.current_stream(dev).cuda_stream
            self.check(fn(*args), name)
