"""The one loader of the HIP libraries: a ``NativeLibrary`` ties a build record (os2d_amd/build.py) to its ctypes signatures.

There is deliberately NO fallback: a library that is missing, does not export its declared ABI or reports another ABI version
fails loudly (``Os2dLibraryError``).  Build with ``python -m os2d_amd.build`` (or ``__graft_entry__.build()``)."""
import ctypes
import os

from . import build as _build


class Os2dLibraryError(RuntimeError):
    pass


class NativeLibrary:
    def __init__(self, record, signatures, abi_version, version_fn, error_fn, what):
        """record: build.Library; signatures: name -> (restype, argtypes), EVERY symbol of the public header; version_fn /
        error_fn: names of the ABI-version and last-error entry points; what: the part of the project it serves, for messages."""
        self.record, self.signatures, self.abi_version = record, signatures, abi_version
        self.version_fn, self.error_fn, self.what = version_fn, error_fn, what
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
