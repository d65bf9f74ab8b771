"""CPU: ``NativeLibrary.call`` (os2d_amd/_native.py), the one checked path of a product call into the four HIP libraries - what it
raises and when, and that it hands everything but tensors and ``STREAM`` to the entry point as it got it.  The refused calls
are those of tests/test_native_libs.py (argument checks of the libraries: nothing is launched, no device is needed); what needs
a device - addresses, the stream, the current device - is in tests/test_native_call_gpu.py."""
import ctypes
import re

import pytest
import torch

from os2d_amd import _lib, _native
from os2d_amd._native import STREAM

from test_native_libs import CASES, KEYS, binding, built, last_error  # noqa: F401  (built: a fixture)


class Recorder(object):
    """Stands for a library handle: the refusal functions of test_native_libs.py call it, it keeps (name, args) and answers 0."""

    def __getattr__(self, name):
        def entry(*args):
            self.name, self.args = name, args
            return 0
        return entry


def refused_call(key):
    """(entry point, arguments, the library's message) of the library's refusal case."""
    rec = Recorder()
    _, message = CASES[key][5](rec)
    return rec.name, rec.args, message.decode()


class FakeHandle(object):
    """A handle whose one function of its own, ``name``, records its arguments and what device is current, and returns ``code``;
    the error text still comes from the real library."""

    def __init__(self, real, name, code, inside=None):
        self._real, self._name, self._code, self._inside = real, name, code, inside
        self.calls = []

    def __getattr__(self, attr):
        if attr != self._name:
            return getattr(self._real, attr)

        def entry(*args):
            self.calls.append(args)
            if self._inside is not None:
                self._inside(self)
            return self._code
        return entry


class fake_handle(object):
    """with fake_handle(binding, name, code) as h: the library's handle is ``h`` inside, the real one afterwards."""

    def __init__(self, b, name, code, inside=None):
        self.library = b.LIBRARY
        self.handle = FakeHandle(b.load(), name, code, inside)

    def __enter__(self):
        self.saved, self.library._handle = self.library._handle, self.handle
        return self.handle

    def __exit__(self, *exc):
        self.library._handle = self.saved


def test_the_helpers_live_in_one_place_and_every_binding_exports_call():
    assert _lib.ptr is _native.ptr and _lib.host_ptr is _native.host_ptr and _lib.current_stream is _native.current_stream
    for key in KEYS:
        b = binding(key)
        assert b.call == b.LIBRARY.call and b.check == b.LIBRARY.check
    cpu = torch.zeros(4)
    for helper in (_native.ptr, _native.raw_ptr):
        with pytest.raises(ValueError, match="device tensor"):
            helper(cpu)
    assert _native.ptr(None) is None and _native.host_ptr(None) is None


@pytest.mark.parametrize("key", KEYS)
def test_a_refused_call_raises_the_librarys_message(built, key):
    name, args, message = refused_call(key)
    others = {k: last_error(k) for k in KEYS if k != key}
    with pytest.raises(RuntimeError) as e:
        binding(key).call(name, *args)
    text = str(e.value)
    assert text.startswith(name + " failed (code -1): ") and message in text
    assert text == "{} failed (code -1): {}".format(name, last_error(key).decode())        # what ``check`` raises
    assert {k: last_error(k) for k in others} == others


@pytest.mark.parametrize("key", KEYS)
def test_a_cpu_tensor_is_refused_before_the_entry_point_runs(built, key):
    name, args, message = refused_call(key)
    with pytest.raises(RuntimeError):
        binding(key).call(name, *args)                 # a text of this thread's that any entry into the library would replace
    before = last_error(key)
    assert message.encode() in before
    with fake_handle(binding(key), name, 0) as h:
        for at in (0, len(args) - 1):
            bad = list(args)
            bad[at] = torch.zeros(8)
            with pytest.raises(ValueError, match=r"{}: argument {} must be a contiguous device tensor".format(re.escape(name), at)):
                binding(key).call(name, *bad)
        assert h.calls == []
    assert last_error(key) == before


@pytest.mark.parametrize("key", KEYS)
def test_stream_without_a_device_unknown_names_and_value_queries(built, key):
    b = binding(key)
    name, args, _ = refused_call(key)
    with fake_handle(b, name, 0) as h:
        with pytest.raises(ValueError, match=r"{}: argument {} is STREAM".format(re.escape(name), len(args) - 1)):
            b.call(name, *args[:-1], STREAM)
        assert h.calls == []
    with pytest.raises(AttributeError, match="os2d_no_such_entry"):
        b.call("os2d_no_such_entry", 1, 2)
    queries = [n for n, (res, _) in b.SIGNATURES.items() if res is not ctypes.c_int]
    assert b.LIBRARY.error_fn in queries            # the error text and every size helper (libos2d_image.so has none)
    assert len(queries) >= 2 or key == "image"
    for n in queries:
        with pytest.raises(TypeError, match=re.escape(n)):
            b.call(n)


@pytest.mark.parametrize("key", KEYS)
def test_other_arguments_reach_the_entry_point_unchanged(built, key):
    b = binding(key)
    name, _, _ = refused_call(key)
    size = ctypes.c_size_t()
    args = (None, 7, -3, 0.25, 1e-5, ctypes.byref(size), (ctypes.c_int * 3)(1, 2, 3), (ctypes.c_void_p * 2)(256, 512),
            ctypes.c_void_p(256), ctypes.c_double(2.5))
    with fake_handle(b, name, 0) as h:
        assert b.call(name, *args) is None
        assert len(h.calls) == 1 and len(h.calls[0]) == len(args)
        assert all(got is sent for got, sent in zip(h.calls[0], args))
    with fake_handle(b, name, 5) as h:
        with pytest.raises(RuntimeError, match=r"^{} failed \(code 5\): ".format(re.escape(name))):
            b.call(name, *args)
        assert len(h.calls) == 1
    assert b.LIBRARY._handle is b.load() and not isinstance(b.load(), FakeHandle)


@pytest.mark.parametrize("key", KEYS)
def test_call_enters_what_the_bindings_load_returns(built, monkeypatch, key):
    """A site that wrote ``binding.load().entry(...)`` could be observed by replacing the binding's ``load`` (the spy of
    tests/test_backward_det_gpu.py); ``call`` keeps that seam."""
    b = binding(key)
    name, _, _ = refused_call(key)
    handle = FakeHandle(b.load(), name, 0)
    with monkeypatch.context() as m:
        m.setattr(b, "load", lambda: handle)
        b.call(name, 1, None)
    assert handle.calls == [(1, None)] and b.load() is b.LIBRARY._handle
