"""GPU: what ``NativeLibrary.call`` (os2d_amd/_native.py) does with a device tensor - the contiguity rule and its one exception
``raw_ptr``, the address, stream and current device the entry point sees (through a recording handle, tests/test_native_call.py),
and that a kernel launched through it writes the bits of the same launch made by hand with ``ptr`` / ``current_stream`` /
``check``."""
import pytest
import torch

import forward_matrix_model as FX
import voc_eval_stage_cases as C
from test_native_call import fake_handle

pytestmark = pytest.mark.gpu


def _bindings():
    from os2d_amd import _eval_lib, _lib, _native
    return _lib, _eval_lib, _native


def test_a_non_contiguous_tensor_is_refused_and_raw_ptr_takes_it(device):
    _lib, _, N = _bindings()
    t = torch.empty(4, 6, device=device).t()
    out = torch.empty(24, device=device)
    assert not t.is_contiguous()
    with fake_handle(_lib, "os2d_fm_sumsq", 0) as h:
        with pytest.raises(ValueError, match=r"os2d_fm_sumsq: argument 1 must be a contiguous device tensor.*not contiguous"):
            _lib.call("os2d_fm_sumsq", out, t, 1, 1, 4, 6, N.STREAM)
        assert h.calls == []
        _lib.call("os2d_fm_sumsq", out, N.raw_ptr(t), 1, 1, 4, 6, N.STREAM)
        assert len(h.calls) == 1 and h.calls[0][1].value == t.data_ptr()
    with pytest.raises(ValueError, match="contiguous device tensor"):
        N.ptr(t)
    with pytest.raises(ValueError, match="device tensor"):
        N.raw_ptr(t.cpu())


def test_address_stream_and_current_device_reach_the_entry_point(device):
    _lib, _, N = _bindings()
    t = torch.empty(8, dtype=torch.int8, device=device)          # a dtype the former whitelist of ``ptr`` refused
    side = torch.cuda.Stream(device)
    seen = {}

    def inside(handle):
        seen["device"] = torch.cuda.current_device()

    with fake_handle(_lib, "os2d_fm_sumsq", 0, inside) as h:
        with torch.cuda.stream(side):
            _lib.call("os2d_fm_sumsq", t, None, 1, 2, 3, 4, N.STREAM)
            _lib.call("os2d_fm_sumsq", None, None, 1, 2, 3, 4, N.STREAM, device=device)      # no tensor: the device is given
    assert h.calls[0] == (t.data_ptr(), None, 1, 2, 3, 4, side.cuda_stream)
    assert h.calls[1] == (None, None, 1, 2, 3, 4, side.cuda_stream)
    assert side.cuda_stream != torch.cuda.current_stream(device).cuda_stream
    assert seen["device"] == t.device.index
    assert N.ptr(t).value == t.data_ptr()


def test_fm_sumsq_through_call_equals_the_raw_path(device):
    _lib, _, N = _bindings()
    case = min(FX.CORR_CASES, key=lambda c: c[0] * c[1] * c[2] * c[3] * c[4])
    A, B, Cf, H, W = case
    fm = FX.corr_inputs(case)[0].detach().to(torch.float32).contiguous().to(device)
    got = torch.full((A, H * W), float("nan"), device=device)
    raw = torch.full((A, H * W), float("nan"), device=device)
    _lib.call("os2d_fm_sumsq", fm, got, A, Cf, H, W, N.STREAM)
    with torch.cuda.device(device):
        _lib.check(_lib.load().os2d_fm_sumsq(_lib.ptr(fm), _lib.ptr(raw), A, Cf, H, W, _lib.current_stream(device)), "os2d_fm_sumsq")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(raw).all()) and torch.equal(got.view(torch.int32), raw.view(torch.int32))


def test_eval_count_gt_through_call_equals_the_raw_path(device):
    _lib, E, N = _bindings()
    # the smallest case that HAS operands (G = 0 passes NULL for both): int32 labels, uint8 difficult bytes
    c = min((c for c in C.count_cases() if len(c["gt_labels"])), key=lambda c: (len(c["gt_labels"]), c["L"]))
    G, L = len(c["gt_labels"]), c["L"]
    labels = torch.from_numpy(c["gt_labels"].copy()).to(device)
    difficult = torch.from_numpy(c["gt_difficult"].copy()).to(device)
    assert labels.dtype == torch.int32 and difficult.dtype == torch.uint8

    def outputs():
        return torch.full((L + 1,), -1, dtype=torch.int32, device=device), torch.full((L,), -1, dtype=torch.int32, device=device)
    n_pos, gt_count = outputs()
    n_pos_raw, gt_count_raw = outputs()
    E.call("os2d_eval_count_gt", labels, difficult, G, L, n_pos, gt_count, N.STREAM)
    with torch.cuda.device(device):
        E.check(E.load().os2d_eval_count_gt(_lib.ptr(labels), _lib.ptr(difficult), G, L, _lib.ptr(n_pos_raw), _lib.ptr(gt_count_raw),
                                            _lib.current_stream(device)), "os2d_eval_count_gt")
    torch.cuda.synchronize()
    assert int(gt_count_raw.min()) >= 0
    assert torch.equal(n_pos, n_pos_raw) and torch.equal(gt_count, gt_count_raw)
