"""GPU: the 64-row shape of the split-half per-bin GEMM (os2d_amd/csrc/spectral_f16.hip), which layers of at most 64 outputs run
(the 5x5 layer 128 -> 64 in the frequency domain): it addresses output-channel half 0 of the packed weight spectra only.

1. Same bits as the 128-row shape, in one process and without a switch: the launcher takes the 64-row shape for Cout <= 64, so
   the same buffers run once with the true Cout and once with Cout = 65 (the 128-row shape; row 64 is a zero row of the packed
   weights) and rows 0 .. Cout - 1 must be equal bit for bit - both entry points, every branch of the k loop and of the masks.
2. Against a float64 product on layer-2-like operands (128 -> 64 channels), with the bound the 128-row shape is held to in
   test_spectral_gpu.py::test_split_half_spectral_gemm_matches_float64: the arithmetic is the same."""
import functools

import pytest
import torch

from freq_util import dft_sizes, weight_spectra
from os2d_amd import _lib
from test_spectral_gpu import blocked_to_quads, quads_to_blocked, y_quads_to_rows

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def run_gemm16(w16, Xrows, NB, C, Cout, nbins, xs, quads, device):
    """Xrows [C, NB, nbins, 2] on the device -> (Y in quads [nbins/4, NB, Cout, 4, 2], the sentinel tail behind the output).
    The output starts as NaN, the tail (one quad block of 64 pairs) as SENTINEL; pad channels of the quads input are NaN."""
    lib = _lib.load()
    st = _lib.current_stream(device)
    n = (nbins // 4) * NB * Cout * 8
    buf = torch.full((n + 64 * Cout * 8,), float("nan"), device=device)
    buf[n:] = SENTINEL
    if quads:
        cpad = lib.os2d_dft_channel_stride(C)
        Xq = torch.full((nbins // 4, NB, cpad, 4, 2), float("nan"), device=device)
        Xq[:, :, :C] = Xrows.view(C, NB, nbins // 4, 4, 2).permute(2, 1, 0, 3, 4)
        Xb = quads_to_blocked(Xq)
        _lib.check(lib.os2d_spectral_gemm_f16_quads(_lib.ptr(w16), _lib.ptr(Xb), _lib.ptr(buf), NB, C, Cout, nbins, xs, st), "gemm16 quads")
        Yq = blocked_to_quads(buf[:n], nbins // 4, NB, Cout)
    else:
        _lib.check(lib.os2d_spectral_gemm_f16(_lib.ptr(w16), _lib.ptr(Xrows), _lib.ptr(buf), NB, C, Cout, nbins, xs, st), "gemm16 rows")
        Yq = buf[:n].view(nbins // 4, NB, Cout, 4, 2)
    torch.cuda.synchronize()
    return Yq, buf[n:]


@functools.lru_cache(maxsize=None)
def same_bits_operands(C, Cout, NB, H, W, device):
    P, Q, nbins, _ = dft_sizes(H, W)
    g = torch.Generator().manual_seed(1000 * C + 10 * Cout + NB)
    wfold = torch.randn(Cout, C, 7, 7, generator=g, dtype=torch.float64) * 0.1
    w16 = weight_spectra(wfold, P, Q, nbins, True, device)
    X = ((torch.rand(C, NB, nbins, 2, generator=g) * 40.0 - 20.0)).to(device)      # |X| <= 20 * sqrt(2): far below 65504 / xscale
    return w16, X, nbins, _lib.load().os2d_dft_xscale(H, W)


# (C, Cout, NB, map): KS = 1 (the clamped prologue) | KS = 3 (odd: the peeled last step; channel mask in the last k-step) |
# layer-2 operands over several bin groups, two pair tiles, the second with 6 pairs | row mask inside the second 32-row tile, three
# pair tiles, the last with one pair | one partial row tile
SAME_BITS = [(5, 64, 2, (9, 11)), (20, 64, 64, (11, 13)), (128, 64, 70, (30, 40)), (31, 33, 129, (11, 13)), (9, 6, 3, (9, 11))]


@pytest.mark.parametrize("quads", [False, True], ids=["rows", "quads"])
@pytest.mark.parametrize("C,Cout,NB,hw", SAME_BITS)
def test_rows64_shape_gives_the_bits_of_the_rows128_shape(C, Cout, NB, hw, quads, device):
    w16, X, nbins, xs = same_bits_operands(C, Cout, NB, hw[0], hw[1], device)
    assert nbins % 8 == 0 and (hw != (30, 40) or nbins // 8 > 8)
    y64, tail64 = run_gemm16(w16, X, NB, C, Cout, nbins, xs, quads, device)
    y128, tail128 = run_gemm16(w16, X, NB, C, 65, nbins, xs, quads, device)
    assert not bool(torch.isnan(y64).any()) and not bool(torch.isnan(y128).any())
    assert bool((tail64 == SENTINEL).all()) and bool((tail128 == SENTINEL).all())
    assert float(y64.abs().max()) > 0.0
    assert torch.equal(y64, y128[:, :, :Cout])
    assert float(y128[:, :, Cout:].abs().max()) == 0.0            # rows beyond the layer's: zero weights


@functools.lru_cache(maxsize=None)
def float64_operands(H, W, NB, device):
    """Layer-2-like operands: 64 filters of 5x5 over 128 channels embedded in 7x7 ones, inputs in [0, 1] with one channel all
    ones (DC bin = H * W, the largest value the scale must hold) and one scaled by 1e-6 (subnormal lo halves)."""
    C, Cout = 128, 64
    P, Q, nbins, _ = dft_sizes(H, W)
    V = Q // 2 + 1
    g = torch.Generator().manual_seed(H + W)
    wfold = torch.zeros(Cout, C, 7, 7, dtype=torch.float64)
    wfold[:, :, 1:6, 1:6] = torch.randn(Cout, C, 5, 5, generator=g, dtype=torch.float64) * 0.05
    x = torch.rand(NB, C, H, W, generator=g, dtype=torch.float64)
    x[:, 0] = 1.0
    x[:, 1] *= 1e-6
    k = torch.zeros(Cout, C, P, Q, dtype=torch.float64, device=device)
    k[:, :, ((3 - torch.arange(7, device=device)) % P).view(-1, 1), ((3 - torch.arange(7, device=device)) % Q).view(1, -1)] = wfold.to(device)
    K = torch.fft.rfft2(k).transpose(2, 3).reshape(Cout, C, P * V)                           # bin = v * P + u
    Xc = torch.fft.rfft2(x.to(device), s=(P, Q)).transpose(2, 3).reshape(NB, C, P * V)
    X = torch.zeros(C, NB, nbins, 2, device=device)
    X[:, :, :P * V] = torch.view_as_real(Xc.to(torch.complex64)).permute(1, 0, 2, 3)
    ref = torch.einsum("ocb,ncb->nob", K, torch.view_as_complex(X[:, :, :P * V].double().permute(1, 0, 2, 3).contiguous()))
    return weight_spectra(wfold, P, Q, nbins, True, device), X, ref, nbins, P * V


@pytest.mark.parametrize("quads", [False, True], ids=["rows", "quads"])
@pytest.mark.parametrize("H,W,NB", [(11, 13, 5), (30, 40, 70)])
def test_rows64_shape_matches_float64(H, W, NB, quads, device):
    w16, X, ref, nbins, used = float64_operands(H, W, NB, device)
    xs = _lib.load().os2d_dft_xscale(H, W)
    assert xs * H * W <= 65504 < 2 * xs * H * W
    Yq, tail = run_gemm16(w16, X, NB, 128, 64, nbins, xs, quads, device)
    got = torch.view_as_complex(y_quads_to_rows(Yq.contiguous(), NB, 64, nbins)[:, :, :used].contiguous()).to(torch.complex128)
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print("rows64 GEMM {} {}x{} NB={}: max err {:.3g} of {:.3g} ({:.3g})".format("quads" if quads else "rows", H, W, NB, err, scale, err / scale))
    assert bool((tail == SENTINEL).all())
    assert err <= 2e-6 * scale
