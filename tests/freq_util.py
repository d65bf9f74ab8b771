"""Test-side plumbing of the frequency-domain layers, shared by the GPU test modules and the diagnostics under tools/: transform
plans, twiddle tables, operand builders and the codec of the split-half blocked activation buffer.

Independent of the product's host code on purpose: the byte-for-byte tests compare what ``os2d_amd.modeling.spectra`` builds
against what is built here, so this module talks to the library through ``os2d_amd._lib`` and makes its own tables.  It must not
import ``os2d_amd.modeling.spectra``."""
import ctypes

import numpy as np
import torch

from os2d_amd import _lib


# ------------------------------------------------------------------------------------------------ plans
def fft_sizes(H, W):
    """(P, Q, nbins) of the in-LDS FFTs (precision "fft" / "fft32")."""
    P, Q, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().os2d_fft_sizes(H, W, ctypes.byref(P), ctypes.byref(Q), ctypes.byref(nb)), "os2d_fft_sizes")
    return P.value, Q.value, nb.value


def fft_tiles(H, W):
    """(TY, TX, TH, TW): the overlap-save tiling of maps beyond the in-LDS transform (1, 1, H, W for the others)."""
    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.load().os2d_fft_tiles(H, W, *[ctypes.byref(x) for x in v]), "os2d_fft_tiles")
    return tuple(x.value for x in v)


def dft_sizes(H, W):
    """(P, Q, nbins, (TY, TX, TH, TW, window rows, window columns)) of the matrix-product transforms (precision "fftx3")."""
    P, Q, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    t = (ctypes.c_int * 6)()
    _lib.check(_lib.load().os2d_dft_sizes(H, W, ctypes.byref(P), ctypes.byref(Q), ctypes.byref(nb), t), "os2d_dft_sizes")
    return P.value, Q.value, nb.value, tuple(t)


def windows(H, W):
    """Per tile of the matrix-product plan (row-major): (y0, x0, oy, ox), and (P, Q, nbins, TY, TX, TH, TW, LH, LW)."""
    P, Q, nbins, (TY, TX, TH, TW, LH, LW) = dft_sizes(H, W)
    oy, ox = (3 if TY > 1 else 0), (3 if TX > 1 else 0)
    return [(ty * TH, tx * TW, oy, ox) for ty in range(TY) for tx in range(TX)], (P, Q, nbins, TY, TX, TH, TW, LH, LW)


# ------------------------------------------------------------------------------------------------ tables and operands
def twiddles(n, device):
    """exp(-2 pi i m / n) as the fp32 [n, 2] table of the in-LDS FFTs."""
    m = torch.arange(n, dtype=torch.float64)
    ang = -2.0 * np.pi * m / n
    return torch.stack([torch.cos(ang), torch.sin(ang)], 1).float().to(device).contiguous()


def table64(n, device):
    m = torch.arange(n, dtype=torch.float64)
    ang = m * (-2.0 * np.pi / n)
    return torch.stack([torch.cos(ang), torch.sin(ang)], 1).to(device).contiguous()


def matrices(P, Q, device):
    """The operand matrices of the matrix-product transforms (os2d_dft_matrices_build)."""
    lib = _lib.load()
    tp, tq = table64(P, device), table64(Q, device)
    out = torch.empty(lib.os2d_dft_matrices_bytes(P, Q), dtype=torch.uint8, device=device)
    _lib.check(lib.os2d_dft_matrices_build(_lib.ptr(tp), _lib.ptr(tq), P, Q, _lib.ptr(out), _lib.current_stream(device)), "os2d_dft_matrices_build")
    torch.cuda.synchronize()
    return out


def weight_spectra(wfold, P, Q, nbins, split, device):
    """Weight spectra of float64 filters [Cout, C, 7, 7] on the P x Q grid: the split fp16 layout (bytes) or the complex64 one."""
    lib = _lib.load()
    Cout, C = wfold.shape[:2]
    wfold = wfold.to(device).contiguous()
    tp, tq = table64(P, device), table64(Q, device)
    scratch = torch.empty(1024, dtype=torch.uint8, device=device)
    st = _lib.current_stream(device)
    if split:
        out = torch.empty(lib.os2d_spectral_weight16_bytes(C, nbins), dtype=torch.uint8, device=device)
        _lib.check(lib.os2d_spectral_weights_build_dft(_lib.ptr(wfold), _lib.ptr(tp), _lib.ptr(tq), C, Cout, P, Q, nbins, _lib.ptr(out),
                                                       _lib.ptr(scratch), st), "os2d_spectral_weights_build_dft")
    else:
        out = torch.empty(lib.os2d_spectral_weight_bytes(C, Cout, nbins) // 4, dtype=torch.float32, device=device)
        _lib.check(lib.os2d_spectral_weights_build(_lib.ptr(wfold), _lib.ptr(tp), _lib.ptr(tq), C, Cout, P, Q, nbins, 0, _lib.ptr(out),
                                                   _lib.ptr(scratch), st), "os2d_spectral_weights_build")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ activation buffers
def plane_interior(H, W):
    """(row stride, offset of cell (0, 0)) inside a zero-bordered plane of os2d_plane_floats(H, W) cells."""
    return W + 3, (3 * (W + 3) + 3 + 3) // 4 * 4


def shb_decode(buf, NB, C, H, W):
    """Split-half blocked buffer (bytes; [NB][C / 8][hi | lo][PLANE][8] halves) -> (hi + lo of the H x W interior as float64
    [NB, C, H, W], still carrying the channel scales; the largest |value| outside the interior)."""
    plane = _lib.load().os2d_plane_floats(H, W)
    Ws, base = plane_interior(H, W)
    units = buf.view(torch.float16).view(NB, C // 8, 2, plane, 8).double()
    val = (units[:, :, 0] + units[:, :, 1]).permute(0, 1, 3, 2).reshape(NB, C, plane)
    inner = val[:, :, base:base + H * Ws].view(NB, C, H, Ws)[..., :W]
    values = inner.clone()
    inner.zero_()
    return values, float(val.abs().max())


def shb_encode(values, scale):
    """float64 [NB, C, H, W] -> the split-half blocked buffer of ``values * scale`` (fp16 hi + lo, zero borders), as bytes."""
    NB, C, H, W = values.shape
    plane = _lib.load().os2d_plane_floats(H, W)
    Ws, base = plane_interior(H, W)
    v = values.double() * scale
    hi = v.to(torch.float16)
    lo = (v - hi.double()).to(torch.float16)
    shb = torch.zeros(NB, C // 8, 2, plane, 8, dtype=torch.float16, device=values.device)
    for part, t in ((0, hi), (1, lo)):
        cells = torch.zeros(NB, C // 8, 8, H, Ws, dtype=torch.float16, device=values.device)
        cells[..., :W] = t.view(NB, C // 8, 8, H, W)
        shb[:, :, part, base:base + H * Ws] = cells.reshape(NB, C // 8, 8, H * Ws).permute(0, 1, 3, 2)
    return shb.view(torch.uint8).view(-1)
