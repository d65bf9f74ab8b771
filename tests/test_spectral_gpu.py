"""GPU: building blocks of the frequency-domain form of the 7x7 TransformNet layer (os2d_amd/csrc/spectral.hip)."""
import pytest
import torch

from freq_util import dft_sizes, fft_sizes, fft_tiles, shb_decode, twiddles
from os2d_amd import _lib

pytestmark = pytest.mark.gpu


def pack_weight_spectra(K, nbins_pad=None):
    """K [Cout, C, nbins] complex64 -> the layout of include/os2d_hip.h: [nbins/8][2][C][8][64] complex."""
    Cout, C, nbins = K.shape
    assert nbins % 8 == 0 and Cout <= 128
    Kp = torch.zeros(128, C, nbins, dtype=K.dtype, device=K.device)
    Kp[:Cout] = K
    # [h, r, c, g, j] -> [g, h, c, j, r]
    return Kp.view(2, 64, C, nbins // 8, 8).permute(3, 0, 2, 4, 1).contiguous()


def run_spectral_gemm(Wp, X, Cout):
    """X [NB,C,nbins] (test order) -> the kernel's channel-major [C,NB,nbins]."""
    lib = _lib.load()
    NB, C, nbins = X.shape
    assert Wp.numel() * 8 == lib.os2d_spectral_weight_bytes(C, Cout, nbins)
    Y = torch.full((NB, Cout, nbins), float("nan"), dtype=torch.complex64, device=X.device)
    Xk = X.permute(1, 0, 2).contiguous()
    _lib.check(lib.os2d_spectral_gemm(_lib.ptr(torch.view_as_real(Wp)), _lib.ptr(torch.view_as_real(Xk)), _lib.ptr(torch.view_as_real(Y)),
                                      NB, C, Cout, nbins, _lib.current_stream(X.device)), "os2d_spectral_gemm")
    return Y


@pytest.mark.parametrize("NB,C,Cout,nbins", [(64, 225, 128, 64), (3, 225, 128, 40), (70, 20, 64, 16), (129, 9, 128, 8), (5, 31, 6, 24)])
def test_spectral_gemm_matches_float64(NB, C, Cout, nbins, device):
    g = torch.Generator().manual_seed(NB * 1000 + C)
    K = torch.complex(torch.randn(Cout, C, nbins, generator=g), torch.randn(Cout, C, nbins, generator=g)).to(device)
    X = torch.complex(torch.randn(NB, C, nbins, generator=g), torch.randn(NB, C, nbins, generator=g)).to(device)
    Y = run_spectral_gemm(pack_weight_spectra(K), X.contiguous(), Cout)
    ref = torch.einsum("ocf,ncf->nof", K.to(torch.complex128), X.to(torch.complex128))
    err = float((Y.to(torch.complex128) - ref).abs().max())
    scale = float(ref.abs().max())
    assert err < 3e-6 * scale, (err, scale)          # fp32 accumulation of 2 * C products


def test_spectral_gemm_full_size_timing(device):
    """The real problem size (3,528 bins, 225 -> 128 channels, 64 classes): correctness on a sample of bins + time."""
    import time
    NB, C, Cout, nbins = 64, 225, 128, 72 * 49
    g = torch.Generator().manual_seed(1)
    K = torch.complex(torch.randn(Cout, C, nbins, generator=g), torch.randn(Cout, C, nbins, generator=g)).to(device)
    X = torch.complex(torch.randn(NB, C, nbins, generator=g), torch.randn(NB, C, nbins, generator=g)).to(device)
    Wp = pack_weight_spectra(K)
    Y = run_spectral_gemm(Wp, X, Cout)
    sel = torch.tensor([0, 7, 8, 1763, 3520, 3527], device=device)
    ref = torch.einsum("ocf,ncf->nof", K[:, :, sel].to(torch.complex128), X[:, :, sel].to(torch.complex128))
    assert float((Y[:, :, sel].to(torch.complex128) - ref).abs().max()) < 3e-6 * float(ref.abs().max())
    torch.cuda.synchronize()
    ms = float("inf")
    for _ in range(3):           # best of 3 x 5 launches (a wall-clock guard must survive one hiccup)
        t0 = time.perf_counter()
        for _ in range(5):
            run_spectral_gemm(Wp, X, Cout)
        torch.cuda.synchronize()
        ms = min(ms, (time.perf_counter() - t0) / 5 * 1e3)
    flops = 8.0 * Cout * C * NB * nbins
    print("spectral GEMM {} bins x {}x{}x{}: {:.3f} ms = {:.1f} TFLOP/s".format(nbins, Cout, C, NB, ms, flops / ms / 1e9))
    assert ms < 5.0


# ------------------------------------------------------------------------------------------------ the transforms
def y_quads_to_rows(Yq, NBT, Cout, nbins):
    """Y [nbins/4, NBT, Cout, 4, 2] (OS2D_SPECTRA_QUADS, what os2d_spectral_gemm_f16 writes) -> [NBT, Cout, nbins, 2]."""
    return Yq.view(nbins // 4, NBT, Cout, 4, 2).permute(1, 2, 0, 3, 4).reshape(NBT, Cout, nbins, 2).contiguous()


def quads_to_blocked(T):
    """[nq, NBT, C, 4, 2] -> the flat buffer in blocks of 64 pairs the matrix-product transforms and the quads GEMM use
    ([pair' / 64][nq][pair' % 64][C][4], include/os2d_hip.h): identical for up to 64 pairs."""
    NBT = T.shape[1]
    return torch.cat([T[:, b0:b0 + 64].contiguous().reshape(-1) for b0 in range(0, NBT, 64)])


def blocked_to_quads(flat, nq, NBT, C):
    out, off = [], 0
    for b0 in range(0, NBT, 64):
        n = min(64, NBT - b0)
        out.append(flat[off:off + nq * n * C * 8].view(nq, n, C, 4, 2))
        off += nq * n * C * 8
    assert off == flat.numel()
    return torch.cat(out, dim=1)


def y_rows_to_quads(Y):
    NBT, Cout, nbins, _ = Y.shape
    return Y.view(NBT, Cout, nbins // 4, 4, 2).permute(2, 0, 1, 3, 4).contiguous()


def tile_windows(H, W):
    """Per tile (row-major): (y0, x0, oy, ox, LH, LW) - the input window starts at map cell (y0 - oy, x0 - ox) and spans
    LH x LW cells; the tile's outputs are map rows y0 .. y0 + TH - 1 found at offset (oy, ox) of the inverse transform."""
    TY, TX, TH, TW = fft_tiles(H, W)
    oy, ox = (3 if TY > 1 else 0), (3 if TX > 1 else 0)
    LH, LW = (TH + 6 if TY > 1 else H), (TW + 6 if TX > 1 else W)
    return [(ty * TH, tx * TW, oy, ox, LH, LW) for ty in range(TY) for tx in range(TX)], (TY, TX, TH, TW)


# the pyramid levels of BASELINE.json configs[4] (+ two more maps) exercise every two-stage register factorisation of
# fft.hip: 36 = 6x6, 42 = 6x7, 48 = 8x6, 54 = 9x6, 64 = 8x8, 72 = 9x8, 84 = 12x7, 96 = 12x8, 108 = 12x9, 128 = 16x8; the
# small / odd maps take the Stockham passes
PYRAMID_LEVELS = [(30, 40), (38, 50), (48, 64), (60, 80), (72, 96), (84, 112)]
MORE_LEVELS = [(44, 90), (90, 60)]


def test_two_stage_factorisations_are_the_pyramid_sizes():
    assert [fft_sizes(h, w)[:2] for h, w in PYRAMID_LEVELS] == [(36, 48), (42, 54), (54, 72), (64, 84), (84, 108), (96, 128)]
    assert [fft_sizes(h, w)[:2] for h, w in MORE_LEVELS] == [(48, 96), (96, 64)]
    # the 96 x 128 level: 2 x 2 overlap-save tiles on the transform of the 48 x 64 level (shared weight spectra)
    assert fft_sizes(96, 128)[:2] == (54, 72) and fft_tiles(96, 128) == (2, 2, 48, 64)


TILED_MAPS = [(96, 128), (100, 132), (157, 209), (64, 209), (200, 100), (97, 129)]   # beyond one in-LDS transform: overlap-save tiles
LARGE_UNTILED = [(120, 50), (50, 150), (3, 209), (150, 60)]      # long thin maps that still fit one transform (Stockham passes: 144, 162, 216)


@pytest.mark.parametrize("H,W,NB,C", [(60, 80, 2, 7), (30, 40, 1, 5), (38, 50, 1, 3), (48, 64, 1, 3), (72, 96, 1, 2), (84, 112, 1, 2),
                                      (44, 90, 1, 2), (90, 60, 1, 2), (11, 13, 3, 4), (9, 16, 2, 2), (2, 5, 1, 2), (1, 1, 1, 1)] +
                         [(h, w, 2, 3) for h, w in TILED_MAPS + LARGE_UNTILED])
def test_fft_forward_matches_torch_fft(H, W, NB, C, device):
    lib = _lib.load()
    P, Q, nbins = fft_sizes(H, W)
    wins, (TY, TX, TH, TW) = tile_windows(H, W)
    T = TY * TX
    assert nbins % 8 == 0 and nbins >= P * (Q // 2 + 1)
    assert P >= (TH + 6 if TY > 1 else H + 3) and Q >= (TW + 6 if TX > 1 else W + 3)
    if (H, W) in TILED_MAPS:
        assert T > 1
    g = torch.Generator().manual_seed(H * 100 + W)
    corr = (torch.rand(NB, C, H, W, generator=g) - 0.3).to(device)
    inv = (0.5 + torch.rand(NB, H, W, generator=g)).to(device)
    X = torch.full((C, NB * T, nbins, 2), float("nan"), device=device)           # channel-major (what the GEMM kernels read)
    tq, tp = twiddles(Q, device), twiddles(P, device)          # keep them alive: the call only takes raw pointers
    _lib.check(lib.os2d_fft_forward(_lib.ptr(corr), _lib.ptr(inv), _lib.ptr(X), _lib.ptr(tq), _lib.ptr(tp),
                                    NB, C, H, W, _lib.current_stream(device)), "os2d_fft_forward")
    x = (corr.clamp(min=0) * inv.unsqueeze(1)).double()
    got = torch.view_as_complex(X)[..., :P * (Q // 2 + 1)].to(torch.complex128).view(C, NB, T, -1)
    for t, (y0, x0, oy, ox, LH, LW) in enumerate(wins):
        # the tile's window of the zero-extended map, then the plain zero-padded transform
        big = torch.zeros(NB, C, H + 2 * LH + 6, W + 2 * LW + 6, dtype=torch.float64, device=device)
        big[:, :, LH:LH + H, LW:LW + W] = x
        win = big[:, :, LH + y0 - oy:LH + y0 - oy + LH, LW + x0 - ox:LW + x0 - ox + LW]
        ref = torch.fft.rfft2(win, s=(P, Q)).reshape(NB, C, -1)                   # [NB,C,P*V], bin = u*V + v
        scale = float(ref.abs().max())
        assert float((got[:, :, t].permute(1, 0, 2) - ref).abs().max()) <= 2e-6 * max(scale, 1e-30), ("tile", t)
    assert float(X[:, :, P * (Q // 2 + 1):].abs().max() if nbins > P * (Q // 2 + 1) else 0.0) == 0.0


@pytest.mark.parametrize("H,W,NB", [(60, 80, 2), (30, 40, 1), (38, 50, 1), (48, 64, 1), (72, 96, 1), (84, 112, 1), (44, 90, 1), (90, 60, 1),
                                    (11, 13, 2), (2, 5, 1)] + [(h, w, 2) for h, w in TILED_MAPS + LARGE_UNTILED])
def test_fft_inverse_matches_torch_fft_and_epilogue(H, W, NB, device):
    """Inverse transform + the layer epilogue (bias, ReLU, per-channel power-of-two scale, fp16 hi|lo split into the
    split-half blocked buffer with zero borders) against torch.fft.irfft2; for tiled maps every tile's spectrum holds its
    part of the map at offset (3, 3) along the tiled axes and arbitrary content elsewhere."""
    lib = _lib.load()
    P, Q, nbins = fft_sizes(H, W)
    wins, (TY, TX, TH, TW) = tile_windows(H, W)
    T = TY * TX
    V = Q // 2 + 1
    Cout = 128
    g = torch.Generator().manual_seed(H + W)
    y_true = torch.randn(NB, Cout, H, W, generator=g).double() * 0.3                 # what the inverse should give back
    Y = torch.zeros(NB, T, Cout, nbins, 2)
    fmax = 0.0
    for t, (y0, x0, oy, ox, LH, LW) in enumerate(wins):
        full = torch.randn(NB, Cout, P, Q, generator=g).double()                     # content outside the crop is arbitrary
        th, tw = min(TH, H - y0), min(TW, W - x0)
        full[:, :, oy:oy + th, ox:ox + tw] = y_true[:, :, y0:y0 + th, x0:x0 + tw]
        fmax = max(fmax, float(full.abs().max()))
        Yc = torch.fft.rfft2(full)                                                   # [NB,Cout,P,V]
        Y[:, t, :, :P * V] = torch.view_as_real(Yc.reshape(NB, Cout, P * V).to(torch.complex64))
    bias = torch.randn(Cout, generator=g) * 0.1
    oexp = torch.randint(0, 6, (Cout,), generator=g)
    bp = torch.zeros(3 * 128)
    bp[:Cout] = bias
    bp[256:256 + Cout] = torch.exp2(oexp.float())
    shb_bytes = lib.os2d_shb_bytes(Cout, H, W)
    out = torch.full((NB * shb_bytes,), 0x5A, dtype=torch.uint8, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    tq, tp, Yd, bpd = twiddles(Q, device), twiddles(P, device), Y.to(device), bp.to(device)
    _lib.check(lib.os2d_fft_inverse(_lib.ptr(Yd), _lib.ptr(bpd), _lib.ptr(out), _lib.ptr(tq), _lib.ptr(tp), NB, Cout, H, W,
                                    _lib.ptr(status), _lib.current_stream(device)), "os2d_fft_inverse")
    val, border = shb_decode(out, NB, Cout, H, W)                                                  # scaled values
    got = val.cpu() / torch.exp2(oexp.double()).view(1, -1, 1, 1)
    ref = torch.relu(y_true + bias.double().view(1, -1, 1, 1))
    assert float((got - ref).abs().max()) < 2e-6 * fmax
    assert border == 0.0
    assert int(status.item()) == 0


def test_weight_spectra_cache_is_keyed_by_transform_size_and_bounded(device, monkeypatch):
    """Map sizes that share a transform size share ONE cached weight spectrum; the cache drops the least recently used
    size above its byte cap and is invalidated when a parameter changes."""
    from os2d_amd.modeling import head as head_mod
    from os2d_amd.utils import synthetic
    net = head_mod.TransformationNet(output_dim=6)
    net.load_state_dict(synthetic.make_transform_net_state(6, seed=2))
    net.to(device).eval()
    a = net.spectra(12, 20)          # P = 16, Q = 24
    b = net.spectra(13, 21)          # same transform size
    assert a[0].data_ptr() == b[0].data_ptr() and len(net._spectra_cache) == 1
    c = net.spectra(20, 30)          # P = 24, Q = 36
    assert len(net._spectra_cache) == 2 and c[0].data_ptr() != a[0].data_ptr()
    one = next(iter(net._spectra_cache.values())).nbytes()
    monkeypatch.setenv("OS2D_FFT_CACHE_BYTES", str(one + 1))
    d = net.spectra(30, 40)          # larger than the cap: everything else goes, the new entry stays
    assert list(net._spectra_cache) == [(36, 48, False)] and d[3] == 36 * 25 + (-36 * 25) % 8
    monkeypatch.delenv("OS2D_FFT_CACHE_BYTES")
    net.spectra(12, 20)
    with torch.no_grad():
        net.conv[0].weight.mul_(1.5)
    e = net.spectra(12, 20)
    assert list(net._spectra_cache) == [(16, 24, False)]
    assert not torch.equal(e[0], a[0])


@pytest.mark.parametrize("H,W", [(11, 13), (30, 40), (60, 80), (96, 128)])
def test_device_built_weight_spectra_match_torch_fft(H, W, device):
    """os2d_spectral_weights_build (spectra_pack.hip: a 7-term DFT per axis in float64, packed on the device) against the
    definition - torch.fft.rfft2 in float64 of the BatchNorm-folded filters placed at ((3 - t) mod P, (3 - s) mod Q): the
    complex64 layout of os2d_spectral_gemm to fp32 round-off, the split-fp16 layout of os2d_spectral_gemm_f16 (hi + lo times
    the row scale) to 2^-21 of the row maximum, padding bins / channels exactly zero, row scales powers of two that put the
    row maximum in (16384, 32768]."""
    from os2d_amd.modeling import head as head_mod
    from os2d_amd.utils import synthetic
    net = head_mod.TransformationNet(output_dim=6)
    net.load_state_dict(synthetic.make_transform_net_state(6, seed=11))
    net.to(device).eval()
    P, Q, nbins = fft_sizes(H, W)
    V = Q // 2 + 1
    (w1, _), _, _ = net._folded()
    k = torch.zeros(128, 225, P, Q, dtype=torch.float64, device=device)
    k[:, :, ((3 - torch.arange(7, device=device)) % P).view(-1, 1), ((3 - torch.arange(7, device=device)) % Q).view(1, -1)] = w1
    K = torch.fft.rfft2(k).reshape(128, 225, P * V)                       # [o, c, bin]
    del k
    G = nbins // 8
    # ---- complex64 layout [g][half][c][j][r]
    w32 = net.spectra(H, W)[0].view(G, 2, 225, 8, 64, 2)
    got = torch.view_as_complex(w32.double().contiguous()).permute(1, 4, 2, 0, 3).reshape(128, 225, nbins)      # [half*64+r, c, g*8+j]
    scale = float(K.abs().max())
    assert float((got[:, :, :P * V] - K).abs().max()) <= 2e-7 * scale
    assert float(got[:, :, P * V:].abs().max()) == 0.0 if nbins > P * V else True
    # ---- split-fp16 layout [g][half][ks][j][grp][hi|lo][o][c4, (re, im)] + 128 row scales, for the transform size and the bin
    # order (bin = v * P + u) of the matrix-product transforms (os2d_dft_sizes)
    P, Q, nbins, _ = dft_sizes(H, W)
    V, G = Q // 2 + 1, nbins // 8
    assert P % 4 == 0 and Q % 2 == 0 and nbins % 8 == 0
    k = torch.zeros(128, 225, P, Q, dtype=torch.float64, device=device)
    k[:, :, ((3 - torch.arange(7, device=device)) % P).view(-1, 1), ((3 - torch.arange(7, device=device)) % Q).view(1, -1)] = w1
    K = torch.fft.rfft2(k).permute(0, 1, 3, 2).reshape(128, 225, V * P)   # [o, c, bin = v * P + u]
    del k
    buf = net.spectra(H, W, split=True)[0]
    KS = 29
    nunits = G * 2 * KS * 8 * 2 * 2 * 64
    units = buf[:nunits * 16].view(torch.float16).view(G, 2, KS, 8, 2, 2, 64, 4, 2).double()
    wscale = buf[nunits * 16:].view(torch.float32).double()
    val = units[:, :, :, :, :, 0] + units[:, :, :, :, :, 1]                  # hi + lo: [g, half, ks, j, grp, o, c4, ri]
    val = val.permute(1, 5, 2, 4, 6, 0, 3, 7).reshape(128, KS * 8, nbins, 2)  # [half*64+o, ks*8+grp*4+c4, g*8+j, ri]
    rec = torch.view_as_complex(val.contiguous()) * wscale.view(-1, 1, 1)
    rowmax = torch.maximum(K.real.abs(), K.imag.abs()).flatten(1).amax(dim=1)
    assert float(((rec[:, :225, :P * V] - K).abs() / rowmax.view(-1, 1, 1)).max()) <= 2.0 ** -21
    assert float(rec[:, 225:].abs().max()) == 0.0 and (float(rec[:, :, P * V:].abs().max()) == 0.0 if nbins > P * V else True)
    scaled = rowmax / wscale
    assert bool(((scaled > 16384.0 * (1 - 1e-12)) & (scaled <= 32768.0)).all())
    assert bool((torch.log2(wscale) == torch.log2(wscale).round()).all())


def test_weight_spectra_miss_cost_is_bounded(device):
    """a dataset fed at its own aspect ratios meets ~50 transform sizes (tools/bench_size_churn.py); every
    new size costs one construction of the weight spectra (a 7-term DFT per axis as float64 matrix products + the fp16 split:
    ~20 ms on the MI355X, 50 ms with the round-2 rfft2 of zero maps).  Bounds: a miss < 120 ms, a hit < 2 ms, and a miss
    reproduces exactly what the first construction gave (the cache is not part of the result)."""
    import time
    from os2d_amd.modeling import head as head_mod
    from os2d_amd.utils import synthetic
    net = head_mod.TransformationNet(output_dim=6)
    net.load_state_dict(synthetic.make_transform_net_state(6, seed=2))
    net.to(device).eval()
    net.spectra(30, 40, split=True)                      # warm-up of the float64 kernels / allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = net.spectra(60, 80, split=True)
    torch.cuda.synchronize()
    miss = time.perf_counter() - t0
    hit = float("inf")
    for _ in range(3):           # (best of 3: wall-clock guards must survive one host hiccup)
        t0 = time.perf_counter()
        again = net.spectra(60, 80, split=True)
        torch.cuda.synchronize()
        hit = min(hit, time.perf_counter() - t0)
    assert again[0].data_ptr() == first[0].data_ptr()
    keep = first[0].clone()
    net._spectra_cache.clear()
    rebuilt = net.spectra(60, 80, split=True)
    assert torch.equal(rebuilt[0], keep)
    print("weight spectra for 64 x 84: miss {:.1f} ms, hit {:.3f} ms, {:.0f} MB".format(miss * 1e3, hit * 1e3, keep.numel() / 1e6))
    assert miss < 0.5 and hit < 0.002        # a miss builds 654 MB of spectra on the device (~5 - 20 ms), a hit is a dictionary lookup


@pytest.mark.parametrize("H,W,NB", [(11, 13, 5), (30, 40, 70)])
def test_split_half_spectral_gemm_matches_float64(H, W, NB, device):
    """os2d_spectral_gemm (fp32 matrix cores) and os2d_spectral_gemm_f16 (spectra split into fp16 hi + lo on the half-precision
    matrix cores; input spectra in rows [C, NB, nbins] or - os2d_spectral_gemm_f16_quads, what the head runs - in quads of
    bins x channels [nbins/4, NB, Cpad, 4]) against a float64 product, with the weight spectra as TransformationNet.spectra
    packs them: the fp32 ones for the sizes / bin order of the in-LDS FFTs, the split ones for those of the matrix-product
    transforms (bin = v * P + u)."""
    from os2d_amd.modeling import head as head_mod
    from os2d_amd.utils import synthetic
    lib = _lib.load()
    net = head_mod.TransformationNet(output_dim=6)
    net.load_state_dict(synthetic.make_transform_net_state(6, seed=3))
    net.to(device).eval()
    # input maps with samples in [0, 1] (what the layer sees), a few channels forced to the extremes of the range
    g = torch.Generator().manual_seed(H + W)
    x = torch.rand(NB, 225, H, W, generator=g, dtype=torch.float64)
    x[:, 0] = 1.0                       # DC bin = H * W: the largest value the scale must hold
    x[:, 1] *= 1e-6                     # tiny channel: its lo halves are subnormal
    (w1, _), _, _ = net._folded()
    st = _lib.current_stream(device)
    for name in ("f32", "f16 rows", "f16 quads"):
        if name == "f32":
            P, Q, nbins = fft_sizes(H, W)
        else:
            P, Q, nbins, _ = dft_sizes(H, W)
        V = Q // 2 + 1
        k = torch.zeros(128, 225, P, Q, dtype=torch.float64)
        k[:, :, ((3 - torch.arange(7)) % P).view(-1, 1), ((3 - torch.arange(7)) % Q).view(1, -1)] = w1.cpu()
        K, Xc = torch.fft.rfft2(k), torch.fft.rfft2(x, s=(P, Q))                          # [.., P, V]
        if name != "f32":
            K, Xc = K.transpose(2, 3), Xc.transpose(2, 3)                               # bin = v * P + u
        K, Xc = K.reshape(128, 225, P * V), Xc.reshape(NB, 225, P * V)
        X = torch.zeros(NB, 225, nbins, 2)
        X[:, :, :P * V] = torch.view_as_real(Xc.to(torch.complex64))
        ref = torch.einsum("ocb,ncb->nob", K, torch.view_as_complex(X[:, :, :P * V].double().contiguous()))
        scale = float(ref.abs().max())
        Xd = X.permute(1, 0, 2, 3).contiguous().to(device)              # channel-major rows
        if name == "f32":
            w32 = net.spectra(H, W)[0]
            Y = torch.full((NB, 128, nbins, 2), float("nan"), device=device)
            _lib.check(lib.os2d_spectral_gemm(_lib.ptr(w32), _lib.ptr(Xd), _lib.ptr(Y), NB, 225, 128, nbins, st), "gemm")
        else:
            w16 = net.spectra(H, W, split=True)[0]
            assert w16.numel() == lib.os2d_spectral_weight16_bytes(225, nbins)
            xs = lib.os2d_dft_xscale(H, W)
            assert xs * H * W <= 65504 < 2 * xs * H * W
            Yq = torch.full((nbins // 4, NB, 128, 4, 2), float("nan"), device=device)      # written in quads of bins (OS2D_SPECTRA_QUADS)
            if name == "f16 rows":
                _lib.check(lib.os2d_spectral_gemm_f16(_lib.ptr(w16), _lib.ptr(Xd), _lib.ptr(Yq), NB, 225, 128, nbins, xs, st), "gemm16")
            else:
                cpad = lib.os2d_dft_channel_stride(225)
                Xq = torch.full((nbins // 4, NB, cpad, 4, 2), float("nan"))                # pad channels: never read as numbers
                Xq[:, :, :225] = X.view(NB, 225, nbins // 4, 4, 2).permute(2, 0, 1, 3, 4)
                Xq = quads_to_blocked(Xq).to(device)                                       # both sides in blocks of 64 pairs
                Yb = torch.full((Yq.numel(),), float("nan"), device=device)
                _lib.check(lib.os2d_spectral_gemm_f16_quads(_lib.ptr(w16), _lib.ptr(Xq), _lib.ptr(Yb), NB, 225, 128, nbins, xs, st), "gemm16 quads")
                Yq = blocked_to_quads(Yb, nbins // 4, NB, 128)
            Y = y_quads_to_rows(Yq.contiguous(), NB, 128, nbins)
        got = torch.view_as_complex(Y.cpu()[:, :, :P * V].contiguous()).to(torch.complex128)
        err = float((got - ref).abs().max())
        print("spectral GEMM {} {}x{} NB={}: max err {:.3g} of {:.3g}".format(name, H, W, NB, err, scale))
        assert err <= 2e-6 * scale, name


@pytest.mark.parametrize("H,W,NB", [(60, 80, 3), (30, 40, 70), (96, 128, 2), (11, 13, 5), (157, 209, 1)])
def test_quad_layout_of_the_inverse_transform_equals_the_row_layout(H, W, NB, device):
    """OS2D_SPECTRA_QUADS (Y [nbins/4, NBT, Cout, 4]: what the split-half GEMM writes) against OS2D_SPECTRA_ROWS, which the
    test above pins to torch.fft: the inverse transform gives the same bytes from the permuted input - untiled and tiled
    maps, more than 64 pairs."""
    lib = _lib.load()
    P, Q, nbins = fft_sizes(H, W)
    TY, TX, _, _ = fft_tiles(H, W)
    NBT = NB * TY * TX
    g = torch.Generator().manual_seed(H + 7 * W)
    tq, tp = twiddles(Q, device), twiddles(P, device)
    st = _lib.current_stream(device)
    Cout = 128
    Yr = torch.randn(NBT, Cout, nbins, 2, generator=g).to(device)
    bp = torch.zeros(3 * 128)
    bp[:Cout] = torch.randn(Cout, generator=g) * 0.1
    bp[256:256 + Cout] = 1.0
    bpd = bp.to(device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    shb = lib.os2d_shb_bytes(Cout, H, W)
    out_r = torch.full((NB * shb,), 0x5A, dtype=torch.uint8, device=device)
    out_q = torch.full((NB * shb,), 0xA5, dtype=torch.uint8, device=device)
    _lib.check(lib.os2d_fft_inverse_ex(_lib.ptr(Yr), _lib.ptr(bpd), _lib.ptr(out_r), _lib.ptr(tq), _lib.ptr(tp), NB, Cout, H, W,
                                       _lib.ptr(status), 0, st), "inv rows")
    Yq = y_rows_to_quads(Yr)
    _lib.check(lib.os2d_fft_inverse_ex(_lib.ptr(Yq), _lib.ptr(bpd), _lib.ptr(out_q), _lib.ptr(tq), _lib.ptr(tp), NB, Cout, H, W,
                                       _lib.ptr(status), 1, st), "inv quads")
    assert torch.equal(out_q, out_r)


@pytest.mark.parametrize("kind", ["fft", "dft", "gemm16", "corr", "corrp", "sample"])
def test_kernels_are_stable_next_to_mfma_kernels(kind, device):
    """Regression test of the packed-FP32 finding (docs/DESIGN_HISTORY_r1-r3.md section 8): a victim kernel on four streams while the direct
    7x7 kernel (half-precision MFMA at full rate) runs on three others must return exactly the bytes it returns alone.
    Victims: the transforms (with v_pk_*_f32 instructions 8 of 16 such runs differed in 16-lane groups of single registers)
    and the two other kernels with hand-made LDS-only barriers and LDS-DMA pipelines - the split-half spectral GEMM and the
    correlation.  tools/diag_aggressor.py runs the same harness for hundreds of rounds."""
    from concurrency_victims import Harness
    h = Harness(device, NB=64)
    ref = h.reference(kind)
    for it in range(8):
        bad, _ = h.contend(kind, ref, aggressor=True)
        assert not bad, (kind, "round", it, "(victim stream, output) that differ:", bad)
