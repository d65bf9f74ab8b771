"""GPU: the 64-row plan (os2d_amd/csrc/dft_mfma.h: step 2 of the forward kernel as two 32-point products and a butterfly; the
inverse kernel next to it) against a float64 numpy DFT of the same inputs, on the headline map
(60 x 80 on 64 x 84) with 1 and 3 pairs and 5 (a partial channel group) and 225 channels; next to it the 72 x 96 level (2 x 2
tiles on 44 x 54: no 64-row transform, asserted) and a 49 x 65 map (52 x 68: the dense product) - the dispatch leaves the
other sizes alone.

Tolerances.  The bound of every case is TWICE the max-abs error against float64 that the dense-product kernels of the parent
commit produced for exactly these inputs (PARENT_ERR below): the radix-2 form sums half as many terms per output and adds one
fp32 rounding in the butterfly, so it should not be worse; the factor covers a different realisation of the roundings on the
few hundred thousand values of a case.  The cases without a 64-row transform run unchanged code: they must reproduce the
parent's figure, and are held to the same rule.

Determinism: two calls give identical bits, and a 1-pair call is bit-equal to the first pair of a 3-pair call."""
import numpy as np
import pytest
import torch

from freq_util import matrices, shb_decode, windows
from os2d_amd import _lib

pytestmark = pytest.mark.gpu

# max |result - float64| of the parent commit eed19fd (dense 64-point products), measured once on an MI355X with the
# inputs of forward_case / inverse_case below
PARENT_ERR = {
    ("forward", 60, 80, 1, 5): 7.6397e-05,
    ("forward", 60, 80, 3, 5): 9.0716e-05,
    ("forward", 60, 80, 1, 225): 1.7648e-04,
    ("forward", 60, 80, 3, 225): 2.0127e-04,
    ("forward", 72, 96, 1, 5): 3.2257e-05,
    ("forward", 49, 65, 1, 5): 3.1758e-05,
    ("inverse", 60, 80, 1): 2.5101e-08,
    ("inverse", 60, 80, 3): 2.7135e-08,
    ("inverse", 72, 96, 1): 3.7471e-08,
    ("inverse", 49, 65, 1): 3.1424e-08,
}
EXPECTED_PLAN = {(60, 80): (64, 84, 1, 1), (72, 96): (44, 54, 2, 2), (49, 65): (52, 68, 1, 1)}      # P, Q, TY, TX
COUT = 128          # the 7x7 layer's output channels (the ABI takes no other count)


def check_plan(H, W):
    wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW) = windows(H, W)
    assert (P, Q, TY, TX) == EXPECTED_PLAN[(H, W)]
    return wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW)


def forward_inputs(H, W, NB, C):
    """Pair nb of any NB has the same content (a generator per pair): the 1-pair input is the first pair of the 3-pair input."""
    corr, inv = [], []
    for nb in range(NB):
        g = torch.Generator().manual_seed(1000 * H + 10 * W + nb)
        corr.append(torch.rand(C, H, W, generator=g) - 0.3)
        inv.append(0.4 + torch.rand(H, W, generator=g))              # relu(corr) * inv <= 0.7 * 1.4 < 1, like the normalised maps
    return torch.stack(corr), torch.stack(inv)


def forward_run(H, W, NB, C, device):
    """-> the spectra buffer [nbins / 4, NB T, cpad, 4, 2] (device)"""
    lib = _lib.load()
    wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW) = check_plan(H, W)
    corr, inv = forward_inputs(H, W, NB, C)
    corr, inv = corr.to(device), inv.to(device)
    cpad = lib.os2d_dft_channel_stride(C)
    X = torch.full((nbins // 4, NB * TY * TX, cpad, 4, 2), float("nan"), device=device)
    mats = matrices(P, Q, device)
    _lib.check(lib.os2d_dft_forward(_lib.ptr(corr), _lib.ptr(inv), _lib.ptr(X), _lib.ptr(mats), NB, C, H, W, _lib.current_stream(device)),
               "os2d_dft_forward")
    torch.cuda.synchronize()
    return X


def forward_case(H, W, NB, C, device):
    """-> (max |X - float64| over every bin of every tile, the spectra buffer)"""
    wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW) = check_plan(H, W)
    T, V = TY * TX, Q // 2 + 1
    X = forward_run(H, W, NB, C, device)
    corr, inv = forward_inputs(H, W, NB, C)
    x = (corr.clamp(min=0) * inv.unsqueeze(1)).double().numpy()         # the fp32 product the kernel forms, then float64
    rows = X.permute(1, 2, 0, 3, 4).reshape(NB * T, X.shape[2], nbins, 2).cpu().double().numpy()
    got = (rows[:, :C, :P * V, 0] + 1j * rows[:, :C, :P * V, 1]).reshape(NB, T, C, V, P)
    worst = 0.0
    for t, (y0, x0, oy, ox) in enumerate(wins):
        big = np.zeros((NB, C, H + 2 * LH + 6, W + 2 * LW + 6))
        big[:, :, LH:LH + H, LW:LW + W] = x
        win = big[:, :, LH + y0 - oy:LH + y0 - oy + LH, LW + x0 - ox:LW + x0 - ox + LW]
        ref = np.fft.rfft2(win, s=(P, Q)).transpose(0, 1, 3, 2)         # [NB, C, V, P]: bin = v * P + u
        d = got[:, t] - ref
        worst = max(worst, float(np.abs(d.real).max()), float(np.abs(d.imag).max()))
    assert float(np.abs(rows[:, :C, P * V:]).max(initial=0.0)) == 0.0      # the padding bins
    return worst, X


def inverse_inputs(H, W, NB, P, Q, nbins, T):
    V = Q // 2 + 1
    Y = torch.zeros(NB * T, COUT, nbins, 2)
    for nb in range(NB):
        g = torch.Generator().manual_seed(7000 * H + 70 * W + nb)
        Y[nb * T:(nb + 1) * T, :, :P * V] = torch.randn(T, COUT, P * V, 2, generator=g)
    g = torch.Generator().manual_seed(H + W)
    bias = torch.randn(COUT, generator=g) * 0.01
    return Y, bias


def inverse_run(H, W, NB, device):
    """-> (the activation buffer as bytes (device), bytes per pair)"""
    lib = _lib.load()
    wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW) = check_plan(H, W)
    T = TY * TX
    Y, bias = inverse_inputs(H, W, NB, P, Q, nbins, T)
    bp = torch.zeros(3 * 128)
    bp[:COUT] = bias
    bp[256:256 + COUT] = 4096.0           # |y| of these spectra is a few hundredths: activations of ~2^7, both halves normal
    Yq = Y.view(NB * T, COUT, nbins // 4, 4, 2).permute(2, 0, 1, 3, 4).contiguous().to(device)      # [nbins / 4, NBT, Cout, 4]
    shb_bytes = lib.os2d_shb_bytes(COUT, H, W)
    out = torch.full((NB * shb_bytes,), 0x5A, dtype=torch.uint8, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    mats, bpd = matrices(P, Q, device), bp.to(device)
    _lib.check(lib.os2d_dft_inverse(_lib.ptr(Yq), _lib.ptr(bpd), _lib.ptr(out), _lib.ptr(mats), NB, COUT, H, W, _lib.ptr(status),
                                    _lib.current_stream(device)), "os2d_dft_inverse")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return out, shb_bytes


def inverse_case(H, W, NB, device):
    """-> (max |relu(y + bias) - float64|, the activation buffer)"""
    wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW) = check_plan(H, W)
    T, V = TY * TX, Q // 2 + 1
    out, _ = inverse_run(H, W, NB, device)
    Y, bias = inverse_inputs(H, W, NB, P, Q, nbins, T)
    Yc = Y.double().numpy()
    Yc = (Yc[..., :P * V, 0] + 1j * Yc[..., :P * V, 1]).reshape(NB, T, COUT, V, P).transpose(0, 1, 2, 4, 3)      # [NB, T, Cout, P, V]
    # the kernel's inverse of a half spectrum: Re of the v sum with weights 1 (v = 0, Q / 2) and 2 - numpy's irfft, which
    # also drops the imaginary parts of those two columns
    full = np.fft.irfft2(Yc, s=(P, Q))
    ref = np.zeros((NB, COUT, H, W))
    for t, (y0, x0, oy, ox) in enumerate(wins):
        th, tw = min(TH, H - y0), min(TW, W - x0)
        ref[:, :, y0:y0 + th, x0:x0 + tw] = full[:, t, :, oy:oy + th, ox:ox + tw]
    ref = np.maximum(ref + bias.double().numpy().reshape(1, -1, 1, 1), 0.0)
    got = (shb_decode(out, NB, COUT, H, W)[0].cpu() / 4096.0).numpy()
    return float(np.abs(got - ref).max()), out


FORWARD_CASES = [(60, 80, 1, 5), (60, 80, 3, 5), (60, 80, 1, 225), (60, 80, 3, 225), (72, 96, 1, 5), (49, 65, 1, 5)]
INVERSE_CASES = [(60, 80, 1), (60, 80, 3), (72, 96, 1), (49, 65, 1)]


@pytest.mark.parametrize("H,W,NB,C", FORWARD_CASES)
def test_forward_against_float64(H, W, NB, C, device):
    err, X = forward_case(H, W, NB, C, device)
    parent = PARENT_ERR[("forward", H, W, NB, C)]
    print("forward {}x{} NB={} C={}: max abs error {:.4e} (parent {:.4e})".format(H, W, NB, C, err, parent))
    assert err <= 2.0 * parent
    again = forward_run(H, W, NB, C, device)
    assert torch.equal(X.view(torch.int32), again.view(torch.int32))          # the same bits, the NaN fill of unwritten channels included


@pytest.mark.parametrize("H,W,NB", INVERSE_CASES)
def test_inverse_against_float64(H, W, NB, device):
    err, out = inverse_case(H, W, NB, device)
    parent = PARENT_ERR[("inverse", H, W, NB)]
    print("inverse {}x{} NB={}: max abs error {:.4e} (parent {:.4e})".format(H, W, NB, err, parent))
    assert err <= 2.0 * parent
    again, _ = inverse_run(H, W, NB, device)
    assert torch.equal(out, again)


@pytest.mark.parametrize("C", [5, 225])
def test_one_pair_is_the_slice_of_three_pairs(C, device):
    H, W = 60, 80
    one, three = forward_run(H, W, 1, C, device), forward_run(H, W, 3, C, device)
    assert torch.equal(one[:, 0].contiguous().view(torch.int32), three[:, 0].contiguous().view(torch.int32))
    if C == 5:
        (o1, nbytes), (o3, _) = inverse_run(H, W, 1, device), inverse_run(H, W, 3, device)
        assert torch.equal(o1, o3[:nbytes])
