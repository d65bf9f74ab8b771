"""GPU: the forward transform of the 64-row plan (os2d_amd/csrc/dft_mfma.h: step 1's accumulators stay in the wave as the B
operand of step 2, the complex combination is a lane swap) through ``os2d_dft_forward`` against ``numpy.fft.rfft2`` in float64.

Cases (H, W, pairs, channels, norms), the plan of each asserted (EXPECTED_PLAN):
  (54, 52, 1, 5)   the smallest map whose plan under the default size policy is the 64-row transform (found by a search of
                   ``os2d_dft_sizes`` over 1 <= H < 140, 1 <= W < 200): the 16-byte ``FAST`` loads, a ragged channel group
  (61, 81, 2, 4)   the largest untiled window, a width not divisible by 4 (the 4-byte aligned loads), two pairs
  (60, 80, 1, 8)   the call form of the 5x5 layer: no norms (``inv_norm`` null), input in [0, 1]
  (61, 97, 1, 5)   the smallest map of that search with a TILED 64-row plan (1 x 2 tiles, windows of 61 x 55): the ``TILED``
                   instantiation
  (54, 8, 1, 5)    a narrow map.  The planner cuts it into 2 x 1 tiles on 36 x 46 (fewer bins than one 64 x 84 transform; every
                   map narrower than 52 columns is cut like this), so a single k-step in step 1 does not occur on the 64-row plan.
                   The case runs code this kernel change leaves alone and must reproduce the parent's figure.

Tolerance: the max-abs error of every case is at most TWICE the error the parent commit's kernel gives for the same seeded
inputs (PARENT_ERR) - the rule of tests/test_dft_radix2_gpu.py, for its reason: the change keeps every operand rounding and
splits one fp32 accumulation chain of 64 terms into two of 32 joined by one add, so it should be no worse; the factor covers a
different realisation of the roundings over the few hundred thousand values of a case.

Also per case: the padding bins are exactly zero and a repeated call gives identical bits; the one-pair call of the two-pair case
is bit-equal to its slice."""
import numpy as np
import pytest
import torch

from freq_util import matrices, windows
from os2d_amd import _lib

pytestmark = pytest.mark.gpu

# (H, W, NB, C, with norms)
CASES = [(54, 52, 1, 5, True), (61, 81, 2, 4, True), (60, 80, 1, 8, False), (61, 97, 1, 5, True), (54, 8, 1, 5, True)]
EXPECTED_PLAN = {(54, 52): (64, 84, 1, 1), (61, 81): (64, 84, 1, 1), (60, 80): (64, 84, 1, 1), (61, 97): (64, 84, 1, 2),
                 (54, 8): (36, 46, 2, 1)}      # P, Q, TY, TX
# max |X - float64| of the parent commit f382c1e (step 1's rows through LDS), measured once on an MI355X with the inputs of
# forward_inputs below
PARENT_ERR = {
    (54, 52, 1, 5, True): 5.0358e-05,
    (61, 81, 2, 4, True): 1.0149e-04,
    (60, 80, 1, 8, False): 1.5241e-04,
    (61, 97, 1, 5, True): 4.8467e-05,
    (54, 8, 1, 5, True): 4.4014e-06,
}


def check_plan(H, W):
    wins, plan = windows(H, W)
    P, Q, nbins, TY, TX = plan[:5]
    assert (P, Q, TY, TX) == EXPECTED_PLAN[(H, W)]
    return wins, plan


def forward_inputs(H, W, NB, C, norms):
    """Pair nb of any NB has the same content (a generator per pair): the 1-pair input is the first pair of the 2-pair input."""
    corr, inv = [], []
    for nb in range(NB):
        g = torch.Generator().manual_seed(3000 * H + 30 * W + nb)
        if norms:
            corr.append(torch.rand(C, H, W, generator=g) - 0.3)
            inv.append(0.4 + torch.rand(H, W, generator=g))          # relu(corr) * inv <= 0.7 * 1.4 < 1, like the normalised maps
        else:
            corr.append(torch.rand(C, H, W, generator=g))            # the 5x5 layer's input: already in [0, 1]
    return torch.stack(corr), (torch.stack(inv) if norms else None)


def forward_run(H, W, NB, C, norms, device):
    """-> the spectra buffer [nbins / 4, NB T, cpad, 4, 2] (device)"""
    lib = _lib.load()
    wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW) = check_plan(H, W)
    corr, inv = forward_inputs(H, W, NB, C, norms)
    corr, inv = corr.to(device), (inv.to(device) if norms else None)
    cpad = lib.os2d_dft_channel_stride(C)
    X = torch.full((nbins // 4, NB * TY * TX, cpad, 4, 2), float("nan"), device=device)
    mats = matrices(P, Q, device)
    _lib.check(lib.os2d_dft_forward(_lib.ptr(corr), _lib.ptr(inv), _lib.ptr(X), _lib.ptr(mats), NB, C, H, W, _lib.current_stream(device)),
               "os2d_dft_forward")
    torch.cuda.synchronize()
    return X


def forward_case(H, W, NB, C, norms, device):
    """-> (max |X - float64| over every bin of every tile, the spectra buffer); asserts the zero padding bins"""
    wins, (P, Q, nbins, TY, TX, TH, TW, LH, LW) = check_plan(H, W)
    T, V = TY * TX, Q // 2 + 1
    X = forward_run(H, W, NB, C, norms, device)
    corr, inv = forward_inputs(H, W, NB, C, norms)
    x = corr.clamp(min=0)
    x = (x * inv.unsqueeze(1) if norms else x).double().numpy()         # the fp32 product the kernel forms, then float64
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


@pytest.mark.parametrize("H,W,NB,C,norms", CASES)
def test_forward_against_float64(H, W, NB, C, norms, device):
    err, X = forward_case(H, W, NB, C, norms, device)
    parent = PARENT_ERR[(H, W, NB, C, norms)]
    print("forward {}x{} NB={} C={} norms={}: max abs error {:.4e} (parent {:.4e})".format(H, W, NB, C, norms, err, parent))
    assert err <= 2.0 * parent
    again = forward_run(H, W, NB, C, norms, device)
    assert torch.equal(X.view(torch.int32), again.view(torch.int32))          # the same bits, the NaN fill of unwritten channels included


def test_one_pair_is_the_slice_of_two_pairs(device):
    H, W, NB, C, norms = CASES[1]
    assert NB == 2
    one, two = forward_run(H, W, 1, C, norms, device), forward_run(H, W, 2, C, norms, device)
    assert torch.equal(one[:, 0].contiguous().view(torch.int32), two[:, 0].contiguous().view(torch.int32))
