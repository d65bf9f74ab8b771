"""Float64 / integer model of the order-independent d corr scatter (os2d_train_decode_backward_det, include/os2d_train.h):
the rule of os2d_amd/csrc_train/decode_det.h restated in Python, and the float64 addends of ``backward_model``'s decode stage
rounded onto the pair's fixed-point grid and added as integers.

Unlike ``backward_model.decode_backward_model`` (which lets autograd differentiate the forward) this has to know the addends one
by one, so the four bilinear taps are written out here, from the SAME float64 sample coordinates ``decode_forward`` returns;
tests/test_backward_det.py checks the two against each other.
"""
import functools

import numpy as np
import torch

import backward_model as M

DET_ZERO, DET_NONFINITE, DET_REFUSED = -1000, -1001, -1002     # OS2D_TRAIN_DET_* of include/os2d_train.h
MAX_LOG2 = 23                                                  # L at most: H W <= 2^21


def float_bits(x):
    """The fp32 bit pattern of |x|."""
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0]) & 0x7FFFFFFF


def log2_addends(H, W):
    """L = ceil(log2(4 H W)), None for a shape the rule refuses."""
    if H < 1 or W < 1:
        return None
    L = max(2, (4 * H * W - 1).bit_length())
    return L if L <= MAX_LOG2 else None


def floor_log2_of_word(bits):
    """floor(log2 m) of the finite non-zero fp32 value with the bit pattern ``bits``."""
    return (bits >> 23) - 127 if bits >> 23 else bits.bit_length() - 1 - 149


def exponent(bits, H, W):
    """os2d_train_decode_det_exponent: m 2^e in [2^(60-L), 2^(61-L))."""
    L = log2_addends(H, W)
    if L is None:
        return DET_REFUSED
    if bits == 0:
        return DET_ZERO
    if bits >= 0x7F800000:
        return DET_NONFINITE
    return 60 - L - floor_log2_of_word(bits)


def workspace_bytes(NB, H, W):
    return (NB * M.K * H * W * 8 + NB * 4 + 255) // 256 * 256


def decode_det_model(corr, params, dcls, dcls_det, inverse, stride, rec_field):
    """corr [NB,225,H,W], params [NB,P,H,W], dcls / dcls_det [NB,H,W] (None = zero).  Returns a dict:
         acc     int64 [NB,225,HW]   the integer sums (units of 2^-e of their pair)
         e       [NB]                the pairs' exponents (DET_ZERO for an all-zero pair)
         count   int64 [NB,225,HW]   addends a cell received (zero-valued ones included)
         added   float64 [NB,225,HW] (float)(acc 2^-e): what the convert pass adds to d corr
         resid   float64 [NB,225,HW] sum over the cell's addends of (addend 2^e - its integer), in grid steps: the unquantised
                                     sum is (acc + resid) 2^-e.  x - rint(x) is exact in float64 and at most 1/2, so the few
                                     hundred of them add up to an error far below 2^-40 of a step
         taps    float64 [NB,225,HW] the plain float64 sum of the unquantised addends (the tap restatement on its own)
    The pair's word is the largest fp32 |dcls + dcls_det|, as the kernel forms it; the addends are float64:
    (dcls + dcls_det) / 121 times the bilinear weight, so that the only difference from the exact model is the grid."""
    NB, _, H, W = corr.shape
    HW = H * W
    zero = torch.zeros(NB, H, W)
    g32 = ((zero if dcls is None else dcls).float() + (zero if dcls_det is None else dcls_det).float()).reshape(NB, HW)
    g64 = ((zero if dcls is None else dcls).to(M.F64) + (zero if dcls_det is None else dcls_det).to(M.F64)).reshape(NB, HW).numpy()
    with torch.no_grad():
        _, _, aux = M.decode_forward(corr.to(M.F64), params.to(M.F64), inverse, stride, rec_field)
    lo, hi = M.O.POOL_BORDER, M.T - M.O.POOL_BORDER
    g_fm = aux["g_fm"].reshape(NB, HW, M.T, M.T, 2)[:, :, lo:hi, lo:hi].numpy()       # [nb, n, row i, col j, xy]
    X, Y = np.clip(g_fm[..., 0], 0.0, W - 1.0), np.clip(g_fm[..., 1], 0.0, H - 1.0)
    x0, y0 = np.floor(X), np.floor(Y)
    ax, ay = X - x0, Y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ii, jj = np.meshgrid(np.arange(lo, hi), np.arange(lo, hi), indexing="ij")
    chan = (jj * M.T + ii).reshape(1, 1, hi - lo, hi - lo)                               # x-major: channel j*15 + i
    acc = np.zeros((NB, M.K * HW), dtype=np.int64)
    count = np.zeros((NB, M.K * HW), dtype=np.int64)
    resid = np.zeros((NB, M.K * HW))
    taps = np.zeros((NB, M.K * HW))
    es = []
    npool = float((hi - lo) ** 2)
    for nb in range(NB):
        e = exponent(float_bits(float(g32[nb].abs().max())) if bool(torch.isfinite(g32[nb]).all()) else 0x7FC00000, H, W)
        es.append(e)
        if e in (DET_ZERO, DET_NONFINITE):
            continue
        wsc = (g64[nb] / npool).reshape(HW, 1, 1)
        for yy, xx, wgt in ((y0, x0, (1 - ax) * (1 - ay)), (y0, x1, ax * (1 - ay)), (y1, x0, (1 - ax) * ay), (y1, x1, ax * ay)):
            addend = wsc * wgt[nb]
            scaled = addend * 2.0 ** e                                   # exact: a power of two
            q = np.rint(scaled)
            assert float(np.abs(q).max()) < 2.0 ** 62
            cell = (chan[0] * HW + yy[nb] * W + xx[nb]).reshape(-1)
            live = np.broadcast_to(wsc != 0, q.shape).reshape(-1)        # a location with a zero upstream gradient adds nothing
            np.add.at(acc[nb], cell[live], q.astype(np.int64).reshape(-1)[live])
            np.add.at(count[nb], cell[live], 1)
            np.add.at(resid[nb], cell[live], (scaled - q).reshape(-1)[live])
            np.add.at(taps[nb], cell[live], addend.reshape(-1)[live])
    added = np.zeros((NB, M.K * HW))
    for nb, e in enumerate(es):
        if e not in (DET_ZERO, DET_NONFINITE):
            added[nb] = (acc[nb].astype(np.float64) * 2.0 ** -e).astype(np.float32).astype(np.float64)
    shape = (NB, M.K, HW)
    return dict(acc=torch.from_numpy(acc).view(shape), e=es, count=torch.from_numpy(count).view(shape),
                added=torch.from_numpy(added).view(shape), resid=torch.from_numpy(resid).view(shape),
                taps=torch.from_numpy(taps).view(shape))


# ---------------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(inputs, exact d corr, exact d params) of a DECODE_CASES entry: computed once, shared, not to be modified."""
    P, inverse, stride, rec_field = M.DECODE_CASES[name][:4]
    inp = M.decode_inputs(name)
    dc, dp, _ = M.decode_backward_model(inp["corr"], inp["params"], inp["dcls"], inp["dcls_det"], inp["dloc"], inverse, stride, rec_field)
    return inp, dc, dp


@functools.lru_cache(maxsize=None)
def hand_reference(inverse):
    inp = M.hand_inputs(inverse)
    dc, dp, _ = M.decode_backward_model(inp["corr"], inp["params"], inp["dcls"], inp["dcls_det"], inp["dloc"], inverse, 16, 16)
    return inp, dc, dp

