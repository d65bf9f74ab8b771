"""GPU: the 5x5 layer 128 -> 64 of the TransformNet in the frequency domain (precision "fftx3", os2d_head_forward_ex2 with the
layer's weight spectra), stage by stage through the ABI - os2d_dft_forward on fp32 planes with unit norms, the per-bin GEMM
128 -> 64, os2d_dft_inverse with the layer-2 bias and scales - against a float64 direct 5x5 convolution in torch.

Tolerance.  On the same inputs the direct kernel (conv_f16x3_kernel<5>, os2d_transform_conv_f16x3 layer 2) was measured against
the same float64 reference before this route existed; the transform route must stay within 3x of that - the margin of the
head's pins.  Error = max over pairs, channels and cells of |got - ref| / (largest |pre-activation| of the channel).
Measured (profiles/conv2_freq/errors.txt):

    case         direct      transform route
    9x11         2.9941e-06  3.9879e-07
    21x30        2.8446e-06  6.3537e-07
    60x80        3.4547e-06  1.2656e-06
    62x82        2.9755e-06  8.4080e-07
    9x11 cout60  2.9941e-06  3.9879e-07

Cases, 7 pairs each (the pair count at which the head switches to the transform route): the smallest canonical transform
(9 x 11, also a width that is no multiple of 4, 8 images per iteration), 21 x 30 (width % 4 == 2), 60 x 80 (the 64-row radix-2
transform), 62 x 82 (the smallest map the planner cuts in two in each direction) and weights whose last live output channel is 59
(the slice ends inside an 8-channel group: the GEMM pads the rows to 64 / 128).  Every input has one channel AT its range-plan
bound (stored value 2^unit_exp * bound, in (0.5, 1]) and one all-zero channel."""
import ctypes

import pytest
import torch

from freq_util import dft_sizes, fft_sizes, matrices, shb_decode, shb_encode, twiddles, weight_spectra
from os2d_amd import _lib
from os2d_amd.utils import synthetic

pytestmark = pytest.mark.gpu

NB = 7
# case -> (H, W, live output channels, error of the direct kernel on these inputs)
CASES = {
    "9x11": (9, 11, 64, 2.9941e-06),
    "21x30": (21, 30, 64, 2.8446e-06),
    "60x80": (60, 80, 64, 3.4547e-06),
    "62x82": (62, 82, 64, 2.9755e-06),
    "9x11_cout60": (9, 11, 60, 2.9941e-06),
}
MARGIN = 3.0


@pytest.fixture(scope="module")
def net(device):
    from os2d_amd.modeling import head as head_mod
    n = head_mod.TransformationNet(output_dim=6)
    n.load_state_dict(synthetic.make_transform_net_state(6, seed=3))
    return n.to(device).eval()


def make_inputs(net, H, W, cout_live, device):
    """(stored h1 [NB,128,H,W] float32 in the "<= 1" convention, float64 reference pre-activation, reference output, packed
    layer-2 bias table, folded float64 weights with the dead rows zeroed)."""
    plan = net.range_plan()
    unit_exp = (plan["out_exp"][0] - 15).to(device).double()                           # = plan["unit_exp"]
    bound1 = plan["bounds"][0].to(device).double()
    g = torch.Generator().manual_seed(1000 * H + W)
    amp = torch.exp2(-torch.randint(2, 11, (128,), generator=g).double())              # typical activations sit far below the bound
    x = torch.rand(NB, 128, H, W, generator=g).double()
    x = torch.relu(x - 0.4) * amp.view(1, -1, 1, 1)                                    # post-ReLU: ~40 % zeros
    stored = x.to(device)
    stored[:, 5] = (bound1[5] * torch.exp2(unit_exp[5]))                               # one channel at its bound
    stored[:, 9] = 0.0                                                                 # one all-zero channel
    stored = stored.float()
    assert float(stored.max()) <= 1.0 and float(stored[:, 5].min()) > 0.5
    (_, _), (w2, b2), _ = net._folded()
    w2, b2 = w2.to(device).clone(), b2.to(device)
    w2[cout_live:] = 0.0
    true = stored.double() * torch.exp2(-unit_exp).view(1, -1, 1, 1)
    pre = torch.nn.functional.conv2d(true, w2, b2, padding=2)
    bp = net.packed("fftx3")[3]                                                        # bias | 2^-weight_exp | 2^out_exp (64 rows each)
    return stored, pre, torch.relu(pre), bp, w2


def error_of(got, pre, ref):
    scale = pre.abs().amax(dim=(0, 2, 3)).clamp_min(1e-300)
    return float(((got - ref).abs() / scale.view(1, -1, 1, 1)).max())


def spectra_of(net, w2fold, H, W, device):
    """the layer's split weight spectra as TransformationNet.spectra2 builds them, from the given folded weights"""
    P, Q, nbins, _ = dft_sizes(H, W)
    unit_exp = net.range_plan()["unit_exp"].to(device).double()
    wfold = torch.nn.functional.pad(w2fold * torch.exp2(-unit_exp).view(1, -1, 1, 1), (1, 1, 1, 1))
    return weight_spectra(wfold, P, Q, nbins, True, device)


def run_freq(net, stored, bp, w16, H, W, device):
    """forward transform (unit norms) -> per-bin GEMM 128 -> 64 -> inverse transform with the layer-2 epilogue; SHB bytes + status"""
    lib = _lib.load()
    P, Q, nbins, (TY, TX, TH, TW, LH, LW) = dft_sizes(H, W)
    T = TY * TX
    st = _lib.current_stream(device)
    mats = matrices(P, Q, device)
    cpad = lib.os2d_dft_channel_stride(128)
    X = torch.full((nbins // 4, NB * T, cpad, 4, 2), float("nan"), device=device)
    Y = torch.full((nbins // 4, NB * T, 64, 4, 2), float("nan"), device=device)
    out = torch.full((NB * lib.os2d_shb_bytes(64, H, W),), 0x5A, dtype=torch.uint8, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    _lib.check(lib.os2d_dft_forward(_lib.ptr(stored), None, _lib.ptr(X), _lib.ptr(mats), NB, 128, H, W, st), "os2d_dft_forward")
    _lib.check(lib.os2d_spectral_gemm_f16_quads(_lib.ptr(w16), _lib.ptr(X), _lib.ptr(Y), NB * T, 128, 64, nbins,
                                                ctypes.c_float(lib.os2d_dft_xscale(H, W)), st), "os2d_spectral_gemm_f16_quads")
    _lib.check(lib.os2d_dft_inverse(_lib.ptr(Y), _lib.ptr(bp), _lib.ptr(out), _lib.ptr(mats), NB, 64, H, W, _lib.ptr(status), st),
               "os2d_dft_inverse")
    torch.cuda.synchronize()
    return out, int(status.item())


def run_direct(net, stored, bp, w2fold, H, W, device):
    """the direct kernel on the same inputs (split-half blocked input with the layer-1 scales); needs unmodified weights"""
    lib = _lib.load()
    shb = shb_encode(stored, 32768.0)                                                  # 2^out_exp1 = 2^(unit_exp + 15)
    w2p = net.packed("fftx3")[2]
    out = torch.full((NB * lib.os2d_shb_bytes(64, H, W),), 0x5A, dtype=torch.uint8, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    _lib.check(lib.os2d_transform_conv_f16x3(2, _lib.ptr(shb), _lib.ptr(w2p), _lib.ptr(bp), _lib.ptr(out), NB, 6,
                                             H, W, 3, _lib.ptr(status), _lib.current_stream(device)), "os2d_transform_conv_f16x3")
    torch.cuda.synchronize()
    return out, int(status.item())


def measure(net, name, device, route):
    H, W, cout_live, _ = CASES[name]
    stored, pre, ref, bp, w2 = make_inputs(net, H, W, cout_live, device)
    out_scale = bp[128:192].double()
    if route == "direct":
        if cout_live != 64:        # the direct kernel takes the net's own packed weights: dead rows are compared on the live ones only
            pre, ref = pre[:, :cout_live], ref[:, :cout_live]
        out, status = run_direct(net, stored, bp, w2, H, W, device)
        got, border = shb_decode(out, NB, 64, H, W)
        return error_of((got / out_scale.view(1, -1, 1, 1))[:, :cout_live], pre, ref), border, status
    out, status = run_freq(net, stored, bp, spectra_of(net, w2, H, W, device), H, W, device)
    got, border = shb_decode(out, NB, 64, H, W)
    return error_of(got / out_scale.view(1, -1, 1, 1), pre, ref), border, status


@pytest.mark.parametrize("name", sorted(CASES))
def test_conv2_in_the_frequency_domain_matches_float64(name, net, device):
    err, border, status = measure(net, name, device, "freq")
    direct = CASES[name][3]
    print("conv2 freq {}: error {:.3e}, direct kernel {:.3e}".format(name, err, direct))
    assert status == 0 and border == 0.0
    assert err <= MARGIN * direct, (err, direct)


def test_spectra2_of_the_net_are_what_the_stage_test_builds(net, device):
    """TransformationNet.spectra2 - what the head passes to os2d_head_forward_ex2 - gives the same bytes."""
    H, W = 9, 11
    _, _, _, _, w2 = make_inputs(net, H, W, 64, device)
    assert torch.equal(net.spectra2(H, W), spectra_of(net, w2, H, W, device))


def test_spectra_of_the_net_are_what_independent_builders_give(net, device):
    """TransformationNet.spectra - both arithmetic families at 9 x 11 - gives, byte for byte, what the test-side builders of
    freq_util make from the folded filters: the split spectra and the transform matrices, the complex64 spectra and both fp32
    twiddle tables."""
    H, W = 9, 11
    (w1, _), _, _ = net._folded()
    P, Q, nbins, _ = dft_sizes(H, W)
    got = net.spectra(H, W, split=True)
    assert torch.equal(got[0], weight_spectra(w1, P, Q, nbins, True, device))
    assert torch.equal(got[1], matrices(P, Q, device))
    assert got[2] is None and got[3] == nbins
    P, Q, nbins = fft_sizes(H, W)
    got = net.spectra(H, W)
    assert torch.equal(got[0], weight_spectra(w1, P, Q, nbins, False, device))
    assert torch.equal(got[1], twiddles(Q, device)) and torch.equal(got[2], twiddles(P, device))
    assert got[3] == nbins


def test_spectra2_alone_drops_the_stale_entries_of_a_changed_net(device):
    """spectra2 on a fresh net BEFORE spectra: after a parameter changes, the next spectra2 call on its own drops the stale
    layer-1 entry (it used to rely on spectra having run first) and returns new bytes."""
    from os2d_amd.modeling import head as head_mod
    H, W = 9, 11
    fresh = head_mod.TransformationNet(output_dim=6)
    fresh.load_state_dict(synthetic.make_transform_net_state(6, seed=3))
    fresh.to(device).eval()
    P, Q, _, _ = dft_sizes(H, W)
    old = fresh.spectra2(H, W).clone()
    fresh.spectra(H, W, split=True)
    assert sorted(fresh._spectra_cache, key=len) == [(P, Q, True), (P, Q, True, "conv2")]
    with torch.no_grad():
        fresh.conv[3].weight.mul_(1.5)
    new = fresh.spectra2(H, W)
    assert list(fresh._spectra_cache) == [(P, Q, True, "conv2")]          # the stale layer-1 entry is gone
    assert not torch.equal(new, old)


def test_inverse_planes_are_the_scaled_activations(net, device):
    """os2d_dft_inverse_planes (the layer-1 output form on this route) = the split-half output of os2d_dft_inverse times 2^-15,
    as fp32 planes without borders."""
    lib = _lib.load()
    H, W, Cout = 21, 30, 128
    P, Q, nbins, _ = dft_sizes(H, W)
    g = torch.Generator().manual_seed(7)
    Y = (torch.randn(nbins // 4, NB, Cout, 4, 2, generator=g) * 3.0).to(device)
    bp = torch.zeros(3 * 128)
    bp[:128] = torch.randn(128, generator=g) * 0.01
    bp[256:] = torch.exp2(torch.randint(8, 12, (128,), generator=g).float())
    bp = bp.to(device)
    mats = matrices(P, Q, device)
    st = _lib.current_stream(device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    shb = torch.full((NB * lib.os2d_shb_bytes(Cout, H, W),), 0x5A, dtype=torch.uint8, device=device)
    planes = torch.full((NB, Cout, H, W), float("nan"), device=device)
    _lib.check(lib.os2d_dft_inverse(_lib.ptr(Y), _lib.ptr(bp), _lib.ptr(shb), _lib.ptr(mats), NB, Cout, H, W, _lib.ptr(status), st), "inverse")
    _lib.check(lib.os2d_dft_inverse_planes(_lib.ptr(Y), _lib.ptr(bp), _lib.ptr(planes), _lib.ptr(mats), NB, Cout, H, W, _lib.ptr(status), st),
               "inverse planes")
    torch.cuda.synchronize()
    got, border = shb_decode(shb, NB, Cout, H, W)
    assert border == 0.0 and int(status.item()) == 0
    # hi + lo carries 22 bits of the fp32 value
    assert float((planes.double() * 32768.0 - got).abs().max()) <= 2.0 ** -21 * float(got.abs().max())
