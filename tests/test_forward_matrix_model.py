"""CPU: the float64 models and case tables of tests/forward_matrix_model.py keep to their own conditions - the models agree
with the oracle, every case has the edge inputs its GPU test relies on, and no operand of the split-fp16 path leaves the fp16
range.  Conditions of the INPUTS are checked here, without a GPU, so that the GPU tests assert on the kernels only."""
import numpy as np
import pytest
import torch

import f16x3_model as X3
import forward_matrix_model as FX
import train_forward_f16x3_model as SHB
from oracle import head_oracle as O


@pytest.mark.parametrize("case", FX.CORR_CASES, ids=FX.corr_case_id)
def test_corr_model_agrees_with_the_oracle_and_has_its_edges(case):
    A, B, C, H, W = case
    fm, q_hat = FX.corr_inputs(case)
    corr, rnorm, inv = FX.corr_reference(case)
    ref = O.correlation(q_hat.double(), fm.double()).reshape(A * B, FX.K, H * W)
    assert float((corr - ref).abs().max()) < 1e-12
    rn = O.l2_normalize_channels(torch.relu(ref), 1e-6)
    assert float((rnorm - rn).abs().max()) < 1e-12
    assert float((inv * (torch.relu(ref).norm(dim=1) + 1e-6) - 1).abs().max()) < 1e-12
    # the operands fit the split format: |q| <= 1
    assert float(q_hat.abs().max()) <= 1.0
    # the zero feature vector: exact zeros for every class
    a0, n0 = FX.corr_zero_at(case)
    assert torch.count_nonzero(fm.reshape(A, C, -1)[a0, :, n0]) == 0
    assert torch.count_nonzero(corr.reshape(A, B, FX.K, -1)[a0, :, :, n0]) == 0
    # the dead column: all 225 values strictly negative, so the normalised values are 0 and inv_norm is 1 / 1e-6
    a1, b1, n1 = FX.corr_dead_at(case)
    assert (a1, n1) != (a0, n0)
    assert float(corr[a1 * B + b1, :, n1].max()) < 0
    assert torch.count_nonzero(rnorm[a1 * B + b1, :, n1]) == 0 and float(inv[a1 * B + b1, n1]) == 1.0 / 1e-6
    # a column is dead or well conditioned (forward_matrix_model.corr_inputs)
    norm = 1.0 / inv - 1e-6
    assert float(norm[norm > 1e-9].min()) >= FX.MIN_LIVE_NORM
    # ... and the ReLU outputs are not all zero: every pair has live positions, unless its image is the single zero vector
    live = rnorm.reshape(A, B, FX.K, -1).amax(dim=(2, 3)) > 0
    assert bool(live[A - 1].all())
    assert bool(live[1:].any()) if H * W == 1 else bool(live.all())


def test_corr_case_table_covers_the_chunk_and_tile_edges():
    cs = {c[2] for c in FX.CORR_CASES}
    hw = {c[3] * c[4] for c in FX.CORR_CASES}
    assert {1, 7, 16, 17, 33, 67} <= cs and {1, 15, 128, 129, 256, 257} <= hw
    assert any(c[0] == 2 and c[1] == 3 for c in FX.CORR_CASES) and any(c[1] == 9 and c[3] * c[4] < 128 for c in FX.CORR_CASES)
    # the 256-position tile of os2d_launch_corr_f16x3 is reached in both forms: more than 256 work-groups of 128 positions
    for A, B, C, H, W in FX.CORR_CASES:
        if B == 97:
            t = (H * W + 127) // 128
            assert t * B * A > 256 and t * ((B * 228 + 255) // 256) * A > 256


def test_class_split_encode_reconstructs_the_operand():
    qp = FX.M.class_operand(FX.corr_inputs((1, 2, 17, 3, 43))[1])
    G = FX.split_groups(17)
    assert G == 4 and FX.split_groups(33) == 8 and FX.split_groups(1) == 4 and FX.split_groups(67) == 12
    halves = FX.class_split_encode(qp).numpy().view(np.float16).reshape(2, G, 2, 256, 8).astype(np.float64)
    rec = (halves[:, :, 0] + halves[:, :, 1]).transpose(0, 1, 3, 2).reshape(2, G * 8, 256) * 2.0 ** -FX.SPLIT_EXP
    assert np.count_nonzero(rec[:, 17:]) == 0 and np.count_nonzero(rec[:, :, FX.K:]) == 0
    v = qp.double().numpy()
    assert float(np.abs(rec[:, :17] - v).max()) <= 2.0 ** -22 * (1 + 2.0 ** -10) + 2.0 ** -36


@pytest.mark.parametrize("kind", FX.STATES)
@pytest.mark.parametrize("P", [6, 4])
def test_conv_layer_models_chained_are_the_oracles_transform_net(kind, P):
    state = FX.conv_state(kind, P)
    corr = torch.randn(2, FX.K, 5, 6, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    x = O.l2_normalize_channels(torch.relu(corr), 1e-6)
    for layer in (1, 2, 3):
        x = FX.conv_layer_model(layer, x, state, P)
    ref = O.transform_net(corr, {k: v.double() if v.is_floating_point() else v for k, v in state.items()})
    assert ref.shape == (2, P, 5, 6)
    assert float((x - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))


def test_edited_state_has_its_batchnorm_edges():
    st = FX.conv_state("edited", 6)
    for bn in ("conv.1", "conv.4"):
        assert float(st[bn + ".weight"][FX.GAMMA_ZERO]) == 0.0 and float(st[bn + ".weight"][FX.GAMMA_NEGATIVE]) < 0.0
        assert float(st[bn + ".running_var"][FX.VAR_ZERO]) == 0.0
    adv = FX.conv_state("adversarial", 6)
    s = adv["conv.1.weight"].abs()
    assert float(s.max() / s.min()) > 1e8 and float(adv["conv.1.running_var"].min()) == pytest.approx(1e-6)


def _cases():
    out = []
    for layer in (1, 2, 3):
        for kind in FX.STATES:
            for shape in (FX.CONV_SHAPES if layer == 1 else FX.CONV_SHAPES_5X5):
                out.append((layer, kind, shape))
    return out


@pytest.mark.parametrize("layer,kind,shape", _cases(), ids=lambda v: FX.shape_id(v) if isinstance(v, tuple) else str(v))
def test_conv_inputs_fit_the_range_plan_and_outputs_are_alive(layer, kind, shape):
    """Every operand of the split-fp16 path of every case passes f16x3_model.split (it raises outside the fp16 range): the
    scaled input, the scaled folded weights and - through f16x3_model.conv_f16x3 - the scaled output.  The model of the split
    arithmetic agrees with the plain float64 layer inside the ceiling the GPU test uses, and the ReLU outputs are not all zero."""
    H, W = shape
    net = FX.conv_net(kind, 6)
    plan, (w, b) = net.range_plan(), net._folded()[layer - 1]
    x = FX.conv_input(layer, kind, shape)
    assert x.shape == (FX.CONV_NB, w.size(1), H, W) and bool((x >= 0).all())
    if layer == 1:
        assert float(x.double().norm(dim=1).max()) <= 1.0 + 1e-6
        assert torch.count_nonzero(x[FX.CONV_NB - 1, :, H - 1, W // 2]) == 0
    else:
        assert bool((x.double().amax(dim=(0, 2, 3)) <= plan["bounds"][layer - 2] * (1 + 2.0 ** -23)).all())
        assert 0.3 < float((x == 0).double().mean()) < 0.8
    e_in, e_out, e_w = plan["in_exp"][layer - 1], plan["out_exp"][layer - 1], plan["weight_exp"][layer - 1]
    xs = x.double() * torch.exp2(e_in.double()).view(1, -1, 1, 1)
    y16 = X3.conv_f16x3(xs, w, b, e_in, e_out, e_w, layer != 3, w.size(-1) // 2)                 # raises on an fp16 overflow
    ref = FX.conv_reference(layer, kind, shape)
    if layer == 3:
        assert float(ref.abs().max()) < 8.0, "layer-3 outputs are O(1): the 1e-5 absolute bound means something"
        assert float((y16 - ref).abs().max()) < 1e-5
        return
    X3.split(y16)                                                                               # the stored output
    assert bool((ref.amax(dim=(1, 2, 3)) > 0).all()), "the ReLU outputs of a pair are all zero"
    got = y16 * torch.exp2(-e_out.double()).view(1, -1, 1, 1)
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err < FX.conv_error_ceiling(layer, kind, shape, "f16x3")
    assert FX.conv_error_ceiling(layer, kind, shape, "f32") < FX.conv_error_ceiling(layer, kind, shape, "f16x3") \
        < FX.conv_error_ceiling(layer, kind, shape, "f16x2")


def test_shb_helpers_round_trip():
    x = FX.conv_input(2, "adversarial", (2, 2))
    exp = FX.conv_net("adversarial", 6).range_plan()["in_exp"][1]
    buf = FX.shb_input(x, exp)
    assert buf.numel() == FX.CONV_NB * SHB.groups(128) * 2 * SHB.plane(2, 2) * 16
    val, halves = FX.shb_output(buf, exp, 128, 2, 2)
    assert float(((val - x.double()).abs() / x.double().abs().clamp_min(1e-300)).max()) < 2.0 ** -21
    assert np.count_nonzero(halves[:, :, :, ~SHB.interior_mask(2, 2)]) == 0
