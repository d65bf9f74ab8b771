"""CPU: the float64 stage models of tests/backward_model.py are themselves right.  Chained in the order of
``_HeadFunction.backward`` they give the gradients torch autograd gives for the whole oracle head (layout helpers, channel
orders, chain rule); the plane layout round-trips; and the inputs the GPU stage tests feed the decode backward keep their share
of fragile locations under the cap."""
import pytest
import torch
import torch.nn.functional as F

import backward_model as M
from test_head_backward_gpu import CASES, PARAM_KEYS, oracle_grads, upstream

F64 = torch.float64
FRAGILE_CAP = 0.05


def _chained(fm, raws, state, inverse, gl, gc, gd):
    """The nine stage models in the order of _HeadFunction.backward, on float64 forward intermediates."""
    from oracle import head_oracle as O
    A, C, H, W = fm.shape
    B = len(raws)
    with torch.no_grad():
        q_hat = O.prepare_class_maps(raws)
        corr = O.correlation(q_hat, fm)
        rnorm = O.l2_normalize_channels(F.relu(corr), 1e-6)
        z1 = F.conv2d(rnorm, state["conv.0.weight"], state["conv.0.bias"], padding=3)
        bn1 = [state["conv.1." + k] for k in ("weight", "bias", "running_mean", "running_var")]
        h1 = M.bn_relu_forward(z1, *bn1, eps=O.BN_EPS)
        z2 = F.conv2d(h1, state["conv.3.weight"], state["conv.3.bias"], padding=2)
        bn2 = [state["conv.4." + k] for k in ("weight", "bias", "running_mean", "running_var")]
        h2 = M.bn_relu_forward(z2, *bn2, eps=O.BN_EPS)
        params = F.conv2d(h2, state["linear.weight"], state["linear.bias"], padding=2)
    NB = A * B
    out = {}
    dcorr, dparams, _ = M.decode_backward_model(corr, params, gc.view(NB, H, W), gd.view(NB, H, W), gl.view(NB, 4, H, W), inverse,
                                                16, 16, fp32_coords=False, mask=O.pool_mask().to(F64))
    dy3, out["linear.bias"] = M.params_backward_model(dparams, H, W)
    dh2, out["linear.weight"] = M.conv_backward_model(M.pack_planes(h2), state["linear.weight"], dy3, H, W)
    dy2, out["conv.4.weight"], out["conv.4.bias"], out["conv.3.bias"] = M.bn_relu_backward_model(dh2, z2, *bn2, H, W, eps=O.BN_EPS)
    dh1, out["conv.3.weight"] = M.conv_backward_model(M.pack_planes(h1), state["conv.3.weight"], dy2, H, W)
    dy1, out["conv.1.weight"], out["conv.1.bias"], out["conv.0.bias"] = M.bn_relu_backward_model(dh1, z1, *bn1, H, W, eps=O.BN_EPS)
    dxn, out["conv.0.weight"] = M.conv_backward_model(M.pack_layer1_input(rnorm), state["conv.0.weight"], dy1, H, W)
    assert dxn.shape == (NB, 225, M.plane_geometry(H, W)[2])
    dcorr = dcorr + M.norm225_backward_model(corr, dxn)
    out["fm"], dq = M.corr_backward_model(fm, M.class_operand(q_hat), dcorr)
    out["class"] = M.class_backward_model(raws, dq)
    return out


@pytest.mark.parametrize("name", ["v2_affine_inverse", "simple_affine_p4"])
def test_chained_stage_models_match_autograd_of_the_oracle(name):
    from os2d_amd.utils import synthetic
    P, inverse, A, C, H, W, sizes, B = CASES[name]
    state = {k: (v.to(F64) if v.is_floating_point() else v) for k, v in synthetic.make_transform_net_state(P, seed=3).items()}
    fm = synthetic.make_feature_map(C, H, W, seed=5, A=A).to(F64)
    raws = [c.to(F64) for c in synthetic.make_class_feature_maps(B, C, sizes=sizes, seed=400)]
    gl, gc, gd = upstream(A, B, H, W, 7)
    ref = oracle_grads(fm, raws, state, inverse, gl, gc, gd)
    got = _chained(fm, raws, state, inverse, gl, gc, gd)
    errs = {k: M.rel_err(got[k], ref[k]) for k in ["fm"] + PARAM_KEYS}
    errs.update({"class{}".format(b): M.rel_err(got["class"][b], ref["class"][b]) for b in range(B)})
    print(name, {k: "{:.1e}".format(v) for k, v in errs.items()})
    for k, g in ref.items():
        if k != "class":
            assert g.dtype == F64 and float(g.abs().max()) > 0, k
    bad = {k: v for k, v in errs.items() if not v < 1e-9}
    assert not bad, bad


@pytest.mark.parametrize("H,W", [(2, 2), (9, 13), (2, 209), (38, 38)])
def test_plane_pack_unpack_round_trip(H, W):
    ws, base, PL = M.plane_geometry(H, W)
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    p = M.pack_planes(x)
    assert p.shape == (2, 3, PL) and PL % 64 == 0
    assert torch.equal(M.unpack_planes(p, H, W), x)
    assert p[0, 0, base + (H - 1) * ws + (W - 1)] == x[0, 0, H - 1, W - 1] and p[0, 0, base] == x[0, 0, 0, 0]
    mask = M.interior_mask(H, W)
    assert int(mask.sum()) == H * W and torch.count_nonzero(p[:, :, ~mask]) == 0
    p1 = M.pack_layer1_input(torch.randn(1, 225, H, W))
    assert p1.shape == (1, 226, PL) and bool((p1[:, 225] == M.SENTINEL).all()) and torch.count_nonzero(p1[:, :225, ~mask]) == 0
    from os2d_amd import build
    if not build.up_to_date():
        pytest.skip("libos2d_hip.so is not built: PLANE not compared with os2d_plane_floats")
    from os2d_amd import _lib
    assert int(_lib.load().os2d_plane_floats(H, W)) == PL


def test_class_operand_layout():
    q = torch.randn(2, 3, 15, 15)
    qp = M.class_operand(q)
    assert qp.shape == (2, 3, 256) and torch.count_nonzero(qp[:, :, 225:]) == 0
    assert qp[1, 2, 4 * 15 + 9] == q[1, 2, 9, 4]                      # m = x*15 + y
    assert torch.equal(M.from_xmajor(qp[:, :, :225]), q) and torch.equal(M.to_xmajor(q), qp[:, :, :225])


def _fragile_share(inp, P, inverse, stride, rec_field):
    _, _, ratio = M.decode_backward_model(inp["corr"], inp["params"], inp["dcls"], inp["dcls_det"], inp["dloc"], inverse, stride,
                                          rec_field)
    return float((ratio < 1).double().mean())


@pytest.mark.parametrize("name", sorted(M.DECODE_CASES))
def test_fragile_share_of_the_decode_inputs_is_capped(name):
    """A condition on the INPUTS of tests/test_backward_stages_gpu.py: at most 5 % of the locations may lie within delta of a
    jump of the gradient (backward_model.fragility); a seed that breaks it is changed, the cap is not."""
    P, inverse, stride, rec_field = M.DECODE_CASES[name][:4]
    share = _fragile_share(M.decode_inputs(name), P, inverse, stride, rec_field)
    print(name, "fragile share {:.4f}".format(share))
    assert share <= FRAGILE_CAP
