"""CPU: the float64 models of tests/bn_live_model.py are themselves right (chained in the order of the live backward they give
the gradients torch autograd gives for the whole live oracle head; the running-statistics update is torch's), the end-to-end inputs
of tests/test_bn_live_head_gpu.py have no fragile location, and the new entry points of libos2d_train.so refuse bad arguments
before anything is launched (no device is needed for that)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import backward_model as M
import bn_live_model as L

F64 = torch.float64
LIVE_PATTERNS = [(True, True), (True, False), (False, True)]


def _chained(fm, raws, state, inverse, live, gl, gc, gd):
    """The stage models in the order of _HeadFunction.backward on a live route, on float64 forward intermediates."""
    from oracle import head_oracle as O
    A, C, H, W = fm.shape
    B = len(raws)
    with torch.no_grad():
        q_hat = O.prepare_class_maps(raws)
        corr = O.correlation(q_hat, fm)
        rnorm = O.l2_normalize_channels(F.relu(corr), 1e-6)
        z, h, x = {}, {}, rnorm
        for layer, pad in ((1, 3), (2, 2)):
            conv, bn = L.BN_KEYS[layer]
            z[layer] = M.unpack_planes(L.conv_forward_model(M.pack_planes(x), state[conv + ".weight"], state[conv + ".bias"], H, W), H, W)
            if live[layer - 1]:
                h[layer] = L.bn_relu_live_forward(z[layer], state[bn + ".weight"], state[bn + ".bias"], O.BN_EPS)
            else:
                h[layer] = M.bn_relu_forward(z[layer], *[state[bn + "." + k] for k in ("weight", "bias", "running_mean", "running_var")],
                                             eps=O.BN_EPS)
            x = h[layer]
        params = F.conv2d(h[2], state["linear.weight"], state["linear.bias"], padding=2)
    NB = A * B
    out = {}
    dcorr, dparams, _ = M.decode_backward_model(corr, params, gc.view(NB, H, W), gd.view(NB, H, W), gl.view(NB, 4, H, W), inverse,
                                                16, 16, fp32_coords=False, mask=O.pool_mask().to(F64))
    dy, out["linear.bias"] = M.params_backward_model(dparams, H, W)
    dh, out["linear.weight"] = M.conv_backward_model(M.pack_planes(h[2]), state["linear.weight"], dy, H, W)
    for layer, below in ((2, M.pack_planes(h[1])), (1, M.pack_layer1_input(rnorm))):
        conv, bn = L.BN_KEYS[layer]
        if live[layer - 1]:
            dy, dg, db, dcb = L.backward_model(dh, M.pack_planes(z[layer]), state[bn + ".weight"], state[bn + ".bias"], H, W, O.BN_EPS)
        else:
            bnp = [state[bn + "." + k] for k in ("weight", "bias", "running_mean", "running_var")]
            dy, dg, db, dcb = M.bn_relu_backward_model(dh, z[layer], *bnp, H, W, eps=O.BN_EPS)
        out[bn + ".weight"], out[bn + ".bias"], out[conv + ".bias"] = dg, db, dcb
        dh, out[conv + ".weight"] = M.conv_backward_model(below, state[conv + ".weight"], dy, H, W)
    dcorr = dcorr + M.norm225_backward_model(corr, dh)
    out["fm"], dq = M.corr_backward_model(fm, M.class_operand(q_hat), dcorr)
    out["class"] = M.class_backward_model(raws, dq)
    return out


@pytest.mark.parametrize("live", LIVE_PATTERNS, ids=str)
@pytest.mark.parametrize("name", ["v2_affine_inverse", "v1_p4_no_inverse"])
def test_chained_stage_models_match_autograd_of_the_live_oracle(name, live):
    P, inverse, A, C, H, W, sizes, B, _ = L.HEAD_CASES[name]
    state, fm, class_fms, (gl, gc, gd) = L.head_inputs(name)
    state = {k: (v.to(F64) if v.is_floating_point() else v) for k, v in state.items()}
    fm, raws = fm.to(F64), [c.to(F64) for c in class_fms]
    ref = L.live_oracle(fm, raws, state, inverse, live, gl, gc, gd)["grads"]
    got = _chained(fm, raws, state, inverse, live, gl, gc, gd)
    live_bias = [L.BN_KEYS[layer][0] + ".bias" for layer in (1, 2) if live[layer - 1]]
    scale = float(gl.abs().sum() + gc.abs().sum() + gd.abs().sum())
    for k in live_bias:        # exactly zero in exact arithmetic: compared as absolute values, both far below the other gradients
        assert float(ref[k].abs().max()) < 1e-9 * scale and float(got[k].abs().max()) < 1e-9 * scale, k
    keys = [k for k in ["fm"] + L.PARAM_KEYS if k not in live_bias]
    errs = {k: M.rel_err(got[k], ref[k]) for k in keys}
    errs.update({"class{}".format(b): M.rel_err(got["class"][b], ref["class"][b]) for b in range(B)})
    print(name, live, {k: "{:.1e}".format(v) for k, v in errs.items()})
    for k in keys:
        assert float(ref[k].abs().max()) > 0, k
    bad = {k: v for k, v in errs.items() if not v < 1e-12}
    assert not bad, bad


def test_stats_and_apply_models_are_batch_norm():
    g = torch.Generator().manual_seed(5)
    NB, C, H, W = 3, 4, 5, 7
    z = torch.randn(NB, C, H, W, generator=g, dtype=F64) * 3 + 1
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    mean, var, invstd = L.stats_model(M.pack_planes(z), H, W, 1e-5)
    h = L.apply_model(M.pack_planes(z), gamma, beta, mean, invstd, H, W)
    ref = L.bn_relu_live_forward(z, gamma, beta, 1e-5)
    assert M.rel_err(M.unpack_planes(h, H, W), ref) < 1e-14
    assert torch.count_nonzero(h[:, :, ~M.interior_mask(H, W)]) == 0


@pytest.mark.parametrize("momentum", [0.1, 0.3])
def test_running_update_model_is_torch(momentum):
    g = torch.Generator().manual_seed(9)
    NB, C, H, W = 3, 6, 4, 5
    bn = torch.nn.BatchNorm2d(C, momentum=momentum).double().train()
    bn.running_mean.copy_(torch.randn(C, generator=g, dtype=F64))
    bn.running_var.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for step in range(2):
        z = torch.randn(NB, C, H, W, generator=g, dtype=F64) * 2 + 0.5
        mean, var, _ = L.stats_model(M.pack_planes(z), H, W)
        rm, rv = L.running_update_model(rm, rv, mean, var, NB * H * W, momentum)
        bn(z)
        assert M.rel_err(rm, bn.running_mean) < 1e-14 and M.rel_err(rv, bn.running_var) < 1e-14
    assert int(bn.num_batches_tracked) == 2


@pytest.mark.parametrize("live", LIVE_PATTERNS, ids=str)
@pytest.mark.parametrize("name", sorted(L.HEAD_CASES))
def test_end_to_end_inputs_have_no_fragile_location(name, live):
    """A condition on the INPUTS of tests/test_bn_live_head_gpu.py: no location of the live oracle lies within delta of a jump of
    the gradient (backward_model.fragility); a seed that breaks it is changed, the condition is not."""
    assert L.head_fragile_share(name, live) == 0.0


@pytest.mark.parametrize("name,live", [(n, lv) for n in sorted(L.HEAD_CASES) for lv in L.GRAD_PATTERNS[n]], ids=str)
def test_end_to_end_inputs_have_no_pre_activation_at_a_relu_kink(name, live):
    """The same for the other jump of the oracle's gradient: where the GPU test compares gradients, every pre-activation of the two
    BatchNorm layers is further from zero than the forward's rounding can move it (bn_live_model.head_relu_margin)."""
    assert L.head_relu_margin(name, live) > 1.0


# ---------------------------------------------------------------------------------------------------------- refusals
fake = ctypes.c_void_p(256)      # never dereferenced: every call below is refused by its argument checks


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import build, _train_lib
    build.build_train(verbose=False)
    return _train_lib.load()


def _err(lib):
    return lib.os2d_train_last_error().decode()


def _conv(lib, arith=0, layer=1, P=6, w=fake, bias=fake, x=fake, NB=2, H=9, W=13, z=fake, ws=fake, room=None):
    room = int(lib.os2d_train_conv_forward_workspace_floats(arith, layer, P, NB)) if room is None else room
    return lib.os2d_train_conv_forward(arith, layer, P, w, bias, x, NB, H, W, z, ws, room, None)


def _stats(lib, layer=1, z=fake, NB=2, H=9, W=13, out=fake, ws=fake, room=None):
    room = int(lib.os2d_train_bn_workspace_bytes(layer, NB)) if room is None else room
    return lib.os2d_train_bn_stats(layer, z, NB, H, W, ctypes.c_float(1e-5), out, out, out, ws, room, None)


def _apply(lib, layer=1, z=fake, NB=2, H=9, W=13, h=fake):
    return lib.os2d_train_bn_relu_forward(layer, z, fake, fake, fake, fake, NB, H, W, h, None)


def _bwd(lib, layer=1, dh=fake, NB=2, H=9, W=13, dy=fake, ws=fake, room=None):
    room = int(lib.os2d_train_bn_workspace_bytes(layer, NB)) if room is None else room
    return lib.os2d_train_bn_relu_backward_batch(layer, dh, fake, fake, fake, fake, fake, NB, H, W, dy, None, None, ws, room, None)


def test_new_entry_points_refuse_bad_arguments_before_any_launch(lib):
    # a null pointer
    for rc in (_conv(lib, w=None), _conv(lib, bias=None), _conv(lib, x=None), _conv(lib, z=None), _conv(lib, ws=None),
               _stats(lib, z=None), _stats(lib, out=None), _stats(lib, ws=None), _apply(lib, z=None), _apply(lib, h=None),
               _bwd(lib, dh=None), _bwd(lib, dy=None), _bwd(lib, ws=None)):
        assert rc == -1 and "null pointer" in _err(lib)
    # layer 3 has no BatchNorm (and the convolution entry point is for the layers that have one)
    for rc in (_stats(lib, layer=3, room=1 << 20), _apply(lib, layer=3), _bwd(lib, layer=3, room=1 << 20), _conv(lib, layer=3, room=64),
               _conv(lib, layer=0, room=64)):
        assert rc == -1 and "layer" in _err(lib)
    assert lib.os2d_train_bn_workspace_bytes(3, 2) == 0 and lib.os2d_train_conv_forward_workspace_floats(0, 3, 6, 2) == 0
    # n < 2
    for rc in (_stats(lib, NB=1, H=1, W=1), _bwd(lib, NB=1, H=1, W=1)):
        assert rc == -1 and "n = 1" in _err(lib)
    # W = 210
    for rc in (_conv(lib, W=210), _stats(lib, W=210), _apply(lib, W=210), _bwd(lib, W=210)):
        assert rc == -1 and "bad shape" in _err(lib)
    # too small a workspace
    assert _conv(lib, arith=1, room=2) == -2 and "workspace" in _err(lib)
    assert _conv(lib, arith=0, room=0) == -2 and "workspace" in _err(lib)
    need = int(lib.os2d_train_bn_workspace_bytes(1, 2))
    assert need > 0
    assert _stats(lib, room=need - 1) == -2 and "workspace" in _err(lib)
    assert _bwd(lib, room=need - 1) == -2 and "workspace" in _err(lib)
    # NB * Cout > 65535
    for rc in (_conv(lib, NB=512, room=1024), _stats(lib, NB=512, room=1 << 24), _apply(lib, NB=512), _bwd(lib, NB=512, room=1 << 24),
               _stats(lib, layer=2, NB=1024, room=1 << 24)):
        assert rc == -1 and "65535" in _err(lib)
    assert lib.os2d_train_bn_workspace_bytes(1, 512) == 0 and lib.os2d_train_bn_workspace_bytes(1, 511) > 0
    # an unknown arith
    assert _conv(lib, arith=2, room=64) == -1 and "arith" in _err(lib)
    assert lib.os2d_train_conv_forward_workspace_floats(2, 1, 6, 2) == 0
    # a plane tensor off the 16-byte grid
    assert _stats(lib, z=ctypes.c_void_p(260)) == -1 and "aligned" in _err(lib)
