"""Plain float64 references of the batch-statistics ("live") BatchNorm entry points of libos2d_train.so (include/os2d_train.h;
DESIGN.md section 16), one per entry point, in the style of tests/backward_model.py: stock torch operators on the CPU, tensors in
the layouts of the C ABI, gradients by ``torch.autograd.grad`` of the float64 forward - no gradient formula is written down here.
The whole head with live BatchNorms restates the oracle's stages (oracle/head_oracle.py) with ``transform_net`` taking
``F.batch_norm(training=True)`` where a layer is live.
"""
import torch
import torch.nn.functional as F

from oracle import head_oracle as O

import backward_model as M

F64 = torch.float64
EPS32 = M.EPS32
BN_KEYS = {1: ("conv.0", "conv.1"), 2: ("conv.3", "conv.4")}


# ---------------------------------------------------------------------------------------------------------- stages
def conv_forward_model(x_planes, w, bias, H, W):
    """os2d_train_conv_forward: x [NB,>=Cin,PLANE] (only the first Cin planes are read), raw w [Cout,Cin,k,k], bias [Cout] ->
    z [NB,Cout,PLANE] float64, zeros at the pad cells."""
    cin, k = w.size(1), w.size(2)
    x = M.unpack_planes(x_planes[:, :cin].to(F64), H, W)
    return M.pack_planes(F.conv2d(x, w.to(F64), bias.to(F64), padding=k // 2))


def stats_model(z_planes, H, W, eps=EPS32):
    """os2d_train_bn_stats: (mean, biased var, 1 / sqrt(var + eps)) [C] in float64 over the NB*H*W data cells of each channel."""
    z = M.unpack_planes(z_planes.to(F64), H, W)
    mean = z.mean(dim=(0, 2, 3))
    var = ((z - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    return mean, var, 1.0 / torch.sqrt(var + eps)


def apply_model(z_planes, gamma, beta, mean32, invstd32, H, W):
    """os2d_train_bn_relu_forward in float64, with the fp32 ``mean`` / ``invstd`` the kernel is given."""
    z = M.unpack_planes(z_planes.to(F64), H, W)
    v = lambda t: t.to(F64).view(1, -1, 1, 1)
    return M.pack_planes(F.relu((z - v(mean32)) * v(invstd32) * v(gamma) + v(beta)))


def bn_relu_live_forward(z, gamma, beta, eps=EPS32):
    """h = relu(BatchNorm_train(z)), z [NB,C,H,W] float64."""
    return F.relu(F.batch_norm(z, None, None, gamma, beta, training=True, eps=eps))


def backward_model(dh_planes, z_planes, gamma, beta, H, W, eps=EPS32):
    """os2d_train_bn_relu_backward_batch: autograd of float64 F.batch_norm(training=True) + ReLU.  -> (dy [NB,C,PLANE], dgamma,
    dbeta, dbias [C]); dbias = the gradient of a constant added to z per channel (the convolution's bias): zero up to rounding."""
    C = z_planes.size(1)
    zl, g, b, cb = M._leaf(M.unpack_planes(z_planes, H, W)), M._leaf(gamma), M._leaf(beta), M._leaf(torch.zeros(C))
    h = bn_relu_live_forward(zl + cb.view(1, C, 1, 1), g, b, eps)
    dz, dg, db, dcb = M._grad(h, [zl, g, b, cb], M.unpack_planes(dh_planes, H, W))
    return M.pack_planes(dz), dg, db, dcb


def running_update_model(running_mean, running_var, mean, var, n, momentum=0.1):
    """torch's training-mode update of the BatchNorm buffers: the variance enters unbiased (n / (n - 1))."""
    return ((1 - momentum) * running_mean.to(F64) + momentum * mean.to(F64),
            (1 - momentum) * running_var.to(F64) + momentum * var.to(F64) * n / (n - 1.0))


# ---------------------------------------------------------------------------------------------------------- the whole head
def live_transform_net(corr, state, live, eps=O.BN_EPS, stats=None):
    """oracle.transform_net with ``training=True`` in the BatchNorm of every layer that is live; ``stats`` (a list) receives
    (mean, biased var, n) of the live layers."""
    x = O.l2_normalize_channels(F.relu(corr), 1e-6)
    for layer, pad in ((1, 3), (2, 2)):
        conv, bn = BN_KEYS[layer]
        x = F.conv2d(x, state[conv + ".weight"], state[conv + ".bias"], padding=pad)
        if live[layer - 1]:
            if stats is not None:
                d = x.detach()
                stats.append((d.mean(dim=(0, 2, 3)), d.var(dim=(0, 2, 3), unbiased=False), d.numel() // d.size(1)))
            x = F.batch_norm(x, None, None, state[bn + ".weight"], state[bn + ".bias"], training=True, eps=eps)
        else:
            if stats is not None:
                stats.append(None)
            x = F.batch_norm(x, state[bn + ".running_mean"], state[bn + ".running_var"], state[bn + ".weight"], state[bn + ".bias"],
                             training=False, eps=eps)
        x = F.relu(x)
    return F.conv2d(x, state["linear.weight"], state["linear.bias"], padding=2)


def _decode(corr, params, A, B, H, W, inverse, stride, rec_field):
    """The oracle's stages after the TransformNet (head_oracle.head_forward:175-194): (loc, cls, corners)."""
    T = O.TEMPLATE
    theta = O.params_to_theta(params, inverse)
    grids = F.affine_grid(theta, [theta.size(0), 1, T, T], align_corners=True).view(A, B, H, W, T, T, 2)
    g_fm = O.local_to_global(grids, O.anchor_grid(H, W, float(T), 1.0).to(corr.dtype).view(1, 1, H, W, 4))
    g_unit = torch.stack([g_fm[..., 0] / (W - 1) * 2 - 1, g_fm[..., 1] / (H - 1) * 2 - 1], dim=-1).clamp(-1, 1)
    cls = O.resample_and_pool(corr.view(A, B, T * T, H, W), g_unit, O.pool_mask())
    anchors = O.anchor_grid(H, W, float(stride * (T - 1) + rec_field), float(stride)).to(corr.dtype)
    g_img = O.local_to_global(grids, anchors.view(1, 1, H, W, 4))
    gx, gy = g_img[..., 0].reshape(-1, T * T), g_img[..., 1].reshape(-1, T * T)
    boxes = torch.stack([gx.min(1)[0], gy.min(1)[0], gx.max(1)[0], gy.max(1)[0]], dim=1)
    corners = g_img[:, :, :, :, [0, -1]][:, :, :, :, :, [0, -1]].reshape(A, B, H, W, 8).permute(0, 1, 4, 2, 3).contiguous()
    loc = O.encode_boxes(O.clip_to_min_size(boxes), O.clip_to_min_size(anchors.repeat(A * B, 1)))
    return loc.view(A, B, H, W, 4).permute(0, 1, 4, 2, 3).contiguous(), cls, corners


def live_head_forward(fm, q_hat, state, inverse, live, stride=16, rec_field=16):
    """The oracle head with live BatchNorms: (loc, cls, cls_det, corners, aux).  cls_det is the resampling on a grid built from
    DETACHED parameters (reference head.py:396-402), as tests/test_head_backward_gpu._cls_detached composes it.  aux: corr,
    params and the batch statistics [(mean, var, n) or None] x 2.  Runs in the dtype of its inputs."""
    A, _, H, W = fm.shape
    B = q_hat.size(0)
    stats = []
    corr = O.correlation(q_hat, fm)
    params = live_transform_net(corr, state, live, stats=stats)
    loc, cls, corners = _decode(corr, params, A, B, H, W, inverse, stride, rec_field)
    _, cls_det, _ = _decode(corr, params.detach(), A, B, H, W, inverse, stride, rec_field)
    return loc, cls, cls_det, corners, dict(corr=corr, params=params, stats=stats)


PARAM_KEYS = ["conv.0.weight", "conv.0.bias", "conv.1.weight", "conv.1.bias", "conv.3.weight", "conv.3.bias", "conv.4.weight",
              "conv.4.bias", "linear.weight", "linear.bias"]


def live_oracle(fm, class_fms, state, inverse, live, gl, gc, gd, stride=16, rec_field=16):
    """float64 autograd of the live oracle head: dict(out=(loc, cls, cls_det, corners), grads={'fm', 'class', <state key>}, aux) for
    the loss sum(gl*loc + gc*cls + gd*cls_det)."""
    fm = M._leaf(fm)
    raws = [M._leaf(c) for c in class_fms]
    st = {k: (M._leaf(v) if k in PARAM_KEYS else v.detach().to(F64) if v.is_floating_point() else v.clone()) for k, v in state.items()}
    loc, cls, cls_det, corners, aux = live_head_forward(fm, O.prepare_class_maps(raws), st, inverse, live, stride, rec_field)
    loss = (loc * gl.to(F64)).sum() + (cls * gc.to(F64)).sum() + (cls_det * gd.to(F64)).sum()
    leaves = [fm] + raws + [st[k] for k in PARAM_KEYS]
    gs = M._grad(loss, leaves, torch.ones((), dtype=F64))
    grads = {"fm": gs[0], "class": list(gs[1:1 + len(raws)])}
    grads.update(dict(zip(PARAM_KEYS, gs[1 + len(raws):])))
    return dict(out=tuple(t.detach() for t in (loc, cls, cls_det, corners)), grads=grads, aux=aux)


# ---------------------------------------------------------------------------------------------------------- end-to-end inputs
# name: (P, inverse, A, C, H, W, class sizes, B, seed): the four cases of tests/test_head_backward_gpu.CASES and the V1
# configuration (simplified affine, no inverse model).  The seeds are chosen so that no location of the oracle is fragile
# (backward_model.fragility) and no ReLU decision hangs on a rounding (head_relu_margin): tests/test_bn_live_model.py, on the CPU.
HEAD_CASES = {
    "v2_affine_inverse": (6, True, 2, 64, 10, 12, [(15, 15), (12, 18)], 3, 5),
    "affine_no_inverse": (6, False, 2, 64, 10, 12, [(15, 15), (12, 18)], 3, 4),
    "simple_affine_p4": (4, True, 2, 64, 10, 12, [(15, 15), (12, 18)], 3, 4),
    "odd_c67_9x13": (6, True, 2, 67, 9, 13, [(15, 15), (12, 18), (17, 13)], 3, 0),
    "v1_p4_no_inverse": (4, False, 2, 64, 10, 12, [(15, 15), (12, 18)], 3, 5),
}
BOTH, FIRST, SECOND = (True, True), (True, False), (False, True)
# the live patterns whose GRADIENTS the GPU test compares, per case: both BatchNorms live everywhere, one live beside one frozen
# for the V2 and the V1 configuration
GRAD_PATTERNS = {name: [BOTH, FIRST, SECOND] if name in ("v2_affine_inverse", "v1_p4_no_inverse") else [BOTH] for name in HEAD_CASES}
# Smooth inputs.  Two things make a gradient of the oracle jump, and an implementation that rounds differently lands on the other
# side: a sample coordinate at a cell edge (backward_model.fragility) and a pre-activation at the kink of a ReLU.  The inputs are
# chosen so that neither happens (tests/test_bn_live_model.py checks both on the CPU):
#   * identity-like theta.  A live BatchNorm hands the last layer activations of unit variance, so linear.weight ~ N(0, 0.02) of the
#     synthetic net would scatter theta by +-0.5 (near-singular inverses).  Full affine: a FIXED near-identity bias and
#     linear.weight ~ N(0, 2e-5) keep every sample coordinate within a few hundredths of a cell of the lattice w + 0.5 + 7.5 (t00 xj +
#     t01 yi), whose points are at least 0.09 cells from every integer (2 x 121 coordinates per location would otherwise put a few
#     of the 360 locations within delta ~ 2e-5 of an edge for every seed), and the corner gaps at 2 * 120 * |t01| = 2.4 px.
#     Simplified affine (t01 = t10 = 0: 2 x 11 coordinates per location): the synthetic bias, linear.weight ~ N(0, 2e-4).
#   * few pre-activations near zero.  Only the first C / 32 channels of each BatchNorm keep the synthetic beta (|beta| ~ 0.1: about
#     half of their values pass the ReLU); the others get beta = +-3.5 |gamma| (three in four positive), 3.5 standard deviations
#     from the kink.
SMOOTH = {6: dict(linear_std=2e-5, linear_bias=[1.0, 0.01, 0.0, -0.01, 1.0, 0.0]), 4: dict(linear_std=2e-4)}
KINK_CHANNELS = 32          # one channel in 32 keeps its values around the kink
# a pre-activation y = gamma xhat + beta is taken to be safe when |y| > RELU_MARGIN * |gamma| invstd max|z_c|: twice the pinned
# error of the convolution that produced z (tests/test_bn_live_stages_gpu.PIN["conv_f32"], relative to the largest |z|) - one for
# the convolution itself, one for what the layer below and the rounding of the statistics add
RELU_MARGIN = 2 * 1.3e-5


def head_inputs(name):
    """(state, fm, class maps, (gl, gc, gd)) of a HEAD_CASES entry, float32 as the head receives them."""
    import numpy as np
    from os2d_amd.utils import synthetic
    P, inverse, A, C, H, W, sizes, B, seed = HEAD_CASES[name]
    kw = dict(SMOOTH[P])
    if "linear_bias" in kw:
        kw["linear_bias"] = np.array(kw["linear_bias"], dtype=np.float32)
    state = synthetic.make_transform_net_state(P, seed=seed + 3, **kw)
    for bn in ("conv.1", "conv.4"):
        gamma, beta = state[bn + ".weight"], state[bn + ".bias"].clone()
        n = gamma.numel()
        sign = torch.where(torch.arange(n) % 4 == 3, -1.0, 1.0)
        beta[n // KINK_CHANNELS:] = (3.5 * gamma.abs() * sign)[n // KINK_CHANNELS:]
        state[bn + ".bias"] = beta
    fm = synthetic.make_feature_map(C, H, W, seed=seed + 5, A=A)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=sizes, seed=seed + 400)
    g = torch.Generator().manual_seed(seed + 7)
    up = tuple(torch.randn(A, B, k, H, W, generator=g, dtype=F64) for k in (4, 1, 1))
    return state, fm, class_fms, up


def head_relu_margin(name, live):
    """The smallest |y| / (RELU_MARGIN |gamma| invstd max|z_c|) over the pre-activations y of both BatchNorm layers of the live
    oracle: above 1, no ReLU decision of the case depends on the rounding of the forward."""
    P, inverse = HEAD_CASES[name][:2]
    state, fm, class_fms, _ = head_inputs(name)
    st = {k: v.to(F64) if v.is_floating_point() else v for k, v in state.items()}
    x = O.l2_normalize_channels(F.relu(O.correlation(O.prepare_class_maps([c.to(F64) for c in class_fms]), fm.to(F64))), 1e-6)
    worst = float("inf")
    for layer, pad in ((1, 3), (2, 2)):
        conv, bn = BN_KEYS[layer]
        z = F.conv2d(x, st[conv + ".weight"], st[conv + ".bias"], padding=pad)
        if live[layer - 1]:
            mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        else:
            mean, var = st[bn + ".running_mean"], st[bn + ".running_var"]
        v = lambda t: t.view(1, -1, 1, 1)
        scale = st[bn + ".weight"].abs() / torch.sqrt(var + O.BN_EPS)
        y = (z - v(mean)) * v(st[bn + ".weight"] / torch.sqrt(var + O.BN_EPS)) + v(st[bn + ".bias"])
        delta = RELU_MARGIN * scale * z.abs().amax(dim=(0, 2, 3))
        worst = min(worst, float((y.abs() / v(delta).clamp_min(1e-300)).min()))
        x = F.relu(y)
    return worst


def head_fragile_share(name, live):
    """Share of the locations of the case that are fragile (backward_model.fragility < 1) in the live oracle."""
    P, inverse, A, C, H, W, sizes, B, _ = HEAD_CASES[name]
    state, fm, class_fms, _ = head_inputs(name)
    st = {k: v.to(F64) if v.is_floating_point() else v for k, v in state.items()}
    q_hat = O.prepare_class_maps([c.to(F64) for c in class_fms])
    corr = O.correlation(q_hat, fm.to(F64))
    params = live_transform_net(corr, st, live)
    _, _, aux = M.decode_forward(corr, params, inverse, 16, 16)
    return float((M.fragility(aux, P, H, W, 16, 16) < 1).double().mean())
