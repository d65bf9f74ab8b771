"""Autograd through the HIP head: the training forward (the strict-fp32 "f32" route or, on request, the direct split-fp16
"f16x3" route; stage by stage, intermediates kept) and the backward pass of libos2d_train.so (include/os2d_train.h), wrapped in
one ``torch.autograd.Function``.

``Os2dHead.forward`` comes here when grad mode is on and the image feature maps, the raw class maps the head was created from
(``Os2dHeadCreator.create_os2d_head``) or a TransformNet parameter require grad.  Gradients reach
  * the image feature maps (through the image L2 normalisation, eps 1e-5),
  * the raw class maps (through the class L2 normalisation and the bilinear resize to 15 x 15),
  * the TransformNet: conv.0 / conv.3 / linear weights and biases and the affine parameters of the frozen (eval-mode)
    BatchNorms conv.1 / conv.4 (weight = gamma, bias = beta); the running statistics stay constants.
The five GEMM-shaped launches of the backward pass run in fp32 or, with ``train_precision = "f16x3"`` on the head or its
creator (or $OS2D_TRAIN_PRECISION), in split-fp16 arithmetic within fp32 rounding of it.
With ``train_forward_precision = "f16x3"`` (or $OS2D_TRAIN_FORWARD_PRECISION) - a switch of its own, independent of
``train_precision`` - the forward runs the f16x3 stage kernels of the inference route (os2d_corr_f16x3, os2d_transform_conv_f16x3 x 3,
os2d_sample_decode: the bits of ``head(fm, precision="f16x3")``) and os2d_train_planes_from_shb turns each split-half blocked
activation buffer into the fp32 planes the backward reads - exactly, so the backward differentiates the values the forward
multiplied with.
With ``deterministic = True`` on the head or its creator (or $OS2D_DETERMINISTIC, or torch.use_deterministic_algorithms(True))
the d corr scatter of the decode backward adds 64-bit integers on a fixed-point grid instead of fp32 atomics: two passes on the
same inputs then return the same bits for every gradient.
A BatchNorm of the TransformNet in training mode ("live": ``TransformationNet.live_batchnorm``) takes the statistics of the call's
own batch, updates its running statistics as torch does - under torch.no_grad() too - and its backward goes through the statistics
(``_stages_live``; os2d_train_conv_forward / _bn_stats / _bn_relu_forward / _bn_relu_backward_batch); the bias
of the convolution in front of it gets an exactly zero gradient.  ``head.last_live_batchnorm`` records which layers were live.
As in the reference (head.py:396-402, 423): ``cls_det`` carries the same values as ``cls`` but its gradient reaches the
correlation only, not the transformation; ``corners`` carries none.
"""
import os

import torch

from .. import _lib
from .. import _train_lib
from .._native import STREAM

TEMPLATE = 15
MAX_W_DIRECT7 = 209
# arithmetic of the backward pass's five GEMM launches (the `arith` argument of the *_ex entry points of include/os2d_train.h):
# "f32" = v_mfma_f32_16x16x4_f32, "f16x3" = split-fp16 operands on v_mfma_f32_32x32x16_f16, within fp32 rounding of "f32".  The
# training FORWARD does not follow it: that is TRAIN_FORWARD_PRECISIONS.
TRAIN_PRECISIONS = ("f32", "f16x3")
DEFAULT_TRAIN_PRECISION = "f32"
# arithmetic of the training forward: "f32" = the strict-fp32 stages (the bits of ``precision="f32"``), "f16x3" = the direct
# split-fp16 stages (the bits of ``precision="f16x3"``) + os2d_train_planes_from_shb
TRAIN_FORWARD_PRECISIONS = ("f32", "f16x3")
DEFAULT_TRAIN_FORWARD_PRECISION = "f32"


def resolve_train_precision(value=None):
    """``value`` (a head's or a creator's ``train_precision``) or, for None, $OS2D_TRAIN_PRECISION (default "f32")."""
    value = value or os.environ.get("OS2D_TRAIN_PRECISION") or DEFAULT_TRAIN_PRECISION
    if value not in TRAIN_PRECISIONS:
        raise ValueError("unknown train_precision {!r}: one of {}".format(value, TRAIN_PRECISIONS))
    return value


def resolve_train_forward_precision(value=None):
    """``value`` (a head's or a creator's ``train_forward_precision``) or, for None, $OS2D_TRAIN_FORWARD_PRECISION (default "f32")."""
    value = value or os.environ.get("OS2D_TRAIN_FORWARD_PRECISION") or DEFAULT_TRAIN_FORWARD_PRECISION
    if value not in TRAIN_FORWARD_PRECISIONS:
        raise ValueError("unknown train_forward_precision {!r}: one of {}".format(value, TRAIN_FORWARD_PRECISIONS))
    return value


def resolve_deterministic(value=None):
    """``value`` (a head's or a creator's ``deterministic``: True / False) or, for None, $OS2D_DETERMINISTIC ("0" / empty: off,
    anything else: on) or, where that is not set, ``torch.are_deterministic_algorithms_enabled()``."""
    if value is not None and not isinstance(value, bool):
        raise ValueError("deterministic must be None, True or False, got {!r}".format(value))
    if value is not None:
        return value
    env = os.environ.get("OS2D_DETERMINISTIC")
    if env is not None:
        return env not in ("0", "")
    return bool(torch.are_deterministic_algorithms_enabled())


def _wgrad_splits(NB, PL):
    """Split-K slices of a weight gradient: one per ~4096 positions of the NB * PLANE reduction, at most 64."""
    return max(1, min(64, (NB * PL + 4095) // 4096))


def _corr_front_f32(head, fm, corr, shape):
    """The fp32 correlation front: fills ``corr``; returns (rnorm [NB,226,PLANE], sumsq), which the caller keeps to its end."""
    A, B, C, H, W, P, PL = shape
    sumsq = torch.empty(A * H * W, dtype=torch.float32, device=fm.device)
    rnorm = torch.empty(A * B * 226 * PL, dtype=torch.float32, device=fm.device)
    _lib.call("os2d_fm_sumsq", fm, sumsq, A, C, H, W, STREAM)
    _lib.call("os2d_corr", fm, head._qp, sumsq, corr, rnorm, A, B, C, H, W, STREAM)
    return rnorm, sumsq


def _corr_front_f16x3(lib, head, fm, corr, shape):
    """The split-fp16 correlation front: fills ``corr``; returns (the blocked rnorm, the workspace: the caller frees it)."""
    A, B, C, H, W, P, PL = shape
    qs = head._split_class_operand()
    ws = torch.empty(int(lib.os2d_corr_f16x3_workspace_bytes(A, C, H, W)), dtype=torch.uint8, device=fm.device)
    rshb = torch.empty(A * B * int(lib.os2d_shb_bytes(225, H, W)), dtype=torch.uint8, device=fm.device)
    _lib.call("os2d_corr_f16x3", fm, qs, corr, rshb, A, B, C, H, W, ws, ws.numel(), STREAM)
    return rshb, ws


def _planes_from_shb(buf, exp, channels, out_channels, shape):
    """A split-half blocked activation buffer as the fp32 planes [NB,out_channels,PLANE] the backward reads (exact)."""
    A, B, C, H, W, P, PL = shape
    out = torch.empty(A * B * out_channels * PL, dtype=torch.float32, device=buf.device)
    _train_lib.call("os2d_train_planes_from_shb", buf, exp, A * B, channels, out_channels, H, W, out, STREAM)
    return out


def _stages_f32(head, fm, corr, prm, shape):
    """The strict-fp32 stages up to the transformation parameters: fills ``corr`` and ``prm``, returns the activations
    (rnorm [NB,226,PLANE], h1 [NB,128,PLANE], h2 [NB,64,PLANE]) as flat fp32 tensors."""
    A, B, C, H, W, P, PL = shape
    NB = A * B
    f32 = dict(dtype=torch.float32, device=fm.device)
    w1, b1, w2, b2, w3, b3 = head.aligner.parameter_regressor.packed("f32")
    rnorm, sumsq = _corr_front_f32(head, fm, corr, shape)
    h1 = torch.empty(NB * 128 * PL, **f32)
    h2 = torch.empty(NB * 64 * PL, **f32)
    for layer, src, wp, bp, dst in ((1, rnorm, w1, b1, h1), (2, h1, w2, b2, h2), (3, h2, w3, b3, prm)):
        _lib.call("os2d_transform_conv", layer, src, wp, bp, dst, NB, P, H, W, STREAM)
    return rnorm, h1, h2


def _stages_f16x3(lib, head, fm, corr, prm, shape):
    """The same on the direct split-fp16 route: the stage entry points the head call of ``precision="f16x3"`` is made of (they
    zero the borders the next layer's taps read themselves: os2d_corr_f16x3 those of its output before the correlation writes
    it, the convolutions in their epilogue).  Each split-half blocked buffer becomes fp32 planes (os2d_train_planes_from_shb:
    exact) as soon as the layer that reads it has been launched, and is freed: at most one activation tensor exists twice.
    An activation outside the fp16 range - a non-finite feature: nothing else gets past the range plan - raises the head's
    sticky status word (``Os2dHead.range_status``), as on the inference route."""
    A, B, C, H, W, P, PL = shape
    NB = A * B
    dev = fm.device
    regressor = head.aligner.parameter_regressor
    w1, b1, w2, b2, w3, b3 = regressor.packed("f16x3")
    exps = regressor.activation_exponents()
    status = _lib.host_ptr(head._status_word())

    def shb(channels):
        return torch.empty(NB * int(lib.os2d_shb_bytes(channels, H, W)), dtype=torch.uint8, device=dev)

    def conv(layer, src, wp, bp, dst):
        _lib.call("os2d_transform_conv_f16x3", layer, src, wp, bp, dst, NB, P, H, W, 3, status, STREAM)

    rshb, ws = _corr_front_f16x3(lib, head, fm, corr, shape)
    del ws
    h1shb = shb(128)
    conv(1, rshb, w1, b1, h1shb)
    rnorm = _planes_from_shb(rshb, exps[0], 225, 226, shape)
    del rshb
    h2shb = shb(64)
    conv(2, h1shb, w2, b2, h2shb)
    h1 = _planes_from_shb(h1shb, exps[1], 128, 128, shape)
    del h1shb
    conv(3, h2shb, w3, b3, prm)
    h2 = _planes_from_shb(h2shb, exps[2], 64, 64, shape)
    del h2shb
    return rnorm, h1, h2


def _update_running_stats(bn, mean, var, n):
    """torch's training-mode update of a BatchNorm's buffers from the batch statistics (biased ``var`` of ``n`` values), as a few
    in-place torch ops on the device: no host synchronisation, and the buffers' ``_version`` moves, which is what the
    packed-weight and spectra caches of the TransformNet are keyed on."""
    m = float(bn.momentum)
    bn.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
    bn.running_var.mul_(1.0 - m).add_(var, alpha=m * n / (n - 1.0))
    bn.num_batches_tracked.add_(1)


def _stages_live(lib, head, fm, corr, prm, shape, live, forward_precision):
    """The stages up to the transformation parameters when a BatchNorm of the TransformNet takes batch statistics (DESIGN.md
    section 16).  Both layers with a BatchNorm run os2d_train_conv_forward (the raw convolution z; arith = the forward
    precision) and os2d_train_bn_relu_forward; a live layer gets its mean and 1 / sqrt(var + eps) from os2d_train_bn_stats and
    updates its running statistics, a frozen layer beside it gets the running ones (its eval-mode fold, applied after the
    convolution instead of folded into it).  Layer 3 has no BatchNorm and keeps its fp32 kernel.  Returns
    (rnorm, h1, h2, [(z, mean, invstd) or None per layer])."""
    A, B, C, H, W, P, PL = shape
    NB, HW = A * B, H * W
    dev = fm.device
    f32 = dict(dtype=torch.float32, device=dev)
    tl = _train_lib.load()
    regressor = head.aligner.parameter_regressor
    arith = TRAIN_FORWARD_PRECISIONS.index(forward_precision)
    if arith:
        rshb, ws = _corr_front_f16x3(lib, head, fm, corr, shape)
        # the exponent of the normalised correlation is a constant of the library: it does not depend on the BatchNorms
        exp0 = torch.full((225,), int(lib.os2d_rnorm_exp()), dtype=torch.int32, device=dev)
        rnorm = _planes_from_shb(rshb, exp0, 225, 226, shape)
        del ws, rshb
    else:
        rnorm, sumsq = _corr_front_f32(head, fm, corr, shape)
    src, acts, kept = rnorm, [], []
    layers = ((1, regressor.conv[0], regressor.conv[1], 128), (2, regressor.conv[3], regressor.conv[4], 64))
    for (layer, conv, bn, cout), is_live in zip(layers, live):
        z = torch.empty(NB * cout * PL, **f32)
        cws = torch.empty(int(tl.os2d_train_conv_forward_workspace_floats(arith, layer, P, NB)), **f32)
        _train_lib.call("os2d_train_conv_forward", arith, layer, P, conv.weight.detach().contiguous(), conv.bias.detach().contiguous(), src,
                        NB, H, W, z, cws, cws.numel(), STREAM)
        if is_live:
            mean, var, invstd = (torch.empty(cout, **f32) for _ in range(3))
            bws = torch.empty(int(tl.os2d_train_bn_workspace_bytes(layer, NB)), dtype=torch.uint8, device=dev)
            _train_lib.call("os2d_train_bn_stats", layer, z, NB, H, W, float(bn.eps), mean, var, invstd, bws, bws.numel(), STREAM)
            _update_running_stats(bn, mean, var, float(NB * HW))
        else:
            mean = bn.running_mean.detach().contiguous()
            invstd = 1.0 / torch.sqrt(bn.running_var.detach() + float(bn.eps))
        h = torch.empty(NB * cout * PL, **f32)
        _train_lib.call("os2d_train_bn_relu_forward", layer, z, bn.weight.detach().contiguous(), bn.bias.detach().contiguous(), mean,
                        invstd, NB, H, W, h, STREAM)
        kept.append((z, mean, invstd) if is_live else None)
        acts.append(h)
        src = h
    w3, b3 = regressor.packed_linear_f32()
    _lib.call("os2d_transform_conv", 3, acts[1], w3, b3, prm, NB, P, H, W, STREAM)
    return rnorm, acts[0], acts[1], kept


class _HeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, n_class, fm, *tensors):
        raws, params = tensors[:n_class], tensors[n_class:]
        lib = _lib.load()
        A, C, H, W = fm.shape
        B = head.class_batch_size
        NB, HW = A * B, H * W
        dev = fm.device
        regressor = head.aligner.parameter_regressor
        P = regressor.output_dim
        inverse = 1 if head.aligner.use_inverse_geom_model else 0
        PL = int(lib.os2d_plane_floats(H, W))
        f32 = dict(dtype=torch.float32, device=dev)
        corr = torch.empty(NB, 225, HW, **f32)
        prm = torch.empty(NB, P, HW, **f32)
        loc = torch.empty(A, B, 4, H, W, **f32)
        cls = torch.empty(A, B, 1, H, W, **f32)
        corners = torch.empty(A, B, 8, H, W, **f32)
        with torch.cuda.device(dev):
            live, kept = head.last_live_batchnorm, [None, None]
            if any(live):
                rnorm, h1, h2, kept = _stages_live(lib, head, fm, corr, prm, (A, B, C, H, W, P, PL), live, head.last_train_forward_precision)
            elif head.last_train_forward_precision == "f16x3":
                rnorm, h1, h2 = _stages_f16x3(lib, head, fm, corr, prm, (A, B, C, H, W, P, PL))
            else:
                rnorm, h1, h2 = _stages_f32(head, fm, corr, prm, (A, B, C, H, W, P, PL))
            _lib.call("os2d_sample_decode", corr, prm, NB, H, W, P, inverse, head._stride, head._rec_field, loc, cls, corners, STREAM)
        q15raw = None
        if any(ctx.needs_input_grad[3:3 + n_class]):
            from .head import _prepare_class_maps
            q15raw, _ = _prepare_class_maps(list(raws), normalise=False)
        ctx.head, ctx.n_class, ctx.shape = head, n_class, (A, B, C, H, W, P, inverse, PL)
        ctx.arith = TRAIN_PRECISIONS.index(head.last_train_precision)
        ctx.deterministic = head.last_deterministic
        ctx.saved = dict(fm=fm, raws=raws, corr=corr, rnorm=rnorm, h1=h1, h2=h2, params=prm, q15raw=q15raw,
                         weights=[p.detach().contiguous() for p in params], live=kept)
        if head.keep_train_activations:
            head.last_train_activations = dict(corr=corr, rnorm=rnorm, h1=h1, h2=h2, params=prm)
        ctx.mark_non_differentiable(corners)
        return loc, cls, cls.clone(), corners

    @staticmethod
    def backward(ctx, dloc, dcls, dcls_det, _dcorners):
        tl = _train_lib.load()
        head, n_class = ctx.head, ctx.n_class
        A, B, C, H, W, P, inverse, PL = ctx.shape
        arith = ctx.arith
        sv = ctx.saved
        NB, HW = A * B, H * W
        fm = sv["fm"]
        dev = fm.device
        need = ctx.needs_input_grad
        need_fm, need_cls = need[2], any(need[3:3 + n_class])
        need_p = need[3 + n_class:]
        w1, b1, g1, be1, w2, b2, g2, be2, w3, b3 = sv["weights"]
        regressor = head.aligner.parameter_regressor
        bn1, bn2 = regressor.conv[1], regressor.conv[4]
        f32 = dict(dtype=torch.float32, device=dev)

        def grad_in(t):
            return None if t is None else t.contiguous()
        dloc, dcls, dcls_det = grad_in(dloc), grad_in(dcls), grad_in(dcls_det)
        grads = [None] * 10
        dfm, draws = None, [None] * n_class
        with torch.cuda.device(dev):
            dcorr = torch.zeros(NB, 225, HW, **f32)
            dparams = torch.empty(NB, P, HW, **f32)
            decode_args = (sv["corr"], sv["params"], dcls, dcls_det, dloc, NB, H, W, P, inverse, head._stride, head._rec_field, dcorr, dparams)
            if ctx.deterministic:
                ws = torch.empty(int(tl.os2d_train_decode_backward_det_workspace_bytes(NB, H, W)), dtype=torch.uint8, device=dev)
                _train_lib.call("os2d_train_decode_backward_det", *decode_args, ws, ws.numel(), STREAM)
                del ws
            else:
                _train_lib.call("os2d_train_decode_backward", *decode_args, STREAM)
            splits = _wgrad_splits(NB, PL)

            def wgrad(layer, x, dy, like):
                n = int(tl.os2d_train_conv_weight_slice_floats_ex(arith, layer, P))
                ws = torch.empty(n * splits, **f32)
                dw = torch.empty_like(like)
                _train_lib.call("os2d_train_conv_backward_weight_ex", arith, layer, P, x, dy, NB, H, W, dw, ws, ws.numel(), STREAM)
                return dw

            def dgrad(layer, w, dy, cin):
                ws = torch.empty(int(tl.os2d_train_conv_data_workspace_floats_ex(arith, layer, P, NB)), **f32)
                dx = torch.empty(NB * cin * PL, **f32)
                _train_lib.call("os2d_train_conv_backward_data_ex", arith, layer, P, w, dy, NB, H, W, dx, ws, ws.numel(), STREAM)
                return dx

            def bn_relu(layer, dh, h, bn, gamma, beta, cout, ig, ib, iw):
                dy = torch.empty(NB * cout * PL, **f32)
                dg = torch.empty(cout, **f32) if need_p[ig] else None
                dbe = torch.empty(cout, **f32) if need_p[ib] else None
                if sv["live"][layer - 1] is not None:
                    # batch statistics: the backward goes through them; the convolution's bias cancels in z - mean
                    z, mean, invstd = sv["live"][layer - 1]
                    ws = torch.empty(int(tl.os2d_train_bn_workspace_bytes(layer, NB)), dtype=torch.uint8, device=dev)
                    _train_lib.call("os2d_train_bn_relu_backward_batch", layer, dh, z, h, gamma, mean, invstd, NB, H, W, dy, dg, dbe, ws,
                                    ws.numel(), STREAM)
                    grads[ig], grads[ib], grads[iw] = dg, dbe, (torch.zeros(cout, **f32) if need_p[iw] else None)
                    return dy
                db = torch.empty(cout, **f32) if need_p[iw] else None
                _train_lib.call("os2d_train_bn_relu_backward", layer, dh, h, gamma, beta, bn.running_var.detach().contiguous(),
                                float(bn.eps), NB, H, W, dy, dg, dbe, db, STREAM)
                grads[ig], grads[ib], grads[iw] = dg, dbe, db
                return dy

            # layer 3 (linear): parameters -> plane gradient, bias gradient
            dy3 = torch.empty(NB * P * PL, **f32)
            db3 = torch.empty(P, **f32) if need_p[9] else None
            _train_lib.call("os2d_train_params_backward", dparams, NB, P, H, W, dy3, db3, STREAM)
            grads[9] = db3
            if need_p[8]:
                grads[8] = wgrad(3, sv["h2"], dy3, w3)
            need_below = need_fm or need_cls or any(need_p[:8])
            if need_below:
                dh2 = dgrad(3, w3, dy3, 64)
                dy2 = bn_relu(2, dh2, sv["h2"], bn2, g2, be2, 64, 6, 7, 5)
                if need_p[4]:
                    grads[4] = wgrad(2, sv["h1"], dy2, w2)
                dh1 = dgrad(2, w2, dy2, 128)
                dy1 = bn_relu(1, dh1, sv["h1"], bn1, g1, be1, 128, 2, 3, 1)
                if need_p[0]:
                    grads[0] = wgrad(1, sv["rnorm"], dy1, w1)
                if need_fm or need_cls:
                    dxn = dgrad(1, w1, dy1, 225)
                    _train_lib.call("os2d_train_norm225_backward", sv["corr"], dxn, NB, H, W, dcorr, STREAM)
            if need_fm or need_cls:
                ws = torch.empty(int(tl.os2d_train_corr_workspace_floats_ex(arith, A, B, C, H, W)), **f32)
                dfm = torch.empty(A, C, H, W, **f32) if need_fm else None
                dq = torch.empty(B, C, 225, **f32) if need_cls else None
                _train_lib.call("os2d_train_corr_backward_ex", arith, fm, head._qp, dcorr, A, B, C, H, W, dfm, dq, ws, ws.numel(), STREAM)
                if need_cls:
                    raws = sv["raws"]
                    draws = [torch.empty(r.shape, **f32) for r in raws]
                    ptrs = torch.tensor([d.data_ptr() for d in draws], dtype=torch.int64).to(dev)
                    sizes = torch.tensor([[r.shape[-2], r.shape[-1]] for r in raws], dtype=torch.int32).to(dev)
                    cws = torch.empty(B * C * 225, **f32)
                    _train_lib.call("os2d_train_class_backward", sv["q15raw"], dq, B, C, ptrs, sizes, cws, cws.numel(), STREAM)
                    draws = [d if need[3 + i] else None for i, d in enumerate(draws)]
        grads = [g if need_p[i] else None for i, g in enumerate(grads)]
        return (None, None, dfm) + tuple(draws) + tuple(grads)


def transform_parameters(regressor):
    """The TransformNet tensors that receive gradients, in the Function's order (reference state-dict names)."""
    c = regressor.conv
    return [c[0].weight, c[0].bias, c[1].weight, c[1].bias, c[3].weight, c[3].bias, c[4].weight, c[4].bias,
            regressor.linear.weight, regressor.linear.bias]


def needs_grad(head, feature_maps):
    """True when grad mode is on and something the head reads requires grad."""
    if not torch.is_grad_enabled():
        return False
    raws = head._raw_class_maps or []
    return (feature_maps.requires_grad or any(r.requires_grad for r in raws)
            or any(p.requires_grad for p in transform_parameters(head.aligner.parameter_regressor)))


def head_forward_train(head, feature_maps):
    """(loc, cls, cls_det, corners) of ``Os2dHead.forward`` with autograd (see the module docstring).  The arithmetic of the
    backward GEMMs is ``head.train_precision`` (None: $OS2D_TRAIN_PRECISION, default "f32"); the one taken is recorded in
    ``head.last_train_precision``; the arithmetic of the forward is ``head.train_forward_precision`` (None:
    $OS2D_TRAIN_FORWARD_PRECISION, default "f32"), recorded in ``head.last_train_forward_precision`` and ``head.last_precision``; whether the backward pass is the bit-reproducible one (``head.deterministic``,
    ``resolve_deterministic``) in ``head.last_deterministic``."""
    head.last_train_precision = resolve_train_precision(head.train_precision)
    head.last_train_forward_precision = head.last_precision = resolve_train_forward_precision(head.train_forward_precision)
    head.last_deterministic = resolve_deterministic(head.deterministic)
    A, C, H, W = feature_maps.shape
    if W > MAX_W_DIRECT7:
        raise RuntimeError("autograd through the HIP head needs feature maps at most {} columns wide (the direct 7x7 kernels of the "
                           "training forward), got W={}: crop the training images".format(MAX_W_DIRECT7, W))
    regressor = head.aligner.parameter_regressor
    regressor.check_ready(allow_live_batchnorm=True)
    # which BatchNorms take the statistics of this call's batch (each follows its own training flag); recorded for the caller
    head.last_live_batchnorm = regressor.live_batchnorm()
    _train_lib.load()                       # a missing backward library is an error now, not at backward time
    raws = list(head._raw_class_maps) if head._raw_class_maps is not None else []
    for r in raws:
        if r.device != feature_maps.device or r.dtype != torch.float32:
            raise RuntimeError("raw class maps must be float32 on {}".format(feature_maps.device))
    out = _HeadFunction.apply(head, len(raws), feature_maps, *raws, *transform_parameters(regressor))
    if not needs_grad(head, feature_maps):
        # a training-mode BatchNorm without autograd (torch.no_grad(), or nothing requires grad): one recognition tensor, as on
        # the inference route
        return out[0], out[1], out[1], out[3]
    return out
