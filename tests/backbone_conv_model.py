"""Float64 model of os2d_backbone_conv1x1 (include/os2d_backbone_conv.h) from torch operators on the CPU, and the chain of it and of
the models of tests/backbone_model.py over a ResNet extractor: what the inference route "fused_conv1x1" computes, in exact-enough
arithmetic.  The model takes the SAME fp32 x, w, s, t, r the kernel gets and does everything in float64."""
import torch
import torch.nn.functional as F

import backbone_model as B

U24 = 2.0 ** -24


def conv1x1(x, w, s, t, r=None, sr=None, tr=None, stride=1, relu=True):
    """x [N, Cin, H, W], w [Cout, Cin] (or conv.weight's [Cout, Cin, 1, 1]), s / t [Cout]; r [N, Cout, Ho, Wo] or None, sr / tr its fold
    or None.  -> (y64, S, v64, d64): the output, S = sum over k of |w x| (what the accumulation's error is proportional to), the value
    of the fold v and the residual term d (zeros without r), all [N, Cout, Ho, Wo] in float64."""
    xs = x.double()[:, :, ::stride, ::stride]
    w2 = w.double().reshape(w.shape[0], -1)
    acc = torch.einsum("ok,nkhw->nohw", w2, xs)
    S = torch.einsum("ok,nkhw->nohw", w2.abs(), xs.abs())
    v = B.bn(acc, s, t)
    if r is None:
        d = torch.zeros_like(v)
        y = v
    else:
        d = B.bn(r, sr, tr) if sr is not None else r.double()
        y = v + d
    return (B.relu_nan(y) if relu else y), S, v, d


def bound(Cin, S, s, v64, d64=None, folds_of_r=0):
    """The derived bound of the entry point against the model.  The accumulator is a chain of Cin fmaf: its error is at most
    Cin * 2^-24 * S to first order (every partial sum is at most S in magnitude and is rounded once), and the fold multiplies it by
    |s|.  The fold's own rounding is 2^-24 |v|, the add's 2^-24 |v + d| <= 2^-24 (|v| + |d|): together 2^-23 |v| and 2^-24 |d|, stated as
    2^-23 |v| + 2^-23 |d| with a residual, and 2^-23 |d| more when the residual has a fold of its own (one more rounding of d, 2^-24 |d|)."""
    b = Cin * U24 * S * s.double().abs().view(1, -1, 1, 1) + B.U23 * v64.abs()
    if d64 is not None:
        b = b + (1 + folds_of_r) * B.U23 * d64.abs()
    return b


def bottleneck64(block, x, fold=B.fold32):
    """One Bottleneck as the route runs it: conv1 + bn1 + relu, conv2 (float64 conv2d) + bn2 + relu, the downsample branch where there is
    one, conv3 + bn3 + residual + relu."""
    w = lambda conv: conv.weight.detach().cpu()
    x = x.detach().cpu().double()
    out = conv1x1(x, w(block.conv1), *fold(block.bn1))[0]
    out = B.bn_relu(F.conv2d(out, w(block.conv2).double(), None, block.stride, 1), *fold(block.bn2))[0]
    if block.downsample is not None:
        x = conv1x1(x, w(block.downsample[0]), *fold(block.downsample[1]), stride=block.downsample[0].stride[0], relu=False)[0]
    return conv1x1(out, w(block.conv3), *fold(block.bn3), r=x)[0]


def extractor_forward64(ex, x, fold=B.fold32):
    """The route over a ResNetFeatureExtractor in float64 (``fold=B.fold_exact``: unrounded folds)."""
    x = x.detach().cpu().double()
    x = B.bn_relu_maxpool(F.conv2d(x, ex.conv1.weight.detach().cpu().double(), None, 2, 3), *fold(ex.bn1))[0]
    for stage in ex.resnet_blocks:
        for block in stage:
            x = bottleneck64(block, x, fold)
    return x


def resnet_c4_layers():
    """The distinct 1x1 convolutions of ResNet50-C4 (ResNet101-C4 only repeats them) as (role, Cin, Cout, stride), read from the module:
    role "conv1" (fold + relu), "conv3" (fold + block input + relu) or "downsample" (fold alone, the layer's stride)."""
    from os2d_amd.modeling.feature_extractor import resnet50_c4
    seen = []
    for stage in resnet50_c4().resnet_blocks:
        for block in stage:
            convs = [("conv1", block.conv1), ("conv3", block.conv3)] + ([("downsample", block.downsample[0])] if block.downsample is not None else [])
            for role, conv in convs:
                case = (role, conv.in_channels, conv.out_channels, conv.stride[0])
                if case not in seen:
                    seen.append(case)
    return seen
