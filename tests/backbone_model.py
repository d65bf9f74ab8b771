"""Float64 models of the entry points of libos2d_backbone.so (include/os2d_backbone.h) and of the BatchNorm fold, written from torch
operators on the CPU, and the chain of them over a ResNet extractor: what the fused inference route computes, in exact-enough
arithmetic.  The models take the SAME fp32 s / t the kernels get and do everything after that in float64."""
import torch
import torch.nn.functional as F

U23 = 2.0 ** -23
SLACK = 1.01


def fold64(weight, bias, running_mean, running_var, eps):
    """The fold in float64, NOT rounded: s = gamma / sqrt(var + eps), t = beta - mean * s."""
    s = weight.double() / torch.sqrt(running_var.double() + eps)
    return s, bias.double() - running_mean.double() * s


def _per_channel(v):
    return v.double().view(1, -1, 1, 1)


def relu_nan(v):
    return torch.where(v < 0, torch.zeros_like(v), v)


def bn(x, s, t):
    return x.double() * _per_channel(s) + _per_channel(t)


def bn_relu(x, s, t):
    """-> (y, v): the output and the value before the ReLU"""
    v = bn(x, s, t)
    return relu_nan(v), v


def bn_add_relu(x, s, t, r, sr=None, tr=None):
    """-> (y, v, d)"""
    v = bn(x, s, t)
    d = bn(r, sr, tr) if sr is not None else r.double()
    return relu_nan(v + d), v, d


def maxpool_nan(a):
    """MaxPool2d(3, 2, 1) of a tensor of values >= 0 or NaN: the padding (0) never wins, a NaN in a window wins."""
    nan = F.max_pool2d(torch.isnan(a).double(), 3, 2, 1) > 0
    m = F.max_pool2d(torch.nan_to_num(a, nan=0.0), 3, 2, 1)
    return torch.where(nan, torch.full_like(m, float("nan")), m)


def bn_relu_maxpool(x, s, t):
    """-> (y, vmax): the output and the largest |value before the ReLU| of each window (what the bound is taken at)"""
    a, v = bn_relu(x, s, t)
    return maxpool_nan(a), F.max_pool2d(torch.nan_to_num(v.abs(), nan=0.0), 3, 2, 1)


def perturb_batchnorms(module, seed):
    """gamma and var uniform in [0.5, 1.5], beta and mean 0.2 * N(0, 1): no BatchNorm of the network is the identity."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))


def fold32(m):
    """(s, t) in fp32 of one BatchNorm, as the route folds it (float64, one rounding)."""
    s, t = fold64(m.weight.detach().cpu(), m.bias.detach().cpu(), m.running_mean.detach().cpu(), m.running_var.detach().cpu(), m.eps)
    return s.float(), t.float()


def fold_exact(m):
    """(s, t) of one BatchNorm in float64, not rounded: the chain with these is the torch module in other words."""
    return fold64(m.weight.detach().cpu(), m.bias.detach().cpu(), m.running_mean.detach().cpu(), m.running_var.detach().cpu(), m.eps)


def extractor_forward64(ex, x, fold32=fold32):
    """The fused route over a ResNetFeatureExtractor (CPU copy or not: parameters are read to the CPU) in float64: float64
    convolutions of the fp32 weights, the models above in between, fp32 folds (``fold32=fold_exact``: unrounded ones)."""
    w = lambda conv: conv.weight.detach().cpu().double()
    x = x.detach().cpu().double()
    x = bn_relu_maxpool(F.conv2d(x, w(ex.conv1), None, 2, 3), *fold32(ex.bn1))[0]
    for stage in ex.resnet_blocks:
        for block in stage:
            out = bn_relu(F.conv2d(x, w(block.conv1)), *fold32(block.bn1))[0]
            out = bn_relu(F.conv2d(out, w(block.conv2), None, block.stride, 1), *fold32(block.bn2))[0]
            out = F.conv2d(out, w(block.conv3))
            if block.downsample is None:
                x = bn_add_relu(out, *fold32(block.bn3), x)[0]
            else:
                x = bn_add_relu(out, *fold32(block.bn3), F.conv2d(x, w(block.downsample[0]), None, block.stride), *fold32(block.downsample[1]))[0]
    return x


def module_forward64(ex, x):
    """The torch module itself in float64 on the CPU (a twin: the extractor is left as it is)."""
    twin = _copy_module(ex)
    twin.inference_route = "torch"
    with torch.no_grad():
        return twin.double().eval()(x.detach().cpu().double())


def _copy_module(ex):
    """A CPU twin of an extractor with the same parameters and statistics."""
    from os2d_amd.modeling.feature_extractor import ResNetFeatureExtractor
    layers = [len(stage) for stage in ex.resnet_blocks]
    twin = ResNetFeatureExtractor(layers, ex._feature_level, ex.feature_map_stride, ex.feature_map_receptive_field)
    twin.load_state_dict({k: v.detach().cpu() for k, v in ex.state_dict().items()})
    twin.train(ex.training)
    return twin


def ulp32(v):
    """The spacing of fp32 numbers at |v| (v float64 tensor of normal fp32 magnitude)."""
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)

