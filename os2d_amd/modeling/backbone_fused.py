"""The frozen-BatchNorm inference route of ``ResNetFeatureExtractor``: MIOpen keeps the convolutions,
everything between them runs as HIP kernels of libos2d_backbone.so (include/os2d_backbone.h).

A BatchNorm in eval mode is one multiply-add per element.  ``fold_batchnorm`` turns its four tensors into a multiplier and an
offset per channel, in float64, rounded once to fp32:

    s = gamma / sqrt(running_var + eps)        t = beta - running_mean * s

so a bottleneck is three convolutions and three kernels (bn + relu in place, twice; bn + residual [+ the downsample branch's bn]
+ relu) where the module path runs seven pointwise kernels, and the stem is one convolution and one kernel (bn + relu + maxpool)
where the module path runs three full-tensor passes.

The folds of all layers live in ONE device buffer that belongs to a ``FusedBackbone``, which an extractor keeps as a plain
attribute: it adds no parameter, buffer or submodule, so ``state_dict()``, ``parameters()`` and ``named_modules()`` of the
extractor are what they were.  The buffer is rebuilt when any of the four tensors of any norm layer was written to
(``_version``) or replaced (``data_ptr``), or when the call's device changes.

``inference_route = "fused_conv1x1"`` goes one step further: the 1x1 convolutions - conv1, conv3 and the
downsample branch of every bottleneck, half of the backbone's arithmetic - run as fp32 GEMMs of libos2d_backbone_conv.so
(include/os2d_backbone_conv.h) with the fold, the residual add and the ReLU as the GEMM's epilogue.  A bottleneck is then two or three
GEMMs of ours, MIOpen's 3x3 convolution and one bn + relu kernel.  The weights go in as ``conv.weight`` lies in memory: no copy, no
cache.  The stem and the fold cache are those of "fused".

``conv1x1_precision = "bf16x3"`` is a second arithmetic for those GEMMs, read on that route alone: every fp32
operand split exactly into three bf16 values, six products on the bf16 matrix instruction, fp32 accumulation
(libos2d_backbone_conv_bf16.so, include/os2d_backbone_conv_bf16.h).  The weights of a frozen backbone are split ONCE, into one device
buffer of the runner beside the folds; it is rebuilt when a weight was written to or replaced.  Activations are split inside the
kernel: no bf16 copy of one exists in memory.  "f32" is the default and stays bit for bit what it is.

There is no fallback in here: a missing library raises ``Os2dLibraryError``.  WHICH calls take this route is part of its
definition (``eligible``): inference calls on a contiguous fp32 device tensor with every BatchNorm in eval mode."""
import torch
import torch.nn as nn

from .. import _backbone_conv_bf16_lib, _backbone_conv_lib, _backbone_lib
from .._native import STREAM

ROUTES = ("torch", "fused", "fused_conv1x1")
FOLDING_ROUTES = ("fused", "fused_conv1x1")          # the routes that fold BatchNorms: they need an extractor without GroupNorm
ROUTE_ENV = "OS2D_BACKBONE_ROUTE"
PRECISIONS = ("f32", "bf16x3")                       # the arithmetic of the 1x1 GEMMs of "fused_conv1x1"
PRECISION_ENV = "OS2D_BACKBONE_CONV_PRECISION"


def fold_batchnorm(weight, bias, running_mean, running_var, eps):
    """(s, t) of one or several concatenated BatchNorms as float32 tensors: float64 arithmetic, one rounding."""
    s = weight.double() / torch.sqrt(running_var.double() + eps)
    t = bias.double() - running_mean.double() * s
    return s.float(), t.float()


def norm_layers(extractor):
    """The norm layers of an extractor in the order the runner meets them: the stem's, then per block bn1, bn2, bn3 and the
    downsample branch's."""
    layers = [extractor.bn1]
    for stage in extractor.resnet_blocks:
        for block in stage:
            layers += [block.bn1, block.bn2, block.bn3]
            if block.downsample is not None:
                layers.append(block.downsample[1])
    return layers


def has_only_batchnorm(extractor):
    return all(isinstance(m, nn.BatchNorm2d) for m in norm_layers(extractor))


def pointwise_convs(extractor):
    """The 1x1 convolutions of an extractor: per block conv1, conv3 and the downsample branch's."""
    convs = []
    for stage in extractor.resnet_blocks:
        for block in stage:
            convs += [block.conv1, block.conv3]
            if block.downsample is not None:
                convs.append(block.downsample[0])
    return convs


def plain_conv1x1(conv):
    """What os2d_backbone_conv1x1 computes: a 1x1 Conv2d without bias, groups 1, dilation 1, no padding, stride 1 or 2 (the same both
    ways), and a contiguous fp32 weight."""
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.bias is None and conv.groups == 1 and conv.dilation == (1, 1)
            and conv.padding == (0, 0) and conv.stride in ((1, 1), (2, 2)) and conv.weight.dtype == torch.float32 and conv.weight.is_contiguous())


def frozen(extractor):
    """Every norm layer is a BatchNorm2d in eval mode that normalises with running statistics (and has an affine part)."""
    return all(isinstance(m, nn.BatchNorm2d) and not m.training and m.running_mean is not None and m.running_var is not None
               and m.weight is not None and m.bias is not None for m in norm_layers(extractor))


def eligible(extractor, x):
    """Does this call take the fused route?  Grad mode off, a non-empty contiguous fp32 [N, 3, H, W] tensor on a HIP device, every
    norm layer frozen.  Any other call (every training call among them) is the module path, unchanged."""
    return (not torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.numel() > 0 and x.is_contiguous() and frozen(extractor))


class FusedBackbone(object):
    """Runner of the fused route over the module tree of one extractor; NOT a module (see the module docstring)."""

    def __init__(self, extractor):
        if not has_only_batchnorm(extractor):
            raise ValueError("the fused backbone route folds BatchNorm2d layers: this extractor has other norm layers (GroupNorm)")
        self.extractor = extractor
        self._key = None
        self._folds = None          # {id(norm layer): (s view, t view)}
        self._buffer = None         # [2, sum of channels] float32 on the device: all s, then all t
        self.rebuilds = 0
        self._weight_key = None
        self._packed = None         # {id(conv): its view of the buffer}
        self._weight_buffer = None  # int16 on the device: the split weights of every 1x1 convolution, one layer after the other
        self.weight_packs = 0

    def _cache_key(self, device):
        key = [device]
        for m in norm_layers(self.extractor):
            key += [id(m), m.eps]                   # the folds are looked up by layer: a copied runner rebuilds them
            for v in (m.weight, m.bias, m.running_mean, m.running_var):
                key += [v._version, v.data_ptr()]
        return tuple(key)

    def folds(self, device):
        """{id(norm layer): (s, t)} as views of the one device buffer, rebuilt when a tensor they come from changed."""
        key = self._cache_key(device)
        if key == self._key:
            return self._folds
        layers = norm_layers(self.extractor)
        with torch.no_grad():
            cat = [torch.cat([getattr(m, name).detach().to(device).reshape(-1) for m in layers]) for name in ("weight", "bias", "running_mean", "running_var")]
            eps = torch.cat([torch.full((m.num_features,), m.eps, dtype=torch.float64, device=device) for m in layers])
            s, t = fold_batchnorm(cat[0], cat[1], cat[2], cat[3], eps)
            self._buffer = torch.stack([s, t]).contiguous()
        self._folds, at = {}, 0
        for m in layers:
            self._folds[id(m)] = (self._buffer[0, at:at + m.num_features], self._buffer[1, at:at + m.num_features])
            at += m.num_features
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()       # the buffer serves calls on every stream from here on
        self._key = key
        self.rebuilds += 1
        return self._folds

    def packed_weights(self, device):
        """{id(conv): wp} of the 1x1 convolutions for the bf16x3 precision, as views of the one device buffer: split again when a weight
        was written to (``_version``) or replaced (``data_ptr``), or when the device changes."""
        convs = pointwise_convs(self.extractor)
        key = (device,) + tuple(v for c in convs for v in (id(c), c.weight._version, c.weight.data_ptr()))
        if key == self._weight_key:
            return self._packed
        sizes = [_backbone_conv_bf16_lib.packed_elems(c.out_channels, c.in_channels) for c in convs]      # each a multiple of 8: 16-byte units
        self._weight_buffer = torch.empty(sum(sizes), dtype=torch.int16, device=device)
        self._packed, at = {}, 0
        for c, n in zip(convs, sizes):
            if not plain_conv1x1(c):
                raise ValueError("the fused_conv1x1 route runs plain 1x1 convolutions, not {}".format(c))
            self._packed[id(c)] = self._weight_buffer[at:at + n]
            _backbone_conv_bf16_lib.call("os2d_backbone_conv_bf16_pack_weights", c.weight.detach(), self._packed[id(c)], c.out_channels,
                                         c.in_channels, STREAM)
            at += n
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()       # the buffer serves calls on every stream from here on
        self._weight_key = key
        self.weight_packs += 1
        return self._packed

    @staticmethod
    def _bn_relu(x, fold):
        n, c, h, w = x.shape
        _backbone_lib.call("os2d_backbone_bn_relu", x, fold[0], fold[1], x, n, c, h * w, STREAM)
        return x

    @staticmethod
    def _bn_add_relu(x, fold, r, fold_r):
        n, c, h, w = x.shape
        if r.shape != x.shape:
            raise ValueError("residual of shape {} for a block output of shape {}".format(tuple(r.shape), tuple(x.shape)))
        sr, tr = fold_r if fold_r is not None else (None, None)
        _backbone_lib.call("os2d_backbone_bn_add_relu", x, fold[0], fold[1], r, sr, tr, x, n, c, h * w, STREAM)
        return x

    @staticmethod
    def _bn_relu_maxpool(x, fold):
        n, c, h, w = x.shape
        y = torch.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=x.dtype, device=x.device)
        _backbone_lib.call("os2d_backbone_bn_relu_maxpool", x, fold[0], fold[1], y, n, c, h, w, STREAM)
        return y

    @staticmethod
    def _conv1x1(x, conv, fold, relu, r=None, wp=None):
        """relu?(fold(conv(x)) [+ r]) as ONE kernel; x and r contiguous, the output is new memory.  wp: the packed weights of conv for
        the bf16x3 arithmetic (``packed_weights``); without them the GEMM is the fp32 one."""
        if not plain_conv1x1(conv):
            raise ValueError("the fused_conv1x1 route runs plain 1x1 convolutions (no bias, groups 1, dilation 1, padding 0, stride 1 or 2, "
                             "contiguous fp32 weight), not {}".format(conv))
        n, cin, h, w = x.shape
        stride, cout = conv.stride[0], conv.out_channels
        y = torch.empty((n, cout, (h - 1) // stride + 1, (w - 1) // stride + 1), dtype=x.dtype, device=x.device)
        if r is not None and r.shape != y.shape:
            raise ValueError("residual of shape {} for a block output of shape {}".format(tuple(r.shape), tuple(y.shape)))
        lib, entry, weights = ((_backbone_conv_bf16_lib, "os2d_backbone_conv1x1_bf16x3", wp) if wp is not None else
                               (_backbone_conv_lib, "os2d_backbone_conv1x1", conv.weight.detach()))
        lib.call(entry, x, weights, fold[0], fold[1], r, None, None, y, n, cin, cout, h, w, stride, int(relu), STREAM)
        return y

    def forward_conv1x1(self, x):
        """The route "fused_conv1x1": as ``forward``, with every 1x1 convolution and what follows it as one GEMM of ours, in the
        arithmetic ``extractor.conv1x1_precision`` names."""
        ex = self.extractor
        folds = self.folds(x.device)
        packed = self.packed_weights(x.device) if ex.conv1x1_precision == "bf16x3" else None
        wp = (lambda conv: packed[id(conv)]) if packed is not None else (lambda conv: None)
        x = self._bn_relu_maxpool(ex.conv1(x).contiguous(), folds[id(ex.bn1)])
        for stage in ex.resnet_blocks:
            for block in stage:
                out = self._conv1x1(x, block.conv1, folds[id(block.bn1)], True, wp=wp(block.conv1))
                out = self._bn_relu(block.conv2(out).contiguous(), folds[id(block.bn2)])
                if block.downsample is not None:
                    x = self._conv1x1(x, block.downsample[0], folds[id(block.downsample[1])], False, wp=wp(block.downsample[0]))
                x = self._conv1x1(out, block.conv3, folds[id(block.bn3)], True, r=x, wp=wp(block.conv3))
        return x

    def forward(self, x):
        """x: contiguous fp32 [N, 3, H, W] on a HIP device, grad mode off (``eligible``).  Returns the C4 feature map."""
        ex = self.extractor
        folds = self.folds(x.device)
        x = self._bn_relu_maxpool(ex.conv1(x).contiguous(), folds[id(ex.bn1)])
        for stage in ex.resnet_blocks:
            for block in stage:
                out = self._bn_relu(block.conv1(x).contiguous(), folds[id(block.bn1)])
                out = self._bn_relu(block.conv2(out).contiguous(), folds[id(block.bn2)])
                out = block.conv3(out).contiguous()
                if block.downsample is None:
                    x = self._bn_add_relu(out, folds[id(block.bn3)], x, None)
                else:
                    x = self._bn_add_relu(out, folds[id(block.bn3)], block.downsample[0](x).contiguous(), folds[id(block.downsample[1])])
        return x

    __call__ = forward
