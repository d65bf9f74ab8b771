"""ResNet-C4 feature extractor.  Its module path is PyTorch-ROCm (MIOpen convolutions, ATen BatchNorm / ReLU / pooling); it is
the default (``inference_route = "torch"``) and the only path of every training call.  With ``inference_route = "fused"`` an
inference call with frozen BatchNorms keeps MIOpen for the convolutions and runs everything between them - the folded BatchNorms,
ReLUs, residual adds and the stem's pooling - as HIP kernels of libos2d_backbone.so (backbone_fused.py).
With ``inference_route = "fused_conv1x1"`` the 1x1 convolutions of such a call run as fp32 MFMA GEMMs of libos2d_backbone_conv.so as
well, with the fold, the residual add and the ReLU as their epilogue; ``conv1x1_precision = "bf16x3"`` runs
those GEMMs in split-bf16 arithmetic on the bf16 matrix instruction (libos2d_backbone_conv_bf16.so).

Mirrors reference os2d/modeling/feature_extractor.py:13-129 (``build_feature_extractor``, ``ResNetFeatureExtractor``,
``resnet50_c4`` / ``resnet101_c4``).  torchvision is not available in this image, so the ResNet (v1.5 bottleneck:
stride on the 3x3 convolution, as torchvision >= 0.5) is defined here with torchvision's module / parameter names
(``conv1, bn1, layer1.0.conv1, layer1.0.downsample.0, ...``) so reference checkpoints load key-for-key.
"""
import os
from itertools import chain

import torch.nn as nn

from ..structures.feature_map import FeatureMapSize
from . import backbone_fused

GROUPNORM_NUMGROUPS = 32


def get_norm_layer(use_group_norm):
    if use_group_norm:
        return lambda width: nn.GroupNorm(GROUPNORM_NUMGROUPS, width)
    return nn.BatchNorm2d


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm_layer=nn.BatchNorm2d):
        super(Bottleneck, self).__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = norm_layer(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class ResNetFeatureExtractor(nn.Module):
    """conv1-bn1-relu-maxpool-layer1..layer{level-1}; level 4 = C4: stride 16, 1024 channels
    (reference feature_extractor.py:23-65).

    ``inference_route``: "torch" (the default; the environment variable OS2D_BACKBONE_ROUTE sets the initial value), "fused" or
    "fused_conv1x1".  The last two need BatchNorm layers (ValueError with GroupNorm), "fused_conv1x1" plain 1x1 convolutions as well
    (``backbone_fused.plain_conv1x1``); they are taken by the calls ``backbone_fused.eligible`` describes: grad mode off, a contiguous
    fp32 HIP tensor, every BatchNorm in eval mode.  Every other call runs the modules below as they are.

    ``conv1x1_precision``: "f32" (the default; OS2D_BACKBONE_CONV_PRECISION sets the initial value) or "bf16x3", the arithmetic of the
    1x1 GEMMs.  It is read on the route "fused_conv1x1" alone."""

    def __init__(self, layers, level, feature_map_stride, feature_map_receptive_field, use_group_norm=False):
        super(ResNetFeatureExtractor, self).__init__()
        assert level in [1, 2, 3, 4, 5], "Feature level should be one of 1, 2, 3, 4, 5"
        norm_layer = get_norm_layer(use_group_norm)
        self._norm_layer = norm_layer
        self.feature_map_receptive_field = feature_map_receptive_field
        self.feature_map_stride = feature_map_stride
        self._feature_level = level
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        names = ["layer1", "layer2", "layer3", "layer4"][:level - 1]
        planes = [64, 128, 256, 512]
        strides = [1, 2, 2, 2]
        for i, name in enumerate(names):
            setattr(self, name, self._make_layer(planes[i], layers[i], strides[i]))
        self._block_names = names
        self._inference_route, self._fused = "torch", None      # plain attributes: no parameter, buffer or submodule
        self.inference_route = os.environ.get(backbone_fused.ROUTE_ENV, "torch")
        self._conv1x1_precision = "f32"
        self.conv1x1_precision = os.environ.get(backbone_fused.PRECISION_ENV, "f32")
        for m in self.modules():   # torchvision's default initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    @property
    def resnet_blocks(self):
        return [getattr(self, n) for n in self._block_names]

    def _make_layer(self, planes, blocks, stride):
        norm_layer = self._norm_layer
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                norm_layer(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, norm_layer)]
        self.inplanes = planes * Bottleneck.expansion
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes, norm_layer=norm_layer))
        return nn.Sequential(*layers)

    @property
    def inference_route(self):
        return self._inference_route

    @inference_route.setter
    def inference_route(self, route):
        if route not in backbone_fused.ROUTES:
            raise ValueError("inference_route is one of {}, not {!r}".format(backbone_fused.ROUTES, route))
        if route in backbone_fused.FOLDING_ROUTES and not backbone_fused.has_only_batchnorm(self):
            raise ValueError("inference_route {!r} folds BatchNorm2d layers: this extractor normalises with GroupNorm".format(route))
        if route == "fused_conv1x1" and not all(backbone_fused.plain_conv1x1(c) for c in backbone_fused.pointwise_convs(self)):
            raise ValueError("inference_route 'fused_conv1x1' runs plain 1x1 convolutions (no bias, groups 1, dilation 1, padding 0, "
                             "stride 1 or 2, contiguous fp32 weight): this extractor has others")
        self._inference_route = route

    @property
    def conv1x1_precision(self):
        return self._conv1x1_precision

    @conv1x1_precision.setter
    def conv1x1_precision(self, precision):
        if precision not in backbone_fused.PRECISIONS:
            raise ValueError("conv1x1_precision is one of {}, not {!r}".format(backbone_fused.PRECISIONS, precision))
        self._conv1x1_precision = precision

    def fused_backbone(self):
        """The runner of the fused route with its fold cache (made on first use)."""
        if self._fused is None:
            self._fused = backbone_fused.FusedBackbone(self)
        return self._fused

    def forward(self, x):
        if self._inference_route == "fused" and backbone_fused.eligible(self, x):
            return self.fused_backbone().forward(x)
        if self._inference_route == "fused_conv1x1" and backbone_fused.eligible(self, x):
            return self.fused_backbone().forward_conv1x1(x)
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        for layer in self.resnet_blocks:
            x = layer(x)
        return x

    def freeze_bn(self):
        for layer in self.modules():
            if isinstance(layer, nn.BatchNorm2d):
                layer.eval()

    def freeze_blocks(self, num_blocks=0):
        """Freeze the first ``num_blocks`` blocks; block 0 = conv1+bn1 (reference feature_extractor.py:73-83)."""
        layer0 = [nn.ModuleList([self.conv1, self.bn1])]
        remaining = num_blocks
        for b in chain(layer0, chain.from_iterable(self.resnet_blocks)):
            if remaining > 0:
                for p in b.parameters():
                    p.requires_grad = False
                remaining -= 1

    def get_num_blocks_in_feature_extractor(self):
        return 1 + sum(len(b) for b in self.resnet_blocks)


def resnet50_c4(use_group_norm=False):
    """R-50-C4 (reference feature_extractor.py:108-117): stride 16, declared receptive field 16."""
    return ResNetFeatureExtractor([3, 4, 6, 3], 4, FeatureMapSize(h=16, w=16), FeatureMapSize(h=16, w=16), use_group_norm)


def resnet101_c4(use_group_norm=False):
    """R-101-C4 (reference feature_extractor.py:120-129)."""
    return ResNetFeatureExtractor([3, 4, 23, 3], 4, FeatureMapSize(h=16, w=16), FeatureMapSize(h=16, w=16), use_group_norm)


def build_feature_extractor(backbone_arch, use_group_norm=False):
    """reference feature_extractor.py:13-20."""
    arch = backbone_arch.lower()
    if arch == "resnet50":
        return resnet50_c4(use_group_norm=use_group_norm)
    if arch == "resnet101":
        return resnet101_c4(use_group_norm=use_group_norm)
    raise RuntimeError("Unknown backbone arch: {0}".format(backbone_arch))
