"""GPU: the precision "bf16x3" of the backbone's inference route "fused_conv1x1" (os2d_amd/modeling/backbone_fused.py, DESIGN.md section
18.7) as a whole, as tests/test_backbone_conv1x1_gpu.py tests the route in fp32: against the float64 CPU module, with the torch route and
the fp32 route measured in the same test on the same input.  The bound is the one that file applies to the fp32 route: twice the torch
route's error.  Every test prints the errors before it asserts."""
import pytest
import torch

import backbone_model as B
import util
from test_backbone_conv1x1_gpu import _extractor

pytestmark = pytest.mark.gpu

ROUTE = "fused_conv1x1"


def three_ways(ex, xd):
    """-> the outputs of the torch route, the fp32 route and the bf16x3 route for one input"""
    out = {}
    with torch.no_grad():
        for name, route, precision in (("torch", "torch", "f32"), ("f32", ROUTE, "f32"), ("bf16x3", ROUTE, "bf16x3")):
            ex.inference_route, ex.conv1x1_precision = route, precision
            out[name] = ex(xd)
    torch.cuda.synchronize()
    ex.inference_route, ex.conv1x1_precision = "torch", "f32"
    return out


def check_against_float64(ex, x, want, device, what):
    out = three_ways(ex, x.to(device))
    err = {name: util.maxdiff(y.double(), want) for name, y in out.items()}
    top = float(want.abs().max())
    print("{}: max abs error against the float64 module: bf16x3 {:.3g}, f32 {:.3g}, torch {:.3g}; bf16x3 / torch {:.3f}, bf16x3 / f32 {:.3f}, at max |y| {:.4g}".format(
        what, err["bf16x3"], err["f32"], err["torch"], err["bf16x3"] / err["torch"], err["bf16x3"] / err["f32"], top))
    ours = out["bf16x3"]
    assert ours.shape == want.shape and ours.is_contiguous() and ours.dtype == torch.float32
    assert top > 1 and err["torch"] > 0
    assert err["bf16x3"] <= 2 * err["torch"]
    return out


@pytest.fixture(scope="module")
def r50(device):
    """ResNet50-C4 at seed 0 with perturbed BatchNorms, its input 2 x 3 x 128 x 176 and the float64 CPU module's output of it."""
    ex = _extractor("resnet50", device)
    x = torch.randn(2, 3, 128, 176, generator=torch.Generator().manual_seed(1))
    return ex, x, B.module_forward64(ex, x)


def test_route_is_as_close_to_float64_as_the_torch_route(r50, device):
    ex, x, want = r50
    assert tuple(want.shape) == (2, 1024, 8, 11)
    check_against_float64(ex, x, want, device, "resnet50 2x3x128x176")
    runner = ex.fused_backbone()
    assert runner.rebuilds == 1 and runner.weight_packs == 1              # one fold cache for both precisions, one pack


def test_resnet101(device):
    ex = _extractor("resnet101", device, seed=3)
    x = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(4))
    check_against_float64(ex, x, B.module_forward64(ex, x), device, "resnet101 1x3x96x128")


def test_class_images_one_by_one_and_as_a_batch(r50, device):
    """The 1x1 GEMMs of ours give an image the same bits wherever it stands; MIOpen's 3x3 convolutions between them need not, so the
    comparison of the whole network is the one tests/test_backbone_conv1x1_gpu.py makes, and the bits are compared on one bottleneck's
    1x1 layers."""
    from os2d_amd.modeling.model import LabelFeatureExtractor
    ex, _, _ = r50
    images = torch.randn(3, 3, 96, 96, generator=torch.Generator().manual_seed(5))
    want = B.module_forward64(ex, images)
    label = LabelFeatureExtractor(ex)
    with torch.no_grad():
        ex.inference_route = "torch"
        plain = label(list(images.to(device)))
        ex.inference_route, ex.conv1x1_precision = ROUTE, "bf16x3"
        ours = label(list(images.to(device)))
        batch = ex(images.to(device))
        # the GEMMs themselves: conv1 and the downsample branch of the first block on a batch and on its images one by one
        runner, block = ex.fused_backbone(), ex.layer1[0]
        folds, packed = runner.folds(device), runner.packed_weights(device)
        feats = torch.randn(3, 64, 24, 24, generator=torch.Generator().manual_seed(6)).to(device)
        for conv, bn, relu in ((block.conv1, block.bn1, True), (block.downsample[0], block.downsample[1], False)):
            together = runner._conv1x1(feats, conv, folds[id(bn)], relu, wp=packed[id(conv)])
            for i in range(3):
                assert torch.equal(together[i:i + 1], runner._conv1x1(feats[i:i + 1].contiguous(), conv, folds[id(bn)], relu, wp=packed[id(conv)]))
    ex.inference_route, ex.conv1x1_precision = "torch", "f32"
    assert len(ours) == 3 and all(tuple(f.shape) == (1, 1024, 6, 6) for f in ours)
    err_torch = util.maxdiff(torch.cat(plain).double(), want)
    print("class images: bf16x3 {:.3g} (one by one) {:.3g} (batch), torch {:.3g}".format(
        util.maxdiff(torch.cat(ours).double(), want), util.maxdiff(batch.double(), want), err_torch))
    assert util.maxdiff(torch.cat(ours).double(), want) <= 2 * err_torch and util.maxdiff(batch.double(), want) <= 2 * err_torch


def test_weight_cache_follows_the_weights(device):
    ex = _extractor("resnet50", device, seed=6)
    x = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(7))
    xd = x.to(device)
    ex.inference_route, ex.conv1x1_precision = ROUTE, "bf16x3"
    runner = ex.fused_backbone()
    with torch.no_grad():
        first = ex(xd)
        ex(xd)
        assert runner.weight_packs == 1 and runner.rebuilds == 1          # one pack per weight version
        ex.layer2[1].conv3.weight.mul_(2)                                  # in place: the version changes, the address does not
        after = ex(xd)
        ex(xd)
        assert runner.weight_packs == 2 and runner.rebuilds == 1
        ex.layer1[0].bn1.running_var.mul_(2)                               # a fold changes: the weights are not packed again
        ex(xd)
        assert runner.weight_packs == 2 and runner.rebuilds == 2
        ex.layer1[0].bn1.running_var.div_(2)
    want = B.module_forward64(ex, x)                                       # of the NEW weight
    ex.inference_route, ex.conv1x1_precision = "torch", "f32"
    with torch.no_grad():
        plain_err = util.maxdiff(ex(xd).double(), want)
    assert util.maxdiff(after.double(), want) <= 2 * plain_err
    assert util.maxdiff(first.double(), want) > 100 * plain_err           # the old weight is far from it: the change is visible


def test_switching_back_gives_the_fp32_route(r50, device):
    """"f32" after "bf16x3" runs the fp32 GEMMs again: the outputs of its own 1x1 layers are bit for bit those of the fp32 entry point, and the
    whole network is the fp32 route within what MIOpen's call-to-call differences allow."""
    from os2d_amd import _backbone_conv_bf16_lib, _backbone_conv_lib
    ex, x, want = r50
    xd = x.to(device)
    calls = []
    real = (_backbone_conv_lib.load, _backbone_conv_bf16_lib.load)
    try:
        _backbone_conv_lib.load = lambda: calls.append("f32") or real[0]()
        _backbone_conv_bf16_lib.load = lambda: calls.append("bf16x3") or real[1]()
        with torch.no_grad():
            ex.inference_route, ex.conv1x1_precision = ROUTE, "f32"
            before = ex(xd)
            assert calls.count("f32") == 2 * 13 + 3 and "bf16x3" not in calls
            del calls[:]
            ex.conv1x1_precision = "bf16x3"
            ex(xd)
            assert calls.count("bf16x3") >= 2 * 13 + 3 and "f32" not in calls            # (packed_elems and pack_weights load it as well)
            del calls[:]
            ex.conv1x1_precision = "f32"
            back = ex(xd)
            assert calls.count("f32") == 2 * 13 + 3 and "bf16x3" not in calls
            # one GEMM of the route in either setting of the runner's call: without packed weights it IS the fp32 entry point
            runner, block = ex.fused_backbone(), ex.layer1[0]
            fold = runner.folds(device)[id(block.bn1)]
            feats = torch.randn(2, 64, 10, 12, generator=torch.Generator().manual_seed(8)).to(device)
            y = torch.empty(2, 64, 10, 12, device=device)
            from os2d_amd._native import STREAM
            real[0]()  # loaded
            _backbone_conv_lib.call("os2d_backbone_conv1x1", feats, block.conv1.weight.detach(), fold[0], fold[1], None, None, None, y, 2, 64, 64, 10, 12, 1, 1, STREAM)
            assert torch.equal(runner._conv1x1(feats, block.conv1, fold, True), y)
    finally:
        _backbone_conv_lib.load, _backbone_conv_bf16_lib.load = real
        ex.inference_route, ex.conv1x1_precision = "torch", "f32"
    err_torch = util.maxdiff(three_ways(ex, xd)["torch"].double(), want)
    assert util.maxdiff(back, before) <= 2 * err_torch


def test_model_level_against_torch(device):
    """Os2dModel with three classes as in tests/test_backbone_conv1x1_gpu.py, within the same tolerances (those of smoke()) of the torch
    route's outputs."""
    from os2d_amd.modeling.model import Os2dModel
    from os2d_amd.utils import synthetic
    torch.manual_seed(5)
    net = Os2dModel(is_cuda=False, merge_branch_parameters=True, backbone_arch="resnet50", use_inverse_geom_model=True, simplify_affine=False)
    net.os2d_head_creator.aligner.parameter_regressor.load_state_dict(synthetic.make_transform_net_state(6, seed=5))
    net.to(device).eval()
    g = torch.Generator().manual_seed(2)
    class_images = [torch.randn(3, 96, 96, generator=g).to(device), torch.randn(3, 96, 96, generator=g).to(device),
                    torch.randn(3, 80, 112, generator=g).to(device)]
    images = torch.randn(1, 3, 128, 176, generator=g).to(device)
    out = {}
    with torch.no_grad():
        for name, route, precision in (("torch", "torch", "f32"), ("bf16x3", ROUTE, "bf16x3")):
            net.net_feature_maps.inference_route, net.net_feature_maps.conv1x1_precision = route, precision
            assert net.net_label_features.net_class_features.conv1x1_precision == precision      # one module, both branches
            loc, cls, _, fm_size, corners = net(images=images, class_images=class_images)
            out[name] = (loc, cls, corners)
    assert (fm_size.w, fm_size.h) == (11, 8) and tuple(out["bf16x3"][1].shape) == (1, 3, 88)
    print("model level: cls {:.3g} loc {:.3g} corners {:.3g}".format(*[util.maxdiff(out["bf16x3"][k], out["torch"][k]) for k in (1, 0, 2)]))
    assert util.maxdiff(out["bf16x3"][1], out["torch"][1]) < 1e-5
    assert util.maxdiff(out["bf16x3"][0], out["torch"][0]) < 1e-4
    assert util.maxdiff(out["bf16x3"][2], out["torch"][2]) < 2e-3
    assert net.net_feature_maps.fused_backbone().weight_packs == 1
