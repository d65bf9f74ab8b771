"""GPU: the fused inference route of the backbone (os2d_amd/modeling/backbone_fused.py) as a whole - against the torch route, both
measured against the float64 CPU module; class images, grad mode, cache invalidation, a side stream, NaN, and the model level.

Image sizes are those of tests/test_model_gpu.py, so MIOpen picks its kernels once per process.

The bound of the whole-network comparison: the fused route rounds once per BatchNorm (one fmaf with a fold rounded once) where the
torch route rounds several times (subtract, scale, multiply, add), and both run the same convolutions; so its error against the
float64 module is at most that of the torch route, and twice the torch route's error, measured in the same test on the same
input, leaves room for the two routes' roundings falling differently."""
import pytest
import torch

import backbone_model as B
import util

pytestmark = pytest.mark.gpu


def _extractor(arch, device, seed=0):
    from os2d_amd.modeling.feature_extractor import build_feature_extractor
    torch.manual_seed(seed)
    ex = build_feature_extractor(arch)
    B.perturb_batchnorms(ex, seed=seed + 1)
    ex.inference_route = "torch"
    return ex.to(device).eval()


@pytest.fixture(scope="module")
def r50(device):
    """ResNet50-C4 at seed 0 with perturbed BatchNorms, its input 2 x 3 x 128 x 176 and the float64 CPU module's output of it."""
    ex = _extractor("resnet50", device)
    x = torch.randn(2, 3, 128, 176, generator=torch.Generator().manual_seed(1))
    return ex, x, B.module_forward64(ex, x)


def both_routes(ex, xd):
    out = {}
    with torch.no_grad():
        for route in ("torch", "fused"):
            ex.inference_route = route
            out[route] = ex(xd)
    torch.cuda.synchronize()
    ex.inference_route = "torch"
    return out["torch"], out["fused"]


def check_against_float64(ex, x, want, device, what):
    plain, fused = both_routes(ex, x.to(device))
    assert fused.shape == plain.shape == want.shape and fused.is_contiguous() and fused.dtype == torch.float32
    err_torch, err_fused, top = util.maxdiff(plain.double(), want), util.maxdiff(fused.double(), want), float(want.abs().max())
    print("{}: max abs error against the float64 module: fused {:.3g}, torch {:.3g}, at max |y| {:.4g}".format(what, err_fused, err_torch, top))
    assert top > 1 and err_torch > 0
    assert err_fused <= 2 * err_torch
    return fused


def test_fused_route_is_as_close_to_float64_as_the_torch_route(r50, device):
    ex, x, want = r50
    assert tuple(want.shape) == (2, 1024, 8, 11)
    fused = check_against_float64(ex, x, want, device, "resnet50 2x3x128x176")
    # and it is the chain of the entry points' models (fp32 folds), to fp32 accuracy of the whole network
    model = B.extractor_forward64(ex, x)
    assert util.maxdiff(fused.double(), model) <= 2 * util.maxdiff(fused.double(), want) + 1e-4 * float(want.abs().max())
    assert ex.fused_backbone().rebuilds == 1


def test_resnet101(device):
    ex = _extractor("resnet101", device, seed=3)
    x = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(4))
    check_against_float64(ex, x, B.module_forward64(ex, x), device, "resnet101 1x3x96x128")


def test_class_image_batch_through_the_label_extractor(r50, device):
    from os2d_amd.modeling.model import LabelFeatureExtractor
    ex, _, _ = r50
    images = torch.randn(3, 3, 96, 96, generator=torch.Generator().manual_seed(5))
    want = B.module_forward64(ex, images)
    label = LabelFeatureExtractor(ex)
    with torch.no_grad():
        ex.inference_route = "torch"
        plain = label(list(images.to(device)))
        ex.inference_route = "fused"
        fused = label(list(images.to(device)))
        batch = ex(images.to(device))
    ex.inference_route = "torch"
    assert len(fused) == 3 and all(tuple(f.shape) == (1, 1024, 6, 6) for f in fused)
    err_torch = util.maxdiff(torch.cat(plain).double(), want)
    assert util.maxdiff(torch.cat(fused).double(), want) <= 2 * err_torch and util.maxdiff(batch.double(), want) <= 2 * err_torch


def test_grad_mode_takes_the_module_path(r50, device):
    """With "fused" set and grad mode on, the call IS the plain module path: what it returns is torch.equal to what the module path's
    last block returned in that call, every norm layer's forward ran, and no kernel of the fused route did.  (Two runs of the module
    path cannot be compared with torch.equal: MIOpen is not bit-reproducible call to call, see tests/test_model_gpu.py - measured
    here too, the two runs differ in the last bits; they are compared to the torch route's own error instead.)"""
    from os2d_amd import _backbone_lib
    from os2d_amd.modeling import backbone_fused
    ex, x, want = r50
    xd = x[:1].contiguous().to(device)
    seen, norm_calls, native_calls = [], [], []
    hooks = [ex.layer3[-1].register_forward_hook(lambda m, i, o: seen.append(o))]
    hooks += [m.register_forward_hook(lambda m, i, o: norm_calls.append(m)) for m in backbone_fused.norm_layers(ex)]
    real_load = _backbone_lib.load
    try:
        ex.inference_route = "torch"
        plain = ex(xd)
        assert len(seen) == 1 and len(norm_calls) == 43
        ex.inference_route = "fused"
        _backbone_lib.load = lambda: native_calls.append(1) or real_load()
        routed = ex(xd)
        assert routed.requires_grad and plain.requires_grad          # the module path, with its graph
        assert len(seen) == 2 and torch.equal(routed, seen[1]) and len(norm_calls) == 86 and not native_calls
        err_torch = util.maxdiff(plain.detach(), want[:1])
        assert util.maxdiff(routed.detach(), plain.detach()) <= 2 * err_torch
        with torch.no_grad():
            out = ex(xd)
        assert not out.requires_grad and len(seen) == 2 and len(norm_calls) == 86 and native_calls       # now the fused route ran
    finally:
        _backbone_lib.load = real_load
        for h in hooks:
            h.remove()
        ex.inference_route = "torch"


def test_cache_follows_the_statistics(device):
    ex = _extractor("resnet50", device, seed=6)
    x = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(7))
    xd = x.to(device)
    ex.inference_route = "fused"
    with torch.no_grad():
        first = ex(xd)
        again = ex(xd)
        assert ex.fused_backbone().rebuilds == 1
        ex.layer2[1].bn2.running_var.mul_(2)
        after = ex(xd)
    assert ex.fused_backbone().rebuilds == 2
    want = B.module_forward64(ex, x)                                  # of the NEW statistics
    ex.inference_route = "torch"
    with torch.no_grad():
        plain_err = util.maxdiff(ex(xd).double(), want)
    assert util.maxdiff(after.double(), want) <= 2 * plain_err
    assert util.maxdiff(first.double(), want) > 100 * plain_err       # the old fold is far from it: the change is visible
    assert util.maxdiff(again, first) <= 2 * plain_err                # (MIOpen is not bit-reproducible call to call)


def test_side_stream(r50, device):
    ex, x, want = r50
    xd = x.to(device)
    with torch.no_grad():
        ex.inference_route = "torch"
        err_torch = util.maxdiff(ex(xd).double(), want)
        ex.inference_route = "fused"
        ex(xd)                                                         # the folds exist before the side stream runs
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            out = ex(xd)
        side.synchronize()
    ex.inference_route = "torch"
    assert util.maxdiff(out.double(), want) <= 2 * err_torch


def test_nan_pixel_reaches_what_it_reaches_on_the_torch_route(r50, device):
    ex, x, _ = r50
    x = x.clone()
    x[1, 1, 60, 90] = float("nan")
    plain, fused = both_routes(ex, x.to(device))
    assert torch.equal(torch.isnan(fused), torch.isnan(plain))
    assert bool(torch.isnan(fused[1]).any()) and not bool(torch.isnan(fused[0]).any())


def test_model_level_fused_against_torch(device):
    """Os2dModel with three classes as in tests/test_model_gpu.py: the head's outputs of the fused route within the project's global
    tolerances (those of smoke()) of the torch route's, and detect() runs."""
    from os2d_amd.engine import evaluate as E
    from os2d_amd.modeling.model import Os2dModel
    from os2d_amd.structures.bounding_box import BoxList
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
        for route in ("torch", "fused"):
            net.net_feature_maps.inference_route = route
            assert net.net_label_features.net_class_features.inference_route == route           # one module, both branches
            loc, cls, _, fm_size, corners = net(images=images, class_images=class_images)
            out[route] = (loc, cls, corners)
        assert (fm_size.w, fm_size.h) == (11, 8) and tuple(out["fused"][1].shape) == (1, 3, 88)
        assert util.maxdiff(out["fused"][1], out["torch"][1]) < 1e-5
        assert util.maxdiff(out["fused"][0], out["torch"][0]) < 1e-4
        assert util.maxdiff(out["fused"][2], out["torch"][2]) < 2e-3
        head = E.build_class_head(net, class_images)
        det = E.detect(net, net.build_box_coder(), [images], head, class_ids=[0, 1, 2], nms_score_threshold=0.0)
    assert isinstance(det, BoxList) and len(det) > 0
    assert net.net_feature_maps.fused_backbone().rebuilds == 1
