"""GPU: the inference route "fused_conv1x1" of the backbone (os2d_amd/modeling/backbone_fused.py) as a whole -
against the torch route, both measured against the float64 CPU module; class images, grad mode, cache invalidation, a side stream,
NaN, and the model level.  The form and the image sizes are those of tests/test_backbone_fused_gpu.py.

The bound of the whole-network comparison is the one DESIGN section 18.3 gives the "fused" route: twice the torch route's error against
the float64 module, measured in the same test on the same input.  The route rounds once per BatchNorm where the torch route rounds
several times; its 1x1 convolutions accumulate in fp32 as one chain per output, as a GEMM of the torch route does in some order of its
own, and the 3x3 and 7x7 convolutions are the same MIOpen calls.  Every test prints both errors before it asserts."""
import pytest
import torch

import backbone_conv_model as C
import backbone_model as B
import util

pytestmark = pytest.mark.gpu

ROUTE = "fused_conv1x1"


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
        for route in ("torch", ROUTE):
            ex.inference_route = route
            out[route] = ex(xd)
    torch.cuda.synchronize()
    ex.inference_route = "torch"
    return out["torch"], out[ROUTE]


def check_against_float64(ex, x, want, device, what):
    plain, ours = both_routes(ex, x.to(device))
    assert ours.shape == plain.shape == want.shape and ours.is_contiguous() and ours.dtype == torch.float32
    err_torch, err_ours, top = util.maxdiff(plain.double(), want), util.maxdiff(ours.double(), want), float(want.abs().max())
    print("{}: max abs error against the float64 module: fused_conv1x1 {:.3g}, torch {:.3g}, ratio {:.3f}, at max |y| {:.4g}".format(
        what, err_ours, err_torch, err_ours / err_torch, top))
    assert top > 1 and err_torch > 0
    assert err_ours <= 2 * err_torch
    return ours


def test_route_is_as_close_to_float64_as_the_torch_route(r50, device):
    ex, x, want = r50
    assert tuple(want.shape) == (2, 1024, 8, 11)
    ours = check_against_float64(ex, x, want, device, "resnet50 2x3x128x176")
    # and it is the chain of the entry points' models (fp32 folds), to fp32 accuracy of the whole network
    model = C.extractor_forward64(ex, x)
    assert util.maxdiff(ours.double(), model) <= 2 * util.maxdiff(ours.double(), want) + 1e-4 * float(want.abs().max())
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
        ex.inference_route = ROUTE
        ours = label(list(images.to(device)))
        batch = ex(images.to(device))
    ex.inference_route = "torch"
    assert len(ours) == 3 and all(tuple(f.shape) == (1, 1024, 6, 6) for f in ours)
    err_torch = util.maxdiff(torch.cat(plain).double(), want)
    print("class images: fused_conv1x1 {:.3g} (one by one) {:.3g} (batch), torch {:.3g}".format(
        util.maxdiff(torch.cat(ours).double(), want), util.maxdiff(batch.double(), want), err_torch))
    assert util.maxdiff(torch.cat(ours).double(), want) <= 2 * err_torch and util.maxdiff(batch.double(), want) <= 2 * err_torch


def test_grad_mode_takes_the_module_path(r50, device):
    """With the route set and grad mode on, the call IS the plain module path: what it returns is torch.equal to what the module path's
    last block returned in that call, every norm layer's forward ran, and no entry point of either backbone library did."""
    from os2d_amd import _backbone_conv_lib, _backbone_lib
    from os2d_amd.modeling import backbone_fused
    ex, x, want = r50
    xd = x[:1].contiguous().to(device)
    seen, norm_calls, native_calls = [], [], []
    hooks = [ex.layer3[-1].register_forward_hook(lambda m, i, o: seen.append(o))]
    hooks += [m.register_forward_hook(lambda m, i, o: norm_calls.append(m)) for m in backbone_fused.norm_layers(ex)]
    real = (_backbone_lib.load, _backbone_conv_lib.load)
    try:
        ex.inference_route = "torch"
        plain = ex(xd)
        assert len(seen) == 1 and len(norm_calls) == 43
        ex.inference_route = ROUTE
        _backbone_lib.load = lambda: native_calls.append("backbone") or real[0]()
        _backbone_conv_lib.load = lambda: native_calls.append("conv") or real[1]()
        routed = ex(xd)
        assert routed.requires_grad and plain.requires_grad          # the module path, with its graph
        assert len(seen) == 2 and torch.equal(routed, seen[1]) and len(norm_calls) == 86 and not native_calls
        err_torch = util.maxdiff(plain.detach(), want[:1])
        assert util.maxdiff(routed.detach(), plain.detach()) <= 2 * err_torch
        with torch.no_grad():
            out = ex(xd)
        assert not out.requires_grad and len(seen) == 2 and len(norm_calls) == 86
        # now the route ran: the stem's kernel and 13 bn + relu of libos2d_backbone.so, 2 * 13 + 3 GEMMs of libos2d_backbone_conv.so
        assert native_calls.count("backbone") == 1 + 13 and native_calls.count("conv") == 2 * 13 + 3
    finally:
        _backbone_lib.load, _backbone_conv_lib.load = real
        for h in hooks:
            h.remove()
        ex.inference_route = "torch"


def test_cache_follows_the_statistics(device):
    ex = _extractor("resnet50", device, seed=6)
    x = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(7))
    xd = x.to(device)
    ex.inference_route = ROUTE
    with torch.no_grad():
        first = ex(xd)
        again = ex(xd)
        assert ex.fused_backbone().rebuilds == 1
        ex.layer2[1].bn3.running_var.mul_(2)                          # a fold that lives in a GEMM's epilogue
        after = ex(xd)
        ex.inference_route = "fused"
        ex(xd)
    assert ex.fused_backbone().rebuilds == 2                          # and the "fused" route shares the cache
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
        ex.inference_route = ROUTE
        ex(xd)                                                         # the folds exist before the side stream runs
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            out = ex(xd)
        side.synchronize()
    ex.inference_route = "torch"
    assert util.maxdiff(out.double(), want) <= 2 * err_torch


def test_nan_pixel_reaches_what_it_reaches_on_the_other_routes(r50, device):
    ex, x, _ = r50
    x = x.clone()
    x[1, 1, 60, 90] = float("nan")
    xd = x.to(device)
    plain, ours = both_routes(ex, xd)
    with torch.no_grad():
        ex.inference_route = "fused"
        fused = ex(xd)
    ex.inference_route = "torch"
    assert torch.equal(torch.isnan(ours), torch.isnan(plain)) and torch.equal(torch.isnan(ours), torch.isnan(fused))
    assert bool(torch.isnan(ours[1]).any()) and not bool(torch.isnan(ours[0]).any())


def test_model_level_against_torch(device):
    """Os2dModel with three classes as in tests/test_backbone_fused_gpu.py, within the same tolerances (those of smoke()) of the torch
    route's outputs, and detect() runs."""
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
        for route in ("torch", ROUTE):
            net.net_feature_maps.inference_route = route
            assert net.net_label_features.net_class_features.inference_route == route           # one module, both branches
            loc, cls, _, fm_size, corners = net(images=images, class_images=class_images)
            out[route] = (loc, cls, corners)
        assert (fm_size.w, fm_size.h) == (11, 8) and tuple(out[ROUTE][1].shape) == (1, 3, 88)
        print("model level: cls {:.3g} loc {:.3g} corners {:.3g}".format(*[util.maxdiff(out[ROUTE][k], out["torch"][k]) for k in (1, 0, 2)]))
        assert util.maxdiff(out[ROUTE][1], out["torch"][1]) < 1e-5
        assert util.maxdiff(out[ROUTE][0], out["torch"][0]) < 1e-4
        assert util.maxdiff(out[ROUTE][2], out["torch"][2]) < 2e-3
        head = E.build_class_head(net, class_images)
        det = E.detect(net, net.build_box_coder(), [images], head, class_ids=[0, 1, 2], nms_score_threshold=0.0)
    assert isinstance(det, BoxList) and len(det) > 0
    assert net.net_feature_maps.fused_backbone().rebuilds == 1
