"""GPU: the head with a training-mode (batch-statistics, "live") BatchNorm in the TransformNet, through ``Os2dHead.forward``
(os2d_amd/modeling/head_train.py), against float64 autograd of the live oracle head
(tests/bn_live_model.py).  The inputs have no fragile location (checked on the CPU by tests/test_bn_live_model.py), so every
difference is rounding.  Every figure is printed (HEAD ...) before it is asserted."""
import functools

import pytest
import torch

import backward_model as M
import bn_live_model as L
import util

pytestmark = pytest.mark.gpu

F64 = torch.float64
BOTH, FIRST, SECOND = L.BOTH, L.FIRST, L.SECOND
# relative max error |g - ref|_max / |ref|_max per gradient tensor: 3x the largest value measured on the MI355X over the cases
# below; the frozen route's figure is 2.1e-5 (tests/test_head_backward_gpu.TOL = 6e-5)
TOL_GRAD = 2.2e-5           # measured 7.1e-6 (conv.1.weight, affine_no_inverse, f32 forward / f16x3 backward); f16x3 forward: 5.0e-6
# running_mean relative to max(|mean|, sqrt(var)) per channel, running_var to its own value, after one and two calls
TOL_RUNNING = 7e-7          # measured 2.3e-7 after two calls, 1.3e-7 after one
ROUTES = [(f, b, d) for f in ("f32", "f16x3") for b in ("f32", "f16x3") for d in (False, True)]


def ids(v):
    if isinstance(v, tuple):
        return "-".join("det" if x is True else "atomic" if x is False else str(x) for x in v) if isinstance(v[0], str) else \
            "live" + "".join(str(int(x)) for x in v)
    return str(v)


@functools.lru_cache(maxsize=None)
def reference(name, live):
    """The live oracle in float64, once per (case, live pattern)."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    P, inverse = L.HEAD_CASES[name][:2]
    state, fm, class_fms, (gl, gc, gd) = L.head_inputs(name)
    return L.live_oracle(fm, class_fms, state, inverse, live, gl, gc, gd)


def set_live(net, live):
    net.train()
    for bn, lv in zip((net.conv[1], net.conv[4]), live):
        bn.train(lv)
    return net


def make(device, name, live, route=("f32", "f32", False), requires=True):
    P, inverse = L.HEAD_CASES[name][:2]
    state, fm, class_fms, up = L.head_inputs(name)
    creator = util.make_head_creator(P, inverse, state, device)
    creator.train_forward_precision, creator.train_precision, creator.deterministic = route
    net = set_live(creator.aligner.parameter_regressor, live)
    fm_d = fm.to(device).requires_grad_(requires)
    raws = [c.to(device).requires_grad_(requires) for c in class_fms]
    return creator, net, creator.create_os2d_head(raws), fm_d, raws, up, state


def run(device, name, live, route=("f32", "f32", False)):
    creator, net, head, fm_d, raws, (gl, gc, gd), state = make(device, name, live, route)
    out = head(fm_d)
    loss = (out[0].double() * gl.to(device)).sum() + (out[1].double() * gc.to(device)).sum() + (out[2].double() * gd.to(device)).sum()
    loss.backward()
    named = dict(net.named_parameters())
    grads = {"fm": fm_d.grad.cpu(), "class": [r.grad.cpu() for r in raws]}
    grads.update({k: (None if named[k].grad is None else named[k].grad.cpu()) for k in L.PARAM_KEYS})
    return dict(out=[t.detach().cpu() for t in out], grads=grads, net=net, head=head, state=state)


def live_bias_keys(live):
    return [L.BN_KEYS[layer][0] + ".bias" for layer in (1, 2) if live[layer - 1]]


def grad_errors(got, ref, live):
    errs = {"fm": M.rel_err(got["fm"], ref["fm"])}
    for b, (g, r) in enumerate(zip(got["class"], ref["class"])):
        errs["class{}".format(b)] = M.rel_err(g, r)
    for k in L.PARAM_KEYS:
        if k not in live_bias_keys(live):
            assert got[k] is not None and got[k].shape == ref[k].shape, k
            errs[k] = M.rel_err(got[k], ref[k])
    return errs


GRAD_CASES = [(n, BOTH, r) for n in sorted(L.HEAD_CASES) for r in ROUTES] + \
             [(n, lv, r) for n in sorted(L.HEAD_CASES) for lv in L.GRAD_PATTERNS[n] if lv != BOTH
              for r in (("f32", "f32", False), ("f16x3", "f16x3", True))]


@pytest.mark.parametrize("name,live,route", GRAD_CASES, ids=ids)
def test_gradients_match_the_live_oracle(device, name, live, route):
    ref = reference(name, live)
    got = run(device, name, live, route)
    head = got["head"]
    assert head.last_live_batchnorm == live
    assert (head.last_train_forward_precision, head.last_precision, head.last_train_precision, head.last_deterministic) == \
        (route[0], route[0], route[1], route[2])
    errs = grad_errors(got["grads"], ref["grads"], live)
    worst = max(errs, key=errs.get)
    print("HEAD grad {:<20s} {} {:<22s} worst {:<14s} {:.3e}".format(name, ids(live), ids(route), worst, errs[worst]))
    # the bias of a convolution in front of a live BatchNorm: an exact zero tensor; the oracle's own value is rounding noise
    scale = sum(float(t.abs().sum()) for t in L.head_inputs(name)[3])
    for k in live_bias_keys(live):
        assert got["grads"][k] is not None and torch.count_nonzero(got["grads"][k]) == 0, k
        assert float(ref["grads"][k].abs().max()) < 1e-9 * scale, k
    bad = {k: v for k, v in errs.items() if not v < TOL_GRAD}
    assert not bad, bad


@pytest.mark.parametrize("live", [BOTH, FIRST, SECOND], ids=ids)
@pytest.mark.parametrize("name", sorted(L.HEAD_CASES))
def test_forward_outputs_match_the_live_oracle(device, name, live):
    ref = reference(name, live)["out"]
    got = run(device, name, live)["out"]
    util.assert_head_outputs_close(name, got[0], got[1], got[3], ref[0], ref[1], ref[3])
    util.assert_close(got[2], ref[2], util.TOL_CLS, 0.0, name + " cls_det")
    assert torch.equal(got[1], got[2])


def _running_errors(net, name, live, calls):
    """Errors of the updated buffers against the model: the batch statistics of the float64 oracle, applied ``calls`` times."""
    state = L.head_inputs(name)[0]
    stats = reference(name, live)["aux"]["stats"]
    worst = 0.0
    for layer, bn in ((1, net.conv[1]), (2, net.conv[4])):
        key = L.BN_KEYS[layer][1]
        rm, rv = state[key + ".running_mean"].to(F64), state[key + ".running_var"].to(F64)
        tracked = int(state[key + ".num_batches_tracked"])
        if live[layer - 1]:
            mean, var, n = stats[layer - 1]
            for _ in range(calls):
                rm, rv = L.running_update_model(rm, rv, mean, var, n, bn.momentum)
            tracked += calls
            e_m = float(((bn.running_mean.cpu().to(F64) - rm).abs() / torch.maximum(rm.abs(), rv.sqrt())).max())
            e_v = float(((bn.running_var.cpu().to(F64) - rv).abs() / rv).max())
            worst = max(worst, e_m, e_v)
        else:           # a frozen layer's buffers keep their bits
            assert torch.equal(bn.running_mean.cpu(), state[key + ".running_mean"]) and torch.equal(bn.running_var.cpu(), state[key + ".running_var"])
        assert int(bn.num_batches_tracked) == tracked, (layer, calls)
    return worst


@pytest.mark.parametrize("no_grad", [False, True], ids=["grad", "no_grad"])
@pytest.mark.parametrize("live", [BOTH, FIRST, SECOND], ids=ids)
@pytest.mark.parametrize("name", ["v2_affine_inverse", "v1_p4_no_inverse", "odd_c67_9x13"])
def test_running_statistics_follow_the_model(device, name, live, no_grad):
    creator, net, head, fm_d, raws, _, _ = make(device, name, live, requires=not no_grad)
    ref = reference(name, live)["out"]
    for calls in (1, 2):
        with torch.set_grad_enabled(not no_grad):
            out = head(fm_d)
        assert head.last_live_batchnorm == live
        assert out[1].requires_grad == (not no_grad)
        if no_grad:
            assert out[2] is out[1]
        err = _running_errors(net, name, live, calls)
        print("HEAD running {:<20s} {} {} call {}: {:.3e}".format(name, ids(live), "no_grad" if no_grad else "grad", calls, err))
        assert err < TOL_RUNNING
        # batch statistics do not depend on the running ones: both calls give the oracle's outputs
        util.assert_head_outputs_close(name, out[0].detach().cpu(), out[1].detach().cpu(), out[3].cpu(), ref[0], ref[1], ref[3])


def test_eval_after_live_steps_uses_the_updated_statistics(device):
    """Cache invalidation: inference before the live steps fills the packed-weight cache; after two live steps an eval-mode call
    must fold the UPDATED running statistics.  The synthetic net's default scales (linear.weight ~ N(0, 0.02)): in eval mode the
    transformation depends visibly on the folded statistics."""
    from oracle import head_oracle as O
    from os2d_amd.utils import synthetic
    name = "v2_affine_inverse"
    P, inverse = L.HEAD_CASES[name][:2]
    state = synthetic.make_transform_net_state(P, seed=3)
    _, fm, class_fms, _ = L.head_inputs(name)
    creator = util.make_head_creator(P, inverse, state, device)
    net = creator.aligner.parameter_regressor
    fm_d = fm.to(device)
    head = creator.create_os2d_head([c.to(device) for c in class_fms])
    with torch.no_grad():
        before = [t.clone() for t in head(fm_d, precision="f32")]
        set_live(net, BOTH)
        head(fm_d)
        head(fm_d)
        net.eval()
        after = head(fm_d, precision="f32")
    st64 = {k: v.to(F64) if v.is_floating_point() else v for k, v in state.items()}
    stats = []
    L.live_transform_net(O.correlation(O.prepare_class_maps([c.to(F64) for c in class_fms]), fm.to(F64)), st64, BOTH, stats=stats)
    updated = {k: v.clone() for k, v in state.items()}
    for layer in (1, 2):
        key = L.BN_KEYS[layer][1]
        rm, rv = st64[key + ".running_mean"], st64[key + ".running_var"]
        for _ in range(2):
            rm, rv = L.running_update_model(rm, rv, *stats[layer - 1], 0.1)
        updated[key + ".running_mean"], updated[key + ".running_var"] = rm.float(), rv.float()
    ref = O.head_forward(fm, O.prepare_class_maps(class_fms), updated, inverse)
    stale = O.head_forward(fm, O.prepare_class_maps(class_fms), state, inverse)
    assert float((ref[0] - stale[0]).abs().max()) > 100 * util.TOL_LOC                # the two sets of statistics are told apart
    util.assert_head_outputs_close(name, after[0].cpu(), after[1].cpu(), after[3].cpu(), ref[0], ref[1], ref[3])
    util.assert_head_outputs_close(name, before[0].cpu(), before[1].cpu(), before[3].cpu(), stale[0], stale[1], stale[3])


@pytest.mark.parametrize("route", [("f32", "f32", True), ("f16x3", "f16x3", True)], ids=ids)
def test_deterministic_runs_give_identical_bits(device, route):
    a = run(device, "v1_p4_no_inverse", BOTH, route)
    b = run(device, "v1_p4_no_inverse", BOTH, route)
    assert torch.equal(a["grads"]["fm"], b["grads"]["fm"])
    for x, y in zip(a["grads"]["class"], b["grads"]["class"]):
        assert torch.equal(x, y)
    for k in L.PARAM_KEYS:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    for bn_a, bn_b in zip((a["net"].conv[1], a["net"].conv[4]), (b["net"].conv[1], b["net"].conv[4])):
        assert torch.equal(bn_a.running_mean, bn_b.running_mean) and torch.equal(bn_a.running_var, bn_b.running_var)


def test_only_the_image_map_requires_grad(device):
    name = "v2_affine_inverse"
    creator, net, head, fm_d, raws, (gl, gc, gd), _ = make(device, name, BOTH, requires=False)
    net.requires_grad_(False)
    fm_d.requires_grad_(True)
    out = head(fm_d)
    ((out[0].double() * gl.to(device)).sum() + (out[1].double() * gc.to(device)).sum()).backward()
    assert all(p.grad is None for p in net.parameters())
    # the loss has no cls_det term: compare with the oracle for the same loss
    state, fm, class_fms, _ = L.head_inputs(name)
    ref = L.live_oracle(fm, class_fms, state, True, BOTH, gl, gc, torch.zeros_like(gd))["grads"]["fm"]
    assert M.rel_err(fm_d.grad.cpu(), ref) < TOL_GRAD


def test_only_a_batchnorm_weight_requires_grad(device):
    name = "v2_affine_inverse"
    creator, net, head, fm_d, raws, (gl, gc, gd), _ = make(device, name, BOTH, requires=False)
    net.requires_grad_(False)
    net.conv[1].weight.requires_grad_(True)
    out = head(fm_d)
    ((out[0].double() * gl.to(device)).sum() + (out[1].double() * gc.to(device)).sum() + (out[2].double() * gd.to(device)).sum()).backward()
    assert fm_d.grad is None and all(r.grad is None for r in raws)
    named = dict(net.named_parameters())
    assert all((named[k].grad is None) == (k != "conv.1.weight") for k in L.PARAM_KEYS)
    assert M.rel_err(named["conv.1.weight"].grad.cpu(), reference(name, BOTH)["grads"]["conv.1.weight"]) < TOL_GRAD


@pytest.mark.parametrize("forward", ["f32", "f16x3"])
def test_eval_mode_route_is_unchanged(device, forward):
    """Both BatchNorms in eval mode inside a net in training mode: the frozen route, bit for bit - the training forward equals
    the inference of the same arithmetic - and nothing is recorded as live or updated."""
    name = "v2_affine_inverse"
    creator, net, head, fm_d, raws, (gl, gc, gd), state = make(device, name, (False, False), route=(forward, "f32", True))
    with torch.no_grad():
        ref = head(fm_d, precision=forward)
    out = head(fm_d)
    assert head.last_live_batchnorm == (False, False)
    for i in (0, 1, 3):
        assert torch.equal(out[i].detach(), ref[i]), i
    (out[1].double() * gc.to(device)).sum().backward()
    g1 = fm_d.grad.clone()
    net.eval()                              # the parent's own state: every module in eval mode
    fm_d.grad = None
    out = head(fm_d)
    (out[1].double() * gc.to(device)).sum().backward()
    assert torch.equal(fm_d.grad, g1)
    for key, bn in (("conv.1", net.conv[1]), ("conv.4", net.conv[4])):
        assert torch.equal(bn.running_mean.cpu(), state[key + ".running_mean"]) and int(bn.num_batches_tracked) == 1


def test_inference_only_callers_keep_the_eval_mode_error(device):
    creator, net, head, fm_d, raws, _, _ = make(device, "v2_affine_inverse", BOTH, requires=False)
    A, B, H, W = fm_d.size(0), head.class_batch_size, fm_d.size(2), fm_d.size(3)
    out = tuple(torch.empty(A, B, k, H, W, device=device) for k in (4, 1, 8))
    with torch.no_grad():
        for call in (lambda: head(fm_d, out=out), lambda: net.packed("f32"), lambda: net.spectra(H, W),
                     lambda: net(torch.zeros(1, 225, H, W, device=device))):
            with pytest.raises(RuntimeError, match=r"call \.eval\(\)"):
                call()


def test_class_sharded_head_keeps_the_eval_mode_error(device, tmp_path):
    """os2d_amd/parallel.py hands the head its gather buffers (``out=``): each shard would see its own statistics."""
    import torch.distributed as dist
    from os2d_amd.parallel import ClassShardedHead
    if dist.is_initialized():
        pytest.skip("a process group is already initialised in this process")
    creator, net, head, fm_d, raws, _, _ = make(device, "v2_affine_inverse", BOTH, requires=False)
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        sharded = ClassShardedHead(creator, local_head=head, num_classes=head.class_batch_size)
        with torch.no_grad(), pytest.raises(RuntimeError, match=r"call \.eval\(\)"):
            sharded.forward(fm_d)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("setting", ["momentum", "track_running_stats"])
def test_unsupported_batchnorm_settings_raise(device, setting):
    creator, net, head, fm_d, raws, _, _ = make(device, "v2_affine_inverse", BOTH)
    if setting == "momentum":
        net.conv[4].momentum = None
    else:
        net.conv[1].track_running_stats = False
    with pytest.raises(ValueError, match=setting):
        head(fm_d)


def test_one_sgd_step_of_the_v1_configuration(device):
    """The reference's V1 recipe: simplified affine, no inverse model, the TransformNet's BatchNorms on batch statistics."""
    import numpy as np
    from test_objective_gpu import make_criterion
    from os2d_amd.engine.train import train_one_batch, get_trainable_parameters
    from os2d_amd.modeling.model import Os2dModel
    from os2d_amd.modeling.box_coder import Os2dBoxCoder
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    from os2d_amd.utils import synthetic
    net = Os2dModel(is_cuda=False, merge_branch_parameters=True, backbone_arch="resnet50", use_inverse_geom_model=False, simplify_affine=True)
    net.load_state_dict(synthetic.fill_model_state(net.state_dict(), seed=31, P=4))
    net.to(device)
    net.train(freeze_bn_in_extractor=True, freeze_bn_transform=False)
    tnet = net.os2d_head_creator.aligner.parameter_regressor
    assert tnet.live_batchnorm() == (True, True)
    A, B = 2, 3
    img_size = FeatureMapSize(w=192, h=160)
    images = synthetic.randn_tensor((A, 3, img_size.h, img_size.w), seed=41).to(device)
    class_images = [synthetic.randn_tensor((3, 64 + 16 * b, 80), seed=50 + b).to(device) for b in range(B)]
    coder = Os2dBoxCoder(0.5, 0.1, 0.8, 0.4, net.os2d_head_creator.box_grid_generator_image_level, net.get_feature_map_size)
    anchors = coder._get_default_boxes(img_size).bbox_xyxy
    batch_boxes = []
    for a in range(A):
        idx = torch.tensor([(7 * a + 5 * b + 3) % anchors.shape[0] for b in range(B)])
        bl = BoxList(anchors[idx].clone(), img_size)
        bl.add_field("labels", torch.arange(B))
        bl.add_field("difficult", torch.zeros(B, dtype=torch.bool))
        batch_boxes.append(bl)
    criterion = make_criterion("RLL", keep_class_loss_on_cpu=False)         # localization_weight 0.2: V1's loc_weight
    optimizer = torch.optim.SGD(get_trainable_parameters(net), lr=1e-2)
    before = {n: p.detach().clone() for n, p in tnet.named_parameters()}
    buffers = {n: b.detach().clone() for n, b in tnet.named_buffers()}
    losses = train_one_batch(net, criterion, optimizer, coder, images, class_images, batch_boxes, img_size, max_grad_norm=100.0)
    assert np.isfinite(float(losses["loss"].detach()))
    # the convolution biases in front of the live BatchNorms have an exactly zero gradient: every other tensor moves
    unchanged = [n for n, p in tnet.named_parameters() if torch.equal(p.detach(), before[n])]
    assert sorted(unchanged) == ["conv.0.bias", "conv.3.bias"], unchanged
    for n, b in tnet.named_buffers():
        assert not torch.equal(b, buffers[n]), n
