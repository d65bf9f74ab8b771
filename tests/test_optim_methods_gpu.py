"""GPU: DeviceAdagrad .. DeviceRprop end to end through create_optimizer(on_device=True) - the eight-step trajectory of
tests/optim_methods_model.py against the stock torch.optim class in float64 within the bound pinned there (twice the model's
measured error), checkpoints into a fresh device optimiser and into the stock class, no host synchronisation in clip_and_step,
and one train_one_batch with the device RMSprop step."""
import copy

import numpy as np
import pytest
import torch

import optim_methods_model as MM
from test_optim_gpu import set_grads, host, sync_mode_is_effective
from os2d_amd.engine import optimization as O

pytestmark = pytest.mark.gpu
S = MM.SETTINGS
SPLIT = 4                # the checkpoint is taken after this many steps


def make_device(method, params, device, state=None):
    ps = [torch.from_numpy(np.array(p, dtype=np.float32)).to(device).requires_grad_() for p in params]
    opt = O.create_optimizer(ps, optim_method=method, lr=S["lr"], weight_decay=S["weight_decay"], on_device=True, optimizer_state=state)
    assert type(opt).__name__ == "Device" + MM.STOCK[method].__name__ and isinstance(opt, MM.STOCK[method])
    return opt, ps


@pytest.fixture(scope="module")
def case():
    """method -> (params, grads, the float64 parameters after each step); computed once, never written"""
    out = {}
    for method in MM.METHODS:
        params, grads = MM.methods_case(method)
        out[method] = (params, grads, MM.torch_float64(method, params, grads)[0])
    return out


@pytest.mark.parametrize("method", MM.METHODS)
def test_trajectory_against_torch_float64(device, case, method):
    params, grads, reference = case[method]
    opt, ps = make_device(method, params, device)
    for t, g in enumerate(grads):
        set_grads(ps, g, device)
        norm = opt.clip_and_step(S["max_norm"])
        err = MM.relative_error(host(ps), reference[t])
        print("\n[optim methods] {} step {}: norm {:.4f} error {:.2f} * 2^-24 (bound {:.2f})".format(
            method, t + 1, float(norm), err / MM.ULP, MM.TRAJECTORY_BOUND[method] / MM.ULP))
        assert err <= MM.TRAJECTORY_BOUND[method]
        assert MM.ulps(float(norm), MM.grad_norm(g)) <= 1.0


@pytest.mark.parametrize("method", MM.METHODS)
def test_checkpoint_into_a_fresh_device_optimiser_and_into_torch(device, case, method):
    """SPLIT steps, state_dict(), then the rest of the trajectory three ways: the optimiser itself, a fresh device optimiser that
    loaded the state, and the stock class in float64 on the CPU that loaded it (`capturable` switched off, as a CPU optimiser
    needs it).  The device pair agrees bit for bit; the stock continuation stays within the trajectory's bound."""
    params, grads, _ = case[method]
    opt, ps = make_device(method, params, device)
    for g in grads[:SPLIT]:
        set_grads(ps, g, device)
        opt.clip_and_step(S["max_norm"])
    saved, now = copy.deepcopy(opt.state_dict()), host(ps)             # as a checkpoint that went through a file
    fresh, fresh_ps = make_device(method, now, device, state=copy.deepcopy(saved))
    for a, b in zip(opt.state.values(), fresh.state.values()):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) and a[k].data_ptr() != b[k].data_ptr() for k in a)
    for_stock = copy.deepcopy(saved)
    for group in for_stock["param_groups"]:
        if "capturable" in group:
            group["capturable"] = False
    stock_after, stock, _ = MM.torch_float64(method, now, grads[SPLIT:], state_dict=for_stock)
    assert all(float(st["step"]) == float(len(grads)) for st in stock.state.values())
    for t, g in enumerate(grads[SPLIT:]):
        for o, tensors in ((opt, ps), (fresh, fresh_ps)):
            set_grads(tensors, g, device)
            o.clip_and_step(S["max_norm"])
        ours, again = host(ps), host(fresh_ps)
        assert all(MM.same_bits(a, b) for a, b in zip(ours, again))
        err = MM.relative_error(ours, stock_after[t])
        print("\n[optim methods] {} checkpoint, step {}: against torch's float64 from the same state: {:.2f} * 2^-24".format(
            method, SPLIT + t + 1, err / MM.ULP))
        assert err <= MM.TRAJECTORY_BOUND[method]
    for a, b in zip(opt.state.values(), fresh.state.values()):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(float(st["step"]) == float(len(grads)) and st["step"].is_cuda for st in fresh.state.values())


@pytest.mark.parametrize("method", MM.METHODS)
def test_clip_and_step_does_not_synchronise(device, case, method):
    params, grads, _ = case[method]
    opt, ps = make_device(method, params, device)
    set_grads(ps, grads[0], device)
    opt.clip_and_step(S["max_norm"])                    # warm-up: library loading, state allocation, first launches
    set_grads(ps, grads[1], device)
    torch.cuda.synchronize()
    if not sync_mode_is_effective(ps[0]):
        pytest.skip("torch.cuda.set_sync_debug_mode has no effect on this torch-ROCm build")
    torch.cuda.set_sync_debug_mode("error")
    try:
        norm = opt.clip_and_step(S["max_norm"])
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert norm.is_cuda and norm.shape == () and np.isfinite(float(norm))


def test_train_one_batch_with_the_device_rmsprop_step(device):
    """train_one_batch on the shape tests/test_optim_gpu.py trains, from the same state with
    create_optimizer(optim_method="rmsprop", on_device=True) and with torch.optim.RMSprop: equal losses.  The parameters are
    compared with torch.optim.RMSprop in float64 on the clipped gradients the step left in p.grad, within one step's share of the
    trajectory's bound (the error grows linearly with the steps).  The float32 torch step on the device is not the yardstick: it
    rounds each parameter once more on its own, so the two float32 results may differ in a parameter's last bit, 2 x 2^-24 of it;
    that difference is printed.  The norm is a device scalar; a NaN gradient leaves every parameter and count as it is."""
    import objective_cases as OC
    from os2d_amd.engine.objective import Os2dObjective
    from os2d_amd.engine.train import train_one_batch, get_trainable_parameters
    from os2d_amd.modeling.model import Os2dModel
    from os2d_amd.modeling.box_coder import Os2dBoxCoder
    from os2d_amd.structures.bounding_box import BoxList
    from os2d_amd.structures.feature_map import FeatureMapSize
    from os2d_amd.utils import synthetic
    net = Os2dModel(is_cuda=False, merge_branch_parameters=True, backbone_arch="resnet50", use_inverse_geom_model=True, simplify_affine=False)
    net.load_state_dict(synthetic.fill_model_state(net.state_dict(), seed=31, P=6))
    net.to(device)
    net.train(freeze_bn_in_extractor=True, freeze_bn_transform=True)
    net.os2d_head_creator.deterministic = True           # the head's backward gives the same bits in both runs
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
    criterion = Os2dObjective("RLL", **dict(OC.CRITERION, keep_class_loss_on_cpu=False))
    params = get_trainable_parameters(net)
    start = [p.detach().clone() for p in params]
    settings = dict(lr=1e-4, weight_decay=1e-4)

    def run(optimizer):
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
        losses = train_one_batch(net, criterion, optimizer, coder, images, class_images, batch_boxes, img_size, max_grad_norm=100.0)
        return losses, [p.detach().cpu().numpy() for p in params]

    def float64_step(clipped):
        ps = [torch.nn.Parameter(s.detach().cpu().double()) for s in start]
        for p, g in zip(ps, clipped):
            p.grad = None if g is None else g.detach().cpu().double()
        torch.optim.RMSprop(ps, **settings).step()
        return [p.detach().numpy() for p in ps]

    # torch's deterministic convolution algorithms, and an uncompared first run in which they are chosen: see test_optim_gpu.py
    flags = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        run(torch.optim.RMSprop(params, **settings))
        stock_losses, stock = run(torch.optim.RMSprop(params, **settings))
        optimizer = O.create_optimizer(params, optim_method="rmsprop", on_device=True, **settings)
        assert type(optimizer) is O.DeviceRMSprop
        losses, ours = run(optimizer)
        reference = float64_step([p.grad for p in params])
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    assert isinstance(losses["grad_norm"], torch.Tensor) and losses["grad_norm"].is_cuda and losses["grad_norm"].shape == ()
    loss, stock_loss = float(losses["loss"].detach()), float(stock_losses["loss"].detach())
    assert loss == stock_loss and np.isfinite(loss)
    err, err32 = MM.relative_error(ours, reference), MM.relative_error(ours, stock)
    moved = sum(not np.array_equal(a, s.cpu().numpy()) for a, s in zip(ours, start))
    print("\n[optim methods] train_one_batch: loss {:.6f}, grad norm {:.4f} (torch {:.4f}), {} of {} tensors moved, device step against "
          "torch's in float64: {:.2f} * 2^-24, against torch's float32 step: {:.2f} * 2^-24".format(
              loss, float(losses["grad_norm"]), float(stock_losses["grad_norm"]), moved, len(params), err / MM.ULP, err32 / MM.ULP))
    assert err <= MM.TRAJECTORY_BOUND["rmsprop"] / MM.STEPS and moved > 0
    assert all(float(st["step"]) == 1.0 for st in optimizer.state.values())
    # a NaN in one parameter's gradient: the step is skipped on the device
    hook = params[len(params) // 2].register_hook(lambda g: torch.full_like(g, float("nan")))
    try:
        losses = train_one_batch(net, criterion, optimizer, coder, images, class_images, batch_boxes, img_size, max_grad_norm=100.0)
    finally:
        hook.remove()
    assert np.isnan(float(losses["grad_norm"]))
    assert all(np.array_equal(p.detach().cpu().numpy(), a) for p, a in zip(params, ours))
    assert all(float(st["step"]) == 1.0 for st in optimizer.state.values())
