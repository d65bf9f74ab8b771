"""GPU: DeviceSGD / DeviceAdam end to end - a five-step trajectory against torch in float64, checkpoints into a fresh device
optimiser and into the stock torch optimiser, no host synchronisation in clip_and_step, and train_one_batch with the device
step against the same step with torch.optim.SGD.  Bounds: tests/optim_model.py (16 * 2^-24 of max(1, |p|) over five steps, a
fifth of it for one step: the error accumulates linearly per step)."""
import copy

import numpy as np
import pytest
import torch

import optim_model as M
from os2d_amd.engine import optimization as O

pytestmark = pytest.mark.gpu
S = M.SETTINGS


def make_device(method, params, device, state=None):
    ps = [torch.from_numpy(np.array(p, dtype=np.float32)).to(device).requires_grad_() for p in params]
    opt = O.create_optimizer(ps, optim_method=method, lr=S["lr"], weight_decay=S["weight_decay"], sgd_momentum=S["momentum"],
                             optimizer_state=state)
    return opt, ps


def set_grads(ps, grads, device):
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g).to(device=device, dtype=p.dtype)


def host(ps):
    return [p.detach().cpu().numpy() for p in ps]


@pytest.fixture(scope="module")
def case():
    params, grads = M.trajectory_case()
    return params, grads, {m: M.torch_float64(m, params, grads)[0] for m in ("sgd", "adam")}


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_trajectory_against_torch_float64(device, case, method):
    params, grads, reference = case
    opt, ps = make_device(method, params, device)
    assert type(opt) is (O.DeviceSGD if method == "sgd" else O.DeviceAdam)
    for t, g in enumerate(grads):
        set_grads(ps, g, device)
        norm = opt.clip_and_step(S["max_norm"])
        err = M.relative_error(host(ps), reference[method][t])
        print("\n[optim] {} step {}: norm {:.4f} error {:.2f} * 2^-24".format(method, t + 1, float(norm), err / M.ULP))
        assert err <= M.TRAJECTORY_BOUND
        assert M.ulps(float(norm), M.grad_norm(g)) <= 1.0


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_checkpoint_into_a_fresh_device_optimiser_and_into_torch(device, case, method):
    """Two steps, state_dict(), then step three three ways: the optimiser itself, a fresh device optimiser and the stock torch
    optimiser (float32, on the device) that loaded the state.  The device pair agrees bit for bit, torch within one step's bound."""
    params, grads, _ = case
    opt, ps = make_device(method, params, device)
    for g in grads[:2]:
        set_grads(ps, g, device)
        opt.clip_and_step(S["max_norm"])
    saved, now = copy.deepcopy(opt.state_dict()), host(ps)             # as a checkpoint that went through a file
    fresh, fresh_ps = make_device(method, now, device, state=copy.deepcopy(saved))
    stock_ps = [torch.from_numpy(p.copy()).to(device).requires_grad_() for p in now]
    stock = M.make_torch(method, stock_ps)
    stock.load_state_dict(saved)
    for o, tensors in ((opt, ps), (fresh, fresh_ps)):
        set_grads(tensors, grads[2], device)
        o.clip_and_step(S["max_norm"])
    set_grads(stock_ps, grads[2], device)
    torch.nn.utils.clip_grad_norm_(stock_ps, S["max_norm"])
    stock.step()
    ours, again, theirs = host(ps), host(fresh_ps), host(stock_ps)
    assert all(M.same_bits(a, b) for a, b in zip(ours, again))
    for a, b in zip(opt.state.values(), fresh.state.values()):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    err = M.relative_error(ours, theirs)
    print("\n[optim] {} checkpoint: device step against torch's from the same state: {:.2f} * 2^-24".format(method, err / M.ULP))
    assert err <= M.STEP_BOUND
    if method == "adam":
        assert all(float(st["step"]) == 3.0 and st["step"].is_cuda for st in fresh.state.values())


def sync_mode_is_effective(probe):
    """Does torch.cuda.set_sync_debug_mode("error") raise on a device-to-host read on this build?"""
    torch.cuda.set_sync_debug_mode("error")
    try:
        float(probe.detach().sum())
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_clip_and_step_does_not_synchronise(device, case, method):
    params, grads, _ = case
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


def test_train_one_batch_with_the_device_step(device):
    """train_one_batch on the shape tests/test_objective_gpu.py trains, from the same state with DeviceSGD and with torch.optim.SGD:
    equal losses, parameters within one step's bound; then a step whose gradient carries a NaN leaves every parameter as it is."""
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
    settings = dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)

    def run(optimizer):
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
        losses = train_one_batch(net, criterion, optimizer, coder, images, class_images, batch_boxes, img_size, max_grad_norm=100.0)
        return losses, [p.detach().cpu().numpy() for p in params]

    # The backbone is torch's own and its convolutions do not give the same bits on every call from the same state (measured:
    # the feature maps of repeated forwards differ, the loss in its last bit), whatever the optimiser: the comparison needs
    # torch's deterministic convolution algorithms.  The first run is not compared: it is where the algorithms are chosen.
    flags = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        run(torch.optim.SGD(params, **settings))
        stock_losses, stock = run(torch.optim.SGD(params, **settings))
        optimizer = O.DeviceSGD(params, **settings)
        losses, ours = run(optimizer)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags
    assert isinstance(losses["grad_norm"], torch.Tensor) and losses["grad_norm"].is_cuda and losses["grad_norm"].shape == ()
    loss, stock_loss = float(losses["loss"].detach()), float(stock_losses["loss"].detach())
    print("\n[optim] train_one_batch: loss {!r} with the device step, {!r} with torch's".format(loss, stock_loss))
    assert loss == stock_loss and np.isfinite(loss)
    err = M.relative_error(ours, stock)
    moved = sum(not np.array_equal(a, s.cpu().numpy()) for a, s in zip(ours, start))
    print("\n[optim] train_one_batch: loss {:.6f}, grad norm {:.4f} (torch {:.4f}), {} of {} tensors moved, device step against torch's: "
          "{:.2f} * 2^-24".format(loss, float(losses["grad_norm"]), float(stock_losses["grad_norm"]), moved, len(params),
                                  err / M.ULP))
    assert err <= M.STEP_BOUND and moved > 0
    # a NaN in one parameter's gradient: the step is skipped on the device
    hook = params[len(params) // 2].register_hook(lambda g: torch.full_like(g, float("nan")))
    try:
        losses = train_one_batch(net, criterion, optimizer, coder, images, class_images, batch_boxes, img_size, max_grad_norm=100.0)
    finally:
        hook.remove()
    assert np.isnan(float(losses["grad_norm"]))
    assert all(np.array_equal(p.detach().cpu().numpy(), a) for p, a in zip(params, ours))
