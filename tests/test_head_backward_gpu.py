"""GPU: autograd through the HIP head (os2d_amd/modeling/head_train.py + libos2d_train.so) against torch autograd of the CPU
oracle (oracle.head_forward, the operator-level twin of the reference), with leaf tensors for the image feature maps, the raw
class maps (through oracle.prepare_class_maps) and every TransformNet tensor.

The recognition output the reference detaches from the transformation (head.py:396-402: ``cls_det`` is resampled on a grid
computed from detached parameters) is restated here from the oracle's own stages with the grid detached."""
import pytest
import torch
import torch.nn.functional as F

import util

pytestmark = pytest.mark.gpu

PARAM_KEYS = ["conv.0.weight", "conv.0.bias", "conv.1.weight", "conv.1.bias", "conv.3.weight", "conv.3.bias", "conv.4.weight",
              "conv.4.bias", "linear.weight", "linear.bias"]

# relative max error |g - ref|_max / |ref|_max per gradient tensor: about 3x the largest value measured on the MI355X over the
# small cases below (2.1e-5, V2)
TOL = 6e-5
# The training shape resamples 2 x 15 x 38 x 38 x 121 points: a few of them sit within one rounding of a cell edge of the bilinear
# interpolation (or of a clamp), where the derivative jumps, and the two implementations round the coordinate differently.  Such a
# point moves the gradient of its pair's class and of the TransformNet as a whole.  Measured on the MI355X: the 9 classes without
# such a point agree to 2.5e-6; the 6 with one, the image map and the TransformNet to 0.4 - 3.5e-3 (max and norm-wise alike).
TOL_TRAIN_MAX = 1e-2
TOL_TRAIN_NORM = 5e-3


def _cls_detached(fm, q_hat, state, inverse):
    """cls_det of the reference: the pooled resampling of the correlation on a grid built from DETACHED parameters."""
    from oracle import head_oracle as O
    A, C, H, W = fm.shape
    B = q_hat.size(0)
    T = O.TEMPLATE
    corr = O.correlation(q_hat, fm)
    params = O.transform_net(corr, state).detach()
    theta = O.params_to_theta(params, inverse)
    grids = F.affine_grid(theta, [theta.size(0), 1, T, T], align_corners=True).view(A, B, H, W, T, T, 2)
    boxes_fm = O.anchor_grid(H, W, float(T), 1.0).view(1, 1, H, W, 4)
    g_fm = O.local_to_global(grids, boxes_fm)
    g_unit = torch.stack([g_fm[..., 0] / (W - 1) * 2 - 1, g_fm[..., 1] / (H - 1) * 2 - 1], dim=-1).clamp(-1, 1)
    return O.resample_and_pool(corr.view(A, B, T * T, H, W), g_unit, O.pool_mask())


def oracle_grads(fm, class_fms, state, inverse, gl, gc, gd, stride=16, rec_field=16):
    """torch autograd on the CPU: {'fm', 'class', <state key>} gradients of sum(gl*loc + gc*cls + gd*cls_det)."""
    from oracle import head_oracle as O
    fm = fm.clone().requires_grad_(True)
    raws = [c.clone().requires_grad_(True) for c in class_fms]
    st = {k: (v.clone().requires_grad_(True) if k in PARAM_KEYS else v.clone()) for k, v in state.items()}
    q_hat = O.prepare_class_maps(raws)
    loc, cls, _, _ = O.head_forward(fm, q_hat, st, inverse, stride=stride, rec_field=rec_field)
    cls_det = _cls_detached(fm, q_hat, st, inverse)
    loss = (loc.double() * gl).sum() + (cls.double() * gc).sum() + (cls_det.double() * gd).sum()
    leaves = [fm] + raws + [st[k] for k in PARAM_KEYS]
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    out = {"fm": gs[0], "class": list(gs[1:1 + len(raws)])}
    out.update({k: g for k, g in zip(PARAM_KEYS, gs[1 + len(raws):])})
    return out


def hip_grads(device, fm, class_fms, state, P, inverse, gl, gc, gd, freeze=False):
    creator = util.make_head_creator(P, inverse, state, device)
    net = creator.aligner.parameter_regressor
    if freeze:
        net.requires_grad_(False)
    fm_d = fm.to(device).requires_grad_(True)
    raws = [c.to(device).requires_grad_(True) for c in class_fms]
    head = creator.create_os2d_head(raws)
    loc, cls, cls_det, corners = head(fm_d)
    assert cls_det is not cls and not corners.requires_grad
    loss = (loc.double() * gl.to(device)).sum() + (cls.double() * gc.to(device)).sum() + (cls_det.double() * gd.to(device)).sum()
    loss.backward()
    named = dict(net.named_parameters())
    out = {"fm": fm_d.grad.cpu(), "class": [r.grad.cpu() for r in raws]}
    out.update({k: (named[k].grad.cpu() if named[k].grad is not None else None) for k in PARAM_KEYS})
    return out, (loc, cls, cls_det, corners), creator


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def rel_norm_err(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def upstream(A, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(A, B, 4, H, W, generator=g, dtype=torch.float64), torch.randn(A, B, 1, H, W, generator=g, dtype=torch.float64),
            torch.randn(A, B, 1, H, W, generator=g, dtype=torch.float64))


CASES = {
    # name: (P, inverse, A, C, H, W, class sizes, B)
    "v2_affine_inverse": (6, True, 2, 64, 10, 12, [(15, 15), (12, 18)], 3),
    "affine_no_inverse": (6, False, 2, 64, 10, 12, [(15, 15), (12, 18)], 3),
    "simple_affine_p4": (4, True, 2, 64, 10, 12, [(15, 15), (12, 18)], 3),
    "odd_c67_9x13": (6, True, 2, 67, 9, 13, [(15, 15), (12, 18), (17, 13)], 3),
}


def _check_case(device, name, P, inverse, A, C, H, W, sizes, B, seed=0, tol=TOL, tol_norm=None):
    from os2d_amd.utils import synthetic
    state = synthetic.make_transform_net_state(P, seed=seed + 3)
    fm = synthetic.make_feature_map(C, H, W, seed=seed + 5, A=A)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=sizes, seed=seed + 400)
    gl, gc, gd = upstream(A, B, H, W, seed + 7)
    ref = oracle_grads(fm, class_fms, state, inverse, gl, gc, gd)
    got, _, _ = hip_grads(device, fm, class_fms, state, P, inverse, gl, gc, gd)
    pairs = {"fm": (got["fm"], ref["fm"])}
    for b in range(B):
        assert got["class"][b].shape == class_fms[b].shape
        pairs["class{}".format(b)] = (got["class"][b], ref["class"][b])
    for k in PARAM_KEYS:
        assert got[k] is not None and got[k].shape == ref[k].shape, k
        pairs[k] = (got[k], ref[k])
    errs = {k: rel_err(*v) for k, v in pairs.items()}
    print(name, "relative max errors:", {k: "{:.2e}".format(v) for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, bad
    if tol_norm is not None:
        nerrs = {k: rel_norm_err(*v) for k, v in pairs.items()}
        print(name, "relative norm errors:", {k: "{:.2e}".format(v) for k, v in nerrs.items()})
        bad = {k: v for k, v in nerrs.items() if not v < tol_norm}
        assert not bad, bad
    return errs


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_match_oracle(device, name):
    _check_case(device, name, *CASES[name])


def test_gradients_match_oracle_training_shape(device):
    """Reference training crops: 2 images x 15 classes x 1024 channels x 38 x 38 maps."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    errs = _check_case(device, "training_shape", 6, True, 2, 1024, 38, 38, [(15, 15), (20, 24), (13, 17)], 15, seed=11,
                       tol=TOL_TRAIN_MAX, tol_norm=TOL_TRAIN_NORM)
    # the bulk agrees at the small cases' level: most classes meet none of those points
    assert sum(errs["class{}".format(b)] < TOL for b in range(15)) >= 8


def _small(device, P=6, inverse=True, seed=0):
    from os2d_amd.utils import synthetic
    A, C, H, W, B = 2, 64, 10, 12, 3
    state = synthetic.make_transform_net_state(P, seed=seed + 3)
    fm = synthetic.make_feature_map(C, H, W, seed=seed + 5, A=A)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=[(15, 15), (12, 18)], seed=seed + 400)
    return state, fm, class_fms, upstream(A, B, H, W, seed + 7)


def test_training_forward_equals_f32_inference(device):
    state, fm, class_fms, _ = _small(device)
    creator = util.make_head_creator(6, True, state, device)
    head = creator.create_os2d_head([c.to(device) for c in class_fms])
    fm_d = fm.to(device)
    with torch.no_grad():
        ref = head(fm_d, precision="f32")
    out = head(fm_d.clone().requires_grad_(True))
    assert out[0].requires_grad and out[1].requires_grad and out[2].requires_grad
    for i in (0, 1, 3):
        assert torch.equal(out[i].detach(), ref[i]), i
    assert torch.equal(out[2].detach(), ref[1])


def test_cls_det_gradient_does_not_reach_the_transformation(device):
    state, fm, class_fms, (gl, gc, gd) = _small(device)
    zero = torch.zeros_like(gl), torch.zeros_like(gc)
    got, _, _ = hip_grads(device, fm, class_fms, state, 6, True, zero[0], zero[1], gd)
    for k in PARAM_KEYS:
        assert got[k] is not None and torch.count_nonzero(got[k]) == 0, k
    assert float(got["fm"].abs().max()) > 0
    ref = oracle_grads(fm, class_fms, state, True, zero[0], zero[1], gd)
    assert rel_err(got["fm"], ref["fm"]) < TOL


def test_frozen_transform_params_give_no_parameter_gradients(device):
    state, fm, class_fms, (gl, gc, gd) = _small(device)
    full, _, _ = hip_grads(device, fm, class_fms, state, 6, True, gl, gc, gd)
    frozen, _, _ = hip_grads(device, fm, class_fms, state, 6, True, gl, gc, gd, freeze=True)
    for k in PARAM_KEYS:
        assert frozen[k] is None, k
    # the data gradients are the same (up to the order of the resampler's atomic additions)
    assert rel_err(frozen["fm"], full["fm"]) < 1e-5
    for a, b in zip(frozen["class"], full["class"]):
        assert rel_err(a, b) < 1e-5


def test_wide_map_under_grad_raises(device):
    state, _, class_fms, _ = _small(device)
    creator = util.make_head_creator(6, True, state, device)
    head = creator.create_os2d_head([c.to(device) for c in class_fms])
    fm = torch.rand(1, 64, 4, 210, device=device, requires_grad=True)
    with pytest.raises(RuntimeError, match="209"):
        head(fm)


def test_no_grad_path_unchanged(device):
    state, fm, class_fms, _ = _small(device)
    creator = util.make_head_creator(6, True, state, device)
    raws = [c.to(device).requires_grad_(True) for c in class_fms]
    head = creator.create_os2d_head(raws)
    fm_d = fm.to(device)
    with torch.no_grad():
        a = head(fm_d)
        b = head(fm_d.clone().requires_grad_(True))
    assert a[2] is a[1] and b[2] is b[1] and not b[1].requires_grad
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_one_sgd_step_matches_oracle(device):
    """One SGD step on the HIP path moves every TransformNet parameter where one step on the oracle moves it."""
    state, fm, class_fms, (gl, gc, gd) = _small(device, seed=21)
    lr = 0.05
    got, _, creator = hip_grads(device, fm, class_fms, state, 6, True, gl, gc, gd)
    net = creator.aligner.parameter_regressor
    torch.optim.SGD(net.parameters(), lr=lr).step()
    ref = oracle_grads(fm, class_fms, state, True, gl, gc, gd)
    named = dict(net.named_parameters())
    for k in PARAM_KEYS:
        want = state[k] - lr * ref[k]
        moved = named[k].detach().cpu()
        assert float((moved - want).abs().max()) <= lr * TOL * float(ref[k].abs().max()) + 1e-7, k
