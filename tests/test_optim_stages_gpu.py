"""GPU: the stages of the device optimiser step (os2d_amd/csrc_train/optim.hip through DeviceSGD / DeviceAdam) against the float32
model of tests/optim_model.py: the norm to 1 float ulp, coef and the per-tensor Adam factors to 1 float ulp, and - with the
device's own coef and factors fed to the model - parameters, state and the written-back gradients bit for bit.  The tensor set
covers one element, sizes around one and two chunks, a 4-byte aligned view, a tensor without elements, a second table, a tensor
without a gradient and two param groups."""
import numpy as np
import pytest
import torch

import optim_model as M
from os2d_amd.engine import optimization as O

pytestmark = pytest.mark.gpu

T = O.MAX_TENSORS
MAX_NORM = 60.0          # the norms of the three steps are about 42, 84, 126: the first is not clipped
MOMENTUM, BETAS, EPS = 0.9, (0.9, 0.999), 1e-8
GROUPS = [dict(lr=1e-2, weight_decay=1e-4), dict(lr=3e-3, weight_decay=0.0)]
# group 0: three sizes + T + 1 one-element tensors (the first table is full within this group); group 1: the rest, in the second
# table, where chunk numbers do not start at zero.  "offset": a view one float into its storage; "none": never gets a gradient
SHAPES = [[1, 3, 4095] + [1] * (T + 1), [4096, 4097, 8193, "offset", 0, "none"]]
OFFSET_NUMEL = 4101
N_STEPS = 3


def make_inputs(seed=5):
    """-> (params [group][tensor] float32 arrays, grads [step][flat index] arrays or None, kinds [flat index])"""
    rng = np.random.RandomState(seed)
    params, kinds = [], []
    for shapes in SHAPES:
        group = []
        for s in shapes:
            n = OFFSET_NUMEL if s == "offset" else (7 if s == "none" else s)
            group.append(rng.standard_normal(n).astype(np.float32))
            kinds.append(s if isinstance(s, str) else "plain")
        params.append(group)
    flat = [p for g in params for p in g]
    grads = []
    for t in range(N_STEPS):
        step = []
        for p, kind in zip(flat, kinds):
            if kind == "none":
                step.append(None)
                continue
            g = (0.3 * (t + 1) * rng.standard_normal(p.shape)).astype(np.float32)      # far from denormals: |g| < 2^-100 does not occur
            g[::5] = 0.0                                                               # exact zeros
            step.append(g)
        grads.append(step)
    return params, grads, kinds


def on_device(a, kind, device):
    """a float32 array as a device tensor; kind "offset": a view with storage offset 1 (4-byte aligned only)"""
    t = torch.from_numpy(a).to(device)
    if kind != "offset":
        return t
    base = torch.empty(a.size + 1, dtype=torch.float32, device=device)
    base[1:].copy_(t)
    view = base[1:]
    assert view.data_ptr() % 16 == 4
    return view


def make_optimizer(method, params, kinds, device):
    tensors, groups, k = [], [], 0
    for arrays, settings in zip(params, GROUPS):
        ps = []
        for a in arrays:
            ps.append(on_device(a, kinds[k], device).requires_grad_())
            k += 1
        tensors += ps
        groups.append(dict(params=ps, **settings))
    if method == "sgd":
        return O.DeviceSGD(groups, lr=1.0, momentum=MOMENTUM), tensors
    return O.DeviceAdam(groups, lr=1.0, betas=BETAS, eps=EPS), tensors


def make_model(method, params):
    flat = [p for g in params for p in g]
    lr = [s["lr"] for g, s in zip(params, GROUPS) for _ in g]
    wd = [s["weight_decay"] for g, s in zip(params, GROUPS) for _ in g]
    return M.ModelOptimizer(method, flat, lr, wd, momentum=MOMENTUM, betas=BETAS, eps=EPS)


def set_grads(tensors, grads, kinds, device):
    for p, g, kind in zip(tensors, grads, kinds):
        p.grad = None if g is None else on_device(g, kind, device)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def snapshot(opt, tensors):
    """everything a step may write: parameters, gradients, state, step counts"""
    keys = ("momentum_buffer", "exp_avg", "exp_avg_sq", "step")
    return dict(params=[host(p) for p in tensors], grads=[host(p.grad) for p in tensors],
                state=[{k: host(opt.state[p][k]) for k in keys if k in opt.state.get(p, {})} for p in tensors])


def device_step(opt, max_norm):
    """-> (norm, record [4], factors {live index: (step_size, sqrt_bc2)} or None)"""
    norm = opt.clip_and_step(max_norm) if max_norm is not None else (opt.step(), opt._last[0][0])[1]
    torch.cuda.synchronize()
    record, factors = opt._last
    assert norm.data_ptr() == record.data_ptr() and norm.shape == ()
    return host(norm), host(record), (None if factors is None else host(factors).reshape(-1, 2))


def check_against_model(method, opt, tensors, model, grads, kinds, max_norm):
    """One step on the device and in the model; returns the device's record."""
    norm, record, factors = device_step(opt, max_norm)
    model_norm = M.grad_norm(grads)
    skip = bool(np.isnan(model_norm))
    assert record[0] == norm or (np.isnan(norm) and np.isnan(record[0]))
    assert record[2] == (1.0 if skip else 0.0) and record[3] == 0.0
    limit = float("inf") if max_norm is None else max_norm
    if np.isfinite(model_norm):
        print("\n[optim stages] {}: norm {!r} (model {!r}), coef {!r}".format(method, float(norm), float(model_norm), float(record[1])))
        assert M.ulps(norm, model_norm) <= 1.0
        # the coefficient is one correctly rounded sum and quotient of the DEVICE's norm: the model on that norm, to 1 ulp
        assert M.ulps(record[1], M.clip_coef(norm, limit)) <= 1.0
    else:
        assert (np.isnan(norm) and np.isnan(model_norm)) or norm == model_norm
        expect = M.clip_coef(model_norm, limit)
        assert (np.isnan(record[1]) and np.isnan(expect)) or record[1] == expect
    live = [i for i, g in enumerate(grads) if g is not None]
    use = None
    if method == "adam" and not skip:
        assert factors.shape == (len(live), 2)
        use = {}
        for row, i in enumerate(live):
            t = (model.steps[i] or 0) + 1
            want = M.adam_factors(model.lr[i], BETAS, t)
            assert M.ulps(factors[row, 0], want[0]) <= 1.0 and M.ulps(factors[row, 1], want[1]) <= 1.0, (i, t, factors[row], want)
            use[i] = (factors[row, 0], factors[row, 1])
    _, _, model_skip, clipped = model.step(grads, limit, coef=record[1], factors=use)
    assert model_skip == skip
    got = snapshot(opt, tensors)
    for i, kind in enumerate(kinds):
        assert M.same_bits(got["params"][i], model.params[i]), ("param", i, kind)
        if clipped[i] is None:
            assert got["grads"][i] is None and got["state"][i] == {}
            continue
        assert M.same_bits(got["grads"][i], clipped[i]), ("grad", i, kind)
        st = got["state"][i]
        if method == "sgd":
            assert sorted(st) == ["momentum_buffer"] and M.same_bits(st["momentum_buffer"], model.state1[i]), ("momentum_buffer", i, kind)
        elif model.steps[i] is not None:
            assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"]
            assert st["step"].shape == () and st["step"] == np.float32(model.steps[i]), ("step", i, kind)
            assert M.same_bits(st["exp_avg"], model.state1[i]) and M.same_bits(st["exp_avg_sq"], model.state2[i]), ("exp_avg", i, kind)
    return record


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_norm_coef_factors_and_update_against_the_model(device, inputs, method):
    """Three clipped steps (state from one feeds the next), then one plain step() (coef = 1) on the last gradients."""
    params, grads, kinds = inputs
    opt, tensors = make_optimizer(method, params, kinds, device)
    model = make_model(method, params)
    coefs = []
    for step in grads:
        set_grads(tensors, step, kinds, device)
        coefs.append(check_against_model(method, opt, tensors, model, step, kinds, MAX_NORM)[1])
    assert coefs[0] == 1.0 and all(c < 1.0 for c in coefs[1:])                   # both sides of the clip
    set_grads(tensors, grads[-1], kinds, device)
    assert check_against_model(method, opt, tensors, model, grads[-1], kinds, None)[1] == 1.0
    assert len(opt._plan.tables) == 2 and opt._plan.tables[0][1] == T            # a full table and a second one
    marks = [rec.aligned for arr, n, _, _ in opt._plan.tables for rec in arr]
    live_kinds = [k for k in kinds if k != "none"]
    assert [m == 0 for m in marks] == [k == "offset" for k in live_kinds]          # only the view takes the 4-byte path


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_a_nan_gradient_skips_the_step(device, inputs, method):
    params, grads, kinds = inputs
    opt, tensors = make_optimizer(method, params, kinds, device)
    model = make_model(method, params)
    set_grads(tensors, grads[0], kinds, device)
    check_against_model(method, opt, tensors, model, grads[0], kinds, MAX_NORM)   # state and counts exist
    before = snapshot(opt, tensors)
    bad = [None if g is None else g.copy() for g in grads[1]]
    bad[kinds.index("offset")][4100] = np.nan                                     # one element, in a chunk's scalar tail
    set_grads(tensors, bad, kinds, device)
    record = check_against_model(method, opt, tensors, model, bad, kinds, MAX_NORM)
    assert np.isnan(record[0]) and np.isnan(record[1]) and record[2] == 1.0
    after = snapshot(opt, tensors)
    for i in range(len(tensors)):
        assert M.same_bits(after["params"][i], before["params"][i])
        assert sorted(after["state"][i]) == sorted(before["state"][i])
        for k, v in after["state"][i].items():
            assert M.same_bits(v, before["state"][i][k]), (k, i)
        if after["grads"][i] is not None:
            assert np.isnan(after["grads"][i]).all()                              # clip_grad_norm_ leaves g * NaN
    # the next good step goes on from the untouched state
    set_grads(tensors, grads[2], kinds, device)
    check_against_model(method, opt, tensors, model, grads[2], kinds, MAX_NORM)


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_an_infinite_gradient_does_not_skip(device, inputs, method):
    """The reference checks math.isnan only: an infinite norm gives coef = 0, the step is taken (0 * inf = NaN reaches that
    one element's parameter, as with clip_grad_norm_ + torch.optim)."""
    params, grads, kinds = inputs
    opt, tensors = make_optimizer(method, params, kinds, device)
    model = make_model(method, params)
    bad = [None if g is None else g.copy() for g in grads[0]]
    bad[3][0] = np.inf
    set_grads(tensors, bad, kinds, device)
    record = check_against_model(method, opt, tensors, model, bad, kinds, MAX_NORM)
    assert np.isinf(record[0]) and record[1] == 0.0 and record[2] == 0.0
    got = snapshot(opt, tensors)
    assert np.isnan(got["params"][3]).all() and np.isnan(got["grads"][3]).all()
    assert not any(np.isnan(p).any() for i, p in enumerate(got["params"]) if i != 3)
    if method == "adam":
        assert all(st["step"] == 1.0 for st, k in zip(got["state"], kinds) if k != "none")


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_two_runs_give_the_same_bits(device, inputs, method):
    params, grads, kinds = inputs
    runs = []
    for _ in range(2):
        opt, tensors = make_optimizer(method, params, kinds, device)
        records = []
        for step in grads:
            set_grads(tensors, step, kinds, device)
            records.append(device_step(opt, MAX_NORM)[1])
        runs.append((records, snapshot(opt, tensors)))
    (ra, a), (rb, b) = runs
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ra, rb))
    for i in range(len(kinds)):
        assert M.same_bits(a["params"][i], b["params"][i])
        assert (a["grads"][i] is None and b["grads"][i] is None) or M.same_bits(a["grads"][i], b["grads"][i])
        assert sorted(a["state"][i]) == sorted(b["state"][i])
        assert all(M.same_bits(v, b["state"][i][k]) for k, v in a["state"][i].items())


def test_non_contiguous_and_non_fp32_parameters_raise(device):
    for p in (torch.zeros(4, 6, device=device).t().requires_grad_(), torch.zeros(8, dtype=torch.float64, device=device).requires_grad_()):
        p.grad = torch.zeros_like(p)
        for opt in (O.DeviceSGD([p], lr=0.1), O.DeviceAdam([p], lr=0.1)):
            with pytest.raises(ValueError, match="contiguous float32"):
                opt.clip_and_step(1.0)
