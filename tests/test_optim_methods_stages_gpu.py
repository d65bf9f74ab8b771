"""GPU: os2d_train_optim_prepare_ex / update_ex through DeviceAdagrad .. DeviceRprop against the float32 model of
tests/optim_methods_model.py: the norm, coef and the step-dependent factors to 1 float ulp (the double pow of the device and of
libm may differ in the last place), and - with the device's own coef and factors fed to the model - parameters, every state
tensor and the written-back gradients bit for bit.  The tensor set is that of test_optim_stages_gpu.py: one element, sizes around
one and two chunks, a 4-byte aligned view, a tensor without elements, 61 one-element tensors (a second table), a tensor without a
gradient, and two param groups, here with different hyperparameters (a third table).

Values: exact zeros in every gradient (Rprop's zero product, Adamax's u = eps, Adagrad's sqrt(0) + eps); signs planned per element
so that every Rprop branch runs on steps 2 and 3; Rprop learning rates 40 and 1.5e-6, which reach both step-size clamps; ASGD with
t0 = 2 and t0 = 0.  mu after step t is 1 / max(1, t - t0), so with t0 = 2 the averaging branch (mu != 1) first runs in step 5:
the trajectory has five steps, three clipped and two plain."""
import numpy as np
import pytest
import torch

import optim_methods_model as MM
from test_optim_stages_gpu import SHAPES, OFFSET_NUMEL, T, on_device, set_grads, host
from os2d_amd.engine import optimization as O

pytestmark = pytest.mark.gpu

F = np.float32
MAX_NORM = 60.0          # the norms of the three steps are about 42, 84, 126: the first is not clipped
N_STEPS = 3
GROUPS = {
    # (torch's Adagrad fills `sum` from its constructor's initial_accumulator_value, not from the group's: left at 0 here)
    "adagrad": [dict(lr=1e-2, weight_decay=1e-4, lr_decay=0.1, eps=1e-10), dict(lr=3e-3, weight_decay=0.0, lr_decay=0.0, eps=1e-8)],
    "adadelta": [dict(lr=1e-2, weight_decay=1e-4, rho=0.9, eps=1e-6), dict(lr=1.0, weight_decay=0.0, rho=0.95, eps=1e-5)],
    "adamax": [dict(lr=1e-2, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-3, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6)],
    "asgd": [dict(lr=1e-2, weight_decay=1e-4, lambd=1e-4, alpha=0.75, t0=2), dict(lr=3e-3, weight_decay=0.0, lambd=1e-2, alpha=0.5, t0=0)],
    "rmsprop": [dict(lr=1e-2, weight_decay=1e-4, alpha=0.99, eps=1e-8), dict(lr=3e-3, weight_decay=0.0, alpha=0.9, eps=1e-6)],
    "rprop": [dict(lr=40.0, etas=(0.5, 1.2), step_sizes=(1e-6, 50)), dict(lr=1.5e-6, etas=(0.4, 1.3), step_sizes=(1e-6, 10))],
}
# the sign of an element's gradient in steps 2 and 3, relative to its sign in step 1 (0: an exact zero)
PLAN_2 = np.array([1, -1, 1, -1, 0, 1], dtype=F)
PLAN_3 = np.array([1, 1, -1, 0, 1, -1, -1], dtype=F)


def make_inputs(seed=7):
    """-> (params [group][tensor] float32 arrays, grads [step][flat index] arrays or None, kinds [flat index]).  |g| >= 1e-3 or
    exactly 0: g * prev neither underflows nor sits at a rounding edge."""
    rng = np.random.RandomState(seed)
    params, kinds = [], []
    for shapes in SHAPES:
        group = []
        for s in shapes:
            n = OFFSET_NUMEL if s == "offset" else (7 if s == "none" else s)
            group.append(rng.standard_normal(n).astype(F))
            kinds.append(s if isinstance(s, str) else "plain")
        params.append(group)
    flat = [p for g in params for p in g]
    first = [np.where(rng.standard_normal(p.shape) < 0, -1, 1).astype(F) for p in flat]
    for s in first:
        s[::5] = 0.0                                                                   # exact zeros in step 1
    grads = []
    for t in range(N_STEPS):
        step = []
        for p, kind, s in zip(flat, kinds, first):
            if kind == "none":
                step.append(None)
                continue
            size = np.maximum(np.abs(0.3 * (t + 1) * rng.standard_normal(p.shape)), 1e-3).astype(F)
            e = np.arange(p.size)
            sign = s if t == 0 else np.where(s == 0, 1, s).astype(F) * (PLAN_2[e % 6] if t == 1 else PLAN_3[e % 7])
            step.append((size * sign).astype(F))
        grads.append(step)
    return params, grads, kinds


def make_optimizer(method, params, kinds, device):
    tensors, groups, k = [], [], 0
    for arrays, settings in zip(params, GROUPS[method]):
        ps = []
        for a in arrays:
            ps.append(on_device(a, kinds[k], device).requires_grad_())
            k += 1
        tensors += ps
        groups.append(dict(params=ps, **settings))
    return getattr(O, "Device" + MM.STOCK[method].__name__)(groups, lr=1.0), tensors


def make_model(method, params):
    flat = [p for g in params for p in g]
    per = [s for g, s in zip(params, GROUPS[method]) for _ in g]
    hyper = [{k: v for k, v in s.items() if k not in ("lr", "weight_decay")} for s in per]
    return MM.MethodModel(method, flat, [s["lr"] for s in per], [s.get("weight_decay", 0.0) for s in per], hyper)


def state_keys(method):
    return ("step",) + MM.STATE_KEYS[method] + (("eta", "mu") if method == "asgd" else ())


def snapshot(opt, tensors):
    """everything a step may write: parameters, gradients, state, step counts, eta and mu"""
    return dict(params=[host(p) for p in tensors], grads=[host(p.grad) for p in tensors],
                state=[{k: host(v) for k, v in opt.state.get(p, {}).items()} for p in tensors])


def device_step(opt, max_norm):
    """-> (norm, record [4], factors [live tensor][4])"""
    norm = opt.clip_and_step(max_norm) if max_norm is not None else (opt.step(), opt._last[0][0])[1]
    torch.cuda.synchronize()
    record, factors = opt._last
    assert norm.data_ptr() == record.data_ptr() and norm.shape == ()
    return host(norm), host(record), host(factors).reshape(-1, MM.FACTORS)


def check_against_model(method, opt, tensors, model, grads, kinds, max_norm):
    """One step on the device and in the model; returns the device's record."""
    before = snapshot(opt, tensors)
    norm, record, factors = device_step(opt, max_norm)
    model_norm = MM.grad_norm(grads)
    skip = bool(np.isnan(model_norm))
    assert record[0] == norm or (np.isnan(norm) and np.isnan(record[0]))
    assert record[2] == (1.0 if skip else 0.0) and record[3] == 0.0
    limit = float("inf") if max_norm is None else max_norm
    if np.isfinite(model_norm):
        print("\n[optim methods stages] {}: norm {!r} (model {!r}), coef {!r}".format(method, float(norm), float(model_norm), float(record[1])))
        assert MM.ulps(norm, model_norm) <= 1.0
        assert MM.ulps(record[1], MM.clip_coef(norm, limit)) <= 1.0                  # the model on the DEVICE's norm
    else:
        assert (np.isnan(norm) and np.isnan(model_norm)) or norm == model_norm
        expect = MM.clip_coef(model_norm, limit)
        assert (np.isnan(record[1]) and np.isnan(expect)) or record[1] == expect
    live = [i for i, g in enumerate(grads) if g is not None]
    assert factors.shape == (len(live), MM.FACTORS)
    use = None if skip else {i: factors[row] for row, i in enumerate(live)}
    _, _, model_skip, clipped, own = model.step(grads, limit, coef=record[1], factors=use)
    assert model_skip == skip
    if not skip:
        for row, i in enumerate(live):
            assert all(MM.ulps(factors[row, j], own[i][j]) <= 1.0 for j in range(MM.FACTORS)), (i, factors[row], own[i])
            if method == "asgd":         # the eta and mu of this step are exactly what the previous step left in the state
                was = before["state"][i]
                eta, mu = (was["eta"], was["mu"]) if was else MM.first_eta_mu(model.lr[i])
                assert MM.same_bits(factors[row, 1], eta) and MM.same_bits(factors[row, 2], mu), (i, factors[row], eta, mu)
    got = snapshot(opt, tensors)
    for i, kind in enumerate(kinds):
        assert MM.same_bits(got["params"][i], model.params[i]), ("param", i, kind)
        st = got["state"][i]
        if clipped[i] is None:           # no gradient: nothing but what Adagrad's constructor made
            assert got["grads"][i] is None and (st == {} or (method == "adagrad" and st["step"] == 0.0)), (i, st)
            continue
        assert MM.same_bits(got["grads"][i], clipped[i]), ("grad", i, kind)
        if model.steps[i] is None:
            continue
        assert sorted(st) == sorted(state_keys(method))
        assert st["step"].shape == () and st["step"] == F(model.steps[i]), ("step", i, kind)
        for key, want in zip(MM.STATE_KEYS[method], (model.state1[i], model.state2[i])):
            assert MM.same_bits(st[key], want), (key, i, kind)
        if method == "asgd":
            assert MM.ulps(st["eta"], model.eta_mu[i][0]) <= 1.0 and MM.ulps(st["mu"], model.eta_mu[i][1]) <= 1.0, (i, st["eta"], st["mu"])
    return record, factors


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


@pytest.mark.parametrize("method", MM.METHODS)
def test_factors_and_update_against_the_model(device, inputs, method):
    """Three clipped steps (state from one feeds the next), then two plain step()s (coef = 1) on the last gradients."""
    params, grads, kinds = inputs
    opt, tensors = make_optimizer(method, params, kinds, device)
    model = make_model(method, params)
    coefs, branches, averaged = [], [], set()
    for step in grads + [grads[-1], grads[-1]]:
        set_grads(tensors, step, kinds, device)
        record, factors = check_against_model(method, opt, tensors, model, step, kinds, MAX_NORM if len(coefs) < N_STEPS else None)
        coefs.append(record[1])
        if method == "rprop":
            branches.append({int(v) for s in model.products if s is not None for v in np.sign(s)})
        if method == "asgd":
            live = [i for i, g in enumerate(step) if g is not None]
            averaged |= {len(coefs) for row, i in enumerate(live) if factors[row, 2] != 1.0 and i < len(params[0])}
    assert coefs[0] == 1.0 and all(c < 1.0 for c in coefs[1:N_STEPS]) and coefs[N_STEPS:] == [1.0, 1.0]        # both sides of the clip
    assert len(opt._plan.tables) == 3 and opt._plan.tables[0][1] == T            # a full table, the group's rest, the second group
    marks = [rec.aligned for arr, n, _, _ in opt._plan.tables for rec in arr]
    live_kinds = [k for k in kinds if k != "none"]
    assert [m == 0 for m in marks] == [k == "offset" for k in live_kinds]          # only the view takes the 4-byte path
    if method == "rprop":
        assert branches[0] == {0} and branches[1] == {-1, 0, 1} and branches[2] == {-1, 0, 1}
        sizes = [model.state2[i] for i, k in enumerate(kinds) if k != "none"]
        split = len(params[0])
        assert max(s.max() for s in sizes[:split] if s.size) == F(50) and min(s.min() for s in sizes[split:] if s.size) == F(1e-6)
        assert max(s.max() for s in sizes[split:] if s.size) < F(10)
    if method == "asgd":
        assert averaged == {5}                                                     # t0 = 2: mu != 1 from the fifth step on
        assert all(f[2] != 1.0 for f in factors[len(params[0]):])                  # t0 = 0: from the third


@pytest.mark.parametrize("method", MM.METHODS)
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
    record, _ = check_against_model(method, opt, tensors, model, bad, kinds, MAX_NORM)
    assert np.isnan(record[0]) and np.isnan(record[1]) and record[2] == 1.0
    after = snapshot(opt, tensors)
    for i in range(len(tensors)):
        assert MM.same_bits(after["params"][i], before["params"][i])
        assert sorted(after["state"][i]) == sorted(before["state"][i])
        for k, v in after["state"][i].items():                                    # step, eta and mu among them
            assert MM.same_bits(v, before["state"][i][k]), (k, i)
        if after["grads"][i] is not None:
            assert np.isnan(after["grads"][i]).all()                              # clip_grad_norm_ leaves g * NaN
    # the next good step goes on from the untouched state
    set_grads(tensors, grads[2], kinds, device)
    check_against_model(method, opt, tensors, model, grads[2], kinds, MAX_NORM)


@pytest.mark.parametrize("method", MM.METHODS)
def test_an_infinite_gradient_does_not_skip(device, inputs, method):
    """An infinite norm gives coef = 0 and the step is taken: 0 * inf = NaN reaches that one element's parameter and state, as
    with clip_grad_norm_ + torch.optim."""
    params, grads, kinds = inputs
    opt, tensors = make_optimizer(method, params, kinds, device)
    model = make_model(method, params)
    bad = [None if g is None else g.copy() for g in grads[0]]
    bad[3][0] = np.inf
    set_grads(tensors, bad, kinds, device)
    record, _ = check_against_model(method, opt, tensors, model, bad, kinds, MAX_NORM)
    assert np.isinf(record[0]) and record[1] == 0.0 and record[2] == 0.0
    got = snapshot(opt, tensors)
    assert np.isnan(got["params"][3]).all() and np.isnan(got["grads"][3]).all()
    assert not any(np.isnan(p).any() for i, p in enumerate(got["params"]) if i != 3)
    assert all(st["step"] == 1.0 for st, k in zip(got["state"], kinds) if k != "none")


@pytest.mark.parametrize("method", MM.METHODS)
def test_two_runs_give_the_same_bits(device, inputs, method):
    params, grads, kinds = inputs
    runs = []
    for _ in range(2):
        opt, tensors = make_optimizer(method, params, kinds, device)
        records = []
        for step in grads:
            set_grads(tensors, step, kinds, device)
            _, record, factors = device_step(opt, MAX_NORM)
            records += [record, factors]
        runs.append((records, snapshot(opt, tensors)))
    (ra, a), (rb, b) = runs
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ra, rb))
    for i in range(len(kinds)):
        assert MM.same_bits(a["params"][i], b["params"][i])
        assert (a["grads"][i] is None and b["grads"][i] is None) or MM.same_bits(a["grads"][i], b["grads"][i])
        assert sorted(a["state"][i]) == sorted(b["state"][i])
        assert all(MM.same_bits(v, b["state"][i][k]) for k, v in a["state"][i].items())


def test_non_contiguous_and_non_fp32_parameters_raise(device):
    for p in (torch.zeros(4, 6, device=device).t().requires_grad_(), torch.zeros(8, dtype=torch.float64, device=device).requires_grad_()):
        p.grad = torch.zeros_like(p)
        for method in MM.METHODS:
            with pytest.raises(ValueError, match="contiguous float32"):
                getattr(O, "Device" + MM.STOCK[method].__name__)([p], lr=0.1).clip_and_step(1.0)
