"""CPU: the float32 model of the six other device optimiser steps (tests/optim_methods_model.py) against the stock torch.optim
classes in float64, the host side of DeviceAdagrad .. DeviceRprop (create_optimizer(on_device=True), state_dict layout,
checkpoints of the stock optimisers, refused options) and the argument checks of os2d_train_optim_prepare_ex / update_ex
(refused before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_methods_model as MM
from os2d_amd import _train_lib
from os2d_amd.engine import optimization as O

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEVICE_CLASS = dict(adagrad="DeviceAdagrad", adadelta="DeviceAdadelta", adamax="DeviceAdamax", asgd="DeviceASGD", rmsprop="DeviceRMSprop",
                    rprop="DeviceRprop")
METHOD_CODE = dict(adagrad=2, adadelta=3, adamax=4, asgd=5, rmsprop=6, rprop=7)
NHYPER = dict(adagrad=2, adadelta=2, adamax=3, asgd=3, rmsprop=2, rprop=4)


def device_class(method):
    return getattr(O, DEVICE_CLASS[method])


def _params():
    return [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3, 4))]


@pytest.mark.parametrize("method", MM.METHODS)
def test_model_tracks_torch_float64(method):
    """Eight steps with SETTINGS (steps 2 - 5 and 7 clip) from the same float32 inputs: the model stays within twice its measured
    error (optim_methods_model.MEASURED, relative to max(1, |p|)) of the stock class + clip_grad_norm_ in float64.  Rprop: the
    float64 run takes the model's branch in every element of every step."""
    params, grads = MM.methods_case(method)
    reference, _, branches = MM.torch_float64(method, params, grads)
    model = MM.make_model(method, params)
    clipped, worst = [], 0.0
    for t, g in enumerate(grads):
        norm, coef, skip, _, _ = model.step(g, MM.SETTINGS["max_norm"])
        clipped.append(bool(coef < 1))
        err = MM.relative_error(model.params, reference[t])
        worst = max(worst, err)
        print("\n[optim methods model] {} step {}: norm {:.4f} coef {:.6f} error {:.2f} * 2^-24".format(method, t + 1, float(norm), float(coef),
                                                                                                     err / MM.ULP))
        if method == "rprop":
            for i, s in enumerate(model.products):
                assert np.abs(g[i]).min() >= np.float32(MM.RPROP_FLOOR)
                assert np.array_equal(np.sign(s.astype(np.float64)), branches[t][i]), ("branch", t, i)
        assert not skip and err <= MM.TRAJECTORY_BOUND[method]
    print("\n[optim methods model] {}: largest error {:.2f} * 2^-24 (pinned: measured {:.2f}, bound {:.2f})".format(
        method, worst / MM.ULP, MM.MEASURED[method], MM.TRAJECTORY_BOUND[method] / MM.ULP))
    assert clipped == MM.CLIPPED and len(grads) == MM.STEPS >= 8


def test_model_guard_and_rprop_branches():
    """A NaN norm skips (no state, no count); an infinite one does not.  Rprop on three planned steps: agreement grows the step
    size, a flip shrinks it and drops the gradient, a zero leaves it; both clamps."""
    for method in MM.METHODS:
        model = MM.MethodModel(method, [np.ones(2, dtype=np.float32)], 0.1)
        _, _, skip, out, own = model.step([np.array([1.0, np.nan], dtype=np.float32)], 1.0)
        assert skip and own == {} and model.steps == [None] and np.isnan(out[0]).all() and np.array_equal(model.params[0], np.ones(2, dtype=np.float32))
        _, coef, skip, out, _ = model.step([np.array([1.0, np.inf], dtype=np.float32)], 1.0)
        assert not skip and coef == 0 and model.steps == [1] and out[0][0] == 0 and np.isnan(out[0][1]) and np.isnan(model.params[0][1])
    f = np.float32
    model = MM.MethodModel("rprop", [np.zeros(4, dtype=f)], 40.0)
    model.step([np.array([1, 1, 1, 0], dtype=f)], float("inf"))          # prev = 0: no change of the step size, p -= sign * 40
    assert np.array_equal(model.state2[0], np.full(4, 40, dtype=f)) and np.array_equal(model.params[0], np.array([-40, -40, -40, 0], dtype=f))
    model.step([np.array([1, -1, 0, 1], dtype=f)], float("inf"))         # agree (48), flip (20, gradient dropped), zero, zero product
    assert np.array_equal(model.state2[0], np.array([48, 20, 40, 40], dtype=f)) and np.array_equal(model.state1[0], np.array([1, 0, 0, 1], dtype=f))
    assert np.array_equal(model.params[0], np.array([-88, -40, -40, -40], dtype=f))
    model.step([np.array([1, -1, 0, 1], dtype=f)], float("inf"))         # 48 * 1.2 clamps at 50; after a dropped gradient no flip
    assert np.array_equal(model.state2[0], np.array([50, 20, 40, 48], dtype=f))
    model = MM.MethodModel("rprop", [np.zeros(1, dtype=f)], 1.5e-6)
    model.step([np.array([1], dtype=f)], float("inf"))
    model.step([np.array([-1], dtype=f)], float("inf"))                  # 0.75e-6 clamps at 1e-6
    assert model.state2[0][0] == f(1e-6)


def test_asgd_factors_follow_torch():
    """eta and mu of the model are torch's float32 `eta` / `mu` state, step for step, with an averaging start inside the run."""
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.ASGD([p], lr=0.05, lambd=1e-2, alpha=0.75, t0=2)
    h = dict(MM.HYPER["asgd"], lambd=1e-2, t0=2)
    eta_mu = MM.first_eta_mu(0.05)
    for t in range(1, 6):
        p.grad = torch.ones(3)
        f = MM.method_factors("asgd", 0.05, h, t, eta_mu)
        assert f[1] == eta_mu[0] and f[2] == eta_mu[1] and f[0] == np.float32(1.0 - 1e-2 * float(eta_mu[0]))
        opt.step()
        eta_mu = MM.next_eta_mu(0.05, h, t)
        assert MM.ulps(eta_mu[0], opt.state[p]["eta"].numpy()) <= 1.0 and eta_mu[1] == np.float32(float(opt.state[p]["mu"]))
    assert eta_mu[1] == np.float32(1.0 / 3.0)


# ---- create_optimizer and the torch.optim.Optimizer contract

def test_create_optimizer_on_device():
    import types
    for method in MM.METHODS:
        opt = O.create_optimizer(_params(), optim_method=method, lr=1e-2, weight_decay=1e-4, sgd_momentum=0.9, on_device=True)
        assert type(opt) is device_class(method) and isinstance(opt, MM.STOCK[method]) and hasattr(opt, "clip_and_step")
        assert opt.defaults["lr"] == 1e-2 and opt.defaults.get("weight_decay", 1e-4) == 1e-4
        cfg = types.SimpleNamespace(optim_method=method.upper(), lr=1e-2, weight_decay=1e-4, sgd_momentum=0.9, on_device=True)
        assert type(O.create_optimizer(_params(), cfg)) is device_class(method)                         # an attribute of cfg
        opt = O.create_optimizer(_params(), cfg, on_device=False)                                       # a keyword wins
        assert type(opt) is MM.STOCK[method] and not hasattr(opt, "clip_and_step")
        cfg.on_device = False
        assert type(O.create_optimizer(_params(), cfg)) is MM.STOCK[method]
        del cfg.on_device
        assert type(O.create_optimizer(_params(), cfg)) is MM.STOCK[method]                             # the default
    assert O.create_optimizer(_params(), optim_method="asgd", lr=1e-2, weight_decay=0.0, on_device=True).defaults["t0"] == 5000
    assert type(O.create_optimizer(_params(), optim_method="sgd", lr=1e-2, weight_decay=0.0, sgd_momentum=0.9, on_device=True)) is O.DeviceSGD
    assert type(O.create_optimizer(_params(), optim_method="adam", lr=1e-2, weight_decay=0.0, on_device=False)) is O.DeviceAdam
    with pytest.raises(TypeError, match="unknown settings"):
        O.create_optimizer(_params(), optim_method="rprop", lr=1e-2, device=True)


@pytest.mark.parametrize("method", MM.METHODS)
def test_refused_options_are_named(method):
    ps = _params()
    for p in ps:
        p.grad = torch.zeros_like(p)
    cls = device_class(method)
    with pytest.raises(ValueError, match="HIP device"):                  # CPU parameters: no fallback
        cls(ps, lr=0.1).clip_and_step(1.0)
    with pytest.raises(ValueError, match="positive"):
        cls(ps, lr=0.1).clip_and_step(0.0)
    options = ["maximize", "differentiable"] + (["momentum", "centered"] if method == "rmsprop" else [])
    for option in options:
        opt = cls(ps, lr=0.1)
        opt.param_groups[0][option] = 0.9 if option == "momentum" else True
        with pytest.raises(ValueError, match=option):
            opt.step()
    opt = cls(ps, lr=0.1)
    opt.param_groups[0]["lr"] = torch.tensor(0.1)
    with pytest.raises(ValueError, match="tensor learning rate"):
        opt.step()


@pytest.mark.parametrize("method", MM.METHODS)
def test_state_dict_layout_is_torchs(method):
    ps = _params()
    ours = device_class(method)(ps, lr=1e-2, **dict(MM.HYPER[method], **({} if method == "rprop" else {"weight_decay": 1e-4})))
    theirs = MM.make_stock(method, ps)
    a, b = ours.state_dict(), theirs.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"]
    assert len(a["param_groups"]) == len(b["param_groups"]) == 1
    assert list(a["param_groups"][0]) == list(b["param_groups"][0])                   # the same entries in the same order
    differing = {k for k in b["param_groups"][0] if a["param_groups"][0][k] != b["param_groups"][0][k]}
    assert differing == ({"capturable"} if method in MM.HAS_CAPTURABLE else set())
    assert sorted(ours.defaults) == sorted(theirs.defaults)
    assert sorted(a["state"]) == sorted(b["state"])                                   # Adagrad has state from its constructor on
    for k, st in b["state"].items():
        assert list(a["state"][k]) == list(st)
        assert a["state"][k]["step"].dtype == torch.float32 and a["state"][k]["step"].shape == ()


@pytest.mark.parametrize("method", MM.METHODS)
def test_a_state_dict_of_the_stock_cpu_optimiser_loads_and_goes_back(method):
    ps = _params()
    theirs = MM.make_stock(method, ps)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn_like(p)
        theirs.step()
    saved = theirs.state_dict()
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ours = O.create_optimizer(fresh, optim_method=method, lr=MM.SETTINGS["lr"], weight_decay=MM.SETTINGS["weight_decay"], on_device=True,
                              optimizer_state=saved)
    keys = ["step"] + list(MM.STATE_KEYS[method]) + (["eta", "mu"] if method == "asgd" else [])
    for p, q in zip(fresh, ps):
        st = ours.state[p]
        assert sorted(st) == sorted(keys) and list(st) == list(theirs.state[q])
        for k in keys:
            assert isinstance(st[k], torch.Tensor) and st[k].dtype == torch.float32 and st[k].is_contiguous()
            assert torch.equal(st[k], torch.as_tensor(theirs.state[q][k], dtype=torch.float32))
            assert st[k].data_ptr() != theirs.state[q][k].data_ptr()                  # a copy, not an alias
        assert st["step"].shape == () and float(st["step"]) == 3.0
        if method == "asgd":                                                          # one two-float tensor behind eta and mu
            assert st["eta"].shape == st["mu"].shape == () and st["mu"].data_ptr() == st["eta"].data_ptr() + 4
    if method in MM.HAS_CAPTURABLE:
        assert ours.param_groups[0]["capturable"] is True
    saved["state"][0]["step"] = 3                                       # a checkpoint of an old torch: a Python number
    if method == "asgd":
        saved["state"][0]["eta"], saved["state"][0]["mu"] = 0.01, 1
    ours.load_state_dict(saved)
    assert ours.state[fresh[0]]["step"].dtype == torch.float32 and float(ours.state[fresh[0]]["step"]) == 3.0
    again = ours.state_dict()                                           # and back into the stock optimiser
    back = MM.make_stock(method, [torch.nn.Parameter(p.detach().clone()) for p in ps])
    back.load_state_dict(again)
    for st, mine in zip(back.state.values(), ours.state.values()):
        assert sorted(st) == sorted(mine) and all(torch.equal(torch.as_tensor(st[k], dtype=torch.float32), mine[k]) for k in mine)


# ---- the C ABI

def test_constants_agree_with_the_header_and_the_binding():
    text = open(os.path.join(REPO, "include", "os2d_train.h")).read()

    def defined(name):
        return int(re.search(r"^#define OS2D_TRAIN_OPTIM_{} (\d+)\b".format(name), text, flags=re.M).group(1))
    for method, code in METHOD_CODE.items():
        assert defined(method.upper()) == code == getattr(_train_lib, "OPTIM_" + method.upper()) == device_class(method)._method
    assert defined("MAX_HYPER") == _train_lib.OPTIM_MAX_HYPER == 8 and max(NHYPER.values()) <= 8
    assert defined("FACTORS") == _train_lib.OPTIM_FACTORS == MM.FACTORS
    assert int(re.search(r"^#define OS2D_TRAIN_ABI_VERSION (\d+)$", text, flags=re.M).group(1)) == _train_lib.ABI_VERSION == 2
    assert ctypes.sizeof(_train_lib.OptimTensor) == 64
    lib = _train_lib.load()                                              # the library has both entry points (load() binds every signature)
    assert lib.os2d_train_optim_prepare_ex and lib.os2d_train_optim_update_ex
    ps = _params()
    for method in MM.METHODS:                                            # the classes hand over arrays of the length the library takes
        assert len(device_class(method)(ps, lr=0.1)._hyper(device_class(method)(ps, lr=0.1).param_groups[0])) == NHYPER[method]


def _table(n, numel=5, first=0, **fields):
    arr = (_train_lib.OptimTensor * max(n, 1))()
    for i in range(n):
        r = arr[i]
        r.param, r.grad, r.state1, r.state2, r.step = 256, 512, 768, 1024, 1280
        r.numel, r.lr, r.weight_decay, r.first_chunk, r.aligned = numel, 0.1, 0.0, first + i * O.chunks_of(numel), 1
        for k, v in fields.items():
            setattr(r, k, v)
    return arr


GOOD_HYPER = dict(adagrad=(0.0, 1e-10), adadelta=(0.9, 1e-6), adamax=(0.9, 0.999, 1e-8), asgd=(1e-4, 0.75, 5000.0), rmsprop=(0.99, 1e-8),
                  rprop=(0.5, 1.2, 1e-6, 50.0))


def test_bad_arguments_fail_before_launch():
    """No device is touched: the pointers are never dereferenced."""
    lib = _train_lib.load()
    fake = ctypes.c_void_p(256)
    err = lib.os2d_train_last_error
    T = O.MAX_TENSORS

    def doubles(values):
        return (ctypes.c_double * len(values))(*values)

    def calls(code, arr, n, hyper, nhyper=None, record=fake, factors=fake):
        h = None if hyper is None else doubles(hyper)
        nh = len(hyper) if nhyper is None else nhyper
        return [lib.os2d_train_optim_prepare_ex(code, arr, n, record, h, nh, factors, None),
                lib.os2d_train_optim_update_ex(code, arr, n, record, factors, h, nh, None)]

    for code in (-1, 0, 1, 8):                                           # SGD and Adam keep their own entry points
        assert calls(code, _table(1), 1, (0.9, 1e-8)) == [-1, -1] and b"method" in err()
    for method, code in METHOD_CODE.items():
        good = GOOD_HYPER[method]
        assert len(good) == NHYPER[method]
        assert calls(code, _table(1), 1, good + (0.0,)) == [-1, -1] and b"nhyper" in err()
        assert calls(code, _table(1), 1, good[:-1]) == [-1, -1] and b"nhyper" in err()
        assert calls(code, _table(1), 1, None, nhyper=len(good)) == [-1, -1] and b"null" in err()
        assert calls(code, _table(1), 1, (float("nan"),) * len(good)) == [-1, -1] and b"range" in err()
        # the table checks of the other entry points
        assert calls(code, _table(T + 1), T + 1, good) == [-1, -1] and b"tensors" in err()
        assert calls(code, _table(1), -1, good) == [-1, -1] and b"tensors" in err()
        assert calls(code, None, 2, good) == [-1, -1] and b"null" in err()
        assert calls(code, _table(2, numel=-3), 2, good) == [-1, -1] and b"negative numel" in err()
        for field in ("param", "grad"):
            assert calls(code, _table(2, **{field: None}), 2, good) == [-1, -1] and b"null" in err()
        assert calls(code, _table(1, param=260), 1, good) == [-1, -1] and b"aligned" in err()
        assert calls(code, _table(1, grad=513, aligned=0), 1, good) == [-1, -1] and b"4-byte" in err()
        arr = _table(2, numel=O.CHUNK + 1)
        arr[1].first_chunk = 1
        assert calls(code, arr, 2, good) == [-1, -1] and b"starts at chunk" in err()
        assert calls(code, _table(1), 1, good, record=None) == [-1, -1] and b"null" in err()
        assert calls(code, _table(1), 1, good, factors=None) == [-1, -1] and b"null" in err()
        # the state the method needs; only the entry point that refuses is called: the other one would launch on these addresses
        h = doubles(good)
        assert lib.os2d_train_optim_update_ex(code, _table(1, state1=None), 1, fake, fake, h, len(good), None) == -1 and b"null" in err()
        if method in ("adadelta", "adamax", "rprop"):
            assert lib.os2d_train_optim_update_ex(code, _table(1, state2=None), 1, fake, fake, h, len(good), None) == -1 and b"null" in err()
        if method == "asgd":                                             # prepare_ex reads and writes {eta, mu}
            assert lib.os2d_train_optim_prepare_ex(code, _table(1, state2=None), 1, fake, h, len(good), fake, None) == -1 and b"null" in err()
            assert lib.os2d_train_optim_prepare_ex(code, _table(2, numel=0, state2=None), 2, fake, h, len(good), fake, None) == -1 and b"state2" in err()
        assert lib.os2d_train_optim_prepare_ex(code, _table(1, step=None), 1, fake, h, len(good), fake, None) == -1 and b"null" in err()
        # a record without elements is counted too
        assert lib.os2d_train_optim_prepare_ex(code, _table(2, numel=0, step=None), 2, fake, h, len(good), fake, None) == -1 and b"step" in err()
        # nothing to do is not an error and launches nothing
        assert calls(code, _table(0), 0, good) == [0, 0]
        empty = _table(2, numel=0, param=None, grad=None, state1=None, state2=None)
        assert lib.os2d_train_optim_update_ex(code, empty, 2, fake, fake, doubles(good), len(good), None) == 0
    assert calls(7, _table(1), 1, (1.5, 1.2, 1e-6, 50.0)) == [-1, -1] and b"range" in err()             # etaminus >= 1
    assert calls(4, _table(1), 1, (1.0, 0.999, 1e-8)) == [-1, -1] and b"range" in err()                 # beta1 = 1
