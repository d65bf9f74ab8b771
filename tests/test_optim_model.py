"""CPU: the float32 model of the device optimiser step (tests/optim_model.py) against torch in float64, the host logic of
os2d_amd/engine/optimization.py (launch plan, create_optimizer, state_dict layout, checkpoints of the stock optimisers,
learning-rate annealing) and the argument checks of os2d_train_optim_* (refused before any launch)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import optim_model as M
from os2d_amd import _train_lib
from os2d_amd.engine import optimization as O

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T, CHUNK = O.MAX_TENSORS, O.CHUNK


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_model_tracks_torch_float64(method):
    """Five steps with SETTINGS (steps 2 - 5 clip) from the same float32 inputs: the model stays within 16 * 2^-24 of
    max(1, |p|) of torch.optim + clip_grad_norm_ in float64 (measured <= 3.8 * 2^-24; the error grows linearly per step)."""
    params, grads = M.trajectory_case()
    reference, _ = M.torch_float64(method, params, grads)
    model = M.make_model(method, params)
    clipped = []
    for t, g in enumerate(grads):
        norm, coef, skip, _ = model.step(g, M.SETTINGS["max_norm"])
        clipped.append(bool(coef < 1))
        err = M.relative_error(model.params, reference[t])
        print("\n[optim model] {} step {}: norm {:.4f} coef {:.6f} error {:.2f} * 2^-24".format(method, t + 1, float(norm), float(coef), err / M.ULP))
        assert not skip and err <= M.TRAJECTORY_BOUND
    assert clipped == [False, True, True, True, True]


def test_model_norm_coef_and_guard():
    g = [np.array([3.0, 4.0], dtype=np.float32), None, np.zeros(0, dtype=np.float32)]
    assert M.grad_norm(g) == np.float32(5.0)
    assert M.clip_coef(np.float32(5.0), 10.0) == np.float32(1.0) and M.clip_coef(np.float32(5.0), float("inf")) == np.float32(1.0)
    assert M.clip_coef(np.float32(5.0), 2.5) == np.float32(2.5) / (np.float32(5.0) + np.float32(1e-6))
    assert np.isnan(M.clip_coef(np.float32("nan"), 2.5)) and M.clip_coef(np.float32("inf"), 2.5) == 0
    model = M.ModelOptimizer("adam", [np.ones(2, dtype=np.float32)], 0.1, 0.0)
    _, _, skip, out = model.step([np.array([1.0, np.nan], dtype=np.float32)], 1.0)
    assert skip and model.steps == [None] and np.isnan(out[0]).all() and np.array_equal(model.params[0], np.ones(2, dtype=np.float32))
    _, coef, skip, out = model.step([np.array([1.0, np.inf], dtype=np.float32)], 1.0)
    assert not skip and coef == 0 and model.steps == [1] and out[0][0] == 0 and np.isnan(out[0][1])


# ---- the launch plan

def test_constants_agree_with_the_header_and_the_library():
    text = open(os.path.join(REPO, "include", "os2d_train.h")).read()
    assert int(re.search(r"^#define OS2D_TRAIN_OPTIM_MAX_TENSORS (\d+)$", text, flags=re.M).group(1)) == T == _train_lib.OPTIM_MAX_TENSORS
    assert int(re.search(r"^#define OS2D_TRAIN_OPTIM_CHUNK (\d+)$", text, flags=re.M).group(1)) == CHUNK == _train_lib.OPTIM_CHUNK
    assert ctypes.sizeof(_train_lib.OptimTensor) == 64 and T * 64 + 128 <= 4096          # the table travels in the kernel arguments
    lib = _train_lib.load()
    assert lib.os2d_train_optim_max_tensors() == T
    for n in (-5, 0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 2 ** 33 + 1):
        assert lib.os2d_train_optim_chunks(n) == O.chunks_of(n)


def test_plan_chunks_and_prefixes():
    numels = [1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 0, 64 * 25]
    tables, total = O.plan_tables(numels)
    assert len(tables) == 1 and [r[0] for r in tables[0]] == list(range(len(numels)))
    assert [r[2] for r in tables[0]] == [1, 1, 1, 1, 2, 3, 0, 1] and total == 10
    assert [r[1] for r in tables[0]] == [0, 1, 2, 3, 4, 6, 9, 9]          # a tensor without elements shares its successor's first chunk
    assert O.plan_tables([], None) == ([], 0)
    assert O.plan_tables([0, 0]) == ([[(0, 0, 0), (1, 0, 0)]], 0)
    with pytest.raises(ValueError):
        O.plan_tables([4, -1])


def test_plan_splits_tables():
    tables, total = O.plan_tables([1] * T)
    assert [len(t) for t in tables] == [T] and total == T
    tables, total = O.plan_tables([1] * (T + 1))
    assert [len(t) for t in tables] == [T, 1] and tables[1] == [(T, T, 1)] and total == T + 1
    tables, total = O.plan_tables([CHUNK + 1] * (2 * T + 3))
    assert [len(t) for t in tables] == [T, T, 3] and tables[2][0] == (2 * T, 4 * T, 2) and total == 4 * T + 6
    # tensors of one launch share its hyperparameters: a new key starts a new table, chunk numbers run on
    tables, total = O.plan_tables([1, CHUNK + 1, 1, 1], keys=["a", "a", "b", "b"])
    assert tables == [[(0, 0, 1), (1, 1, 2)], [(2, 3, 1), (3, 4, 1)]] and total == 5
    assert O.plan_tables([1, 1, 1], max_tensors=2)[0] == [[(0, 0, 1), (1, 1, 1)], [(2, 2, 1)]]


def test_alignment_mark():
    assert O.pointers_aligned(256, 1024, None, None) == 1 and O.pointers_aligned(256, 1024, 512, 4096) == 1
    assert O.pointers_aligned(260, 1024, None, None) == 0 and O.pointers_aligned(256, 1024, 512, 4104) == 0
    base = torch.zeros(9)
    assert O.pointers_aligned(base.data_ptr()) == 1 and O.pointers_aligned(base[1:].data_ptr()) == 0


# ---- create_optimizer and the torch.optim.Optimizer contract

def _params():
    return [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3, 4))]


def test_create_optimizer_classes():
    cfg = types.SimpleNamespace(optim_method="SGD", lr=1e-2, weight_decay=1e-4, sgd_momentum=0.9)
    opt = O.create_optimizer(_params(), cfg)
    assert type(opt) is O.DeviceSGD and isinstance(opt, torch.optim.Optimizer) and hasattr(opt, "clip_and_step")
    assert opt.defaults["momentum"] == 0.9 and opt.defaults["weight_decay"] == 1e-4 and O.get_learning_rate(opt) == 1e-2
    opt = O.create_optimizer(_params(), optim_method="adam", lr=1e-3, weight_decay=0.0, sgd_momentum=0.9)
    assert type(opt) is O.DeviceAdam and hasattr(opt, "clip_and_step")
    opt = O.create_optimizer(_params(), cfg, optim_method="adam")                      # a keyword wins over cfg
    assert type(opt) is O.DeviceAdam and opt.defaults["lr"] == 1e-2
    stock = {"adagrad": torch.optim.Adagrad, "adadelta": torch.optim.Adadelta, "adamax": torch.optim.Adamax, "asgd": torch.optim.ASGD,
             "rmsprop": torch.optim.RMSprop, "rprop": torch.optim.Rprop}
    for name, cls in stock.items():
        opt = O.create_optimizer(_params(), optim_method=name, lr=1e-2, weight_decay=1e-4, sgd_momentum=0.9)
        assert type(opt) is cls and not hasattr(opt, "clip_and_step")
    with pytest.raises(RuntimeError, match="Invalid optim method"):
        O.create_optimizer(_params(), optim_method="lbfgs", lr=1e-2, weight_decay=0.0, sgd_momentum=0.0)
    with pytest.raises(TypeError):
        O.create_optimizer(_params(), optim_method="sgd", lr=1e-2)
    O.set_learning_rate(opt, 0.5)
    assert O.get_learning_rate(opt) == 0.5


def test_device_optimisers_refuse_what_the_kernels_do_not_do():
    ps = _params()                                                      # CPU parameters with gradients: no fallback
    for p in ps:
        p.grad = torch.zeros_like(p)
    for opt in (O.DeviceSGD(ps, lr=0.1), O.DeviceAdam(ps, lr=0.1)):
        with pytest.raises(ValueError, match="HIP device"):
            opt.clip_and_step(1.0)
        with pytest.raises(ValueError, match="positive"):
            opt.clip_and_step(0.0)
    opt = O.DeviceSGD(ps, lr=0.1, momentum=0.9)
    opt.param_groups[0]["nesterov"] = True
    with pytest.raises(ValueError, match="Nesterov"):
        opt.step()
    opt = O.DeviceAdam(ps, lr=0.1)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_state_dict_layout_is_torchs(method):
    ps = _params()
    ours = O.DeviceSGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-4) if method == "sgd" else O.DeviceAdam(ps, lr=1e-2, weight_decay=1e-4)
    theirs = M.make_torch(method, ps)
    a, b = ours.state_dict(), theirs.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"]
    assert len(a["param_groups"]) == len(b["param_groups"]) == 1
    assert list(a["param_groups"][0]) == list(b["param_groups"][0])                   # the same entries in the same order
    differing = {k for k in b["param_groups"][0] if a["param_groups"][0][k] != b["param_groups"][0][k]}
    assert differing == (set() if method == "sgd" else {"capturable"})
    assert sorted(ours.defaults) == sorted(theirs.defaults)


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_a_state_dict_of_the_stock_cpu_optimiser_loads(method):
    ps = _params()
    theirs = M.make_torch(method, ps)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn_like(p)
        theirs.step()
    saved = theirs.state_dict()
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ours = O.create_optimizer(fresh, optim_method=method, lr=M.SETTINGS["lr"], weight_decay=M.SETTINGS["weight_decay"],
                              sgd_momentum=M.SETTINGS["momentum"], optimizer_state=saved)
    keys = ["momentum_buffer"] if method == "sgd" else ["step", "exp_avg", "exp_avg_sq"]
    for p, q in zip(fresh, ps):
        st = ours.state[p]
        assert sorted(st) == sorted(keys)
        for k in keys:
            assert isinstance(st[k], torch.Tensor) and st[k].dtype == torch.float32 and st[k].is_contiguous()
            assert torch.equal(st[k], torch.as_tensor(theirs.state[q][k], dtype=torch.float32))
        if method == "adam":
            assert st["step"].shape == () and float(st["step"]) == 3.0
    if method == "adam":
        assert ours.param_groups[0]["capturable"] is True
        saved["state"][0]["step"] = 3                                   # a checkpoint of an old torch: a Python int
        ours.load_state_dict(saved)
        assert ours.state[fresh[0]]["step"].dtype == torch.float32 and float(ours.state[fresh[0]]["step"]) == 3.0
    again = ours.state_dict()                                           # and back into the stock optimiser
    M.make_torch(method, [torch.nn.Parameter(p.detach().clone()) for p in ps]).load_state_dict(again)


def test_setup_lr():
    def optimizer():
        return O.DeviceSGD(_params(), lr=1.0, momentum=0.9)
    opt = optimizer()
    scheduler, anneal = O.setup_lr(opt, {}, types.SimpleNamespace(type="none"), eval_iter=10)
    assert scheduler is None and anneal(0) == 1.0 and anneal(10, anneal_now=False) == 1.0

    opt = optimizer()
    cfg = types.SimpleNamespace(type="MultiStepLR", milestones=[15, 30], gamma=0.1)           # in iterations: evaluations 2 and 3
    scheduler, anneal = O.setup_lr(opt, {}, cfg, eval_iter=10)
    opt._opt_called = True
    rates = [anneal(i) for i in range(4)]
    assert isinstance(scheduler, torch.optim.lr_scheduler.MultiStepLR)
    assert rates == pytest.approx([1.0, 0.1, 0.01, 0.01]) and O.get_learning_rate(opt) == pytest.approx(0.01)

    opt = optimizer()
    log = {"loss": []}
    cfg = types.SimpleNamespace(type="ReduceLROnPlateau", reduce_factor=0.5, min_value=0.2, quantity_epsilon=1e-3, quantity_mode="min",
                                patience=10, cooldown=0, quantity_to_monitor="loss", quantity_smoothness=30)
    scheduler, anneal = O.setup_lr(opt, log, cfg, eval_iter=10)
    assert isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau)
    rates = []
    for value in [5.0, 4.0, 100.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0]:                   # the outlier never reaches the scheduler: median of 3
        log["loss"].append(value)
        rates.append(anneal(len(log["loss"])))
    assert rates[:5] == [1.0] * 5 and rates[-1] == 0.2 and 0.5 in rates
    assert scheduler.best == 3.0
    with pytest.raises(RuntimeError, match="Unknown"):
        O.setup_lr(optimizer(), {}, types.SimpleNamespace(type="cosine"), eval_iter=10)


# ---- the C ABI refuses bad arguments before it launches anything (no device is touched: the pointers are never dereferenced)

def _table(n, numel=5, first=0, **fields):
    arr = (_train_lib.OptimTensor * max(n, 1))()
    for i in range(n):
        r = arr[i]
        r.param, r.grad, r.state1, r.state2, r.step = 256, 512, 768, 1024, 1280
        r.numel, r.lr, r.weight_decay, r.first_chunk, r.aligned = numel, 0.1, 0.0, first + i * O.chunks_of(numel), 1
        for k, v in fields.items():
            setattr(r, k, v)
    return arr


def test_bad_arguments_fail_before_launch():
    lib = _train_lib.load()
    fake = ctypes.c_void_p(256)
    err = lib.os2d_train_last_error

    def calls(arr, n):
        """every table entry point on the same table"""
        return [lib.os2d_train_optim_sumsq(arr, n, fake, 10 ** 6, None),
                lib.os2d_train_optim_prepare(arr, n, fake, 0.9, 0.999, fake, None),
                lib.os2d_train_optim_update(_train_lib.OPTIM_SGD, arr, n, fake, None, 0.9, 0.0, 0.0, None),
                lib.os2d_train_optim_update(_train_lib.OPTIM_ADAM, arr, n, fake, fake, 0.9, 0.999, 1e-8, None)]

    assert calls(_table(T + 1), T + 1) == [-1] * 4 and b"tensors" in err()                    # a count above T
    assert calls(_table(1), -1) == [-1] * 4 and b"tensors" in err()                           # and below 0
    assert calls(None, 2) == [-1] * 4 and b"null" in err()
    assert calls(_table(2, numel=-3), 2) == [-1] * 4 and b"negative numel" in err()
    for field in ("param", "grad"):
        assert calls(_table(2, **{field: None}), 2) == [-1] * 4 and b"null" in err()
    assert lib.os2d_train_optim_update(_train_lib.OPTIM_SGD, _table(1, state1=None), 1, fake, None, 0.9, 0.0, 0.0, None) == -1 and b"null" in err()
    assert lib.os2d_train_optim_update(_train_lib.OPTIM_ADAM, _table(1, state2=None), 1, fake, fake, 0.9, 0.999, 1e-8, None) == -1 and b"null" in err()
    assert lib.os2d_train_optim_update(_train_lib.OPTIM_ADAM, _table(1), 1, fake, None, 0.9, 0.999, 1e-8, None) == -1 and b"null" in err()
    assert lib.os2d_train_optim_update(_train_lib.OPTIM_ADAM, _table(1), 1, None, fake, 0.9, 0.999, 1e-8, None) == -1 and b"null" in err()
    assert lib.os2d_train_optim_update(2, _table(1), 1, fake, fake, 0.9, 0.999, 1e-8, None) == -1 and b"method" in err()
    assert lib.os2d_train_optim_update(_train_lib.OPTIM_ADAM, _table(1), 1, fake, fake, 1.0, 0.999, 1e-8, None) == -1 and b"betas" in err()
    assert lib.os2d_train_optim_prepare(_table(1, step=None), 1, fake, 0.9, 0.999, fake, None) == -1 and b"null" in err()
    assert lib.os2d_train_optim_prepare(_table(1), 1, fake, 0.9, 0.999, None, None) == -1 and b"null" in err()
    assert lib.os2d_train_optim_sumsq(_table(1), 1, None, 10, None) == -1 and b"null" in err()
    assert calls(_table(1, param=260), 1) == [-1] * 4 and b"aligned" in err()                 # marked 16-byte aligned and is not
    assert calls(_table(1, grad=513, aligned=0), 1) == [-1] * 4 and b"4-byte" in err()
    arr = _table(2, numel=CHUNK + 1)
    arr[1].first_chunk = 1                                                                     # overlaps its predecessor's two chunks
    assert calls(arr, 2) == [-1] * 4 and b"starts at chunk" in err()
    # a partials buffer that is too small: -2
    arr = _table(3, numel=CHUNK + 1, first=4)                                                  # chunks 4 .. 9
    assert lib.os2d_train_optim_sumsq(arr, 3, fake, 9, None) == -2 and b"partials" in err()
    # max_norm
    for bad in (0.0, -1.0, float("nan")):
        assert lib.os2d_train_optim_finalize(fake, 4, bad, fake, None) == -1 and b"max_norm" in err()
    assert lib.os2d_train_optim_finalize(None, 4, 1.0, fake, None) == -1 and b"null" in err()
    assert lib.os2d_train_optim_finalize(fake, 4, 1.0, None, None) == -1 and b"null" in err()
    # nothing to do is not an error and launches nothing
    assert calls(_table(0), 0) == [0] * 4
    empty = _table(2, numel=0, param=None, grad=None, state1=None, state2=None)
    assert lib.os2d_train_optim_sumsq(empty, 2, fake, 0, None) == 0
    assert lib.os2d_train_optim_update(_train_lib.OPTIM_ADAM, empty, 2, fake, fake, 0.9, 0.999, 1e-8, None) == 0
