"""Optimisers and learning-rate annealing (reference os2d/engine/optimization.py), with the per-step work of every method -
gradient norm, clipping, the NaN guard and the update - on the multi-tensor HIP kernels of libos2d_train.so
(os2d_train_optim_*, include/os2d_train.h).

``create_optimizer`` builds the reference's optimiser from its settings: "sgd" and "adam" give ``DeviceSGD`` / ``DeviceAdam``,
the other six methods the stock ``torch.optim`` classes or, with ``on_device=True``, ``DeviceAdagrad``, ``DeviceAdadelta``,
``DeviceAdamax``, ``DeviceASGD``, ``DeviceRMSprop``, ``DeviceRprop`` (os2d_train_optim_prepare_ex / update_ex).  The device
classes subclass the ``torch.optim`` class of their method for its constructor, ``defaults``, ``param_groups`` and
``state_dict()`` layout only: state lives in ``self.state[p]`` under torch's own keys (``momentum_buffer``; ``step`` as a 0-dim
device float tensor, ``exp_avg``, ``exp_avg_sq`` - the layout of ``Adam(capturable=True)``; ``sum``, ``square_avg``, ... for the
other methods), so checkpoints and torch's LR schedulers work unchanged.  ``clip_and_step(max_grad_norm)`` is ``clip_grad_norm_``
+ ``if not isnan(norm): step()`` decided on the device: it returns the norm as a device scalar and never waits for the device.
"""
import ctypes
import logging
from statistics import median

import torch
from torch import optim

from .. import _train_lib
from .._native import STREAM

MAX_TENSORS = _train_lib.OPTIM_MAX_TENSORS      # tensors per launch (the table travels in the kernel arguments)
CHUNK = _train_lib.OPTIM_CHUNK                  # elements per work-group


def ceildiv(a, b):
    return -(-a // b)


def chunks_of(numel, chunk=CHUNK):
    return ceildiv(numel, chunk) if numel > 0 else 0


def pointers_aligned(*addresses):
    """The `aligned` mark of a tensor record: every non-null address is a multiple of 16 bytes."""
    bits = 0
    for a in addresses:
        bits |= a or 0
    return int(bits & 15 == 0)


def plan_tables(numels, keys=None, max_tensors=MAX_TENSORS, chunk=CHUNK):
    """The launch plan of one step.  numels: the element count of every tensor that has a gradient, in order.  Chunks are
    numbered over the whole step; a table holds at most ``max_tensors`` consecutive tensors, and (``keys``: one hashable per
    tensor) only tensors with equal keys - those that share the launch's hyperparameters.
    -> (tables, total_chunks); a table is a list of (tensor index, first_chunk, chunks)."""
    tables, first = [], 0
    for i, n in enumerate(numels):
        if n < 0:
            raise ValueError("tensor {} has negative numel {}".format(i, n))
        if not tables or len(tables[-1]) >= max_tensors or (keys is not None and keys[i] != keys[tables[-1][0][0]]):
            tables.append([])
        c = chunks_of(n, chunk)
        tables[-1].append((i, first, c))
        first += c
    return tables, first


class _Plan(object):
    """What stays the same from step to step while the same parameters have gradients: the records of every table with the
    parameter-independent fields filled in, and the tensors they point to (kept alive here)."""

    def __init__(self, entries, keys, tables, total_chunks):
        self.entries, self.keys, self.total_chunks = entries, keys, total_chunks       # entries: (p, state1, state2, step)
        self.tables = []                      # (ctypes array, n, offset of its first tensor, hyper key)
        self.records, self.state_bits = [], []
        for rows in tables:
            arr = (_train_lib.OptimTensor * len(rows))()
            for k, (i, first, _) in enumerate(rows):
                rec = arr[k]
                p, s1, s2, step = entries[i]
                rec.state1 = None if s1 is None else s1.data_ptr()
                rec.state2 = None if s2 is None else s2.data_ptr()
                rec.step = None if step is None else step.data_ptr()
                rec.numel, rec.first_chunk = p.numel(), first
                self.records.append(rec)
                self.state_bits.append((rec.state1 or 0) | (rec.state2 or 0))
            self.tables.append((arr, len(rows), rows[0][0], keys[rows[0][0]]))


class _DeviceStep(object):
    """The step of every device optimiser: everything but the method's state and hyperparameters."""
    _method = None

    # ---- what a subclass provides
    def _check_group(self, group):
        raise NotImplementedError

    def _hyper(self, group):
        """The hyperparameters of a group that tensors of one launch share: (momentum or beta1, beta2, eps) for SGD / Adam, the
        method's `hyper` array of os2d_train_optim_*_ex for the others."""
        raise NotImplementedError

    def _state_of(self, p, group):
        """(state1, state2, step) tensors of a parameter, created as zeros on first use."""
        raise NotImplementedError

    # ---- torch.optim.Optimizer
    def load_state_dict(self, state_dict):
        super(_DeviceStep, self).load_state_dict(state_dict)
        self._adopt_state()

    def __setstate__(self, state):
        super(_DeviceStep, self).__setstate__(state)
        self._adopt_state()

    def add_param_group(self, param_group):
        super(_DeviceStep, self).add_param_group(param_group)
        self._plan = None

    def _adopt_state(self):
        """After state arrived from outside (a checkpoint of this class or of the stock torch optimiser, of any device): put it
        into the layout the kernels read."""
        self._plan = None
        for group in self.param_groups:
            self._adopt_group(group)
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    self._adopt_param_state(p, st)

    def _adopt_group(self, group):
        pass

    def _adopt_param_state(self, p, st):
        pass

    @staticmethod
    def _like(p, value):
        # a copy: torch's load_state_dict hands over the checkpoint's own tensor where device and dtype already fit, and two
        # optimisers that loaded the same state_dict() would update one buffer
        return value.detach().to(device=p.device, dtype=torch.float32, copy=True).reshape(p.shape).contiguous()

    @torch.no_grad()
    def step(self, closure=None):
        """A step without clipping (coef = 1); the NaN guard is still on: a NaN anywhere in the gradients leaves parameters
        and state untouched."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._run(float("inf"))
        return loss

    @torch.no_grad()
    def clip_and_step(self, max_grad_norm):
        """``clip_grad_norm_(params, max_grad_norm)`` followed by ``step()`` unless the norm is NaN, without a host wait.
        Returns the total gradient norm as a 0-dim device tensor; ``p.grad`` holds the clipped gradients afterwards."""
        norm = self._run(float(max_grad_norm))
        self._opt_called = True           # what torch's LR schedulers look at to tell that a step preceded scheduler.step()
        return norm

    def _groups(self):
        """-> [(group, lr, weight_decay, hyper key)], checked"""
        out = []
        for group in self.param_groups:
            self._check_group(group)
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                raise ValueError("{}: a tensor learning rate would need a host wait; use a float".format(type(self).__name__))
            out.append((group, lr, group.get("weight_decay", 0.0), self._hyper(group)))      # (Rprop has no weight decay)
        return out

    def _build_plan(self, groups):
        entries, keys = [], []
        for group, _, _, key in groups:
            for p in group["params"]:
                if p.grad is not None:
                    self._validate(p, p.grad)
                    entries.append((p,) + tuple(self._state_of(p, group)))
                    keys.append(key)
        tables, total = plan_tables([e[0].numel() for e in entries], keys)
        return _Plan(entries, keys, tables, total)

    def _validate(self, p, g):
        if not (p.is_cuda and p.dtype is torch.float32 and p.is_contiguous()):
            raise ValueError("{} needs contiguous float32 parameters on the HIP device (no fallback), got {} {} {}".format(
                type(self).__name__, p.device, p.dtype, "contiguous" if p.is_contiguous() else "non-contiguous"))
        if g.is_sparse or not (g.is_cuda and g.dtype is torch.float32 and g.is_contiguous() and g.shape == p.shape):
            raise ValueError("{} needs dense contiguous float32 gradients of the parameter's shape on its device".format(type(self).__name__))

    def _refresh(self, plan, groups):
        """One pass over the parameters: checks them and fills in the fields that may change between two steps - both pointers
        (zero_grad(set_to_none=True) frees the gradients, module.to() replaces a parameter's storage), with them the
        alignment mark, and the group's rate and decay.  False: other parameters have gradients than the plan was made for, or
        a group's hyperparameters changed."""
        entries, keys, records, state_bits, n = plan.entries, plan.keys, plan.records, plan.state_bits, len(plan.entries)
        k, dev = 0, None
        for group, lr, wd, key in groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if k >= n or entries[k][0] is not p or keys[k] != key:
                    return False
                self._validate(p, g)
                if dev is None:
                    dev = p.get_device()
                if p.get_device() != dev or g.get_device() != dev or p.numel() != records[k].numel:
                    raise ValueError("{}: parameters and gradients must stay on one device and keep their size".format(type(self).__name__))
                rec = records[k]
                pa, ga = p.data_ptr(), g.data_ptr()
                rec.param, rec.grad, rec.aligned = pa, ga, pointers_aligned(pa, ga, state_bits[k])
                rec.lr, rec.weight_decay = lr, wd
                k += 1
        return k == n

    def _run(self, max_norm):
        if not max_norm > 0:
            raise ValueError("max_grad_norm must be positive, got {}".format(max_norm))
        groups = self._groups()
        plan = getattr(self, "_plan", None)
        if plan is None or not self._refresh(plan, groups):
            plan = self._plan = self._build_plan(groups)
            if not self._refresh(plan, groups):
                raise RuntimeError("{}: the launch plan does not fit the parameters it was made for".format(type(self).__name__))
        if not plan.entries:                  # no gradient anywhere: the norm of nothing, as clip_grad_norm_ returns it
            for group, _, _, _ in groups:
                for p in group["params"]:
                    return torch.zeros((), dtype=torch.float32, device=p.device)
        dev = plan.entries[0][0].device
        method = self._method
        adam = method == _train_lib.OPTIM_ADAM
        ex = method not in (_train_lib.OPTIM_SGD, _train_lib.OPTIM_ADAM)         # the *_ex entry points
        per = _train_lib.OPTIM_FACTORS if ex else (2 if adam else 0)            # floats of prepare per tensor
        partials = torch.empty(max(plan.total_chunks, 1), dtype=torch.float64, device=dev)
        record = torch.empty(4, dtype=torch.float32, device=dev)
        factors = torch.empty(per * len(plan.entries), dtype=torch.float32, device=dev) if per else None
        call = _train_lib.call
        for arr, n, _, _ in plan.tables:
            call("os2d_train_optim_sumsq", arr, n, partials, plan.total_chunks, STREAM)
        call("os2d_train_optim_finalize", partials, plan.total_chunks, max_norm, record, STREAM)
        for arr, n, offset, hyper in plan.tables:
            fp = factors[per * offset:] if per else None         # this table's factors
            if ex:
                h = (ctypes.c_double * len(hyper))(*hyper)       # a host array: it travels in the kernel arguments
                call("os2d_train_optim_prepare_ex", method, arr, n, record, h, len(hyper), fp, STREAM)
                call("os2d_train_optim_update_ex", method, arr, n, record, fp, h, len(hyper), STREAM)
                continue
            h0, h1, h2 = hyper
            if adam:
                call("os2d_train_optim_prepare", arr, n, record, h0, h1, fp, STREAM)
            call("os2d_train_optim_update", method, arr, n, record, fp, h0, h1, h2, STREAM)
        self._last = (record, factors)        # read by the stage tests: {norm, coef, skip, 0} and the per-tensor factors of prepare
        return record[0]


class DeviceSGD(_DeviceStep, optim.SGD):
    """``torch.optim.SGD`` (momentum, L2 weight decay; dampening 0, no Nesterov, no maximize) whose step runs as multi-tensor
    HIP kernels.  State: ``momentum_buffer`` per parameter when momentum != 0, zeros before the first step (equal in value to
    torch's first-step clone of the gradient)."""
    _method = _train_lib.OPTIM_SGD

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0):
        optim.SGD.__init__(self, params, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self._plan = None

    def _check_group(self, group):
        if group["dampening"] != 0 or group["nesterov"] or group["maximize"]:
            raise ValueError("DeviceSGD supports dampening 0, no Nesterov momentum and no maximize")

    def _hyper(self, group):
        return (float(group["momentum"]), 0.0, 0.0)

    def _state_of(self, p, group):
        if group["momentum"] == 0:
            return None, None, None
        st = self.state[p]
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st["momentum_buffer"], None, None

    def _adopt_param_state(self, p, st):
        if st.get("momentum_buffer") is not None:
            st["momentum_buffer"] = self._like(p, st["momentum_buffer"])


class DeviceAdam(_DeviceStep, optim.Adam):
    """``torch.optim.Adam`` (L2 weight decay; no amsgrad, no maximize) whose step runs as multi-tensor HIP kernels.  State as
    ``Adam(capturable=True)`` keeps it: ``step`` a 0-dim float32 tensor on the parameter's device, advanced on the device and
    only on a step that is not skipped; ``exp_avg``; ``exp_avg_sq``."""
    _method = _train_lib.OPTIM_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        optim.Adam.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True)
        self._plan = None

    def _check_group(self, group):
        if group["amsgrad"] or group["maximize"] or group.get("decoupled_weight_decay", False):
            raise ValueError("DeviceAdam supports no amsgrad, no maximize and no decoupled weight decay")

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return (float(b1), float(b2), float(group["eps"]))

    def _state_of(self, p, group):
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st["exp_avg"], st["exp_avg_sq"], st["step"]

    def _adopt_group(self, group):
        group["capturable"] = True            # a checkpoint of the stock optimiser carries False: `step` would stay on the host

    def _adopt_param_state(self, p, st):
        step = st["step"]
        if not isinstance(step, torch.Tensor):                # checkpoints of old torch versions: a Python int
            step = torch.tensor(float(step))
        st["step"] = step.detach().to(device=p.device, dtype=torch.float32).reshape(()).clone()
        st["exp_avg"] = self._like(p, st["exp_avg"])
        st["exp_avg_sq"] = self._like(p, st["exp_avg_sq"])


class _MethodStep(_DeviceStep):
    """The step of the reference's other six methods (os2d_train_optim_prepare_ex / update_ex).  A subclass names torch's keys of
    its one or two per-element state tensors (``_keys``: state1, state2); ``step`` is a 0-dim float32 tensor on the parameter's
    device for all of them, advanced on the device and only on a step that is not skipped."""
    _keys = ()
    _refused = ("maximize", "differentiable")          # group options that must be false

    def _check_group(self, group):
        for name in self._refused:
            if group.get(name):
                raise ValueError("{} does not support {}={!r}".format(type(self).__name__, name, group[name]))

    def _new_state(self, p, group, key):
        return torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _state_of(self, p, group):
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            for key in self._keys:
                st[key] = self._new_state(p, group, key)
        return st[self._keys[0]], (st[self._keys[1]] if len(self._keys) > 1 else None), st["step"]

    def _adopt_group(self, group):
        if "capturable" in group:             # a checkpoint of the stock optimiser carries False: `step` would stay on the host
            group["capturable"] = True

    @staticmethod
    def _scalar(p, value):
        """a count, eta or mu of a checkpoint (a tensor of any device, or a number of old torch versions) as a fresh 0-dim
        float32 tensor on the parameter's device"""
        if not isinstance(value, torch.Tensor):
            value = torch.tensor(float(value))
        return value.detach().to(device=p.device, dtype=torch.float32).reshape(()).clone()

    def _adopt_param_state(self, p, st):
        st["step"] = self._scalar(p, st["step"])
        for key in self._keys:
            st[key] = self._like(p, st[key])


class DeviceAdagrad(_MethodStep, optim.Adagrad):
    """``torch.optim.Adagrad`` (``lr_decay``, L2 weight decay, ``initial_accumulator_value``) as multi-tensor HIP kernels.
    State: ``step``, ``sum``.  The stock class creates both in its constructor, the count on the host; it is moved to the
    parameter's device here."""
    _method = _train_lib.OPTIM_ADAGRAD
    _keys = ("sum",)
    _refused = ("maximize", "differentiable", "fused")

    def __init__(self, params, lr=1e-2, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10):
        optim.Adagrad.__init__(self, params, lr=lr, lr_decay=lr_decay, weight_decay=weight_decay,
                               initial_accumulator_value=initial_accumulator_value, eps=eps)
        self._adopt_state()

    def _hyper(self, group):
        return (float(group["lr_decay"]), float(group["eps"]))

    def _new_state(self, p, group, key):
        return torch.full_like(p, group["initial_accumulator_value"], memory_format=torch.contiguous_format)


class DeviceAdadelta(_MethodStep, optim.Adadelta):
    """``torch.optim.Adadelta`` (L2 weight decay) as multi-tensor HIP kernels.  State: ``step``, ``square_avg``, ``acc_delta``."""
    _method = _train_lib.OPTIM_ADADELTA
    _keys = ("square_avg", "acc_delta")

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0):
        optim.Adadelta.__init__(self, params, lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, capturable=True)
        self._plan = None

    def _hyper(self, group):
        return (float(group["rho"]), float(group["eps"]))


class DeviceAdamax(_MethodStep, optim.Adamax):
    """``torch.optim.Adamax`` (L2 weight decay) as multi-tensor HIP kernels, with the arithmetic of the stock class's
    ``capturable=False`` route (the bias correction in double).  State: ``step``, ``exp_avg``, ``exp_inf``."""
    _method = _train_lib.OPTIM_ADAMAX
    _keys = ("exp_avg", "exp_inf")

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        optim.Adamax.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True)
        self._plan = None

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return (float(b1), float(b2), float(group["eps"]))


class DeviceASGD(_MethodStep, optim.ASGD):
    """``torch.optim.ASGD`` (L2 weight decay) as multi-tensor HIP kernels.  State: ``step``, ``eta``, ``mu``, ``ax``.

    ``eta`` and ``mu`` are torch's 0-dim tensors, and here the two elements of ONE two-float device tensor per parameter, which
    the tensor record's ``state2`` points to: the prepare kernel hands the update the pair the previous step left and writes
    the next one, both functions of the step count alone.  ``state_dict()`` shows them as torch does; state that arrives from
    outside is copied into a fresh pair."""
    _method = _train_lib.OPTIM_ASGD
    _keys = ("ax",)

    def __init__(self, params, lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0.0):
        optim.ASGD.__init__(self, params, lr=lr, lambd=lambd, alpha=alpha, t0=t0, weight_decay=weight_decay, capturable=True)
        self._plan = None

    def _hyper(self, group):
        return (float(group["lambd"]), float(group["alpha"]), float(group["t0"]))

    def _state_of(self, p, group):
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            start = torch.ones(2, dtype=torch.float32, device=p.device)      # eta = lr, mu = 1 before the first step
            start[0] = group["lr"]
            st["eta"], st["mu"] = start[0], start[1]
            st["ax"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st["ax"], st["eta"], st["step"]

    def _adopt_param_state(self, p, st):
        super(DeviceASGD, self)._adopt_param_state(p, st)
        pair = torch.stack([self._scalar(p, st["eta"]), self._scalar(p, st["mu"])])
        st["eta"], st["mu"] = pair[0], pair[1]


class DeviceRMSprop(_MethodStep, optim.RMSprop):
    """``torch.optim.RMSprop`` (L2 weight decay; no momentum, not centered) as multi-tensor HIP kernels.  State: ``step``,
    ``square_avg``."""
    _method = _train_lib.OPTIM_RMSPROP
    _keys = ("square_avg",)
    _refused = ("maximize", "differentiable", "momentum", "centered")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0):
        optim.RMSprop.__init__(self, params, lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, capturable=True)
        self._plan = None

    def _hyper(self, group):
        return (float(group["alpha"]), float(group["eps"]))


class DeviceRprop(_MethodStep, optim.Rprop):
    """``torch.optim.Rprop`` as multi-tensor HIP kernels.  State: ``step``, ``prev``, ``step_size`` (filled with the group's
    learning rate at creation).  No weight decay, as in torch."""
    _method = _train_lib.OPTIM_RPROP
    _keys = ("prev", "step_size")

    def __init__(self, params, lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50)):
        optim.Rprop.__init__(self, params, lr=lr, etas=etas, step_sizes=step_sizes, capturable=True)
        self._plan = None

    def _hyper(self, group):
        return tuple(float(v) for v in tuple(group["etas"]) + tuple(group["step_sizes"]))

    def _new_state(self, p, group, key):
        if key == "prev":
            return torch.zeros_like(p, memory_format=torch.contiguous_format)
        return torch.full_like(p, group["lr"], memory_format=torch.contiguous_format)


def _setting(cfg, keywords, name):
    if name in keywords:
        return keywords[name]
    if cfg is None or not hasattr(cfg, name):
        raise TypeError("create_optimizer needs `{}` (a keyword, or an attribute of cfg)".format(name))
    return getattr(cfg, name)


def create_optimizer(parameters, cfg=None, optimizer_state=None, **keywords):
    """reference optimization.py:9-35.  The settings ``optim_method``, ``lr``, ``weight_decay``, ``sgd_momentum`` come from
    ``cfg`` (any object with these attributes, e.g. the reference's cfg.train.optim) or from keywords, which win.  "sgd" and
    "adam" give the device optimisers; the other six methods give the stock ``torch.optim`` classes, or with ``on_device=True`` (a
    keyword or an attribute of ``cfg``; default False) ``DeviceAdagrad`` .. ``DeviceRprop``.  ``optimizer_state`` is a
    ``state_dict()`` of either kind of optimiser."""
    unknown = set(keywords) - {"optim_method", "lr", "weight_decay", "sgd_momentum", "on_device"}
    if unknown:
        raise TypeError("create_optimizer: unknown settings {}".format(sorted(unknown)))
    lr = _setting(cfg, keywords, "lr")
    method = _setting(cfg, keywords, "optim_method")
    optim_method = method.casefold()
    on_device = bool(keywords["on_device"] if "on_device" in keywords else getattr(cfg, "on_device", False))

    def wd():
        return _setting(cfg, keywords, "weight_decay")
    if optim_method == "sgd":
        optimizer = DeviceSGD(parameters, lr=lr, weight_decay=wd(), momentum=_setting(cfg, keywords, "sgd_momentum"))
    elif optim_method == "adagrad":
        optimizer = (DeviceAdagrad if on_device else optim.Adagrad)(parameters, lr=lr, weight_decay=wd())
    elif optim_method == "adadelta":
        optimizer = (DeviceAdadelta if on_device else optim.Adadelta)(parameters, lr=lr, weight_decay=wd())
    elif optim_method == "adam":
        optimizer = DeviceAdam(parameters, lr=lr, weight_decay=wd())
    elif optim_method == "adamax":
        optimizer = (DeviceAdamax if on_device else optim.Adamax)(parameters, lr=lr, weight_decay=wd())
    elif optim_method == "asgd":
        optimizer = (DeviceASGD if on_device else optim.ASGD)(parameters, lr=lr, t0=5000, weight_decay=wd())
    elif optim_method == "rmsprop":
        optimizer = (DeviceRMSprop if on_device else optim.RMSprop)(parameters, lr=lr, weight_decay=wd())
    elif optim_method == "rprop":
        optimizer = (DeviceRprop if on_device else optim.Rprop)(parameters, lr=lr)
    else:
        raise RuntimeError("Invalid optim method: " + method)
    if optimizer_state is not None:
        optimizer.load_state_dict(optimizer_state)
        set_learning_rate(optimizer, lr)
    return optimizer


def set_learning_rate(optimizer, learning_rate):
    logger = logging.getLogger("OS2D")
    for p in optimizer.param_groups:
        if "lr" in p:
            if p["lr"] != learning_rate:
                logger.info("Changing learning rate from {} to {}".format(p["lr"], learning_rate))
                p["lr"] = learning_rate


def get_learning_rate(optimizer):
    for p in optimizer.param_groups:
        if "lr" in p:
            return p["lr"]


def setup_lr(optimizer, full_log, cfg, eval_iter):
    """reference optimization.py:53-94: -> (scheduler or None, anneal_lr_func(i_iter, anneal_now=True) -> the learning rate).
    ``cfg.type``: "none", "MultiStepLR" (``milestones``, ``gamma``; in iterations, stepped once per evaluation) or
    "ReduceLROnPlateau" (``reduce_factor``, ``min_value``, ``quantity_epsilon``, ``quantity_mode``, ``patience``, ``cooldown``,
    ``quantity_to_monitor``, ``quantity_smoothness``: the scheduler sees the median of the last values of ``full_log``)."""
    kind = cfg.type.lower()
    averaging_buffer, averaging_buffer_max_length = [], 1
    if kind == "none":
        lr_scheduler = None
    elif kind == "multisteplr":
        lr_scheduler = optim.lr_scheduler.MultiStepLR(optimizer, milestones=[ceildiv(m, eval_iter) for m in cfg.milestones], gamma=cfg.gamma)
    elif kind == "reducelronplateau":
        lr_scheduler = optim.lr_scheduler.ReduceLROnPlateau(
            optimizer, factor=cfg.reduce_factor, min_lr=cfg.min_value, threshold=cfg.quantity_epsilon, threshold_mode="rel",
            mode=cfg.quantity_mode, patience=ceildiv(cfg.patience, eval_iter), cooldown=ceildiv(cfg.cooldown, eval_iter))
        averaging_buffer_max_length = max(1, ceildiv(cfg.quantity_smoothness, eval_iter))
    else:
        raise RuntimeError("Unknown annel_lr type: {}".format(cfg.type))

    def anneal_lr_func(i_iter, anneal_now=True):
        if kind == "multisteplr":
            lr_scheduler.step()
        elif kind == "reducelronplateau":
            averaging_buffer.append(full_log[cfg.quantity_to_monitor][-1])
            if len(averaging_buffer) > averaging_buffer_max_length:
                averaging_buffer.pop(0)
            if anneal_now:
                lr_scheduler.step(median(averaging_buffer))
        return get_learning_rate(optimizer)

    return lr_scheduler, anneal_lr_func
