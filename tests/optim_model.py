"""A numpy float32 model of the device optimiser step (os2d_amd/csrc_train/optim.hip, include/os2d_train.h): the formulas of
os2d_train_optim_finalize / prepare / update with one rounding per operation (numpy rounds every float32 operation once, and
its division and square root are correctly rounded), plus the shared inputs of the optimiser tests and the torch float64
reference they are compared with."""
import numpy as np
import torch

F = np.float32
ULP = 2.0 ** -24                      # half the spacing of float32 at 1: the unit the bounds are written in
TRAJECTORY_BOUND = 16 * ULP           # five steps against torch in float64, relative to max(1, |p|) (measured: <= 3.8 * ULP)
STEPS = 5
STEP_BOUND = TRAJECTORY_BOUND / STEPS      # the error accumulates linearly per step: one step's share
SIZES = [(1,), (3,), (4095,), (4096,), (4097,), (8193,), (64, 25)]
SETTINGS = dict(lr=1e-2, weight_decay=1e-4, momentum=0.9, betas=(0.9, 0.999), eps=1e-8, max_norm=50.0)


def grad_norm(grads):
    """float32(sqrt(float64 sum of squares)) over every gradient that is not None."""
    total = 0.0
    for g in grads:
        if g is not None:
            total += float(np.sum(np.asarray(g, dtype=np.float64) ** 2))
    with np.errstate(invalid="ignore"):
        return F(np.sqrt(np.float64(total)))


def clip_coef(norm, max_norm):
    """min(max_norm / (norm + 1e-6f), 1) in float32; NaN for a NaN norm; 1 for an infinite max_norm (no clipping)."""
    if np.isinf(max_norm):
        return F(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        c = F(max_norm) / (F(norm) + F(1e-6))
    return F(1.0) if c > F(1.0) else c


def adam_factors(lr, betas, t):
    """(float32(lr / bc1), float32(sqrt(bc2))) with bc = 1 - beta^t in double; lr as the record carries it (float32)."""
    lr = float(F(lr))
    return F(lr / (1.0 - betas[0] ** t)), F(np.sqrt(1.0 - betas[1] ** t))


def _decayed(g, p, wd):
    return g + F(wd) * p if wd != 0 else g


def sgd_update(p, g, buf, lr, wd, mu):
    """-> (p, buf); buf None = no momentum."""
    d = _decayed(g, p, wd)
    if mu != 0:
        buf = F(mu) * buf + d
        d = buf
    return p - F(lr) * d, buf


def adam_update(p, g, m, v, wd, step_size, sqrt_bc2, betas, eps):
    """-> (p, m, v)"""
    d = _decayed(g, p, wd)
    m = m + (d - m) * F(1.0 - betas[0])
    v = F(betas[1]) * v + (F(1.0 - betas[1]) * d) * d
    den = np.sqrt(v) / F(sqrt_bc2) + F(eps)
    return p - F(step_size) * (m / den), m, v


class ModelOptimizer(object):
    """clip_and_step of DeviceSGD ("sgd") / DeviceAdam ("adam") on lists of float32 arrays; lr and weight_decay per tensor."""

    def __init__(self, method, params, lr, weight_decay, momentum=0.0, betas=(0.9, 0.999), eps=1e-8):
        n = len(params)
        self.method, self.momentum, self.betas, self.eps = method, momentum, betas, eps
        self.params = [np.array(p, dtype=F) for p in params]
        self.lr = list(lr) if isinstance(lr, (list, tuple)) else [lr] * n
        self.wd = list(weight_decay) if isinstance(weight_decay, (list, tuple)) else [weight_decay] * n
        self.state1 = [None] * n          # momentum_buffer / exp_avg
        self.state2 = [None] * n          # exp_avg_sq
        self.steps = [None] * n           # Adam: the count of the steps that were not skipped and had a gradient

    def step(self, grads, max_norm, coef=None, factors=None):
        """grads: float32 arrays or None per tensor.  coef / factors ({tensor index: (step_size, sqrt_bc2)}): the values to
        use instead of the model's own (the device's, read back).  -> (norm, coef, skip, clipped gradients)."""
        norm = grad_norm(grads)
        own = clip_coef(norm, max_norm)
        coef = own if coef is None else F(coef)
        skip = bool(np.isnan(norm))
        out = []
        with np.errstate(all="ignore"):
            for i, g in enumerate(grads):
                if g is None:
                    out.append(None)
                    continue
                g = np.asarray(g, dtype=F) * coef
                out.append(g)
                if skip:
                    continue
                p = self.params[i]
                if self.method == "sgd":
                    if self.momentum != 0 and self.state1[i] is None:
                        self.state1[i] = np.zeros_like(p)
                    self.params[i], self.state1[i] = sgd_update(p, g, self.state1[i], self.lr[i], self.wd[i], self.momentum)
                else:
                    if self.steps[i] is None:
                        self.steps[i], self.state1[i], self.state2[i] = 0, np.zeros_like(p), np.zeros_like(p)
                    self.steps[i] += 1
                    f = adam_factors(self.lr[i], self.betas, self.steps[i]) if factors is None else factors[i]
                    self.params[i], self.state1[i], self.state2[i] = adam_update(p, g, self.state1[i], self.state2[i], self.wd[i], f[0], f[1],
                                                                                 self.betas, self.eps)
        return norm, coef, skip, out


def trajectory_case(seed=0):
    """The shared inputs of the trajectory tests: N(0,1) parameters of SIZES and, for step t = 1 .. STEPS, gradients N(0, (0.2 t)^2)
    (total norm about 32 t: with max_norm 50 steps 2 .. 5 clip).  -> (params, [grads of step 1, ...]) as float32 arrays."""
    rng = np.random.RandomState(seed)
    params = [rng.standard_normal(s).astype(F) for s in SIZES]
    grads = [[(0.2 * t * rng.standard_normal(s)).astype(F) for s in SIZES] for t in range(1, STEPS + 1)]
    return params, grads


def torch_float64(method, params, grads_per_step, state_dict=None):
    """torch.optim.SGD / Adam + clip_grad_norm_ in float64 on the CPU from the same float32 inputs, with SETTINGS.
    -> ([params after each step], optimizer)"""
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float64).copy())) for p in params]
    opt = make_torch(method, ps)
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    after = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(np.asarray(g, dtype=np.float64).copy())
        norm = torch.nn.utils.clip_grad_norm_(ps, SETTINGS["max_norm"])
        if not np.isnan(float(norm)):
            opt.step()
        after.append([p.detach().numpy().copy() for p in ps])
    return after, opt


def make_torch(method, ps):
    s = SETTINGS
    if method == "sgd":
        return torch.optim.SGD(ps, lr=s["lr"], weight_decay=s["weight_decay"], momentum=s["momentum"])
    return torch.optim.Adam(ps, lr=s["lr"], weight_decay=s["weight_decay"], betas=s["betas"], eps=s["eps"])


def make_model(method, params):
    s = SETTINGS
    return ModelOptimizer(method, params, s["lr"], s["weight_decay"], momentum=s["momentum"], betas=s["betas"], eps=s["eps"])


def relative_error(ours, reference):
    """max over tensors and elements of |ours - reference| / max(1, |reference|)"""
    worst = 0.0
    for a, b in zip(ours, reference):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if a.size:
            worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))))
    return worst


def same_bits(a, b):
    """Equal float32 arrays bit for bit, except that any NaN equals any NaN (the sign and payload of a generated NaN differ
    between processors)."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~na]))


def ulps(a, b):
    """distance of two finite float32 values in units of the spacing at the larger one"""
    a, b = F(a), F(b)
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b), F(1e-30))))
