"""A numpy float32 model of the device step of the reference's other six optimisation methods (os2d_train_optim_prepare_ex /
update_ex, os2d_amd/csrc_train/optim.hip, include/os2d_train.h): the per-tensor factors in double, rounded once, and the element
updates with one rounding per operation in the kernels' operation order (numpy rounds every float32 operation once, and its
division and square root are correctly rounded).  Norm, clip coefficient and the comparison helpers are those of optim_model.py.
Also the shared inputs of the tests of these methods and ``torch_float64``, the stock torch.optim class run in float64."""
import numpy as np
import torch

from optim_model import F, ULP, grad_norm, clip_coef, same_bits, ulps, relative_error, trajectory_case  # noqa: F401  (re-exported)

METHODS = ("adagrad", "adadelta", "adamax", "asgd", "rmsprop", "rprop")
STOCK = dict(adagrad=torch.optim.Adagrad, adadelta=torch.optim.Adadelta, adamax=torch.optim.Adamax, asgd=torch.optim.ASGD,
             rmsprop=torch.optim.RMSprop, rprop=torch.optim.Rprop)
# torch's defaults, and t0 = 5000 as the reference's create_optimizer passes it
HYPER = dict(adagrad=dict(lr_decay=0.0, eps=1e-10, initial_accumulator_value=0.0), adadelta=dict(rho=0.9, eps=1e-6),
             adamax=dict(betas=(0.9, 0.999), eps=1e-8), asgd=dict(lambd=1e-4, alpha=0.75, t0=5000), rmsprop=dict(alpha=0.99, eps=1e-8),
             rprop=dict(etas=(0.5, 1.2), step_sizes=(1e-6, 50)))
STATE_KEYS = dict(adagrad=("sum",), adadelta=("square_avg", "acc_delta"), adamax=("exp_avg", "exp_inf"), asgd=("ax",),
                  rmsprop=("square_avg",), rprop=("prev", "step_size"))
HAS_CAPTURABLE = ("adadelta", "adamax", "asgd", "rmsprop", "rprop")          # Adagrad has no such option
FACTORS = 4                               # floats per tensor that prepare_ex writes

# The trajectory of the tests: the five steps of optim_model.trajectory_case (gradient norms about 32 t) and three more with
# norms about 16, 80, 32; max_norm 50 clips steps 2 - 5 and 7 and leaves 1, 6 and 8 alone.
SETTINGS = dict(lr=1e-2, weight_decay=1e-4, max_norm=50.0)
EXTRA_SCALES = (0.1, 0.5, 0.2)
STEPS = 5 + len(EXTRA_SCALES)
CLIPPED = [False, True, True, True, True, False, True, False]
RPROP_FLOOR = 1e-3                        # |g| of the Rprop trajectory: g * prev neither underflows in float32 nor sits at a rounding edge
# The largest error of the model against torch in float64 over the STEPS steps, relative to max(1, |p|), in units of 2^-24,
# measured on the CPU by test_optim_methods_model.py::test_model_tracks_torch_float64; the bound is twice that.
# (The error grows about linearly with the steps; ASGD rounds the parameter twice per step, in p * (1 - lambd eta) and in p - eta d.)
MEASURED = dict(adagrad=4.61, adadelta=5.02, adamax=4.93, asgd=12.43, rmsprop=4.97, rprop=3.78)
TRAJECTORY_BOUND = {m: 2.0 * v * ULP for m, v in MEASURED.items()}


def methods_case(method, seed=0):
    """-> (params, [grads of step 1 .. STEPS]) as float32 arrays.  Rprop: every |g| raised to RPROP_FLOOR, the sign kept."""
    params, grads = trajectory_case(seed)
    rng = np.random.RandomState(seed + 1000)
    grads = grads + [[(s * rng.standard_normal(p.shape)).astype(F) for p in params] for s in EXTRA_SCALES]
    if method == "rprop":
        grads = [[np.where(g < 0, -1, 1).astype(F) * np.maximum(np.abs(g), F(RPROP_FLOOR)) for g in step] for step in grads]
    return params, grads


def _hyper_of(method, hyper):
    h = dict(HYPER[method])
    h.update(hyper or {})
    return h


def first_eta_mu(lr):
    """ASGD before the first step: eta = lr, mu = 1"""
    return F(lr), F(1.0)


def next_eta_mu(lr, h, t):
    """ASGD after step t: (float32(lr / (1 + lambd lr t)^alpha), float32(1 / max(1, t - t0))) in double; lr as the record carries it"""
    lr = float(F(lr))
    return F(lr / (1.0 + h["lambd"] * lr * t) ** h["alpha"]), F(1.0 / max(1.0, t - h["t0"]))


def method_factors(method, lr, h, t, eta_mu=None):
    """What prepare_ex writes for a tensor at its step t (the count after the increment): FACTORS float32 values, computed in
    double from the float32 learning rate of the record.  eta_mu: ASGD's pair as the previous step left it."""
    lr = float(F(lr))
    f = np.zeros(FACTORS, dtype=F)
    if method == "adagrad":
        f[0] = F(lr / (1.0 + (t - 1.0) * h["lr_decay"]))
    elif method == "adamax":
        f[0] = F(lr / (1.0 - h["betas"][0] ** t))
    elif method == "asgd":
        f[0], f[1], f[2] = F(1.0 - h["lambd"] * float(eta_mu[0])), eta_mu[0], eta_mu[1]
    return f


def _maximum(x, y):
    """the larger one, NaN where either is (torch.maximum)"""
    return np.where(np.isnan(x) | np.isnan(y), F(np.nan), np.maximum(x, y)).astype(F)


def method_update(method, p, g, a, b, lr, wd, f, h):
    """One tensor's update: p, g float32 arrays, a / b the method's state1 / state2, f its factors.  -> (p, a, b, s) with s the
    Rprop product d * prev whose sign decides the branch (None for the other methods)."""
    d = g + F(wd) * p if (wd != 0 and method != "rprop") else g
    lr, s = F(lr), None
    if method == "adagrad":
        a = a + d * d
        p = p - f[0] * (d / (np.sqrt(a) + F(h["eps"])))
    elif method == "adadelta":
        rho, omr, eps = F(h["rho"]), F(1.0 - h["rho"]), F(h["eps"])
        a = rho * a + (omr * d) * d
        delta = np.sqrt(b + eps) / np.sqrt(a + eps) * d
        b = rho * b + (omr * delta) * delta
        p = p - lr * delta
    elif method == "adamax":
        a = a + (d - a) * F(1.0 - h["betas"][0])
        b = _maximum(F(h["betas"][1]) * b, np.abs(d) + F(h["eps"]))
        p = p - f[0] * (a / b)
    elif method == "asgd":
        p = p * f[0]
        p = p - f[1] * d
        a = a + (p - a) * f[2] if f[2] != F(1.0) else p.copy()
    elif method == "rmsprop":
        alpha, oma, eps = F(h["alpha"]), F(1.0 - h["alpha"]), F(h["eps"])
        a = alpha * a + (oma * d) * d
        p = p - lr * (d / (np.sqrt(a) + eps))
    else:
        etaminus, etaplus = (F(v) for v in h["etas"])
        smin, smax = (F(v) for v in h["step_sizes"])
        s = d * a
        eta = np.where(s > 0, etaplus, np.where(s < 0, etaminus, np.where(s == 0, F(1.0), s))).astype(F)
        size = b * eta
        size = np.where(size < smin, smin, np.where(size > smax, smax, size)).astype(F)       # a NaN stays
        b = size
        d = np.where(s < 0, F(0.0), d).astype(F)
        sign = np.where(d > 0, F(1.0), np.where(d < 0, F(-1.0), np.where(d == 0, F(0.0), d))).astype(F)
        p = p - sign * size
        a = d
    return p, a, b, s


class MethodModel(object):
    """clip_and_step of DeviceAdagrad .. DeviceRprop on lists of float32 arrays; lr, weight_decay and the method's
    hyperparameters (a dict over HYPER[method], or None) per tensor."""

    def __init__(self, method, params, lr, weight_decay=0.0, hyper=None):
        n = len(params)
        self.method = method
        self.params = [np.array(p, dtype=F) for p in params]
        self.lr = list(lr) if isinstance(lr, (list, tuple)) else [lr] * n
        self.wd = list(weight_decay) if isinstance(weight_decay, (list, tuple)) else [weight_decay] * n
        self.hyper = [_hyper_of(method, h) for h in (hyper if isinstance(hyper, (list, tuple)) else [hyper] * n)]
        self.state1, self.state2 = [None] * n, [None] * n
        self.steps = [None] * n           # the count of the steps that were not skipped and had a gradient
        self.eta_mu = [None] * n          # ASGD
        self.products = [None] * n        # Rprop: d * prev of the last step

    def _create(self, i):
        p, h, m = self.params[i], self.hyper[i], self.method
        self.steps[i] = 0
        self.state1[i] = np.full_like(p, h["initial_accumulator_value"]) if m == "adagrad" else np.zeros_like(p)
        if m in ("adadelta", "adamax"):
            self.state2[i] = np.zeros_like(p)
        elif m == "rprop":
            self.state2[i] = np.full_like(p, F(self.lr[i]))
        elif m == "asgd":
            self.eta_mu[i] = first_eta_mu(self.lr[i])

    def step(self, grads, max_norm, coef=None, factors=None):
        """grads: float32 arrays or None per tensor.  coef / factors ({tensor index: FACTORS floats}): the values to use
        instead of the model's own (the device's, read back).  -> (norm, coef, skip, clipped gradients, the model's own factors)."""
        norm = grad_norm(grads)
        coef = clip_coef(norm, max_norm) if coef is None else F(coef)
        skip = bool(np.isnan(norm))
        out, own = [], {}
        with np.errstate(all="ignore"):
            for i, g in enumerate(grads):
                if g is None:
                    out.append(None)
                    continue
                g = np.asarray(g, dtype=F) * coef
                out.append(g)
                if skip:
                    continue
                if self.steps[i] is None:
                    self._create(i)
                self.steps[i] += 1
                h = self.hyper[i]
                own[i] = method_factors(self.method, self.lr[i], h, self.steps[i], self.eta_mu[i])
                if self.method == "asgd":
                    self.eta_mu[i] = next_eta_mu(self.lr[i], h, self.steps[i])
                f = own[i] if factors is None else np.asarray(factors[i], dtype=F)
                self.params[i], self.state1[i], self.state2[i], self.products[i] = method_update(
                    self.method, self.params[i], g, self.state1[i], self.state2[i], self.lr[i], self.wd[i], f, h)
        return norm, coef, skip, out, own


def make_stock(method, ps, lr=None, weight_decay=None, **hyper):
    """the stock torch.optim class as the reference's create_optimizer builds it, on the parameters ps"""
    h = _hyper_of(method, hyper)
    lr = SETTINGS["lr"] if lr is None else lr
    if method != "rprop":
        h["weight_decay"] = SETTINGS["weight_decay"] if weight_decay is None else weight_decay
    return STOCK[method](ps, lr=lr, **h)


def make_model(method, params):
    return MethodModel(method, params, SETTINGS["lr"], SETTINGS["weight_decay"])


def torch_float64(method, params, grads_per_step, state_dict=None):
    """The stock class + clip_grad_norm_ in float64 on the CPU from the same float32 inputs, with SETTINGS.
    -> ([params after each step], optimizer, [Rprop: per step and tensor the sign of d * prev in float64; else None])"""
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float64).copy())) for p in params]
    opt = make_stock(method, ps)
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    after, branches = [], []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(np.asarray(g, dtype=np.float64).copy())
        norm = torch.nn.utils.clip_grad_norm_(ps, SETTINGS["max_norm"])
        if method == "rprop":
            branches.append([np.sign(p.grad.numpy() * opt.state[p]["prev"].numpy()) if opt.state[p] else np.zeros(p.shape) for p in ps])
        else:
            branches.append(None)
        if not np.isnan(float(norm)):
            opt.step()
        after.append([p.detach().numpy().copy() for p in ps])
    return after, opt, branches
