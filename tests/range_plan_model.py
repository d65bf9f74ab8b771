"""A numpy float64 model of the device range plan (os2d_amd/csrc_train/range_plan.hip, os2d_train_range_plan), written from the formulas:
eval-mode BatchNorm fold, the bounds B1 / B2 of the two hidden layers' outputs, and the activation, unit and weight exponents
of the split-fp16 ("f16x3") packing.  floor(log2) is exact (the exponent field, ``np.frexp``).  It does not call
``TransformationNet.range_plan``: tests compare the two.

    B1[o]    = 7 * ||w1'[o]||_2 + |b1'[o]|                    w', b': BatchNorm folded
    B2[o]    = min(sum_c B1[c] * ||w2'[o,c]||_1, 5 * ||B1||_2 * ||w2'[o]||_2) + |b2'[o]|
    e<l>[o]  = out_exp(B<l>[o]),  unit_exp = e1 - 15
    wexp<l>[o] = weight_exp(max_c,tap |w<l>'[o,c]| * 2^-in_exp[c]),  in_exp = rnorm_exp | e1 | e2
"""
import numpy as np

RNORM_EXP = 12          # os2d_rnorm_exp()
CLAMP = 60
# layout of the int32 buffer of os2d_train_range_plan: wexp1 [128] | e1 [128] | unit_exp [128] | wexp2 [64] | e2 [64] | wexp3 [8]
INT_FIELDS = (("wexp1", 128), ("e1", 128), ("unit_exp", 128), ("wexp2", 64), ("e2", 64), ("wexp3", 8))
INTS = sum(n for _, n in INT_FIELDS)
DOUBLES = 128 + 64      # B1 | B2


def floor_log2(x):
    """Exact floor(log2(x)) for finite x > 0, clamped to [-60, 60]; 0 for zero, negative, NaN and Inf."""
    x = np.asarray(x, dtype=np.float64)
    ok = np.isfinite(x) & (x > 0)
    _, e = np.frexp(np.where(ok, x, 1.0))          # x = m * 2^e, m in [0.5, 1)
    return np.where(ok, np.clip(e.astype(np.int64) - 1, -CLAMP, CLAMP), 0).astype(np.int32)


def _exp_of(numerator, x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        pos = x > 0                                # false for NaN
        q = numerator / np.maximum(np.where(pos, x, 1.0), 1e-300)
    return np.where(pos, floor_log2(q), 0).astype(np.int32), np.where(pos, q, np.nan)


def out_exp(bound):
    return _exp_of(32768.0, bound)[0]


def weight_exp(amax):
    return _exp_of(16384.0, amax)[0]


def params_of(net):
    """The raw parameters of a TransformationNet as numpy arrays + the two eps (Python floats)."""
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    return sd, float(net.conv[1].eps), float(net.conv[4].eps)


def _fold(w, b, sd, bn, eps):
    w, b = w.astype(np.float64), b.astype(np.float64)
    if bn is None:
        return w, b
    g, beta, mean, var = (sd["{}.{}".format(bn, k)].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(var + eps)
    return w * s.reshape(-1, 1, 1, 1), (b - mean) * s + beta


def plan(sd, eps1, eps2, rnorm_exp=RNORM_EXP):
    """sd: state dict of numpy arrays.  Returns a dict of the six int32 fields, B1, B2 and ``quotients``: every 32768 / B and
    16384 / amax that a floor(log2) was taken of (NaN where none was)."""
    with np.errstate(all="ignore"):
        w1, b1 = _fold(sd["conv.0.weight"], sd["conv.0.bias"], sd, "conv.1", eps1)
        w2, b2 = _fold(sd["conv.3.weight"], sd["conv.3.bias"], sd, "conv.4", eps2)
        w3 = sd["linear.weight"].astype(np.float64)
        B1 = 7.0 * np.sqrt((w1 * w1).sum(axis=(1, 2, 3))) + np.abs(b1)
        e1, q_e1 = _exp_of(32768.0, B1)
        l1 = (np.abs(w2).sum(axis=(2, 3)) * B1[None, :]).sum(axis=1)
        l2 = 5.0 * np.sqrt((B1 * B1).sum()) * np.sqrt((w2 * w2).sum(axis=(1, 2, 3)))
        B2 = np.minimum(l1, l2) + np.abs(b2)       # np.minimum keeps a NaN
        e2, q_e2 = _exp_of(32768.0, B2)
        out = dict(B1=B1, B2=B2, e1=e1, e2=e2, unit_exp=(e1 - 15).astype(np.int32))
        quotients = [q_e1, q_e2]
        for name, w, in_exp in (("wexp1", w1, np.full(w1.shape[1], rnorm_exp)), ("wexp2", w2, e1), ("wexp3", w3, e2)):
            amax = np.max(np.abs(w) * np.exp2(-in_exp.astype(np.float64)).reshape(1, -1, 1, 1), axis=(1, 2, 3))      # np.max keeps a NaN
            out[name], q = _exp_of(16384.0, amax)
            quotients.append(q)
        out["wexp3"] = np.concatenate([out["wexp3"], np.zeros(8 - len(out["wexp3"]), np.int32)])
        out["quotients"] = np.concatenate(quotients)
    return out


def ints(p):
    """The int32 buffer of os2d_train_range_plan."""
    return np.concatenate([np.asarray(p[name], dtype=np.int32) for name, _ in INT_FIELDS])


def doubles(p):
    return np.concatenate([p["B1"], p["B2"]])


# ---- the nets the CPU and GPU tests share
SEEDED = [(kind, P, seed) for kind in ("plain", "adversarial") for P in (6, 4) for seed in (5, 11, 12, 13)]
DEGENERATE = ("zero_linear", "zero_channel", "huge_conv2")
NONFINITE = ("nan_w1_row", "inf_running_var", "fold_divides_by_zero", "inf_bias2")


def seeded_net(kind, P, seed):
    import torch  # noqa: F401
    import util
    from os2d_amd.modeling.head import TransformationNet
    from os2d_amd.utils import synthetic
    state = synthetic.make_transform_net_state(P, seed=seed) if kind == "plain" else util.adversarial_transform_net_state(P, seed=seed)
    net = TransformationNet(output_dim=P, use_cuda=False)
    net.load_state_dict(state)
    return net.eval()


def degenerate_net(kind):
    """The nets of test_range_plan.py::test_degenerate_weights_give_a_valid_plan: a zero ``linear.weight`` (the initial state),
    then a zeroed channel of layer 1, then ``conv[3].weight * 1e30``."""
    import torch
    from os2d_amd.modeling.head import TransformationNet
    with torch.random.fork_rng(devices=[]):      # the constructor draws its weights: the same ones every time, the global generator untouched
        torch.manual_seed(20)
        net = TransformationNet(output_dim=6, use_cuda=False).eval()
    if kind == "zero_linear":
        return net
    with torch.no_grad():
        net.conv[0].weight[3].zero_()
        net.conv[0].bias[3] = 0.0
        net.conv[1].bias[3] = 0.0
        net.conv[1].running_mean[3] = 0.0
        if kind == "huge_conv2":
            net.conv[3].weight.mul_(1e30)
    return net


def nonfinite_net(kind):
    """The plain net (P = 6, seed 11) with one non-finite parameter, or a BatchNorm channel whose var + eps is exactly zero
    (eps = 2^-16 and running_var = -2^-16, both exact in fp32: the folded scale of the channel is infinite)."""
    import torch
    net = seeded_net("plain", 6, 11)
    with torch.no_grad():
        if kind == "nan_w1_row":
            net.conv[0].weight[5, 7, 3, 3] = float("nan")
        elif kind == "inf_running_var":
            net.conv[1].running_var[9] = float("inf")
        elif kind == "fold_divides_by_zero":
            net.conv[1].eps = 2.0 ** -16
            net.conv[1].running_var[4] = -2.0 ** -16
        elif kind == "inf_bias2":
            net.conv[3].bias[7] = float("inf")
        else:
            raise KeyError(kind)
    return net


def reference(net):
    """(integers in the layout of os2d_train_range_plan, bounds B1 | B2) of ``TransformationNet.range_plan`` on a CPU net."""
    import torch
    p = net.range_plan()
    w3 = torch.zeros(8, dtype=torch.int32)
    w3[:net.output_dim] = p["weight_exp"][2]
    assert p["in_exp"][0].numel() == 225 and int(p["in_exp"][0].min()) == int(p["in_exp"][0].max()) == RNORM_EXP
    assert torch.equal(p["in_exp"][1], p["out_exp"][0]) and torch.equal(p["in_exp"][2], p["out_exp"][1]) and p["out_exp"][2] is None
    parts = [p["weight_exp"][0], p["out_exp"][0], p["unit_exp"], p["weight_exp"][1], p["out_exp"][1], w3]
    return torch.cat([t.to(torch.int32) for t in parts]).numpy(), torch.cat(p["bounds"]).numpy()


def fairness(p):
    """Smallest distance, in log2, of a quotient from an integer: where floor(log2) could flip under rounding noise."""
    q = p["quotients"]
    q = q[np.isfinite(q) & (q > 0)]
    if q.size == 0:
        return np.inf
    lg = np.log2(q)
    return float(np.min(np.abs(lg - np.round(lg))))
