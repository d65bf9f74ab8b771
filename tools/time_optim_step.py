"""Times the last line of a training step on the parameter set of the model (ResNet50-C4 + TransformNet, synthetic weights,
random gradients), both routes in one process:

    device   clip_and_step of the device optimiser (os2d_amd/engine/optimization.py, os2d_train_optim_* kernels):
             create_optimizer(..., on_device=True)
    parent   clip_grad_norm_ + float(norm) + the stock torch.optim class's step, what train_one_batch does with a stock optimiser

Per route and method: host time until the step is enqueued (the parent's includes its host wait: float(norm)), device time
between two events around the step (it spans the gaps in which the device waits for the host), and from torch.profiler, where
it works, the number of kernel launches and the sum of the kernels' durations (the device route's launch count also from its
launch plan).  The device kernels' bytes - SGD 28 B / element (norm pass 4; update: read p, g, buf 12, write p, g, buf 12),
Adam 36; Adagrad, RMSprop, ASGD 28 (one state tensor), Adadelta, Adamax, Rprop 36 (two) - over the kernels' durations, as a
fraction of HBM_COPY, the copy rate of tools/hbm_peak.hip.
Medians of 20 after warm-up.

    python tools/time_optim_step.py                        # one JSON line: sgd and adam
    python tools/time_optim_step.py adagrad rprop          # the named methods; "all": the eight of the reference
"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from os2d_amd.engine import optimization as O  # noqa: E402
from os2d_amd.engine.train import get_trainable_parameters  # noqa: E402
from os2d_amd.modeling.model import Os2dModel  # noqa: E402
from os2d_amd.utils import synthetic  # noqa: E402

HBM_COPY = 4.8e12        # bytes / s read + written, tools/hbm_peak.hip
MAX_NORM = 100.0
SETTINGS = dict(lr=1e-3, weight_decay=1e-4)
BYTES = {"sgd": 28, "adam": 36, "adagrad": 28, "adadelta": 36, "adamax": 36, "asgd": 28, "rmsprop": 28, "rprop": 36}
STOCK = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adagrad": torch.optim.Adagrad, "adadelta": torch.optim.Adadelta,
         "adamax": torch.optim.Adamax, "asgd": torch.optim.ASGD, "rmsprop": torch.optim.RMSprop, "rprop": torch.optim.Rprop}
REPS, WARMUP = 20, 5


def parameter_set(device):
    net = Os2dModel(is_cuda=False, merge_branch_parameters=True, backbone_arch="resnet50", use_inverse_geom_model=True, simplify_affine=False)
    net.load_state_dict(synthetic.fill_model_state(net.state_dict(), seed=31, P=6))
    return [p.detach().to(device) for p in get_trainable_parameters(net)]


def make(route, method, shapes_from):
    ps = [p.clone().requires_grad_() for p in shapes_from]
    opt = O.create_optimizer(ps, optim_method=method, sgd_momentum=0.9, on_device=route == "device", **SETTINGS)
    if route == "device":
        return ps, opt, lambda: opt.clip_and_step(MAX_NORM)
    if method in ("sgd", "adam"):          # create_optimizer has no stock route for these two
        opt = torch.optim.SGD(ps, momentum=0.9, **SETTINGS) if method == "sgd" else torch.optim.Adam(ps, **SETTINGS)
    assert type(opt) is STOCK[method]

    def step():
        norm = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, norm_type=2)
        if not np.isnan(float(norm)):
            opt.step()
        return norm
    return ps, opt, step


def launches(fn):
    """(kernel launches of one call, the sum of their durations in us) from torch.profiler; (the reason, None) where the
    profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        if not kernels:
            return "torch.profiler recorded no device events", None
        return len(kernels), float(sum(e.time_range.elapsed_us() for e in kernels))
    except Exception as e:  # noqa: BLE001  (a tool: report, do not hide)
        return "torch.profiler failed: {}".format(e), None


def measure(route, method, params, grads):
    ps, opt, step = make(route, method, params)

    def refill():
        for p, g in zip(ps, grads):
            p.grad = g.clone()        # fresh gradient tensors every step, as zero_grad(set_to_none=True) + backward leave them
    host, dev = [], []
    for i in range(WARMUP + REPS):
        refill()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        a.record()
        step()
        b.record()
        t = time.perf_counter() - t
        b.synchronize()
        if i >= WARMUP:
            host.append(t * 1e6)
            dev.append(a.elapsed_time(b) * 1e3)
    out = dict(host_us=float(np.median(host)), device_us=float(np.median(dev)))
    if route == "device":
        tables = len(opt._plan.tables)
        out["launches"] = 2 * tables + 1 + (0 if method == "sgd" else tables)      # sumsq, update (+ prepare) per table; finalize
    refill()
    out["launches_profiled"], out["kernels_us"] = launches(step)
    return out


def main(methods):
    device = torch.device("cuda:0")
    params = parameter_set(device)
    gen = torch.Generator(device=device).manual_seed(3)
    grads = [torch.randn(p.shape, device=device, generator=gen) * 1e-2 for p in params]
    elements = sum(p.numel() for p in params)
    result = dict(tensors=len(params), elements=elements, hbm_copy_bytes_per_s=HBM_COPY)
    for method in methods:
        for route in ("device", "parent"):
            r = measure(route, method, params, grads)
            if route == "device":
                r["bytes"] = BYTES[method] * elements
                busy = r["kernels_us"] or r["device_us"]      # the events also span the gaps in which the device waits for the host
                r["fraction_of_hbm_copy"] = r["bytes"] / (busy * 1e-6) / HBM_COPY
            result["{}_{}".format(method, route)] = r
    print(json.dumps(result))


if __name__ == "__main__":
    names = [a.lower() for a in sys.argv[1:]] or ["sgd", "adam"]
    if names == ["all"]:
        names = list(BYTES)
    unknown = [a for a in names if a not in BYTES]
    if unknown:
        sys.exit("unknown methods {} (known: {}, or all)".format(unknown, " ".join(BYTES)))
    main(names)
