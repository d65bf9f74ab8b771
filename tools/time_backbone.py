"""Device-event timing of the backbone's two inference routes, alternated in ONE process:

    python tools/time_backbone.py                         # every configuration, torch / fused / torch again (the spread)
    python tools/time_backbone.py --only r50_960x1280     # one of them
    python tools/time_backbone.py --route fused --only r50_960x1280 --rounds 3      # one route (for a kernel trace)
    python tools/time_backbone.py --stem                  # the two stem variants alone at 960 x 1280

One JSON line per configuration on stdout (and appended to --out): the median and the minimum over --rounds rounds of the mean
time of --iters calls.  Random weights and perturbed BatchNorms: the time does not depend on the values."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PYRAMID = [(640, 480), (800, 600), (1024, 768), (1280, 960), (1536, 1152), (1792, 1344), (2048, 1536)]      # (w, h) of engine/pyramid.py
CONFIGS = [("r50_960x1280", "resnet50", (1, 3, 960, 1280)), ("r101_960x1280", "resnet101", (1, 3, 960, 1280)),
           ("r50_64x240x240", "resnet50", (64, 3, 240, 240))]
CONFIGS += [("r50_level_{}x{}".format(h, w), "resnet50", (1, 3, h, w)) for w, h in PYRAMID if (w, h) != (1280, 960)]


def timed(fn, iters):
    """mean milliseconds of `iters` calls between two device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(arms, rounds, iters):
    """arms: [(name, callable)].  Every round runs every arm once, in order: drift of the clock falls on all alike."""
    for _, fn in arms:
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            times[name].append(timed(fn, iters))
    return {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for name, v in times.items()}


def make_extractor(arch, device):
    from os2d_amd.modeling.feature_extractor import build_feature_extractor
    torch.manual_seed(0)
    ex = build_feature_extractor(arch)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in ex.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
    return ex.to(device).eval()


def run_route(ex, route, x):
    def fn():
        ex.inference_route = route
        with torch.no_grad():
            return ex(x)
    return fn


def emit(record, out):
    line = json.dumps(record)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["both", "torch", "fused"], default="both")
    ap.add_argument("--only", action="append", help="configuration name (repeatable); default: all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--stem", action="store_true", help="time the stem variants instead of the routes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_backbone.py needs a HIP device")
    device = torch.device("cuda:0")
    if args.stem:
        return stem(device, args)
    for name, arch, shape in CONFIGS:
        if args.only and name not in args.only:
            continue
        ex = make_extractor(arch, device)
        x = torch.randn(*shape, device=device)
        if args.route == "both":
            arms = [("torch", run_route(ex, "torch", x)), ("fused", run_route(ex, "fused", x)), ("torch_again", run_route(ex, "torch", x))]
        else:
            arms = [(args.route, run_route(ex, args.route, x))]
        result = alternate(arms, args.rounds, args.iters)
        record = {"config": name, "arch": arch, "shape": list(shape), "rounds": args.rounds, "iters": args.iters, "ms": result}
        if args.route == "both":
            t = min(result["torch"]["median_ms"], result["torch_again"]["median_ms"])
            record["torch_spread"] = round(abs(result["torch"]["median_ms"] - result["torch_again"]["median_ms"]) / t, 4)
            record["fused_over_torch"] = round(result["fused"]["median_ms"] / t, 4)
        emit(record, args.out)
        del ex, x
        torch.cuda.empty_cache()


def stem(device, args):
    """conv1 (MIOpen) + os2d_backbone_bn_relu_maxpool against the torch stem (conv1, bn1, relu, maxpool) at 960 x 1280."""
    from os2d_amd.modeling.backbone_fused import FusedBackbone
    ex = make_extractor("resnet50", device)
    runner = ex.fused_backbone()
    x = torch.randn(1, 3, 960, 1280, device=device)
    fold = runner.folds(device)[id(ex.bn1)]
    with torch.no_grad():
        arms = [("torch_stem", lambda: ex.maxpool(ex.relu(ex.bn1(ex.conv1(x))))),
                ("conv1_only", lambda: ex.conv1(x)),
                ("conv1_then_pool_kernel", lambda: FusedBackbone._bn_relu_maxpool(ex.conv1(x), fold))]
        emit({"config": "stem_960x1280", "rounds": args.rounds, "iters": args.iters, "ms": alternate(arms, args.rounds, args.iters)}, args.out)


if __name__ == "__main__":
    main()
