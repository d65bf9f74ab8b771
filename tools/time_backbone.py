"""Device-event timing of the backbone's three inference routes (DESIGN.md sections 18 and 18.6), alternated in ONE process:

    python tools/time_backbone.py                         # every configuration, torch / fused / torch again (the spread)
    python tools/time_backbone.py --route all             # torch / fused / fused_conv1x1 / fused again (the spread of "fused") / fused_conv1x1 in bf16x3
    python tools/time_backbone.py --route fused_conv1x1 --precision both      # the two arithmetics of the 1x1 GEMMs
    python tools/time_backbone.py --only r50_960x1280     # one of them
    python tools/time_backbone.py --route fused --only r50_960x1280 --rounds 3      # one route (for a kernel trace)
    python tools/time_backbone.py --stem                  # the two stem variants alone at 960 x 1280
    python tools/time_backbone.py --layers                # os2d_backbone_conv1x1 alone at every 1x1 layer of ResNet50 at 960 x 1280
    python tools/time_backbone.py --layers --precision bf16x3                 # os2d_backbone_conv1x1_bf16x3 at the same layers (or: both)

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


def run_route(ex, route, x, precision="f32"):
    def fn():
        ex.inference_route, ex.conv1x1_precision = route, precision
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
    ap.add_argument("--route", choices=["both", "all", "torch", "fused", "fused_conv1x1"], default="both")
    ap.add_argument("--precision", choices=["f32", "bf16x3", "both"], default="f32", help="the arithmetic of the 1x1 GEMMs of the fused_conv1x1 arm")
    ap.add_argument("--only", action="append", help="configuration name (repeatable); default: all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--stem", action="store_true", help="time the stem variants instead of the routes")
    ap.add_argument("--layers", action="store_true", help="time the 1x1 GEMM of the fused_conv1x1 route layer by layer instead of the routes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_backbone.py needs a HIP device")
    device = torch.device("cuda:0")
    if args.stem:
        return stem(device, args)
    if args.layers:
        return layers(device, args)
    for name, arch, shape in CONFIGS:
        if args.only and name not in args.only:
            continue
        ex = make_extractor(arch, device)
        x = torch.randn(*shape, device=device)
        if args.route == "both":
            arms = [("torch", run_route(ex, "torch", x)), ("fused", run_route(ex, "fused", x)), ("torch_again", run_route(ex, "torch", x))]
        elif args.route == "all":
            arms = [("torch", run_route(ex, "torch", x)), ("fused", run_route(ex, "fused", x)), ("fused_conv1x1", run_route(ex, "fused_conv1x1", x)),
                    ("fused_again", run_route(ex, "fused", x)), ("fused_conv1x1_bf16x3", run_route(ex, "fused_conv1x1", x, "bf16x3"))]
        elif args.route == "fused_conv1x1":
            arms = [("fused_conv1x1" + ("" if q == "f32" else "_" + q), run_route(ex, "fused_conv1x1", x, q))
                    for q in (("f32", "bf16x3") if args.precision == "both" else (args.precision,))]
        else:
            arms = [(args.route, run_route(ex, args.route, x))]
        result = alternate(arms, args.rounds, args.iters)
        record = {"config": name, "arch": arch, "shape": list(shape), "rounds": args.rounds, "iters": args.iters, "ms": result}
        if args.route == "both":
            t = min(result["torch"]["median_ms"], result["torch_again"]["median_ms"])
            record["torch_spread"] = round(abs(result["torch"]["median_ms"] - result["torch_again"]["median_ms"]) / t, 4)
            record["fused_over_torch"] = round(result["fused"]["median_ms"] / t, 4)
        if args.route == "all":
            f = min(result["fused"]["median_ms"], result["fused_again"]["median_ms"])
            record["fused_spread"] = round(abs(result["fused"]["median_ms"] - result["fused_again"]["median_ms"]) / f, 4)
            record["fused_over_torch"] = round(f / result["torch"]["median_ms"], 4)
            record["fused_conv1x1_over_fused"] = round(result["fused_conv1x1"]["median_ms"] / f, 4)
            record["fused_conv1x1_bf16x3_over_fused"] = round(result["fused_conv1x1_bf16x3"]["median_ms"] / f, 4)
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


def layers(device, args):
    """os2d_backbone_conv1x1 with the epilogue of its place in the block, at the input each 1x1 convolution of ResNet50-C4 sees for a
    1 x 3 x 960 x 1280 image (240 x 320 after the stem, halved by layer2 and layer3): median time of a call, the TFLOP/s that time
    implies (2 Cin Cout pixels) and the bytes/s (x, y, the residual and w, each once).  --precision bf16x3 times os2d_backbone_conv1x1_bf16x3
    on the packed weights instead, both the two alternately."""
    from os2d_amd.modeling.backbone_fused import FusedBackbone
    ex = make_extractor("resnet50", device)
    folds = ex.fused_backbone().folds(device)
    packed = ex.fused_backbone().packed_weights(device) if args.precision != "f32" else None
    h, w, seen = 240, 320, set()
    with torch.no_grad():
        for stage in ex.resnet_blocks:
            for block in stage:
                ho, wo = (h - 1) // block.stride + 1, (w - 1) // block.stride + 1
                sites = [("conv1", block.conv1, block.bn1, (h, w), True, False), ("conv3", block.conv3, block.bn3, (ho, wo), True, True)]
                if block.downsample is not None:
                    sites.append(("downsample", block.downsample[0], block.downsample[1], (h, w), False, False))
                for role, conv, bn, (hi, wi), relu, residual in sites:
                    key = (role, conv.in_channels, conv.out_channels, conv.stride[0], hi, wi)
                    if key in seen:
                        continue
                    seen.add(key)
                    x = torch.randn(1, conv.in_channels, hi, wi, device=device)
                    so, wo_ = (hi - 1) // conv.stride[0] + 1, (wi - 1) // conv.stride[0] + 1
                    r = torch.randn(1, conv.out_channels, so, wo_, device=device) if residual else None
                    arms = []
                    if args.precision != "bf16x3":
                        arms.append(("conv1x1", lambda: FusedBackbone._conv1x1(x, conv, folds[id(bn)], relu, r)))
                    if args.precision != "f32":
                        arms.append(("conv1x1_bf16x3", lambda: FusedBackbone._conv1x1(x, conv, folds[id(bn)], relu, r, wp=packed[id(conv)])))
                    times = alternate(arms, args.rounds, 20)
                    pixels = so * wo_
                    flop = 2.0 * conv.in_channels * conv.out_channels * pixels
                    moved = 4.0 * (x.numel() if conv.stride[0] == 1 else conv.in_channels * pixels) + 4.0 * conv.out_channels * pixels * (2 if residual else 1) \
                        + 4.0 * conv.weight.numel()
                    for name, ms in times.items():
                        emit({"config": "layer", "entry": name, "role": role, "Cin": conv.in_channels, "Cout": conv.out_channels, "stride": conv.stride[0],
                              "H": hi, "W": wi, "ms": ms, "tflops": round(flop / ms["median_ms"] / 1e9, 1),
                              "tbytes_per_s": round(moved / ms["median_ms"] / 1e9, 2)}, args.out)
                h, w = ho, wo


if __name__ == "__main__":
    main()
