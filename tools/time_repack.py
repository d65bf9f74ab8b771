"""Time the re-pack of the split-fp16 TransformNet weights after a parameter change: ``TransformationNet.packed("f16x3")``
right after an in-place ``add_(0)`` on linear.bias (what an optimiser step does to the caches), with the range plan on the
"torch" route (``range_plan``: a chain of float64 torch operators), on the "device" route (one os2d_train_range_plan call) and on
"torch" again in one process - the two torch figures show the spread of the box.

    python tools/time_repack.py [--reps 50] [--warmup 5] [--P 6]

Wall-clock time (``time.perf_counter``) between two stream synchronisations: the cost the device route removes is host time -
operators launched one by one with the host in between - which device events would not see.  Per route: the median, the
fastest and the slowest of ``--reps`` calls after ``--warmup`` untimed ones, in microseconds.  ``gain_us`` = the faster torch
median - the device median; ``spread_us`` = the difference of the two torch medians; ``clears_bar``: gain > 10 * spread.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=6)
    a = ap.parse_args()
    from os2d_amd.modeling.head import TransformationNet
    from os2d_amd.utils import synthetic

    dev = torch.device("cuda:0")
    net = TransformationNet(output_dim=a.P)
    net.load_state_dict(synthetic.make_transform_net_state(a.P, seed=3))
    net.to(dev).eval()
    stream = torch.cuda.current_stream(dev)

    def repack_us():
        with torch.no_grad():
            net.linear.bias.add_(0)
        stream.synchronize()
        t0 = time.perf_counter()
        net.packed("f16x3")
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6

    res = {"P": a.P, "reps": a.reps, "warmup": a.warmup}
    for key, route in (("torch", "torch"), ("device", "device"), ("torch_again", "torch")):
        net.range_plan_route = route
        for _ in range(a.warmup):
            repack_us()
        ts = sorted(repack_us() for _ in range(a.reps))
        res[key] = {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}
    torch_medians = (res["torch"]["median_us"], res["torch_again"]["median_us"])
    res["gain_us"] = round(min(torch_medians) - res["device"]["median_us"], 1)
    res["spread_us"] = round(abs(torch_medians[0] - torch_medians[1]), 1)
    res["clears_bar"] = bool(res["gain_us"] > 10 * res["spread_us"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
