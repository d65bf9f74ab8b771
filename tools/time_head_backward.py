"""Time the training step of the head at the reference training shape (A = 4 images, B = 15 classes, C = 1024, 38 x 38):
the HIP training forward (the "f32" or the "f16x3" route with its intermediates kept) and the HIP backward pass
(libos2d_train.so), against the same step done eagerly by torch: the oracle's ``head_forward`` under autograd on the same GPU.

    python tools/time_head_backward.py [--reps N] [--no-eager] [--A 4 --B 15 --C 1024 --H 38 --W 38]
                                       [--train-precision f32|f16x3|both] [--deterministic off|on|both]
                                       [--train-forward-precision f32|f16x3|both] [--live-bn]

A training step changes the TransformNet parameters, so the packed weights (and, on the f16x3 forward, the range plan) are
rebuilt every step: every timed iteration first bumps a parameter's version (an in-place ``add_(0)`` on linear.bias) inside the
timed region - ``hip_forward_ms``; ``hip_forward_cached_pack_ms`` is the same forward without the bump (packed weights cached).
``forward_peak_bytes``: what one forward adds to ``torch.cuda.max_memory_allocated`` (intermediates and outputs included).
``--train-forward-precision``: the arithmetic of the training forward (default: $OS2D_TRAIN_FORWARD_PRECISION, else "f32");
``both`` runs everything below under f32, f16x3 and f32 again in one process (keys ``forward_f32``, ``forward_f16x3``,
``forward_f32_again``) - the two f32 figures show the spread of the box.

``--train-precision``: the arithmetic of the backward GEMMs (default: $OS2D_TRAIN_PRECISION, else "f32"); ``both`` times
f32, f16x3 and f32 again in one process - the two f32 figures show the spread of the box.
``--deterministic``: the d corr scatter of the decode backward (default: what the head resolves, see
``head_train.resolve_deterministic``); ``both`` times off, on and off again in one process, under the one train precision given
(or each of the three runs of ``--train-precision both``) - the two "off" figures show the spread of the box.
``--live-bn``: after the figures above (the BatchNorms of the TransformNet frozen, as always), the same figures with both of
them in training mode - batch statistics, DESIGN.md section 16 - under key ``live_bn``, in the same process; the eager column
then has ``eager_live_forward_ms`` / ``eager_live_backward_ms`` too: the oracle with ``F.batch_norm(training=True)``.
Per-kernel times: run it under ``rocprofv3 --kernel-trace --stats -- python tools/time_head_backward.py --reps 1 --no-eager``.
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--A", type=int, default=4)
    ap.add_argument("--B", type=int, default=15)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--H", type=int, default=38)
    ap.add_argument("--W", type=int, default=38)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--train-precision", choices=["f32", "f16x3", "both"], default=None)
    ap.add_argument("--deterministic", choices=["off", "on", "both"], default=None)
    ap.add_argument("--train-forward-precision", choices=["f32", "f16x3", "both"], default=None)
    ap.add_argument("--live-bn", action="store_true")
    a = ap.parse_args()
    from os2d_amd.modeling.head import build_os2d_head_creator
    from os2d_amd.structures.feature_map import FeatureMapSize
    from os2d_amd.utils import synthetic
    from oracle import head_oracle as O

    dev = torch.device("cuda:0")
    state = synthetic.make_transform_net_state(6, seed=3)
    creator = build_os2d_head_creator(False, False, True, FeatureMapSize(w=16, h=16), FeatureMapSize(w=16, h=16))
    creator.aligner.parameter_regressor.load_state_dict(state)
    creator.to(dev).eval()
    fm = synthetic.make_feature_map(a.C, a.H, a.W, seed=5, A=a.A).to(dev).requires_grad_(True)
    raws = [c.to(dev).requires_grad_(True) for c in synthetic.make_class_feature_maps(a.B, a.C, sizes=[(15, 15), (20, 24)], seed=9)]
    g = torch.Generator().manual_seed(1)
    gl = torch.randn(a.A, a.B, 4, a.H, a.W, generator=g).to(dev)
    gc = torch.randn(a.A, a.B, 1, a.H, a.W, generator=g).to(dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            out = fn(e1)
            e2.record()
            torch.cuda.synchronize()
            ts.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
            del out
        ts.sort(key=lambda t: t[0] + t[1])
        return ts[len(ts) // 2]

    bias = creator.aligner.parameter_regressor.linear.bias

    def hip_step(mid=None, bump=True):
        if bump:                        # what an optimizer step does to the caches: the packed weights are stale
            with torch.no_grad():
                bias.add_(0)
        head = creator.create_os2d_head(raws)
        loc, cls, cls_det, _ = head(fm)
        if mid is not None:
            mid.record()
        ((loc * gl).sum() + (cls * gc).sum() + (cls_det * gc).sum()).backward()
        return loc

    def figures():
        fwd, bwd = timed(hip_step)
        cached, _ = timed(lambda mid=None: hip_step(mid, bump=False))
        return {"hip_forward_ms": round(fwd, 3), "hip_backward_ms": round(bwd, 3), "hip_step_ms": round(fwd + bwd, 3),
                "hip_forward_cached_pack_ms": round(cached, 3)}

    def timed_step():
        """One timing of hip_step under the creator's settings; with --deterministic both: off, on, off."""
        if a.deterministic != "both":
            creator.deterministic = None if a.deterministic is None else a.deterministic == "on"
            return figures()
        out = {}
        for key, flag in (("off", False), ("on", True), ("off_again", False)):
            creator.deterministic = flag
            out["deterministic_" + key] = figures()
        return out

    def forward_peak_bytes():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = creator.create_os2d_head(raws)(fm)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        return int(peak)

    def under_forward_precision():
        """Everything --train-precision / --deterministic ask for, under the creator's train_forward_precision."""
        out = {}
        if a.train_precision == "both":
            for key, precision in (("f32", "f32"), ("f16x3", "f16x3"), ("f32_again", "f32")):
                creator.train_precision = precision
                out[key] = timed_step()
        else:
            creator.train_precision = a.train_precision
            out.update(timed_step())
        head = creator.create_os2d_head(raws)
        head(fm)
        out["train_forward_precision"] = head.last_train_forward_precision
        if a.train_precision != "both":
            out["train_precision"] = head.last_train_precision
            if a.deterministic != "both":
                out["deterministic"] = head.last_deterministic
        out["forward_peak_bytes"] = forward_peak_bytes()
        return out

    def under_every_forward_precision(res):
        if a.train_forward_precision == "both":
            for key, precision in (("forward_f32", "f32"), ("forward_f16x3", "f16x3"), ("forward_f32_again", "f32")):
                creator.train_forward_precision = precision
                res[key] = under_forward_precision()
        else:
            creator.train_forward_precision = a.train_forward_precision
            res.update(under_forward_precision())
        return res

    res = under_every_forward_precision({"shape": [a.A, a.B, a.C, a.H, a.W]})
    if a.live_bn:
        net = creator.aligner.parameter_regressor
        net.train()                     # both BatchNorms on batch statistics
        res["live_bn"] = under_every_forward_precision({})
        net.eval()
    if not a.no_eager:
        st = {k: v.to(dev).requires_grad_(k.endswith("weight") or k.endswith("bias")) for k, v in state.items()}

        import torch.nn.functional as F

        def live_transform_net(corr, state):
            """oracle.transform_net with both BatchNorms in training mode (they update the running statistics, as the head does)."""
            x = O.l2_normalize_channels(F.relu(corr), 1e-6)
            for conv, bn, pad in (("conv.0", "conv.1", 3), ("conv.3", "conv.4", 2)):
                x = F.conv2d(x, state[conv + ".weight"], state[conv + ".bias"], padding=pad)
                x = F.relu(F.batch_norm(x, state[bn + ".running_mean"], state[bn + ".running_var"], state[bn + ".weight"],
                                        state[bn + ".bias"], training=True, momentum=0.1, eps=O.BN_EPS))
            return F.conv2d(x, state["linear.weight"], state["linear.bias"], padding=2)

        def eager_step(mid=None):
            with torch.device(dev):          # the oracle builds its grids / masks with default-device factories
                q = O.prepare_class_maps(raws)
                loc, cls, cls_det, _ = O.head_forward(fm, q, st, True)
            if mid is not None:
                mid.record()
            ((loc * gl).sum() + (cls * gc).sum() + (cls_det * gc).sum()).backward()
            return loc
        frozen_transform_net = O.transform_net
        try:
            efwd, ebwd = timed(eager_step)
            res.update({"eager_forward_ms": round(efwd, 3), "eager_backward_ms": round(ebwd, 3)})
            if a.live_bn:
                O.transform_net = live_transform_net        # head_forward looks the function up in its module
                efwd, ebwd = timed(eager_step)
                res.update({"eager_live_forward_ms": round(efwd, 3), "eager_live_backward_ms": round(ebwd, 3)})
        except RuntimeError as e:       # report, do not hide: the comparison point is missing
            res["eager_error"] = str(e)[:300]
        finally:
            O.transform_net = frozen_transform_net
    print(json.dumps(res))


if __name__ == "__main__":
    main()
