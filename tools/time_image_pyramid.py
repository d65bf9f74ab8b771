"""Times the image pyramid built on the HIP device from a uint8 image (libos2d_image.so) at 1280x960 and the seven default
scales: per level, the whole pyramid, a batch of 4; torch's own path on the same GPU (uint8 -> float, ``F.interpolate`` bilinear
with antialias per level, normalisation - float arithmetic, not bit-compatible with PIL: a speed comparator only); the host
path it replaces when Pillow is importable (seven ``Image.BILINEAR`` resizes + tensor conversion, 1 and 16 threads); and
``evaluate`` per image from uint8 images against host-built pyramids with the synthetic model at 64 classes.  HIP events,
median of 10 after warm-up.

    python tools/time_image_pyramid.py                 # one JSON line
    python tools/time_image_pyramid.py --no-evaluate   # the pyramid timings only
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import image_model as M  # noqa: E402
from os2d_amd.engine import evaluate as E  # noqa: E402
from os2d_amd.engine.image_pyramid import IMAGENET_NORMALIZATION, ImagePyramidBuilder  # noqa: E402
from os2d_amd.engine.pyramid import DEFAULT_SCALES  # noqa: E402
from os2d_amd.structures.bounding_box import BoxList  # noqa: E402
from os2d_amd.structures.feature_map import FeatureMapSize  # noqa: E402

HBM_PEAK = 8e12         # bytes / s, the figure DESIGN.md uses


def median_ms(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def host_median_ms(fn, reps=5):
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times))


def torch_pyramid(img_u8, sizes, mean, std):
    x = img_u8.permute(0, 3, 1, 2).float().div(255)
    return [(F.interpolate(x, size=(s.h, s.w), mode="bilinear", antialias=True, align_corners=False) - mean) / std for s in sizes]


def host_paths(img, result):
    try:
        from PIL import Image
    except ImportError:
        result["host_pil"] = None
        return None
    from concurrent.futures import ThreadPoolExecutor
    pil = Image.fromarray(img)
    sizes = M.pyramid_sizes(pil.size[0], pil.size[1])
    mean = torch.tensor(IMAGENET_NORMALIZATION["mean"])[:, None, None]
    std = torch.tensor(IMAGENET_NORMALIZATION["std"])[:, None, None]

    def level(size):
        return torch.from_numpy(np.array(pil.resize(size, Image.BILINEAR))).permute(2, 0, 1).float().div(255).sub_(mean).div_(std)

    for threads in (1, 16):
        torch.set_num_threads(threads)
        with ThreadPoolExecutor(threads) as pool:
            result["host_pil_resizes_only_{}t".format(threads)] = host_median_ms(
                lambda: list(pool.map(lambda s: pil.resize(s, Image.BILINEAR), sizes)))
            result["host_pil_resizes_and_tensors_{}t".format(threads)] = host_median_ms(lambda: list(pool.map(level, sizes)))
    result["host_pil"] = "Pillow {} on this machine's CPU".format(__import__("PIL").__version__)
    return lambda im: [level(s)[None] for s in M.pyramid_sizes(im.shape[1], im.shape[0])]


def time_evaluate(dev, result, host_pyramid):
    from os2d_amd.modeling.model import Os2dModel
    from os2d_amd.utils import synthetic
    torch.manual_seed(3)
    net = Os2dModel(is_cuda=False, merge_branch_parameters=True, backbone_arch="resnet50", use_inverse_geom_model=True, simplify_affine=False)
    net.os2d_head_creator.aligner.parameter_regressor.load_state_dict(synthetic.make_transform_net_state(6, seed=3))
    net.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    n_classes, n_images, w, h = 64, 4, 640, 480
    class_ids = list(range(n_classes))
    head = E.build_class_head(net, [torch.randn(3, 240, 240, generator=g).to(dev) for _ in class_ids])
    coder = net.build_box_coder()
    images = [np.random.RandomState(90 + i).randint(0, 256, size=(h, w, 3)).astype(np.uint8) for i in range(n_images)]
    if host_pyramid is not None:
        pyramids = [[x for x in host_pyramid(im)] for im in images]
    else:
        pyramids = [[torch.from_numpy(x) for x in M.pyramid(im)] for im in images]
    gts = []
    for _ in images:
        b = BoxList(torch.tensor([[10.0, 10.0, 100.0, 100.0]]), FeatureMapSize(w=w, h=h))
        b.add_field("labels", torch.tensor([0]))
        gts.append(b)
    orig = [FeatureMapSize(w=w, h=h)] * n_images
    raw = [torch.from_numpy(im) for im in images]

    def run(items, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        E.evaluate(net, coder, items, gts, head, class_ids, orig_sizes=orig, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / n_images

    raw_kw = dict(pyramid_scales=DEFAULT_SCALES, img_normalization=IMAGENET_NORMALIZATION)
    run(pyramids), run(raw, **raw_kw)           # warm-up of both
    result["evaluate"] = dict(
        shape="{} classes, {} images of {}x{}, 7 scales".format(n_classes, n_images, w, h), unit="ms per image, median of 5 runs",
        host_pyramids=float(np.median([run(pyramids) for _ in range(5)])),
        uint8_images=float(np.median([run(raw, **raw_kw) for _ in range(5)])),
        h2d_bytes_per_image_host_pyramids=int(sum(x.numel() * 4 for x in pyramids[0])),
        h2d_bytes_per_image_uint8=int(raw[0].numel()))


def main():
    if not torch.cuda.is_available():
        raise RuntimeError("needs a HIP device")
    dev = torch.device("cuda:0")
    w, h = 1280, 960
    img = np.random.RandomState(0).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    one = torch.from_numpy(img).to(dev)
    four = one.unsqueeze(0).repeat(4, 1, 1, 1).contiguous()
    result = dict(shape="{}x{} uint8, scales {}".format(w, h, list(DEFAULT_SCALES)), unit="ms, median of 10")
    builder = ImagePyramidBuilder(device=dev)
    sizes = builder.sizes(FeatureMapSize(w=w, h=h))
    per_level = {}
    for s, size in zip(DEFAULT_SCALES, sizes):
        single = ImagePyramidBuilder(scales=(s,), device=dev)
        ms = median_ms(lambda: single.build(one))
        written = 3 * 4 * size.w * size.h
        per_level[str(s)] = dict(ms=ms, bytes_written=written, fraction_of_hbm_peak=written / (ms * 1e-3) / HBM_PEAK)
    result["hip_per_level"] = per_level
    total = sum(3 * 4 * s.w * s.h for s in sizes)
    for name, x, A in (("hip_pyramid", one, 1), ("hip_pyramid_batch4", four, 4)):
        ms = median_ms(lambda: builder.build(x))
        result[name] = dict(ms=ms, bytes_written=A * total, fraction_of_hbm_peak=A * total / (ms * 1e-3) / HBM_PEAK)
    mean = torch.tensor(IMAGENET_NORMALIZATION["mean"], device=dev)[None, :, None, None]
    std = torch.tensor(IMAGENET_NORMALIZATION["std"], device=dev)[None, :, None, None]
    result["torch_interpolate_pyramid"] = median_ms(lambda: torch_pyramid(one[None], sizes, mean, std))
    result["torch_interpolate_pyramid_batch4"] = median_ms(lambda: torch_pyramid(four, sizes, mean, std))
    host_pyramid = host_paths(img, result)
    if "--no-evaluate" not in sys.argv:
        time_evaluate(dev, result, host_pyramid)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
