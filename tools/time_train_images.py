#!/usr/bin/env python3
"""Time the training-image chain on the device against the same chain with Pillow on the host.

    python tools/time_train_images.py [--out FILE.json] [--images 4] [--repeats 10]

A batch is 4 random uint8 images of 1280x960 with three boxes each and the reference's V2 training settings: random crop to
600x600 with scale jitter 0.7 and aspect jitter 0.9, random interpolation, colour distortion, flips.  Every repeat replays the
same seeds, so every repeat does the same work; for the colour numbers a seed is chosen whose draws apply all four operations.

Measured with HIP events around the enqueued work, median of ``--repeats`` after 3 warm-up runs (tables uploaded, library
loaded): each kernel alone on one image, and the whole chain per batch (also as wall-clock time with a final synchronisation:
the host's share - the crop search and the draws - is in it).  The Pillow chain does what the reference's dataloader does per
image (transpose, crop, resize, ColorJitter's operations, ToTensor, Normalize) with the same windows, filters and factors, on
one thread and with the batch's images on four threads.  Pillow is needed by this tool only, not by the package.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from os2d_amd.engine import image_pyramid as IP  # noqa: E402
from os2d_amd.engine.augmentation import DataAugmentation, transform_image_to_pyramid  # noqa: E402
from os2d_amd.structures import transforms as T  # noqa: E402
from os2d_amd.structures.bounding_box import BoxList  # noqa: E402
from os2d_amd.structures.feature_map import FeatureMapSize  # noqa: E402

W, H, CROP = 1280, 960, 600
BOXES = [[100.0, 120.0, 420.0, 400.0], [600.0, 300.0, 900.0, 700.0], [950.0, 500.0, 1200.0, 900.0]]


def augmentation():
    return DataAugmentation(random_flip_batches=True, random_crop_size=FeatureMapSize(w=CROP, h=CROP), random_crop_scale=1.0,
                            jitter_aspect_ratio=0.9, scale_jitter=0.7, random_color_distortion=True, random_crop_label_images=False,
                            min_box_coverage=0.7)


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def plan(seed, hflip, vflip):
    """the draws of one image without touching it: (window in the flipped image, crop filter, colour chain, level filter)"""
    seed_all(seed)
    aug = augmentation()
    size = FeatureMapSize(w=W, h=H)
    view = T.DeviceImage(torch.empty(H, W, 3, dtype=torch.uint8, device="cuda"))
    view, boxes = T.transpose(view, hflip=hflip, vflip=vflip, boxes=BoxList(torch.tensor(BOXES), size))
    view = aug.random_crop(view, boxes=boxes)[0]
    return view.window, T.choose_filter(True), aug.draw_distortion(), T.choose_filter(True)


def find_seeds(flips):
    """per image the next seed whose colour draws apply all four operations (the costly case)"""
    out = []
    seed = 0
    for hflip, vflip in flips:
        while len(plan(seed, hflip, vflip)[2]) != 4:
            seed += 1
        out.append(seed)
        seed += 1
    return out


def device_batch(images, seeds, flips):
    out = []
    for img, seed, (hflip, vflip) in zip(images, seeds, flips):
        seed_all(seed)
        out.append(transform_image_to_pyramid(img, BoxList(torch.tensor(BOXES), FeatureMapSize(w=W, h=H)), augmentation(), hflip=hflip, vflip=vflip))
    return out


def event_ms(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times, walls = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        times.append(a.elapsed_time(b))
    return dict(event_ms_median=statistics.median(times), event_ms_min=min(times), event_ms_max=max(times), wall_ms_median=statistics.median(walls))


def host_ms(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(wall_ms_median=statistics.median(times), wall_ms_min=min(times), wall_ms_max=max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(1)
    host_images = [rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(args.images)]
    images = [torch.from_numpy(x).to(dev) for x in host_images]
    flips = [(bool(i & 1), bool(i & 2)) for i in range(args.images)]
    seeds = find_seeds(flips)
    plans = [plan(s, *f) for s, f in zip(seeds, flips)]
    result = dict(device=torch.cuda.get_device_name(0), image=[W, H], crop=CROP, images=args.images, repeats=args.repeats, seeds=seeds,
                  plans=[dict(window=p[0], crop_filter=p[1], color_ops=p[2], level_filter=p[3]) for p in plans])

    # ---- each kernel alone, on image 0 with its plan's window
    window = plans[0][0]
    size = FeatureMapSize(w=CROP, h=CROP)
    kernels = {}
    for name in IP.RANDOM_INTERPOLATION_FILTERS:
        kernels["resample_padded_u8_" + name] = event_ms(lambda: IP.resize_image(images[0], size, crop_xyxy=window, filter=name, pad=True), args.repeats)
    cropped = IP.resize_image(images[0], size, crop_xyxy=window, pad=True)
    ops = plans[0][2]
    kernels["color_4ops_u8"] = event_ms(lambda: IP.distort_image(cropped, ops), args.repeats)
    kernels["color_4ops_float"] = event_ms(lambda: IP.distort_image(cropped, ops, to_float=True), args.repeats)
    kernels["color_no_contrast_float"] = event_ms(lambda: IP.distort_image(cropped, [o for o in ops if o[0] != IP.CONTRAST], to_float=True), args.repeats)
    kernels["color_hue_only_u8"] = event_ms(lambda: IP.distort_image(cropped, [(IP.HUE, 0.05)]), args.repeats)
    builder = IP.ImagePyramidBuilder((1.0,), device=dev)
    kernels["level_same_size_float"] = event_ms(lambda: builder.build(cropped), args.repeats)
    result["kernels"] = kernels

    # ---- the whole chain per batch
    result["device_chain_per_batch"] = event_ms(lambda: device_batch(images, seeds, flips), args.repeats)
    pinned = [torch.from_numpy(x).pin_memory() for x in host_images]
    result["device_chain_per_batch_with_upload"] = event_ms(lambda: device_batch(pinned, seeds, flips), args.repeats)

    # ---- Pillow on this machine's CPU
    try:
        import PIL
        result["pillow_version"] = PIL.__version__
        torch.set_num_threads(1)
        work = list(zip(host_images, plans, flips))
        on_device = [out[0][0].cpu() for out in device_batch(images, seeds, flips)]
        result["pillow_equals_device"] = all(torch.equal(a, pillow_image(*w)) for a, w in zip(on_device, work))
        result["pillow_one_thread_per_batch"] = host_ms(lambda: [pillow_image(*a) for a in work], args.repeats)
        with ThreadPoolExecutor(max_workers=4) as pool:
            result["pillow_four_threads_per_batch"] = host_ms(lambda: list(pool.map(lambda a: pillow_image(*a), work)), args.repeats)
    except ImportError:
        result["pillow_version"] = None
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def pillow_image(image, planned, flips):
    """what the reference's dataloader does to one image with PIL, with the draws made beforehand (no shared generator: the
    batch's images can run on threads)"""
    from PIL import Image, ImageEnhance
    names = dict(box=Image.BOX, nearest=Image.NEAREST, hamming=Image.HAMMING, bicubic=Image.BICUBIC, lanczos=Image.LANCZOS, bilinear=Image.BILINEAR)
    window, crop_filter, ops, _ = planned
    hflip, vflip = flips
    img = Image.fromarray(image)
    if hflip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    img = img.crop(window).resize((CROP, CROP), names[crop_filter])
    for kind, f in ops:
        if kind == IP.BRIGHTNESS:
            img = ImageEnhance.Brightness(img).enhance(f)
        elif kind == IP.CONTRAST:
            img = ImageEnhance.Contrast(img).enhance(f)
        elif kind == IP.SATURATION:
            img = ImageEnhance.Color(img).enhance(f)
        else:
            h, s, v = img.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.int32(f * 255).astype(np.uint8)
            img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    x = torch.from_numpy(np.array(img, np.uint8, copy=True)).permute(2, 0, 1).contiguous().float().div(255)
    mean = torch.as_tensor(IP.IMAGENET_NORMALIZATION["mean"])[:, None, None]
    std = torch.as_tensor(IP.IMAGENET_NORMALIZATION["std"])[:, None, None]
    return x.sub_(mean).div_(std)


if __name__ == "__main__":
    main()
