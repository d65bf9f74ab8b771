"""Inputs of the VOC evaluation tests (tests/golden/voc_eval_*.npz are recorded from the reference on exactly these).

A case is a list of images; an image is a dict of numpy arrays
    pred_boxes [n,4] f32 (in the PREDICTION image size), scores [n] f32, labels [n] i64, pred_size (w, h),
    gt_boxes [m,4] f32, gt_labels [m] i64, difficult [m] u8, gt_size (w, h).
``small`` is written out by hand, the others are drawn from a seed.  tests/golden/make_voc_eval_golden.py asserts that all
scores of a case differ and that no detection's best IoU lies within 1e-5 of a recorded threshold, so the tests demand
equality."""
import numpy as np

THRESHOLDS = (0.5, 0.75)
CASES = ("small", "medium", "resize_equal", "resize_unequal")
NUM_LABELS = dict(small=5, medium=64, resize_equal=8, resize_unequal=8)


def tag(thr):
    return "t{:02d}".format(int(round(thr * 100)))


def _image(pred, gt, pred_size, gt_size=None):
    pred = np.asarray(pred, np.float64).reshape(-1, 6)
    gt = np.asarray(gt, np.float64).reshape(-1, 6)
    return dict(pred_boxes=pred[:, :4].astype(np.float32), scores=pred[:, 4].astype(np.float32), labels=pred[:, 5].astype(np.int64),
                pred_size=tuple(pred_size), gt_boxes=gt[:, :4].astype(np.float32), gt_labels=gt[:, 4].astype(np.int64),
                difficult=gt[:, 5].astype(np.uint8), gt_size=tuple(gt_size or pred_size))


def small():
    """3 images, 5 labels.  Label 0: duplicated ground-truth boxes (first argmax) and several detections on one box; label 1:
    ground truth without detections; label 2: detections without ground truth; label 3: only difficult boxes; label 4: a
    difficult and a plain box.  Image 1 has no detections, image 2 no ground truth."""
    im0 = _image(
        # x1, y1, x2, y2, score, label
        [[10, 10, 50, 50, 0.90, 0], [12, 11, 52, 49, 0.95, 0], [9, 12, 47, 51, 0.40, 0],      # three on the duplicated box
         [100, 100, 140, 150, 0.65, 0], [104, 108, 150, 160, 0.70, 0],                        # the better-scored one: IoU 0.53
         [200, 20, 260, 90, 0.80, 2], [30, 200, 80, 260, 0.30, 2],                            # label without ground truth
         [300, 300, 350, 360, 0.85, 3], [302, 303, 352, 357, 0.20, 3],                        # on a difficult box
         [400, 50, 460, 120, 0.60, 4], [402, 52, 462, 118, 0.55, 4], [500, 400, 560, 470, 0.50, 4], [0, 0, 5, 5, 0.10, 4]],
        # x1, y1, x2, y2, label, difficult
        [[10, 10, 50, 50, 0, 0], [10, 10, 50, 50, 0, 0], [100, 100, 140, 150, 0, 0],
         [600, 10, 630, 40, 1, 0],
         [300, 300, 350, 360, 3, 1],
         [400, 50, 460, 120, 4, 1], [500, 400, 560, 470, 4, 0]],
        (640, 480))
    im1 = _image([], [[20, 20, 90, 80, 0, 0], [50, 60, 120, 160, 1, 0], [200, 200, 260, 280, 3, 1]], (500, 375))
    im2 = _image([[15, 25, 75, 95, 0.75, 0], [210, 190, 270, 260, 0.45, 2], [300, 40, 380, 100, 0.35, 4]], [], (320, 240))
    return [im0, im1, im2]


def _drawn(seed, n_images, n_labels, n_det, pred_scale=(1.0, 1.0)):
    """Detections = jittered ground truth (mostly the right label) + random false positives; scores are a permutation of an
    evenly spaced grid (all different), higher on average for the jittered boxes."""
    rng = np.random.RandomState(seed)
    images = []
    for _ in range(n_images):
        w, h = int(rng.randint(320, 800)), int(rng.randint(240, 600))
        m = int(rng.randint(2, 9))
        x1, y1 = rng.uniform(0, w - 120, m), rng.uniform(0, h - 120, m)
        bw, bh = rng.uniform(30, 110, m), rng.uniform(30, 110, m)
        gt = np.stack([x1, y1, x1 + bw, y1 + bh], 1)
        gt_labels = rng.randint(0, n_labels, m)
        difficult = (rng.rand(m) < 0.15).astype(np.uint8)
        boxes, labels, hot = [], [], []
        for g in range(m):
            for _ in range(int(rng.randint(1, 4))):
                jitter = rng.uniform(-0.18, 0.18, 4) * np.array([bw[g], bh[g], bw[g], bh[g]])
                boxes.append(gt[g] + jitter)
                labels.append(gt_labels[g] if rng.rand() < 0.9 else rng.randint(0, n_labels))
                hot.append(1.0)
        while len(boxes) < n_det:
            fx, fy = rng.uniform(0, w - 60), rng.uniform(0, h - 60)
            boxes.append(np.array([fx, fy, fx + rng.uniform(10, 120), fy + rng.uniform(10, 120)]))
            labels.append(rng.randint(0, n_labels))
            hot.append(0.0)
        images.append(dict(pred_boxes=np.array(boxes), labels=np.array(labels, np.int64), hot=np.array(hot), gt_boxes=gt.astype(np.float32),
                           gt_labels=gt_labels.astype(np.int64), difficult=difficult, gt_size=(w, h)))
    raw = np.concatenate([im["hot"] * 0.5 + rng.rand(len(im["hot"])) for im in images])
    rank = np.argsort(np.argsort(raw))
    scores = (0.01 + 0.98 * (rank + 0.5) / len(raw)).astype(np.float32)
    start = 0
    for im in images:
        n = len(im.pop("hot"))
        im["scores"] = scores[start:start + n]
        start += n
        w, h = im["gt_size"]
        im["pred_size"] = (int(round(w * pred_scale[0])), int(round(h * pred_scale[1])))
        ratio = np.array([im["pred_size"][0] / w, im["pred_size"][1] / h] * 2)
        im["pred_boxes"] = (im["pred_boxes"] * ratio).astype(np.float32)
    return images


def case(name):
    if name == "small":
        return small()
    if name == "medium":
        return _drawn(41, 40, 64, 150)
    if name == "resize_equal":
        return _drawn(42, 6, 8, 30, pred_scale=(2.0, 2.0))
    if name == "resize_unequal":
        return _drawn(43, 6, 8, 30, pred_scale=(2.0, 1.5))
    raise KeyError(name)


def boxlists(images, BoxList, FeatureMapSize, device=None):
    """(predictions, ground truth) as lists of BoxList of the given classes; predictions on ``device`` when given, ground
    truth on the host."""
    import torch
    preds, gts = [], []
    for im in images:
        p = BoxList(torch.from_numpy(im["pred_boxes"]).reshape(-1, 4), FeatureMapSize(w=im["pred_size"][0], h=im["pred_size"][1]))
        p.add_field("scores", torch.from_numpy(im["scores"]))
        p.add_field("labels", torch.from_numpy(im["labels"]))
        g = BoxList(torch.from_numpy(im["gt_boxes"]).reshape(-1, 4), FeatureMapSize(w=im["gt_size"][0], h=im["gt_size"][1]))
        g.add_field("labels", torch.from_numpy(im["gt_labels"]))
        g.add_field("difficult", torch.from_numpy(im["difficult"]))
        preds.append(p.to(device) if device is not None else p)
        gts.append(g)
    return preds, gts


def large(seed=7, n_images=2000, n_labels=1024, n_det=1000, n_gt=8):
    """The shape too large to record (torch tensors on the host, packed): boxes [N,n,4], scores, labels and ground truth
    [N,m,4], labels, difficult; all images 1000 x 1000.  A third of the detections are jittered ground truth."""
    import torch
    g = torch.Generator().manual_seed(seed)
    N, n, m = n_images, n_det, n_gt
    xy = torch.rand(N, m, 2, generator=g) * 850
    wh = 30 + torch.rand(N, m, 2, generator=g) * 110
    gt = torch.cat([xy, xy + wh], 2)
    gt_labels = torch.randint(0, n_labels, (N, m), generator=g)
    difficult = (torch.rand(N, m, generator=g) < 0.15).to(torch.uint8)
    src = torch.randint(0, m, (N, n), generator=g)
    hot = torch.rand(N, n, generator=g) < 0.33
    jit = (torch.rand(N, n, 4, generator=g) - 0.5) * 0.4 * torch.gather(wh, 1, src.unsqueeze(2).expand(-1, -1, 2)).repeat(1, 1, 2)
    near = torch.gather(gt, 1, src.unsqueeze(2).expand(-1, -1, 4)) + jit
    fxy = torch.rand(N, n, 2, generator=g) * 850
    far = torch.cat([fxy, fxy + 10 + torch.rand(N, n, 2, generator=g) * 120], 2)
    boxes = torch.where(hot.unsqueeze(2), near, far).float()
    labels = torch.where(hot, torch.gather(gt_labels, 1, src), torch.randint(0, n_labels, (N, n), generator=g))
    scores = ((torch.randperm(N * n, generator=g).double() + 0.5) / (N * n)).float().reshape(N, n)
    return dict(boxes=boxes, scores=scores, labels=labels, gt_boxes=gt.float(), gt_labels=gt_labels, difficult=difficult, size=(1000, 1000))
