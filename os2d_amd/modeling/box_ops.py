"""Box-op chains: what a box transform of the reference (a ``TransformList`` of BoxList.resize / transpose / crop closures)
amounts to, recorded as a chain of (kind, ax, ay) operations that the HIP kernels apply op by op with the reference's roundings
(``os2d_apply_box_ops`` of csrc/detect_common.h).  Decode, target assignment, ``BoxGridGenerator.get_box_to_cut_anchor`` and
engine/mining.py all hand their transforms to the kernels through this module.

    _BoxTrace                                             reference bounding_box.py:138-226 (resize / transpose / crop)
    transform_level_boxes                                 reference box_coder.py:509-521
    trace_box_transform                                   the closures of reference structures/transforms.py:12-52, called at
                                                          box_coder.py:499-503
    traced_box_ops / as_box_ops                           the transforms of reference box_coder.py:250-254, 352-354, 439-446
"""
import collections
import weakref
import ctypes

import torch

from ..structures.feature_map import FeatureMapSize
from ..structures.bounding_box import BoxList, FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM

OP_SCALE, OP_HFLIP, OP_VFLIP, OP_SHIFT = 1, 2, 3, 4   # OS2D_BOX_OP_* of include/os2d_hip.h
MAX_BOX_OPS = 6                                       # OS2D_BOX_MAX_OPS
MAX_DEFAULT_BOX_OPS = 12                              # OS2D_BOX_MAX_DEFAULT_OPS


class ResizeBoxes(object):
    """``inverse_box_transforms`` entry that maps a level's boxes to ``target_size`` (what the reference's
    ``TransformList`` inverse amounts to for a resized image, box_coder.py:499-503): ``boxlist.resize(target_size)``.
    (Any entry made of BoxList.resize / transpose / crop calls - this class, the reference's ``TransformList`` of lambdas -
    reaches the fused decode kernels: ``trace_box_transform`` records the chain.)"""

    def __init__(self, target_size):
        self.target_size = target_size

    def __call__(self, boxlist):
        return boxlist.resize(self.target_size)

    def ratios(self, img_size):
        return float(self.target_size.w) / img_size.w, float(self.target_size.h) / img_size.h


class _BoxTrace(object):
    """Stand-in for a ``BoxList`` that RECORDS what an ``inverse_box_transforms`` entry does to it.  The reference hands
    ``decode_pyramid`` one ``TransformList`` of closures per level (os2d/structures/transforms.py:12-27; the closures are
    ``lambda boxes: boxes.resize(size)`` / ``boxes.transpose(FLIP_*)`` / ``boxes.crop(uncrop_xyxy)``, appended by
    transforms.py:32-52, 78-79, 188-191 from os2d/data/dataloader.py:286-336) and calls it on BoxLists
    (os2d/modeling/box_coder.py:499-503).  Called on this object instead, the same closures leave the exact sequence of
    operations with their parameters - which the fused decode kernels then apply op by op with the reference's roundings
    (a numerical probe could only recover the composite map, not where it rounds).  Anything else a closure might touch
    (``bbox_xyxy``, fields, ...) is not defined here: the AttributeError sends the caller to the generic chain."""

    def __init__(self, image_size, ops=(), fields=None):
        self.image_size = image_size
        self.ops = tuple(ops)
        self.extra_fields = dict(fields or {})     # name -> _BoxTrace (BoxList-valued fields: "default_boxes")

    def add_field(self, field, field_data):
        self.extra_fields[field] = field_data

    def get_field(self, field):
        return self.extra_fields[field]

    def has_field(self, field):
        return field in self.extra_fields

    def resize(self, target_size):                      # BoxList.resize, reference bounding_box.py:138-163
        op = (OP_SCALE, float(target_size.w) / self.image_size.w, float(target_size.h) / self.image_size.h)
        return _BoxTrace(target_size, self.ops + (op,), self.extra_fields)          # fields are copied AS THEY ARE (:162)

    def transpose(self, method):                        # reference bounding_box.py:165-200
        if method == FLIP_LEFT_RIGHT:
            op = (OP_HFLIP, float(self.image_size.w), 0.0)
        elif method == FLIP_TOP_BOTTOM:
            op = (OP_VFLIP, 0.0, float(self.image_size.h))
        else:
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        # BoxList-valued fields are flipped too, each inside ITS OWN image (:196-199)
        return _BoxTrace(self.image_size, self.ops + (op,), {k: v.transpose(method) for k, v in self.extra_fields.items()})

    def crop(self, box):                                # reference bounding_box.py:202-226
        size = FeatureMapSize(w=box[2] - box[0], h=box[3] - box[1])
        return _BoxTrace(size, self.ops + ((OP_SHIFT, float(box[0]), float(box[1])),),
                         {k: v.crop(box) for k, v in self.extra_fields.items()})


def apply_box_ops(boxes, ops):
    """The recorded chain on a [n,4] xyxy tensor with the arithmetic of the BoxList methods (one float32 rounding per
    product / difference) - what os2d_apply_box_ops does on the device."""
    x1, y1, x2, y2 = boxes.unbind(1)
    for kind, ax, ay in ops:
        if kind == OP_SCALE:
            x1, y1, x2, y2 = x1 * ax, y1 * ay, x2 * ax, y2 * ay
        elif kind == OP_HFLIP:
            x1, x2 = ax - x2, ax - x1
        elif kind == OP_VFLIP:
            y1, y2 = ay - y2, ay - y1
        else:
            x1, y1, x2, y2 = x1 - ax, y1 - ay, x2 - ax, y2 - ay
    return torch.stack([x1, y1, x2, y2], dim=1)


_PROBE_BOXES = ((0.0, 0.0, 1.0, 1.0), (13.25, 7.5, 211.0, 95.75), (3.0, 250.5, 640.125, 479.0))


def transform_level_boxes(transform, boxes, default_boxes, corners, img_size):
    """What reference box_coder.py:509-521 does with a level's ``inverse_box_transforms`` entry, on plain tensors:
    boxes [n,4] -> transform(boxes); the anchors ride along as the BoxList FIELD "default_boxes" (BoxList.transpose / crop
    transform BoxList-valued fields as well, each inside its own image; resize copies them as they are) and the transform is
    applied to that field once more afterwards; the corners [m,4] go through as boxes of their own.  For a resize-only chain
    (the evaluation's) all three see the same map; with flips / crops the anchors see them twice - reproduced as is, so that
    a caller of the reference gets the reference's numbers.  Returns (boxes, default_boxes, corners or None, output size)."""
    bl = BoxList(boxes, img_size)
    bl.add_field("default_boxes", BoxList(default_boxes, img_size))
    out = transform(bl)
    dflt = transform(out.get_field("default_boxes"))
    cor = transform(BoxList(corners, img_size)).bbox_xyxy if corners is not None else None
    return out.bbox_xyxy, dflt.bbox_xyxy, cor, out.image_size


def trace_box_transform(transform, img_size):
    """-> (box ops, anchor ops, output image size) of one ``inverse_box_transforms`` entry applied to a level on an image of
    ``img_size`` (see ``transform_level_boxes`` for why the anchors have a chain of their own), or None when the entry is not a
    chain of BoxList.resize / transpose / crop - then only the generic decode can run it.  ``None`` entries trace to empty
    chains.  The recorded chains are checked against the entry itself on three probe boxes (unit, generic, near the border):
    bit-equal coordinates and the same output size, or they are not used."""
    if transform is None:
        return (), (), img_size
    # Two steps: the TRACE (the closures run on _BoxTrace objects: no tensors, a few Python calls) is made on every call, the
    # PROBE CHECK (three closure runs on CPU BoxLists) only once per (callable, image size, traced chains).  Keyed on the chains
    # themselves, a hit cannot be stale: a TransformList that was appended to (whatever the attribute its list lives in - the
    # reference keeps it in ``_transforms``, structures/transforms.py:18-22), or a closure whose captured state changed, traces to
    # other chains and is probed again (round 5 keyed on object identity + an attribute named ``transforms`` only).
    # The cache holds WEAK references: it keeps no transform (nor what it captured) alive, a dead entry's id may be reused and
    # is then not a hit; callables that cannot be weakly referenced are not cached.
    traced = _trace_chains(transform, img_size)
    if traced is None:
        return None
    try:
        ref = weakref.ref(transform)
    except TypeError:
        return traced if _probe_check(transform, img_size, traced) else None
    ckey = (id(transform), int(img_size.w), int(img_size.h), traced[0], traced[1], int(traced[2].w), int(traced[2].h))
    hit = _TRACE_CACHE.get(ckey)
    if hit is not None and hit[0]() is transform:
        _TRACE_CACHE.move_to_end(ckey)
        return traced if hit[1] else None
    ok = _probe_check(transform, img_size, traced)
    _TRACE_CACHE[ckey] = (ref, ok)
    while len(_TRACE_CACHE) > 64:
        _TRACE_CACHE.popitem(last=False)
    return traced if ok else None


_TRACE_CACHE = collections.OrderedDict()


def _trace_chains(transform, img_size):
    """(box ops, anchor ops, output size) recorded by running the entry on _BoxTrace objects, or None."""
    try:
        root = _BoxTrace(img_size)
        root.add_field("default_boxes", _BoxTrace(img_size))
        traced = transform(root)
        if not isinstance(traced, _BoxTrace) or len(traced.ops) > MAX_BOX_OPS:
            return None
        anchors = transform(traced.get_field("default_boxes"))
        if not isinstance(anchors, _BoxTrace) or len(anchors.ops) > MAX_DEFAULT_BOX_OPS:
            return None
    except Exception:   # noqa: BLE001 - a closure that does anything else than the three BoxList operations
        return None
    return traced.ops, anchors.ops, traced.image_size


def _probe_check(transform, img_size, traced):
    """The recorded chains against the entry itself on the probe boxes: bit-equal coordinates and the same output size."""
    try:
        probe = torch.tensor(_PROBE_BOXES, dtype=torch.float32)
        b, d, c, size = transform_level_boxes(transform, probe.clone(), probe.clone() + 0.5, probe.clone(), img_size)
        return bool(size == traced[2] and torch.equal(b, apply_box_ops(probe, traced[0])) and torch.equal(c, b)
                    and torch.equal(d, apply_box_ops(probe + 0.5, traced[1])))
    except Exception:   # noqa: BLE001
        return False


def _trace_box_transform(transform, img_size):
    """Uncached trace + probe check (tests)."""
    traced = _trace_chains(transform, img_size)
    return traced if traced is not None and _probe_check(transform, img_size, traced) else None


def ops_tables(ops_per_level, width=MAX_BOX_OPS):
    """ctypes tables (counts [L], kinds [L][width], args [L][width][2]) of os2d_detect_level_ops / os2d_detect_pyramid_ops."""
    L = len(ops_per_level)
    counts = (ctypes.c_int * L)(*[len(o) for o in ops_per_level])
    kinds = (ctypes.c_int * (L * width))()
    args = (ctypes.c_float * (L * width * 2))()
    for l, ops in enumerate(ops_per_level):
        for k, (kind, ax, ay) in enumerate(ops):
            kinds[l * width + k] = kind
            args[(l * width + k) * 2] = ax
            args[(l * width + k) * 2 + 1] = ay
    return counts, kinds, args


_ops_tables = ops_tables   # for importers of the private name


def traced_box_ops(transform, img_size):
    """-> (box-op chain, output image size) of a box transform of the target / mining code, recorded by ``trace_box_transform``;
    ValueError when the transform is not a chain of at most MAX_BOX_OPS BoxList.resize / transpose / crop calls."""
    traced = trace_box_transform(transform, img_size)
    if traced is None:
        raise ValueError("the box transform is not a chain of at most {} BoxList.resize / transpose / crop calls: the HIP kernels "
                         "cannot express it".format(MAX_BOX_OPS))
    return traced[0], traced[2]


def as_box_ops(transform, img_size):
    """A transform of the target code as a box-op chain: a callable is traced, a sequence of (kind, ax, ay) is taken as it is."""
    if isinstance(transform, (tuple, list)):
        ops = tuple((int(k), float(ax), float(ay)) for k, ax, ay in transform)
        if len(ops) > MAX_BOX_OPS or any(k not in (OP_SCALE, OP_HFLIP, OP_VFLIP, OP_SHIFT) for k, _, _ in ops):
            raise ValueError("a box-op chain has at most {} entries of kind 1..4, got {}".format(MAX_BOX_OPS, ops))
        return ops
    return traced_box_ops(transform, img_size)[0]
