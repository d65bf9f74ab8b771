"""The OS2D training objective (reference os2d/engine/objective.py) on the HIP kernels of libos2d_train.so:

    loss = ClassificationLoss(cls_preds, cls_targets) + localization_weight * SmoothL1Loss(loc_preds, loc_targets)

``Os2dObjective`` has the reference's constructor and ``forward`` signature and returns its ``OrderedDict``.  The forward is
a short chain of launches (os2d_train_objective_forward), the backward one kernel (os2d_train_objective_backward); counts,
per-label maxima and the hard-negative selection stay on the device, so nothing in a step synchronises with the host.

RLL uses every negative: the reference sets ``neg_to_pos_ratio = inf`` for it and evaluates ``(inf * num_pos).long()``,
which saturates to the largest int64 on a device (and to the smallest on the CPU, where no negative would be used); the
device's behaviour is the one the reference's comment intends and the one implemented here.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import _train_lib
from .._native import STREAM

CLASS_LOSSES = {"contrastiveloss": 0, "rll": 1}
F_POS, F_NEG, F_POSREG = 1, 2, 4        # bits of the per-element flags (include/os2d_train.h)
F_CAND, F_HINGE = 8, 16                 # candidate negative; hinge active for the gradient (clamp argument >= 0)


class _ObjectiveFunction(torch.autograd.Function):
    """(loss, loc, cls, cls_pos, cls_neg) as a [5] tensor + per-element outputs; only element 0 (the loss) carries a gradient."""

    @staticmethod
    def forward(ctx, crit, patch, loc_preds, loc_targets, cls_preds, cls_targets, cls_targets_remapped, cls_preds_for_neg):
        tl = _train_lib.load()
        dev = cls_preds.device
        A, B, HW = cls_preds.shape
        f32 = dict(dtype=torch.float32, device=dev)
        losses = torch.empty(5, **f32)
        cls_loss = torch.empty(A, B, HW, **f32)
        loc_loss = torch.empty(A, B, HW, **f32) if patch else None
        flags = torch.empty(A, B, HW, dtype=torch.uint8, device=dev)
        coef = torch.empty(A, B, HW, **f32)
        ws = torch.empty(int(tl.os2d_train_objective_workspace_floats(A, B, HW)), **f32)
        _train_lib.call("os2d_train_objective_forward", crit._kind, 1 if patch else 0, loc_preds, loc_targets, cls_preds, cls_targets,
                        cls_targets_remapped, cls_preds_for_neg, A, B, HW, crit.margin, crit.margin_pos, crit.class_loss_neg_weight,
                        crit.localization_weight, float(crit.neg_to_pos_ratio), float(crit.rll_neg_weight_ratio), losses, cls_loss,
                        loc_loss, flags, coef, ws, ws.numel(), STREAM)
        ctx.crit, ctx.shape = crit, (A, B, HW)
        ctx.has_neg = cls_preds_for_neg is not None
        ctx.saved = (loc_preds, loc_targets, flags, coef, ws)
        outs = (losses, cls_loss, flags) + ((loc_loss,) if patch else ())
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    def backward(ctx, dlosses, *_):
        crit, (A, B, HW) = ctx.crit, ctx.shape
        loc_preds, loc_targets, flags, coef, ws = ctx.saved
        dev = flags.device
        need_loc, need_cls, need_neg = ctx.needs_input_grad[2], ctx.needs_input_grad[4], ctx.needs_input_grad[7]
        f32 = dict(dtype=torch.float32, device=dev)
        dloc = torch.empty(A, B, 4, HW, **f32) if need_loc else None
        dcls = torch.empty(A, B, HW, **f32) if need_cls else None
        has_neg = ctx.has_neg
        dneg = torch.empty(A, B, HW, **f32) if has_neg else None     # with cls_preds_for_neg the negatives' term goes there
        g = dlosses.contiguous()                                    # element 0 = d loss; the other scalars are for logging
        if need_loc or need_cls or has_neg:
            _train_lib.call("os2d_train_objective_backward", g, loc_preds, loc_targets, flags, coef, ws, A, B, HW,
                            crit.class_loss_neg_weight, crit.localization_weight, dloc, dcls, dneg, STREAM)
        return None, None, dloc, None, dcls, None, None, (dneg if need_neg else None)


class PerAnchorLosses(OrderedDict):
    """The reference's per-anchor dictionary of the patch-mining mode; ``flags`` carries the kernel's flag bytes (bits F_POS,
    F_NEG, F_POSREG) the masks were made from, split like them - what os2d_train_mine_select reads."""
    flags = None


def _apply(*args):
    return _ObjectiveFunction.apply(*args)


class Os2dObjective(nn.Module):
    """reference objective.py:12-313.  Supported classification losses: "ContrastiveLoss", "RLL".

    ``keep_class_loss_on_cpu`` (ours): fill ``class_loss_per_element_detached_cpu`` through a non-blocking copy into pinned
    memory (valid after the stream is synchronised); False leaves the key out."""

    def __init__(self, class_loss, margin, margin_pos, class_loss_neg_weight, remap_classification_targets, localization_weight,
                 neg_to_pos_ratio, rll_neg_weight_ratio, keep_class_loss_on_cpu=True):
        super(Os2dObjective, self).__init__()
        if class_loss.lower() not in CLASS_LOSSES:
            raise RuntimeError("Unknown class_loss: {0}".format(class_loss))
        self.neg_to_pos_ratio = neg_to_pos_ratio
        self.class_loss = class_loss
        self.margin = margin
        self.margin_pos = margin_pos
        self.localization_weight = localization_weight
        self.class_loss_neg_weight = class_loss_neg_weight
        self.rll_neg_weight_ratio = rll_neg_weight_ratio
        self.remap_classification_targets = remap_classification_targets
        self.keep_class_loss_on_cpu = keep_class_loss_on_cpu
        self._kind = CLASS_LOSSES[class_loss.lower()]
        if self._kind == 1:
            self.neg_to_pos_ratio = float("inf")       # RLL does no hard-negative mining: every negative is used

    @staticmethod
    def merge_pyramids(loc_preds, loc_targets, cls_preds, cls_targets, cls_preds_for_neg, cls_targets_remapped):
        """reference objective.py:83-105: pyramid levels given as lists are concatenated along the anchors."""
        if isinstance(cls_targets, torch.Tensor):
            return loc_preds, loc_targets, cls_preds, cls_targets, cls_preds_for_neg, cls_targets_remapped, None
        pyramid_sizes = [t.size(2) for t in cls_targets]

        def cat(ts, dim):
            return None if ts is None else torch.cat(list(ts), dim=dim)
        return (cat(loc_preds, 3), cat(loc_targets, 3), cat(cls_preds, 2), cat(cls_targets, 2), cat(cls_preds_for_neg, 2),
                cat(cls_targets_remapped, 2), pyramid_sizes)

    def loss_names(self):
        """(localisation, class, class positives, class negatives) keys of the returned dictionary."""
        cls, neg = "cls_" + self.class_loss, "cls_" + self.class_loss + "_neg"
        if self.neg_to_pos_ratio != float("inf"):
            suffix = "_hardneg{0}".format(self.neg_to_pos_ratio)
            cls, neg = cls + suffix, neg + suffix
        return "loc_smoothL1", cls, "cls_" + self.class_loss + "_pos", neg

    def forward(self, loc_preds, loc_targets, cls_preds, cls_targets, cls_targets_remapped=None, cls_preds_for_neg=None,
                patch_mining_mode=False):
        """reference objective.py:107-313.  loc_preds / loc_targets [A,B,4,HW], cls_preds [A,B,HW], cls_targets [A,B,HW]
        (1 positive, 0 negative, -1 ignored), all on the HIP device; lists = pyramid levels.  Returns the losses
        (``losses["loss"]`` is the one to backpropagate) and, in patch-mining mode, the per-anchor dictionary as well."""
        loc_preds, loc_targets, cls_preds, cls_targets, cls_preds_for_neg, cls_targets_remapped, pyramid_sizes = \
            self.merge_pyramids(loc_preds, loc_targets, cls_preds, cls_targets, cls_preds_for_neg, cls_targets_remapped)
        dev = cls_preds.device
        for name, t in (("loc_preds", loc_preds), ("loc_targets", loc_targets), ("cls_preds", cls_preds), ("cls_targets", cls_targets),
                        ("cls_targets_remapped", cls_targets_remapped), ("cls_preds_for_neg", cls_preds_for_neg)):
            if t is not None and not (t.is_cuda and t.device == dev):
                raise RuntimeError("Os2dObjective runs on the HIP device only (no CPU fallback): {} is on {}".format(name, t.device))
        A, B, HW = cls_preds.shape
        if tuple(loc_preds.shape) != (A, B, 4, HW) or loc_targets.shape != loc_preds.shape or tuple(cls_targets.shape) != (A, B, HW):
            raise ValueError("inconsistent shapes: loc_preds {}, loc_targets {}, cls_preds {}, cls_targets {}".format(
                tuple(loc_preds.shape), tuple(loc_targets.shape), tuple(cls_preds.shape), tuple(cls_targets.shape)))
        if not self.remap_classification_targets:
            cls_targets_remapped = None

        def f32(t):
            return None if t is None else t.to(torch.float32).contiguous()

        def i64(t):
            return None if t is None else t.to(torch.int64).contiguous()
        outs = _apply(self, bool(patch_mining_mode), f32(loc_preds), f32(loc_targets).detach(), f32(cls_preds), i64(cls_targets),
                      i64(cls_targets_remapped), f32(cls_preds_for_neg))
        scalars, cls_loss, flags = outs[0], outs[1], outs[2]
        loc_name, cls_name, pos_name, neg_name = self.loss_names()
        losses = OrderedDict()
        losses["loss"] = scalars[0]
        if self.keep_class_loss_on_cpu:
            host = torch.empty(cls_loss.shape, dtype=cls_loss.dtype, pin_memory=True)
            host.copy_(cls_loss, non_blocking=True)
            losses["class_loss_per_element_detached_cpu"] = host
        detached = scalars.detach()
        losses[loc_name] = detached[1]
        losses[cls_name] = detached[2]
        losses[pos_name] = detached[3]
        losses[neg_name] = detached[4]
        if not patch_mining_mode:
            return losses
        per_anchor = PerAnchorLosses()
        per_anchor.flags = torch.split(flags, pyramid_sizes, dim=2) if pyramid_sizes else flags
        per_anchor["pos_mask"] = (flags & F_POS) != 0
        per_anchor["neg_mask"] = (flags & F_NEG) != 0
        per_anchor["cls_loss"] = cls_loss
        per_anchor["loc_loss"] = outs[3]
        per_anchor["pos_for_regression"] = (flags & F_POSREG) != 0
        if pyramid_sizes:
            for k in per_anchor:
                per_anchor[k] = torch.split(per_anchor[k], pyramid_sizes, dim=2)
        return losses, per_anchor

    def element_masks(self, loc_preds, loc_targets, cls_preds, cls_targets, cls_targets_remapped=None, cls_preds_for_neg=None,
                      patch_mining_mode=False):
        """(cls_loss, pos_mask, neg_mask, pos_for_regression) [A,B,HW] of a forward: the per-element class loss and the
        masks the backward uses (neg_mask is the set of negatives AFTER hard-negative mining).  For tests and diagnostics."""
        loc_preds, loc_targets, cls_preds, cls_targets, cls_preds_for_neg, cls_targets_remapped, _ = \
            self.merge_pyramids(loc_preds, loc_targets, cls_preds, cls_targets, cls_preds_for_neg, cls_targets_remapped)
        if not self.remap_classification_targets:
            cls_targets_remapped = None
        with torch.no_grad():
            outs = _apply(self, bool(patch_mining_mode), loc_preds.float().contiguous(), loc_targets.float().contiguous(),
                          cls_preds.float().contiguous(), cls_targets.long().contiguous(),
                          None if cls_targets_remapped is None else cls_targets_remapped.long().contiguous(),
                          None if cls_preds_for_neg is None else cls_preds_for_neg.float().contiguous())
        flags = outs[2]
        return outs[1], (flags & F_POS) != 0, (flags & F_NEG) != 0, (flags & F_POSREG) != 0
