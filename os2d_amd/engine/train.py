"""The training step on the HIP head (reference os2d/engine/train.py:47-113 and os2d/modeling/model.py:262-276): the forward
with autograd through the head (os2d_amd/modeling/head_train.py), target remapping, the objective and the optimiser step.
Hard-patch mining, which the reference's V2 recipe alternates with this step, is os2d_amd/engine/mining.py.  Data loading and the
gradient all-reduce of a multi-device run are out of scope."""
import math

import torch

from ..structures.feature_map import FeatureMapSize


def get_trainable_parameters(net):
    return [p for p in net.parameters() if p.requires_grad]


def forward_train(net, images, class_images, fine_tune_features=True):
    """What the reference's ``Os2dModel.forward(train_mode=True)`` does: the feature extractors under
    ``set_grad_enabled(fine_tune_features)``, the head under grad.  -> (loc [A,B,4,HW], cls [A,B,HW], cls_detached [A,B,HW],
    FeatureMapSize, corners [A,B,8,HW]); ``cls_detached`` carries the scores whose gradient does not reach the transformation."""
    with torch.set_grad_enabled(bool(fine_tune_features)):
        feature_maps = net.net_feature_maps(images)
        class_feature_maps = net.net_label_features(class_images)
    with torch.enable_grad():
        class_head = net.os2d_head_creator.create_os2d_head(class_feature_maps)
        loc, cls, cls_det, corners = net.apply_class_heads_to_feature_maps(feature_maps, class_head)
    return loc, cls, cls_det, FeatureMapSize(img=feature_maps), corners


def train_one_batch(net, criterion, optimizer, box_coder, images, class_images, batch_boxes, img_size, loc_targets=None,
                    class_targets=None, max_grad_norm=100.0, fine_tune_features=True, train_transform_on_negs=False):
    """One training iteration (reference train.py:47-113): forward, target remapping, the criterion with
    ``cls_preds_for_neg`` = the transform-detached scores (unless ``train_transform_on_negs``), backward, gradient-norm
    clipping, and an optimiser step unless the norm is NaN.  ``loc_targets`` / ``class_targets`` are the encoded targets of
    the batch; None = encoded here with ``box_coder.encode_batch``.  Returns the criterion's losses with "grad_norm" added
    (device scalars).  An optimiser with ``clip_and_step`` (os2d_amd/engine/optimization.py: DeviceSGD, DeviceAdam, and with
    ``create_optimizer(..., on_device=True)`` the device classes of the reference's other six methods) clips,
    checks and steps on the device over ITS parameters, and nothing here waits for the device; with any other optimiser the
    NaN check of the norm is a host wait, as in the reference."""
    optimizer.zero_grad()
    loc, cls, cls_det, fm_size, _ = forward_train(net, images, class_images, fine_tune_features=fine_tune_features)
    if loc_targets is None or class_targets is None:
        loc_targets, class_targets = box_coder.encode_batch(batch_boxes, img_size, cls.shape[1], cls.device)
    remapped, _, _ = box_coder.remap_anchor_targets(loc, [img_size] * loc.shape[0], None, batch_boxes)
    losses = criterion(loc, loc_targets, cls, class_targets, cls_targets_remapped=remapped,
                       cls_preds_for_neg=None if train_transform_on_negs else cls_det)
    losses["loss"].backward()
    if hasattr(optimizer, "clip_and_step"):
        grad_norm = optimizer.clip_and_step(max_grad_norm)
    else:
        grad_norm = torch.nn.utils.clip_grad_norm_(get_trainable_parameters(net), max_grad_norm, norm_type=2)
        if not math.isnan(float(grad_norm)):
            optimizer.step()
    losses["grad_norm"] = grad_norm
    return losses
