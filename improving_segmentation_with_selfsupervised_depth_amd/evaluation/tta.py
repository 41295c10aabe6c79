"""Test-time ensembling of the segmentation head (not in the reference, which evaluates one view): the views of a batch -- the
input at several scales, each optionally mirrored horizontally -- and one forward pass per view.  Averaging and scoring the views'
logits at label resolution is ``hipops.seg_eval_ensemble`` (``runningScore.update_from_views``, one launch for all views); this
module only makes the views.  Evaluation only: everything runs under ``no_grad``."""
import math

import torch

from .. import hipops as H

IMAGE_KEY = ("color_aug", 0, 0)


def view_sizes(hw, scales, multiple_of=32):
    """(H, W), [s, ...] -> [(h, w), ...]: each scaled side rounded to the nearest multiple of ``multiple_of`` (halves round up),
    at least one multiple -- the encoder-decoder halves its input five times"""
    m = int(multiple_of)
    if m < 1:
        raise ValueError("multiple_of = %r" % (multiple_of,))
    sizes = []
    for s in scales:
        s = float(s)
        if not (s > 0.0 and math.isfinite(s)):
            raise ValueError("scale %r: scales are finite and positive" % (s,))
        sizes.append(tuple(max(m, int(math.floor(side * s / m + 0.5)) * m) for side in (int(hw[0]), int(hw[1]))))
    return sizes


def make_views(images, scales, flip, multiple_of=32):
    """images float [B,3,H,W] -> [(image tensor, flipped), ...]: per scale the resized batch (``hipops.resize_bilinear`` with
    align_corners=False, what the loaders' resize does to a float image) and, with ``flip``, its horizontal mirror right after it.
    A view of the input's own size is the input tensor itself, not a copy."""
    if not (torch.is_tensor(images) and images.dim() == 4):
        raise TypeError("images must be a [B,C,H,W] tensor")
    hw = tuple(int(s) for s in images.shape[-2:])
    views = []
    for size in view_sizes(hw, scales, multiple_of):
        if size == hw:
            img = images
        else:
            nhwc = images.detach().float().permute(0, 2, 3, 1).contiguous()
            img = H.resize_bilinear(nhwc, size, False).permute(0, 3, 1, 2).contiguous()
        views.append((img, False))
        if flip:
            views.append((torch.flip(img, dims=[-1]), True))
    return views


def ensemble_forward(model, inputs, scales, flip, base_semantics=None, amp=False, multiple_of=32):
    """One forward pass per view with ``inputs[("color_aug", 0, 0)]`` replaced by the view -> (list of ``outputs["semantics"]``,
    list of flip flags), in the order of ``make_views``.  Pose prediction is switched off for the passes (``model.use_pose_net``,
    as the unlabeled training step does for the teacher: only the segmentation head is read) and restored afterwards.
    ``base_semantics``: the semantics of a forward pass the caller has already made on the unmodified inputs; it stands for the
    (input size, not flipped) view, which is then not run again.  The model's mode is the caller's."""
    views = make_views(inputs[IMAGE_KEY], scales, flip, multiple_of)
    had_pose = getattr(model, "use_pose_net", None)
    semantics = []
    try:
        if had_pose is not None:
            model.use_pose_net = False
        with torch.no_grad(), torch.autocast(device_type="cuda", enabled=bool(amp)):
            for img, flipped in views:
                if base_semantics is not None and img is inputs[IMAGE_KEY] and not flipped:
                    semantics.append(base_semantics)
                    continue
                view_inputs = dict(inputs)
                view_inputs[IMAGE_KEY] = img
                semantics.append(model(view_inputs)["semantics"])
    finally:
        if had_pose is not None:
            model.use_pose_net = had_pose
    return semantics, [flipped for _, flipped in views]
