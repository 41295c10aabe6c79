"""Mirror of loss/loss.py: cross_entropy2d on the fused HIP log-softmax + NLL kernels (reads NHWC logits in place:
the reference's NCHW -> (NHW, C) transpose copy, loss.py:25, disappears)."""
import torch

from .. import functional as Fn
from .. import hipops as H

IGNORE_INDEX = 250


class _CrossEntropyFn(Fn.Function):
    @staticmethod
    def forward(ctx, logits, target, class_weight, pixel_weights, mean_over_all):
        logits = Fn._c(logits)
        target = target.contiguous()
        out = H.cross_entropy_forward(logits, target, IGNORE_INDEX, class_weight, pixel_weights)
        M = target.numel()
        den = torch.full((), float(M), device=logits.device) if mean_over_all else out[1]
        ctx.save_for_backward(logits, target, class_weight, pixel_weights, den)
        return out[0] / den

    @staticmethod
    def backward(ctx, g):
        logits, target, cw, pw, den = ctx.saved_tensors
        scale = (g / den).reshape(1).contiguous()
        return H.cross_entropy_backward(logits, target, IGNORE_INDEX, scale, cw, pw), None, None, None, None


@Fn.fp32_region
def cross_entropy2d(input, target, class_weight=None, pixel_weights=None):
    """reference loss.py:17-37.  input: [N,C,H,W] logits (NCHW-logical), target: int64 [N,Ht,Wt]."""
    n, c, h, w = input.size()
    nt, ht, wt = target.size()
    x = Fn.to_nhwc(input)
    if h != ht and w != wt:
        x = Fn.resize_bilinear(x, (ht, wt), align_corners=True)
    mean_over_all = False
    if pixel_weights is not None:
        mean_over_all = True          # reduction="none" followed by torch.mean over every pixel (loss.py:28-36)
        # reference loss.py:29-31 checks the weights for NaN on the host (a device sync per call).  Weights made by
        # hipops.pseudo_label (count / total, a finite number by construction) carry a marker and skip that check.
        if not getattr(pixel_weights, "_segsde_finite", False) and torch.any(torch.isnan(pixel_weights)):
            print("WARN cross_entropy2d pixel_weights contains NaN. Skip weighting.")
            pixel_weights = None
        else:
            pixel_weights = pixel_weights.detach().reshape(-1).float().contiguous()
    return _CrossEntropyFn.apply(x, target.reshape(-1), class_weight, pixel_weights, mean_over_all)


class _BerHuFn(Fn.Function):
    """hipops.berhu_forward / berhu_backward (csrc/berhu.hip).  Nothing but the operands and the two floats {max, C} is kept for the
    backward pass, which recomputes; the gradient goes to ``input`` only."""

    @staticmethod
    def forward(ctx, input, target, mask, keep_rows, apply_log):
        loss, state = H.berhu_forward(input, target, mask, keep_rows, apply_log)
        ctx.save_for_backward(input, target, mask, state)
        ctx.keep_rows, ctx.apply_log = keep_rows, apply_log
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        input, target, mask, state = ctx.saved_tensors
        dx = H.berhu_backward(input, target, state, g.detach().float().reshape(1), mask, ctx.keep_rows, ctx.apply_log)
        if dx.shape != input.shape:           # input was broadcast against a larger target / mask
            dx = dx.sum_to_size(input.shape)
        return dx.to(input.dtype), None, None, None, None


def _berhu(input, target, mask, keep_rows, apply_log):
    if not torch.is_tensor(input) or not torch.is_tensor(target):
        raise TypeError("berhu: input and target must be tensors")
    if mask is not None and not torch.is_tensor(mask):
        mask = torch.as_tensor(mask, dtype=torch.float32, device=input.device)
    if torch.is_grad_enabled() and (target.requires_grad or (mask is not None and mask.requires_grad)):
        raise NotImplementedError("berhu: the gradient goes to `input` only; detach the target and the mask")
    return _BerHuFn.apply(input, target, mask, keep_rows, bool(apply_log))


@Fn.fp32_region
def berhu(input, target, mask, apply_log=False):
    """reference loss.py:5-15, the pseudo-depth distillation loss: a = |target - input| * mask (log(1 + .) of both first with
    ``apply_log``), C = 0.2 max(a), mean over every element of a where a <= C, else (a^2 + C^2) / (2 C) -> 0-dim tensor on the
    device.  Three HIP launches forward, one backward, and no host synchronisation: the reference's read of the maximum on the host
    is gone, C stays on the device (a constant for the gradient, as the reference's detached float is).  The gradient goes to
    ``input`` only: a ``target`` or ``mask`` that requires grad raises NotImplementedError.  The operands are broadcast against
    each other; one that is not dense float32 afterwards costs a copy.
    Deviation: when max(a) == 0 (target == input on every unmasked element) the loss is 0 and the gradient all zeros; the
    reference returns NaN gradients there (the 0/0 of ``torch.where``'s unselected branch).  NaN inputs are unspecified."""
    return _berhu(input, target, mask, None, apply_log)


@Fn.fp32_region
def berhu_own_car(input, target, apply_log=False, keep=0.9):
    """``berhu`` with the mask both callers build (train.py:491-494, 871-874: ones with the rows from ``int(H * 0.9)`` on zeroed,
    the ego vehicle at the bottom of the frame) derived from the element index inside the kernels: no mask tensor is allocated
    or read.  ``input``: [.., H, W]; bit for bit the result of ``berhu`` with that mask."""
    return _berhu(input, target, None, int(input.shape[-2] * keep), apply_log)


def pixel_wise_entropy(logits, normalize=False):
    """reference loss.py:40-47: -sum_c p log2(p + 1e-30) / log2(C) of the class softmax -> [N,H,W], one pass of the score kernel
    of csrc/labelsel.hip over the logits in whatever layout they have (forward only).  ``normalize``: (e - min) / (max - min)
    over the whole tensor."""
    assert logits.dim() == 4
    ent = H.labelsel_score(logits.detach().float(), want_maps=True)[1]
    if normalize:
        ent = H.minmax_normalize(ent.reshape(1, -1)).reshape(ent.shape)
    return ent


def feature_distance(a, b):
    """``torch.dist(outputs["encoder_features"], outputs["imnet_features"], p=2)`` of the feature-distance term (train.py:480-483)
    on the HIP kernels: deterministic, the result a 0-dim tensor on the device"""
    return Fn.feature_distance(a, b)
