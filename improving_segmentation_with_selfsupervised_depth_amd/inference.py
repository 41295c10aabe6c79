"""The device part of the reference's inference.py (``Inference.run``, :84-116) and of the image block that ends
``Trainer.validate`` (train.py:904-923): what is done with a forward pass before it becomes files or TensorBoard images.

The reference does this on the host, per image: an int64 argmax map is copied down, ``decode_segmap_tocolor`` makes 19 x 3 mask
passes over float64 planes, ``save_image`` multiplies, adds, clamps and casts, the disparity goes through a second ``save_image`` or
through ``_colorize`` and matplotlib.  Here each output kind is one launch per batch (csrc/render.hip) that leaves on the device
the uint8 image the reference hands to its file writer, byte for byte, and ``write_predictions`` copies each tensor to the host
once.  Config parsing, the data loader, ``MachineConfig`` and the command line stay with the reference.

The package hard-codes no dataset's colours and does not import matplotlib: the palette (``val_loader.label_colours``, Mapillary's
``class_colors[:n_classes]``, CamVid's table) and the colour-map table are arguments."""
import os

import numpy as np
import torch

from . import hipops as H


def render_segmentation(semantics=None, pred=None, label_colors=None, unmapped="keep", return_ids=False):
    """``decode_segmap_tocolor(semantics.data.max(1)[1])`` followed by ``save_image``'s conversion, as uint8 [B,H,W,3].

    semantics: logits [B,C,H,W] (float32, or half precision under autocast; dense NCHW, channels-last or a slice: no copy), or
    pred: class ids [B,H,W] / [H,W], int64 or uint8.  label_colors: [n,3] with n <= 256 -- a tensor, an array, a list, or the
    loaders' ``{id: colour}`` dict.  unmapped: what an id outside 0..n-1 becomes -- ``"keep"`` is Cityscapes' decoder (the id in all
    three channels, clamped to 255), ``"zero"`` the Mapillary / CamVid decoders (black).  return_ids: also the uint8 id plane
    [B,H,W].  A single [H,W] map gives [H,W,3].  Pixels whose logits hold NaN, and negative ids, are unspecified."""
    if label_colors is None:
        raise ValueError("label_colors is required: the package holds no dataset's palette")
    if (semantics is None) == (pred is None):
        raise ValueError("give either semantics (logits) or pred (class ids)")
    if semantics is not None:
        x = semantics.detach()
        if x.dtype in (torch.float16, torch.bfloat16):
            x = x.float()
        return H.render_labels(label_colors, logits=x, unmapped=unmapped, return_ids=return_ids)
    ids = pred.detach()
    single = ids.dim() == 2
    out = H.render_labels(label_colors, ids=ids[None] if single else ids, unmapped=unmapped, return_ids=return_ids)
    if single:
        return (out[0][0], out[1][0]) if return_ids else out[0]
    return out


def render_unit_image(x):
    """torchvision 0.7.0 ``save_image``'s ``x.mul(255).add_(0.5).clamp_(0, 255)`` + uint8 truncation of a float image
    [B,C,H,W] (C = 1 or 3) or [C,H,W] -> uint8 [B,H,W,C] / [H,W,C].  A single-channel image stays one plane (the file holds it
    three times: ``write_predictions`` repeats it)."""
    x = x.detach()
    if x.dtype in (torch.float16, torch.bfloat16):
        x = x.float()
    if x.dim() == 3:
        return H.render_unit_image(x[None])[0]
    return H.render_unit_image(x)


def colorize(img, lut, mask_zero=False, max_percentile=100):
    """The reference's ``_colorize(img, cmap, mask_zero, max_percentile)`` for ``max_percentile == 100`` (all it ever passes), per
    image: img [B,H,W], [B,1,H,W] or [H,W] -> float32 [B,H,W,3] / [H,W,3] (the reference's float64 image rounded to float32).

    lut stands for ``cmap``: float32 [N+3,3] = ``cm(np.arange(N))[:, :3]``, then ``cm.get_under()``, ``cm.get_over()``,
    ``cm.get_bad()`` (three columns each)."""
    if max_percentile != 100:
        raise NotImplementedError("max_percentile = %r: only 100 (np.max) is implemented" % (max_percentile,))
    x = img.detach().float()
    lut = torch.as_tensor(np.asarray(lut, dtype=np.float32)) if not torch.is_tensor(lut) else lut.float()
    if x.dim() == 2:
        return H.colorize(x[None], lut, mask_zero)[0]
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    return H.colorize(x, lut, mask_zero)


def predict_batch(model, monodepth_loss_calculator, inputs_val, label_colors, segmentation=True, monodepth=True, amp=False,
                  unmapped="keep", tta=None):
    """The body of ``Inference.run`` for one batch already on the model's device: the forward pass under ``no_grad`` and
    ``autocast(enabled=amp)``, ``generate_depth_test_pred``, then the renders.  Returns device tensors:
    ``image`` uint8 [B,H,W,3] (the input ``("color_aug", 0, 0)``), ``label`` uint8 [B,H,W,3] and ``pred_ids`` uint8 [B,H,W]
    (None without segmentation), ``depth`` uint8 [B,H,W,1] (the disparity ``("disp", 0)``; None without monodepth), and
    ``outputs``, the model's dict.  The model's mode is the caller's (the reference calls ``model.eval()`` once, before its loop);
    ``functional.frozen_bn_fold()`` applies if the caller is inside it.
    ``tta`` (not in the reference): ``{"scales": [...], "flip": bool, "weights": optional}`` -- ``label`` and ``pred_ids`` are
    then the test-time ensemble of ``evaluation.tta`` at the input size (``hipops.seg_eval_ensemble`` without labels); the forward
    pass above doubles as its (scale 1.0, not flipped) view.  ``outputs`` stays the plain pass."""
    with torch.no_grad():
        with torch.autocast(device_type="cuda", enabled=bool(amp)):
            outputs = model(inputs_val)
        result = {"outputs": outputs, "label": None, "pred_ids": None, "depth": None}
        result["image"] = render_unit_image(inputs_val[("color_aug", 0, 0)])
        if segmentation and tta is not None:
            from .evaluation.tta import ensemble_forward
            views, flips = ensemble_forward(model, inputs_val, tta["scales"], tta.get("flip", False),
                                            base_semantics=outputs["semantics"], amp=amp)
            size = tuple(inputs_val[("color_aug", 0, 0)].shape[-2:])
            ids = H.seg_eval_ensemble(views, flips=flips, weights=tta.get("weights"), size=size)[2]
            result["label"], result["pred_ids"] = H.render_labels(label_colors, ids=ids, unmapped=unmapped), ids
        elif segmentation:
            result["label"], result["pred_ids"] = render_segmentation(semantics=outputs["semantics"], label_colors=label_colors,
                                                                      unmapped=unmapped, return_ids=True)
        if monodepth:
            monodepth_loss_calculator.generate_depth_test_pred(outputs)
            result["depth"] = render_unit_image(outputs[("disp", 0)])
    return result


def write_predictions(result, filenames, logdir):
    """Host helper: the reference's three files per sample -- ``<logdir>/<filename>``, and beside it ``_depth.png`` and
    ``_label.png`` in place of ``.jpg`` -- from the uint8 tensors of ``predict_batch`` (device or CPU), one copy to the host per
    tensor for the whole batch.  Returns the list of paths written."""
    from PIL import Image
    host = {k: result[k].cpu().numpy() for k in ("image", "depth", "label") if result.get(k) is not None}
    written = []
    for i, filename in enumerate(filenames):
        fn = "%s/%s" % (logdir, filename)
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        for key, path in (("image", fn), ("depth", fn.replace(".jpg", "_depth.png")), ("label", fn.replace(".jpg", "_label.png"))):
            if key not in host:
                continue
            a = host[key][i]
            if a.ndim == 2:
                a = a[:, :, None]
            if a.shape[2] == 1:
                a = np.repeat(a, 3, axis=2)      # make_grid repeats a single channel
            Image.fromarray(np.ascontiguousarray(a), "RGB").save(path)
            written.append(path)
    return written
