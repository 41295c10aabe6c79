"""Mirror of loader/transformmasks.py mask builders + the depthcomp mask of Trainer.generate_mix_mask
(train.py:585-604), each one HIP kernel, bit-exact (comparisons only), and the masks of the other modes of that method for a whole
batch (train.py:573-584 "class", 605-615 "depth", 616-636 "depthhist"; csrc/mixmask.hip)."""
import numpy as np
import torch

from .. import hipops as H


def generate_cutout_mask(img_size, seed=None):
    """transformmasks.py:8-24 (CutMix-style box mask; unused by the reference's trainer, kept for scripts that import it):
    host-side numpy like the reference -- a [H, W] float64 array of ones with one zeroed box of half the image area, drawn
    from numpy's global generator after ``np.random.seed(seed)`` (same draws, same order: bit-identical masks)."""
    np.random.seed(seed)
    area = img_size[0] * img_size[1] / 2
    w = np.random.randint(img_size[1] / 2, img_size[1] + 1)
    h = np.round(area / w)
    x0 = np.random.randint(0, img_size[1] - w + 1)
    y0 = np.random.randint(0, img_size[0] - h + 1)
    mask = np.ones(img_size)
    mask[y0:int(y0 + h), x0:int(x0 + w)] = 0
    return mask.astype(float)


def generate_class_mask(pred, classes):
    """transformmasks.py:27-30 -> int64, same shape as pred"""
    return H.class_mask(pred, classes)


def generate_depth_mask(depth, threshold):
    """transformmasks.py:33-41"""
    if threshold.shape[0] == 1:
        return H.depth_threshold_mask(depth.float(), float(threshold[0]))
    if threshold.shape[0] == 2:
        return H.depth_threshold_mask(depth.float(), float(torch.min(threshold)), float(torch.max(threshold)), True)
    raise NotImplementedError


def _stacked(mask, depths):
    """the shape ``torch.cat`` of the per-image masks has: [B,1,H,W] depths give [B,H,W]"""
    return mask.reshape((depths.shape[0] * depths.shape[1],) + tuple(depths.shape[2:]))


def generate_depth_masks(depths, thresholds):
    """``torch.cat([generate_depth_mask(depths[i], thresholds[i:i+1]) for i in range(B)])`` in one launch (train.py:605-615).
    depths: [B,1,H,W]; thresholds: float32 [B], a host tensor (uploaded once, the host does not wait) or a device tensor."""
    depths = depths.float()
    if thresholds.device != depths.device:
        thresholds = H.upload(thresholds, depths.device)
    return _stacked(H.depth_threshold_mask_batch(depths, thresholds), depths)


def generate_depthhist_mask(depths, u=None, return_table=False):
    """The "depthhist" mask of train.py:616-636 for the whole batch, nothing copied to the host: per image the threshold
    u * (max_depth - min_depth) + min_depth from the 100-bin density histogram of log(1 + depth) (hipops.depth_hist_thresholds
    restates np.histogram in fp32), applied to the depth itself like the reference does.  depths: [B,1,H,W] -> float32 [B,H,W].
    ``u``: float32 [B]; by default one ``torch.rand(1)`` per image from the host generator, in image order (the reference's
    draws, the same numbers the "depth" mode consumes).  Where the reference fails or silently reuses the previous image's
    max_depth -- no bin below the top one with a density above 1.5 -- max_depth is that of the image before it in the batch, for
    the first image the top edge; ``return_table`` also returns the [B,4] table {min_depth, max_depth, threshold, found}."""
    depths = depths.float()
    if u is None:
        u = torch.cat([torch.rand(1) for _ in range(depths.shape[0])])
    if u.device != depths.device:
        u = H.upload(u, depths.device)
    table, _ = H.depth_hist_thresholds(depths, u, apply_log=True)
    mask = _stacked(H.depth_threshold_mask_batch(depths, table[:, 2]), depths)
    return (mask, table) if return_table else mask


def generate_class_mix_masks(argmax_u_w):
    """The ClassMix masks of train.py:573-584 for the whole batch: argmax_u_w int64 [B,H,W] -> int64 [B,H,W].  One presence
    count on the device, ONE copy of B x 256 counters to the host, there per image in order the reference's draw -- the ids that
    are present in ascending order without 250, n of them, np.random.choice(n, int((n - n % 2) / 2), replace=False) from numpy's
    global generator, called also when it selects nothing -- then one upload of the selection and one mask launch.  Class ids
    -1 .. 254 (hipops.pseudo_label writes -1 for ignore_index = -1); other ids count as absent."""
    counts = H.class_presence(argmax_u_w).cpu().numpy()
    selected = np.zeros(counts.shape, dtype=np.uint8)
    for i in range(counts.shape[0]):
        classes = np.nonzero(counts[i])[0] - 1
        classes = classes[classes != 250]
        n = classes.shape[0]
        pick = np.random.choice(n, int((n - n % 2) / 2), replace=False)
        selected[i, classes[pick] + 1] = 1
    return H.class_mask_batch(argmax_u_w, H.upload(torch.from_numpy(selected), argmax_u_w.device))


def generate_depthcomp_mask(depths, margin, foreground_threshold):
    """train.py:585-604 with partner (i+1) % B (identical to the reference at its asserted batch size 2).
    depths: [B,1,H,W] min-max-normalised disparities -> int64 [B,H,W]."""
    return H.depthcomp_mask(depths.float(), margin, foreground_threshold)
