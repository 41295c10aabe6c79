"""Mirror of evaluation/metrics.py ``runningScore`` with the confusion matrix accumulated on the
device: the reference copies predictions and labels to the host every validation batch and runs ``np.bincount`` per
image (metrics.py:12-25, train.py:848-851); here ``update`` is one kernel (optionally fused with the class argmax,
``update_from_logits``) into a device-resident int64 histogram, copied to the host only when the scores are read."""
import numpy as np
import torch

from .. import _lib
from .. import hipops as H


class runningScore(object):
    def __init__(self, n_classes):
        self.n_classes = n_classes
        self._host = np.zeros((n_classes, n_classes))      # contributions that arrived as numpy arrays
        self._dev = None

    def _hist(self, device):
        if self._dev is None or self._dev.device != device:
            assert self._dev is None, "runningScore was updated from two devices"
            self._dev = torch.zeros(self.n_classes * self.n_classes, dtype=torch.int64, device=device)
        return self._dev

    @property
    def confusion_matrix(self):
        """float64 [n, n] like the reference's attribute (metrics.py:10)"""
        m = self._host.copy()
        if self._dev is not None:
            m += self._dev.cpu().numpy().reshape(self.n_classes, self.n_classes).astype(np.float64)
        return m

    def _fast_hist(self, label_true, label_pred, n_class):
        """metrics.py:12-17 (host fallback for numpy inputs)"""
        mask = (label_true >= 0) & (label_true < n_class)
        return np.bincount(n_class * label_true[mask].astype(int) + label_pred[mask], minlength=n_class ** 2).reshape(
            n_class, n_class)

    def update(self, label_trues, label_preds):
        """metrics.py:19-25; device tensors stay on the device"""
        if torch.is_tensor(label_trues) and torch.is_tensor(label_preds) and (label_trues.is_cuda or _lib.HOST_POINTERS_OK):
            H.confusion_update(self._hist(label_trues.device), label_trues.detach(), pred=label_preds.detach())
            return
        if torch.is_tensor(label_trues):
            label_trues = label_trues.detach().cpu().numpy()
        if torch.is_tensor(label_preds):
            label_preds = label_preds.detach().cpu().numpy()
        for lt, lp in zip(label_trues, label_preds):
            self._host += self._fast_hist(lt.flatten(), lp.flatten(), self.n_classes)

    def update_from_logits(self, label_trues, semantics, return_loss=False, return_ids=False):
        """train.py:839-851 in one kernel: ``pred = semantics.data.max(1)[1]`` fused with the histogram.  Labels of another size
        than the logits: the logits are interpolated to the label grid inside the kernel (``hipops.seg_eval``: the reference's
        ``F.interpolate(..., mode="bilinear", align_corners=True)`` without the resized tensor).  ``return_loss``: also the value
        of the reference's ``cross_entropy2d(input=semantics, target=label_trues)`` without class or pixel weights, its resize
        included, from the same pass -- a 0-dim float32 tensor on the device, NaN when no pixel counts.  ``return_ids``: also the
        prediction as a uint8 [B,Ht,Wt] plane.  Returns None, the loss, the ids, or (loss, ids).  No host synchronisation."""
        if not (return_loss or return_ids) and tuple(label_trues.shape[-2:]) == tuple(semantics.shape[-2:]):
            H.confusion_update(self._hist(semantics.device), label_trues.detach(), logits=semantics.detach())
            return None
        _, pair, ids = H.seg_eval(semantics.detach(), label_trues.detach(), hist=self._hist(semantics.device),
                                  want_loss=return_loss, want_ids=return_ids)
        loss = (pair[0] / pair[1]).float() if return_loss else None
        return (loss, ids) if return_loss and return_ids else (loss if return_loss else ids)

    def update_from_views(self, label_trues, views, flips=None, weights=None, return_loss=False, return_ids=False):
        """Test-time ensembling (not in the reference, which scores one view): ``views`` is a list of logit tensors [B,C,h_k,w_k]
        of the same images at any sizes, ``flips[k]`` marks the output of a horizontally mirrored pass, ``weights`` default to 1.
        Each view is interpolated to the label grid, softmaxed and averaged inside ``hipops.seg_eval_ensemble`` (one launch);
        the histogram takes the argmax of the mean probability.  ``return_loss``: the mean over the counted pixels of -log(mean
        probability of the label), a 0-dim float32 tensor on the device, NaN when no pixel counts.  ``return_ids``: the
        prediction as a uint8 [B,Ht,Wt] plane.  Returns None, the loss, the ids, or (loss, ids), as ``update_from_logits`` does.
        No host synchronisation."""
        views = [v.detach() for v in views]
        _, pair, ids = H.seg_eval_ensemble(views, label_trues.detach(), flips=flips, weights=weights,
                                           hist=self._hist(views[0].device), want_loss=return_loss, want_ids=return_ids)
        loss = (pair[0] / pair[1]).float() if return_loss else None
        return (loss, ids) if return_loss and return_ids else (loss if return_loss else ids)

    def get_scores(self):
        """metrics.py:27-56"""
        hist = self.confusion_matrix
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.diag(hist) / hist.sum(axis=1)
        acc_cls = np.nanmean(acc_cls)
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        mean_iu = np.nanmean(iu)
        freq = hist.sum(axis=1) / hist.sum()
        fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
        cls_iu = dict(zip(range(self.n_classes), iu))
        return ({"Overall Acc: \t": acc, "Mean Acc : \t": acc_cls, "FreqW Acc : \t": fwavacc, "Mean IoU : \t": mean_iu},
                cls_iu)

    def reset(self):
        self._host = np.zeros((self.n_classes, self.n_classes))
        if self._dev is not None:
            self._dev.zero_()


DEPTH_METRIC_NAMES = H.DEPTH_ERROR_COLUMNS[:7]      # MonodepthLoss.depth_metric_names


class runningDepthScore(object):
    """Depth counterpart of ``runningScore``: the median-scaled monocular-depth errors, per image by one call of
    ``hipops.depth_errors`` and averaged over the images that have a valid pixel (the evaluation protocol the metric names come
    from).  ``update`` stays on the device and never synchronises; ``get_scores`` is one copy to the host."""

    def __init__(self, min_depth=1e-3, max_depth=80.0, median_scaling=True, scale=1.0, crop=None):
        self.min_depth, self.max_depth = min_depth, max_depth
        self.median_scaling, self.scale, self.crop = median_scaling, scale, crop
        self._acc = None      # float64 [10]: the sums of the seven metrics and of the ratio, the images counted, the images skipped

    def update(self, depth_gt, depth_pred):
        """depth_gt, depth_pred: float32 [B,H,W] or [B,1,H,W] of one size"""
        table = H.depth_errors(depth_gt.detach(), depth_pred.detach(), self.min_depth, self.max_depth, self.median_scaling,
                               self.scale, self.crop)
        has = table[:, 7:8] > 0                                            # n > 0; the other columns of a skipped image are NaN
        vals = torch.cat([table[:, :7], table[:, 13:14]], 1)
        vals = torch.where(has, vals, torch.zeros_like(vals))
        hasf = has.to(torch.float64)
        add = torch.cat([vals.sum(0), hasf.sum(0), (1.0 - hasf).sum(0)])
        if self._acc is None:
            self._acc = add
        else:
            assert self._acc.device == add.device, "runningDepthScore was updated from two devices"
            self._acc += add

    def get_scores(self):
        """-> ({name: mean over images}, {"n_images", "n_skipped", "mean_ratio"}); NaN means when no image was counted"""
        acc = np.zeros(10) if self._acc is None else self._acc.cpu().numpy()
        n = acc[8]
        mean = acc[:8] / n if n > 0 else np.full(8, np.nan)
        return ({k: float(mean[i]) for i, k in enumerate(DEPTH_METRIC_NAMES)},
                {"n_images": int(n), "n_skipped": int(acc[9]), "mean_ratio": float(mean[7])})

    def reset(self):
        self._acc = None


def _detached(v):
    return v.detach() if torch.is_tensor(v) else v


class AverageMeter(object):
    """Running average with the attributes of the reference's meter (evaluation/metrics.py:58-76): ``val`` the last value, ``sum``
    of ``val * n``, ``count`` of ``n``, ``avg = torch.true_divide(sum, count)``.  Device tensors stay on the device and the count
    is a Python number, so an update never synchronises."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = _detached(val)
        self.sum = self.sum + self.val * n
        self.count = self.count + n
        self.avg = torch.true_divide(self.sum, self.count)


class AverageMeterDict(object):
    """One running average per key (the reference's evaluation/metrics.py:79-99): ``sums``, ``counts`` and ``avgs`` are dicts over
    the keys seen so far; a key first seen later starts from zero then."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.avgs, self.sums, self.counts = {}, {}, {}

    def update(self, vals, n=1):
        for key, v in vals.items():
            total = self.sums.get(key, 0) + _detached(v) * n
            seen = self.counts.get(key, 0) + n
            self.sums[key], self.counts[key] = total, seen
            self.avgs[key] = torch.true_divide(total, seen)
