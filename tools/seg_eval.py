#!/usr/bin/env python
"""Measure segmentation validation at label resolution on the GPU and write profiles/seg_eval.md.

Two formulations of the segmentation block of one validation batch (train.py:836-851), in one process on the same tensors:
  * fused: ``runningScore.update_from_logits(labels, logits, return_loss=True)`` -- one launch of csrc/segeval.hip (plus its
    one-block fold): interpolation to the label grid, argmax, confusion matrix, cross-entropy;
  * unfused, what the package offered before: ``Fn.resize_bilinear`` of the logits to the label size (skipped when the sizes are
    equal), the cross-entropy kernel on the resized tensor, ``argmax(1)`` and ``runningScore.update``.
Workloads: 16 x 19 x 512 x 1024 logits against 1024 x 2048 labels (a Cityscapes validation batch scored at the annotation's size) and
4 x 19 x 1024 x 2048 at equal size.  Logits 3 * randn, channels-last as the models return them; labels uniform with 5 % ignored.

Per formulation: the median (min .. max) of the timed calls, each between its own pair of device events, after a warm-up; and
``torch.cuda.max_memory_allocated`` over one call, less what was allocated before it.  The share of the HBM rate is on the bytes
the fused pass must move: the logits once and the int64 labels once.  Needs a GPU: there is no fallback.

  python tools/seg_eval.py [--out profiles/seg_eval.md] [--calls 30]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from improving_segmentation_with_selfsupervised_depth_amd import _lib  # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn  # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H  # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd.evaluation import runningScore  # noqa: E402

HBM_MEASURED_GBS = 6362.5      # bench.py MEASURED_PEAKS["hbm_gbs"]: the streaming rate measured on this GPU model
HBM_NOMINAL_GBS = 8000.0
IGNORE = 250


def fused(rs, logits, labels):
    return rs.update_from_logits(labels, logits, return_loss=True)


def unfused(rs, logits, labels):
    x = Fn.to_nhwc(logits)
    if tuple(labels.shape[-2:]) != tuple(logits.shape[-2:]):
        x = Fn.resize_bilinear(x, tuple(labels.shape[-2:]), align_corners=True)
    out = H.cross_entropy_forward(x, labels.reshape(-1), IGNORE)
    rs.update(labels, Fn.to_nchw(x).argmax(1))
    return out[0] / out[1]


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_eval.md"))
    ap.add_argument("--calls", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/seg_eval.py measures on the GPU"
    assert args.calls >= 20
    dev = "cuda"
    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t      # noqa: E731
    lines = ["# Segmentation validation at label resolution: times and memory", "",
             "Written by `tools/seg_eval.py` on %s (torch %s)." % (torch.cuda.get_device_name(0), torch.__version__), "",
             "Milliseconds per call: median (min .. max) of %d calls, each between its own pair of device events, after a warm-up.  "
             "Memory: `torch.cuda.max_memory_allocated` over one call, less what was allocated before it.  Fused: "
             "`runningScore.update_from_logits(labels, logits, return_loss=True)`, one launch of `csrc/segeval.hip` and its one-block "
             "fold.  Unfused: `Fn.resize_bilinear` (when the sizes differ), the cross-entropy kernel on the resized tensor, `argmax(1)`, "
             "`runningScore.update`.  Same process, same tensors; logits channels-last.  One shared machine, one run." % args.calls, ""]
    with torch.no_grad():
        for B, C, Hi, Wi, Ht, Wt in ((16, 19, 512, 1024, 1024, 2048), (4, 19, 1024, 2048, 1024, 2048)):
            gen = torch.Generator(device=dev).manual_seed(0)
            logits = (3.0 * torch.randn((B, C, Hi, Wi), device=dev, generator=gen)).contiguous(memory_format=torch.channels_last)
            labels = torch.randint(0, C, (B, Ht, Wt), device=dev, generator=gen)
            labels[torch.rand((B, Ht, Wt), device=dev, generator=gen) < 0.05] = IGNORE
            rs_f, rs_u = runningScore(C), runningScore(C)
            loss_f, loss_u = float(fused(rs_f, logits, labels)), float(unfused(rs_u, logits, labels))
            differ = int(np.abs(rs_f.confusion_matrix - rs_u.confusion_matrix).sum()) // 2
            assert abs(loss_f - loss_u) <= 1e-5 * abs(loss_u), (loss_f, loss_u)
            assert differ <= 1e-6 * B * Ht * Wt, differ
            t_f = timed(lambda: fused(rs_f, logits, labels), args.calls)
            t_u = timed(lambda: unfused(rs_u, logits, labels), args.calls)
            m_f = peak_bytes(lambda: fused(rs_f, logits, labels))
            m_u = peak_bytes(lambda: unfused(rs_u, logits, labels))
            nbytes = 4.0 * B * C * Hi * Wi + 8.0 * B * Ht * Wt
            gbs = nbytes / t_f[0] / 1e6
            plan = _lib.lib().segsde_seg_eval_plan(C, Hi, Wi, Ht, Wt)
            route = "tiles of %d x 64 label pixels, source footprint staged in LDS" % plan if plan > 0 else "taps read from memory"
            lines += ["## %d x %d x %d x %d -> %d x %d" % (B, C, Hi, Wi, Ht, Wt), "",
                      "| | ms per call | peak memory of one call |", "|---|---|---|",
                      "| fused | %s | %.1f MB |" % (fmt(t_f), m_f / 1e6), "| unfused | %s | %.1f MB |" % (fmt(t_u), m_u / 1e6), "",
                      "Ratio unfused / fused: %.2f.  The fused pass (%s) moves %.2f GB (logits and int64 labels once each) at %.0f GB/s = "
                      "%.0f %% of the %.0f GB/s measured streaming rate (%.0f %% of the %.0f nominal).  Memory saved: %.1f MB.  Mean "
                      "losses %.7f (fused) and %.7f (unfused); pixels counted in different bins of the two confusion matrices: %d of %d."
                      % (t_u[0] / t_f[0], route, nbytes / 1e9, gbs, 100 * gbs / HBM_MEASURED_GBS, HBM_MEASURED_GBS,
                         100 * gbs / HBM_NOMINAL_GBS, HBM_NOMINAL_GBS, (m_u - m_f) / 1e6, loss_f, loss_u, differ, B * Ht * Wt), ""]
            del logits, labels
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
