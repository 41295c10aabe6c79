#!/usr/bin/env python
"""Measure segmentation evaluation with test-time ensembling on the GPU and write profiles/seg_eval_ensemble.md.

Two formulations of the same result, in one process on the same tensors:
  * fused: ``runningScore.update_from_views(labels, views, flips, return_loss=True)`` -- one launch of csrc/segens.hip (plus its
    one-block fold) for all views: interpolation to the label grid, softmax, weighted mean, argmax, confusion matrix, NLL;
  * composed, from what the package offered before: per view ``torch.flip`` (flipped views), ``Fn.resize_bilinear(...,
    align_corners=True)`` to the label size (skipped at equal size), ``torch.softmax`` and an accumulate; then ``argmax``,
    ``runningScore.update`` and the NLL of the label's mean probability in torch.
Problems: 16 x 19 with views 256 x 512 .. 896 x 1792 in steps of 128 x 256, each plain and flipped (12 views), against 1024 x 2048
labels; and 4 x 19 with a plain and a flipped view at 1024 x 2048, equal size.  Logits 3 * randn, channels-last as the models return
them; labels uniform with 5 % ignored.

Per formulation: the median (min .. max) of ``--repeats`` timed windows of ``--calls`` calls each, every window between its own
pair of device events, fused and composed windows alternating, after a warm-up; ``torch.cuda.max_memory_allocated`` over one call,
less what was allocated before it.  The bytes the fused call must move (every view once, the int64 labels once) are set against
the streaming rate of a device-to-device copy measured in the same run.  Needs a GPU: there is no fallback.

  python tools/seg_eval_ensemble.py [--out profiles/seg_eval_ensemble.md] [--repeats 5] [--calls 3]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn  # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H  # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd.evaluation import runningScore  # noqa: E402

IGNORE = 250
PROBLEMS = (
    ("12 views", 16, 19, [(128 * k, 256 * k) for k in range(2, 8) for _ in (0, 1)], [0, 1] * 6, (1024, 2048)),
    ("flip pair", 4, 19, [(1024, 2048)] * 2, [0, 1], (1024, 2048)),
)


def fused(rs, views, flips, labels):
    return rs.update_from_views(labels, views, flips=flips, return_loss=True)


def composed(rs, views, flips, labels):
    size = tuple(labels.shape[-2:])
    acc = None
    for x, f in zip(views, flips):
        if f:
            x = torch.flip(x, dims=[-1])
        x = Fn.to_nhwc(x)
        if tuple(x.shape[1:3]) != size:
            x = Fn.resize_bilinear(x, size, align_corners=True)
        p = torch.softmax(x, dim=-1)
        acc = p if acc is None else acc.add_(p)
    acc.mul_(1.0 / len(views))
    rs.update(labels, acc.argmax(-1))
    C = acc.shape[-1]
    counted = (labels >= 0) & (labels < C) & (labels != IGNORE)
    at = acc.gather(-1, torch.where(counted, labels, torch.zeros_like(labels))[..., None])[..., 0]
    nll = torch.where(counted, -torch.log(at), torch.zeros_like(at))
    return nll.sum(dtype=torch.float64) / counted.sum()


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternating(fns, repeats, calls, warmup=2):
    """-> per fn (median, min, max) of the per-call milliseconds of ``repeats`` windows, the fns taking turns"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            ms[i].append(window(fn, calls))
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def streaming_rate(repeats):
    """GB/s of a 1 GiB device-to-device copy (bytes read plus bytes written): median (min .. max)"""
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    (t,) = alternating([lambda: dst.copy_(src)], repeats, 4)
    return tuple(2.0 * src.numel() * 4 / ms / 1e6 for ms in (t[0], t[2], t[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_eval_ensemble.md"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/seg_eval_ensemble.py measures on the GPU"
    dev = "cuda"
    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t      # noqa: E731
    rate = streaming_rate(args.repeats)
    lines = ["# Segmentation evaluation with test-time ensembling: times and memory", "",
             "Written by `python tools/seg_eval_ensemble.py --repeats %d --calls %d` on %s (torch %s)."
             % (args.repeats, args.calls, torch.cuda.get_device_name(0), torch.__version__), "",
             "Milliseconds per call: median (min .. max) of %d windows of %d calls, each window between its own pair of device events, "
             "fused and composed windows alternating, after a warm-up.  Memory: `torch.cuda.max_memory_allocated` over one call, less "
             "what was allocated before it.  Fused: `runningScore.update_from_views(labels, views, flips, return_loss=True)`, one launch "
             "of `csrc/segens.hip` and its one-block fold.  Composed: per view `torch.flip` (flipped views), `Fn.resize_bilinear(..., "
             "align_corners=True)` (when the sizes differ), `torch.softmax`, an accumulate; then `argmax`, `runningScore.update` and the "
             "NLL in torch.  Same process, same tensors; logits channels-last.  One shared machine, one run." % (args.repeats, args.calls),
             "", "Streaming rate of a 1 GiB device-to-device copy in this run (read plus written bytes): %.0f (%.0f .. %.0f) GB/s." % rate,
             ""]
    with torch.no_grad():
        for name, B, C, sizes, flips, (Ht, Wt) in PROBLEMS:
            gen = torch.Generator(device=dev).manual_seed(0)
            views = [(3.0 * torch.randn((B, C, h, w), device=dev, generator=gen)).contiguous(memory_format=torch.channels_last)
                     for h, w in sizes]
            labels = torch.randint(0, C, (B, Ht, Wt), device=dev, generator=gen)
            labels[torch.rand((B, Ht, Wt), device=dev, generator=gen) < 0.05] = IGNORE
            rs_f, rs_c = runningScore(C), runningScore(C)
            loss_f, loss_c = float(fused(rs_f, views, flips, labels)), float(composed(rs_c, views, flips, labels))
            differ = int(np.abs(rs_f.confusion_matrix - rs_c.confusion_matrix).sum()) // 2
            assert abs(loss_f - loss_c) <= 1e-5 * abs(loss_c), (loss_f, loss_c)
            assert differ <= 1e-4 * B * Ht * Wt, differ
            t_f, t_c = alternating([lambda: fused(rs_f, views, flips, labels), lambda: composed(rs_c, views, flips, labels)],
                                   args.repeats, args.calls)
            m_f = peak_bytes(lambda: fused(rs_f, views, flips, labels))
            m_c = peak_bytes(lambda: composed(rs_c, views, flips, labels))
            nbytes = sum(4.0 * v.numel() for v in views) + 8.0 * B * Ht * Wt
            gbs = nbytes / t_f[0] / 1e6
            th, routes = H.seg_eval_ensemble_plan(views, (Ht, Wt), flips=flips)
            faster = t_c[1] > t_f[2]
            lines += ["## %s: %d x %d, views %s -> %d x %d" % (name, B, C, ", ".join("%dx%d%s" % (h, w, "f" if f else "")
                                                                                       for (h, w), f in zip(sizes, flips)), Ht, Wt), "",
                      "| | ms per call | peak memory of one call |", "|---|---|---|",
                      "| fused | %s | %.1f MB |" % (fmt(t_f), m_f / 1e6), "| composed | %s | %.1f MB |" % (fmt(t_c), m_c / 1e6), "",
                      "Ratio composed / fused (medians): %.2f; the slowest fused window is %s the fastest composed one, so the "
                      "difference is %s the observed spread.  Plan: tiles of %d x 64 label pixels, routes %s.  The fused call must move "
                      "%.2f GB (every view once, the int64 labels once; +%.3f GB with the uint8 ids) and does so at %.0f GB/s = %.1f %% of "
                      "the streaming rate measured above (per class, view and label pixel the kernel makes three interpolating passes "
                      "over LDS and two exponentials; no counters were collected).  Mean losses %.7f (fused) and %.7f (composed); pixels "
                      "counted in different bins of the two confusion matrices: %d of %d."
                      % (t_c[0] / t_f[0], "faster than" if faster else "NOT faster than", "larger than" if faster else "within",
                         th, "/".join(sorted(set(routes))), nbytes / 1e9, B * Ht * Wt / 1e9, gbs, 100 * gbs / rate[0], loss_f, loss_c,
                         differ, B * Ht * Wt), ""]
            del views, labels
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
