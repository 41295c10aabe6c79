#!/usr/bin/env python
"""Measure the mix masks of trainer.generate_mix_mask (csrc/mixmask.hip) on the GPU and write profiles/mix_masks.md.

Workloads: 2 x 512 x 512 (the reference's batch and crop) and 16 x 512 x 1024.  Depths: a min-max normalised vertical ramp with
noise (smooth: neighbouring pixels share a histogram bin, the hard case for the LDS counters); labels: blocks of 19 classes.
Each mode is timed against the formulation it replaces, kept here:
  "class", "depth"  the per-image loops of the parent commit (torch.unique + boolean index + numpy draw + one class_mask launch per
                    image; one depth_threshold_mask launch per image; torch.cat);
  "depthhist"       the reference's lines (train.py:616-636) on a host copy of the depths: np.histogram per image, the thresholds
                    back to the device through generate_depth_mask.
"depthcomp" and None are the parent's code and are timed alone.

Call time: host clock around as many back-to-back calls as fill about 100 ms, ending in a device synchronise, after a warm-up; the two
versions alternate window by window; median (min .. max) of the repeats.  Kernel time comes from a run of its own under
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mix_masks.py --kernels-only
whose kernel trace `--summarise-trace CSV` appends as a table: the median duration of every kernel and, for the passes that stream
the batch, the rate on the bytes they must move.  Needs a GPU: there is no fallback.

  python tools/mix_masks.py [--out profiles/mix_masks.md] [--repeats 7]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from improving_segmentation_with_selfsupervised_depth_amd import trainer as T  # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd.loader import transformmasks as TM  # noqa: E402

WINDOW_MS = 100.0
HBM_MEASURED_GBS = 6362.5      # bench.py MEASURED_PEAKS["hbm_gbs"]: the streaming rate measured on this GPU model
SIZES = ((2, 512, 512), (16, 512, 1024))
TRACE_CALLS = 10
# kernel -> bytes per pixel it must move (0: no pass over the batch)
KERNEL_BYTES = {"dh_minmax_kernel": 4, "dh_hist_kernel": 4, "dh_finish_kernel": 0, "thr_mask_batch_kernel": 8,
                "class_presence_kernel": 8, "class_mask_batch_kernel": 16}
KERNELS_PER_SIZE = (("depthhist", ("dh_minmax_kernel", "dh_hist_kernel", "dh_finish_kernel", "thr_mask_batch_kernel")),
                    ("depth", ("thr_mask_batch_kernel",)), ("class", ("class_presence_kernel", "class_mask_batch_kernel")))


def inputs(B, Hh, W, dev):
    g = torch.Generator().manual_seed(B)
    d = torch.linspace(0, 1, Hh).reshape(1, 1, Hh, 1) + 0.2 * torch.rand(B, 1, Hh, W, generator=g)
    lo, hi = d.amin(dim=(1, 2, 3), keepdim=True), d.amax(dim=(1, 2, 3), keepdim=True)
    depths = ((d - lo) / (hi - lo)).to(dev)
    rows, cols = torch.arange(Hh).reshape(1, Hh, 1) // 32, torch.arange(W).reshape(1, 1, W) // 64
    pred = ((rows * 7 + cols * 3 + torch.arange(B).reshape(B, 1, 1)) % 19).to(torch.int64).to(dev)
    imgs = torch.zeros((B, 3, Hh, W), device=dev)
    return depths, pred, imgs


def parent_class(pred):
    masks = []
    for i in range(pred.shape[0]):
        classes = torch.unique(pred[i])
        classes = classes[classes != 250]
        n = classes.shape[0]
        pick = torch.as_tensor(np.random.choice(n, int((n - n % 2) / 2), replace=False), dtype=torch.int64, device=pred.device)
        masks.append(TM.generate_class_mask(pred[i], classes[pick]).unsqueeze(0))
    return torch.cat(masks)


def parent_depth(depths):
    masks = []
    for i in range(depths.shape[0]):
        thr = torch.rand(1) * (0.4 - 0.1) + 0.1
        masks.append(TM.generate_depth_mask(depths[i], thr))
    return torch.cat(masks)


def reference_depthhist(depths):
    """train.py:616-636 on a host copy (np.histogram does not take a device tensor)"""
    host = depths.cpu()
    masks = []
    for i in range(depths.shape[0]):
        hist, bin_edges = np.histogram(torch.log(1 + host[i]).flatten(), bins=100, density=True)
        for v, e in zip(np.flip(hist)[1:], np.flip(bin_edges)[1:]):
            if v > 1.5:
                max_depth = torch.tensor([e])
                break
        hist = np.cumsum(hist) / np.sum(hist)
        for v, e in zip(hist, bin_edges):
            if v > 0.4:
                min_depth = torch.tensor([e])
                break
        thr = torch.rand(1) * (max_depth - min_depth) + min_depth
        masks.append(TM.generate_depth_mask(depths[i], thr))
    return torch.cat(masks)


def _window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def timed(fns, repeats, warmup=3):
    """versions alternating window by window -> [(median, min, max) ms per call] per version"""
    inner = []
    for fn in fns:
        for _ in range(warmup):
            fn()
        inner.append(int(min(5000, max(1, round(WINDOW_MS / max(_window(fn, 3), 1e-3))))))
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            ms[k].append(_window(fn, inner[k]))
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def summarise_trace(path):
    """the kernel trace (CSV) of a --kernels-only run -> markdown lines"""
    import csv
    import re
    pat = re.compile("|".join(KERNEL_BYTES))
    rows = sorted((r for r in csv.DictReader(open(path)) if pat.search(r["Kernel_Name"])), key=lambda r: int(r["Start_Timestamp"]))
    per_size = sum(len(k) for _, k in KERNELS_PER_SIZE) * TRACE_CALLS
    assert len(rows) == per_size * len(SIZES), "%d mix-mask dispatches in %s, expected %d" % (len(rows), path, per_size * len(SIZES))
    lines = ["## Kernel times", "",
             "From `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/mix_masks.py --kernels-only` (a run of its own; %d "
             "calls per mode and size, the first 2 left out): median microseconds per launch and, for the passes over the batch, the "
             "rate on the bytes that launch must move (depths 4 B, labels and int64 masks 8 B per pixel) against the %.0f GB/s measured "
             "streaming rate.  The difference between the sum and the call time above is launch gaps and the host."
             % (TRACE_CALLS, HBM_MEASURED_GBS), "",
             "| size | mode | kernel | us | B/pixel | GB/s | of %.0f measured |" % HBM_MEASURED_GBS, "|---|---|---|---|---|---|---|"]
    at = 0
    for B, Hh, W in SIZES:
        n = B * Hh * W
        for mode, kernels in KERNELS_PER_SIZE:
            chunk = rows[at:at + len(kernels) * TRACE_CALLS]
            at += len(chunk)
            total = 0.0
            for j, k in enumerate(kernels):
                mine = chunk[j::len(kernels)]
                assert all(k in r["Kernel_Name"] for r in mine), (mode, k, [r["Kernel_Name"] for r in mine][:3])
                med = float(np.median([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine[2:]]))
                total += med
                bpe = KERNEL_BYTES[k]
                gbs = bpe * n / med / 1e3
                lines.append("| %d x %d x %d | %s | `%s` | %.2f | %s | %s | %s |" % (
                    B, Hh, W, mode, k, med, bpe or "-", "%.0f" % gbs if bpe else "-", "%.0f %%" % (100 * gbs / HBM_MEASURED_GBS) if bpe else "-"))
            lines.append("| %d x %d x %d | %s | sum | %.2f | | | |" % (B, Hh, W, mode, total))
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise-trace", metavar="CSV", help="append the kernel-time table of a --kernels-only trace to --out and exit "
                    "(needs no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_masks.md"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels-only", action="store_true", help="%d calls of \"depthhist\", \"depth\" and \"class\" per size and nothing "
                    "else: the run to put under a kernel trace" % TRACE_CALLS)
    args = ap.parse_args()
    if args.summarise_trace:
        lines = summarise_trace(args.summarise_trace)
        open(args.out, "a").write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    assert torch.cuda.is_available(), "tools/mix_masks.py measures on the GPU"
    dev = "cuda"
    if args.kernels_only:
        for B, Hh, W in SIZES:
            depths, pred, imgs = inputs(B, Hh, W, dev)
            for mode, _ in KERNELS_PER_SIZE:
                for _ in range(TRACE_CALLS):
                    T.generate_mix_mask(mode, pred, imgs, depths)
                torch.cuda.synchronize()
        return
    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t      # noqa: E731
    lines = ["# Mix masks: call times", "",
             "Written by `python tools/mix_masks.py` on %s (torch %s, numpy %s)." % (torch.cuda.get_device_name(0), torch.__version__,
                                                                                   np.__version__), "",
             "Milliseconds per call of `trainer.generate_mix_mask`: host clock around as many back-to-back calls as fill about %d ms, "
             "ending in a device synchronise, after a warm-up, the versions alternating window by window; median (min .. max) of %d "
             "windows.  \"before\" is the formulation the mode replaces: for \"class\" and \"depth\" the per-image loops of the parent "
             "commit, for \"depthhist\" the reference's lines (train.py:616-636) on a host copy of the depths.  \"depthcomp\" and None "
             "did not change.  One shared machine, one run." % (WINDOW_MS, args.repeats), ""]
    verdicts = []
    for B, Hh, W in SIZES:
        depths, pred, imgs = inputs(B, Hh, W, dev)
        np.random.seed(0)
        assert torch.equal(T.generate_mix_mask("class", pred, imgs, depths), (np.random.seed(0), parent_class(pred))[1])
        torch.manual_seed(0)
        assert torch.equal(T.generate_mix_mask("depth", pred, imgs, depths), (torch.manual_seed(0), parent_depth(depths))[1])
        torch.manual_seed(0)
        new = T.generate_mix_mask("depthhist", pred, imgs, depths)
        torch.manual_seed(0)
        agree = float((new == reference_depthhist(depths)).float().mean())
        lines += ["## %d x %d x %d" % (B, Hh, W), "",
                  "\"depthhist\" against the reference's lines on the host, same draws: %.6f of the pixels agree." % agree, "",
                  "| mode | now ms | before ms | before / now |", "|---|---|---|---|"]
        pairs = (("depthhist", reference_depthhist, depths), ("depth", parent_depth, depths), ("class", parent_class, pred))
        for mode, before, arg in pairs:
            t_n, t_b = timed([lambda: T.generate_mix_mask(mode, pred, imgs, depths), lambda: before(arg)], args.repeats)
            lines.append("| %s | %s | %s | %.2f |" % (mode, fmt(t_n), fmt(t_b), t_b[0] / t_n[0]))
            if mode != "depthhist":
                # slower only if even the fastest window of the new path is slower than the slowest of the parent's
                verdicts.append("%s at %d x %d x %d: %s" % (mode, B, Hh, W, "SLOWER than the parent's loop beyond the spread"
                                                            if t_n[1] > t_b[2] else "not slower than the parent's loop"))
        for mode in ("depthcomp", None):
            (t_n,) = timed([lambda: T.generate_mix_mask(mode, pred, imgs, depths)], args.repeats)
            lines.append("| %s | %s | - | - |" % (mode, fmt(t_n)))
        lines.append("")
        del depths, pred, imgs
        torch.cuda.empty_cache()
    lines += ["## \"class\" and \"depth\" against the parent's loops", ""] + ["* " + v for v in verdicts] + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
