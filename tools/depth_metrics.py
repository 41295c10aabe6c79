#!/usr/bin/env python
"""Measure hipops.depth_errors on the GPU and write profiles/depth_metrics.md.

Workloads: 4 x 1024 x 2048 (Cityscapes at the native size) and 16 x 512 x 1024 (a validation batch at the training size); ground
truth log-uniform in [0.5, 120] with 30 % of the pixels zeroed, predictions off by a scale and log-normal noise.  Beside the call
the torch formulation of the same evaluation on the same device: per image a boolean gather, two sorts for the medians, the
elementwise errors and their means.  The share of the HBM rate is on the bytes the five passes of csrc/depthmetrics.hip must move
(four counting passes and the error pass read gt and pred once each: 40 bytes per pixel); the floor of any exact scheme is one
pass, 8 bytes per pixel, which is quoted too.

Every time is a pair of device events around as many back-to-back calls as fill about 100 ms, after a warm-up; median (min .. max)
of the repeats.  Needs a GPU: there is no fallback.

  python tools/depth_metrics.py [--out profiles/depth_metrics.md] [--repeats 5]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from improving_segmentation_with_selfsupervised_depth_amd import hipops as H  # noqa: E402

WINDOW_MS = 100.0
HBM_MEASURED_GBS = 6362.5      # bench.py MEASURED_PEAKS["hbm_gbs"]: the streaming rate measured on this GPU model
HBM_NOMINAL_GBS = 8000.0
LO, HI = 1e-3, 80.0


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    inner = int(min(2000, max(1, round(WINDOW_MS / max(_window(fn, 3), 1e-3)))))
    ms = [_window(fn, inner) for _ in range(repeats)]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def torch_depth_errors(gt, pred):
    """the same evaluation in torch operators: [B,H,W] twice -> float64 [B,7]; one host synchronisation per image (the size of the
    boolean gather)"""
    rows = []
    for b in range(gt.shape[0]):
        mask = (gt[b] > LO) & (gt[b] < HI)
        g, p = gt[b][mask], pred[b][mask]
        n = g.numel()
        gs, ps = g.sort()[0], p.sort()[0]
        med_g = (gs[(n - 1) // 2] + gs[n // 2]) / 2
        med_p = (ps[(n - 1) // 2] + ps[n // 2]) / 2
        p = (p * (med_g / med_p)).clamp(LO, HI)
        t = torch.max(g / p, p / g)
        d = g - p
        rows.append(torch.stack([(d.abs() / g).double().mean(), (d * d / g).double().mean(), (d * d).double().mean().sqrt(),
                                 ((g.log() - p.log()) ** 2).double().mean().sqrt(), (t < 1.25).double().mean(),
                                 (t < 1.25 ** 2).double().mean(), (t < 1.25 ** 3).double().mean()]))
    return torch.stack(rows)


def inputs(B, Hh, W, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    u = lambda: torch.rand((B, Hh, W), device=dev, generator=gen)      # noqa: E731
    gt = torch.exp(u() * (np.log(120.0) - np.log(0.5)) + np.log(0.5))
    gt[u() < 0.3] = 0
    pred = gt * torch.exp(torch.randn((B, Hh, W), device=dev, generator=gen) * 0.25) * 0.37 + u() * 0.2
    invalid = ~((gt > LO) & (gt < HI))
    pred[invalid] = (u() * 99.9 + 0.1)[invalid]
    return gt.contiguous(), pred.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_metrics.md"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/depth_metrics.py measures on the GPU"
    dev = "cuda"
    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t      # noqa: E731
    lines = ["# Depth evaluation: times", "",
             "Written by `tools/depth_metrics.py` on %s (torch %s)." % (torch.cuda.get_device_name(0), torch.__version__), "",
             "Milliseconds per call: one pair of device events around as many back-to-back calls as fill about %d ms, after a warm-up; "
             "median (min .. max) of %d windows.  `hipops.depth_errors` is eleven launches (a memset, four counting passes each followed "
             "by a one-block digit choice, the error pass, the finish) and moves 40 bytes per pixel; an exact single-pass scheme would "
             "move 8.  The torch formulation runs on the same device: per image a boolean gather (one host synchronisation), two sorts, "
             "the elementwise errors.  One shared machine, one run." % (WINDOW_MS, args.repeats), ""]
    for B, Hh, W in ((4, 1024, 2048), (16, 512, 1024)):
        px = B * Hh * W
        gt, pred = inputs(B, Hh, W, dev)
        table = H.depth_errors(gt, pred)
        ref = torch_depth_errors(gt, pred)
        worst = float(((table[:, :7] - ref).abs() / ref.abs().clamp_min(1e-12)).max())
        assert worst < 1e-3, "the two formulations disagree: %g" % worst
        t_k = timed(lambda: H.depth_errors(gt, pred), args.repeats)
        t_t = timed(lambda: torch_depth_errors(gt, pred), args.repeats)
        gbs = 40.0 * px / t_k[0] / 1e6
        lines += ["## %d x %d x %d" % (B, Hh, W), "", "| | ms per call |", "|---|---|",
                  "| `hipops.depth_errors` | %s |" % fmt(t_k), "| torch formulation, same device | %s |" % fmt(t_t), "",
                  "Ratio torch / kernels: %.1f.  The kernels move 40 bytes per pixel at %.0f GB/s = %.0f %% of the %.0f GB/s measured "
                  "streaming rate (%.0f %% of the %.0f nominal); against the 8 bytes per pixel of a single pass the call reaches %.0f %% of "
                  "the measured rate.  Largest relative difference between the two formulations over the seven metrics: %.1e."
                  % (t_t[0] / t_k[0], gbs, 100 * gbs / HBM_MEASURED_GBS, HBM_MEASURED_GBS, 100 * gbs / HBM_NOMINAL_GBS, HBM_NOMINAL_GBS,
                     100 * gbs / 5 / HBM_MEASURED_GBS, worst), ""]
        del gt, pred
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
