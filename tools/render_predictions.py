#!/usr/bin/env python
"""Measure the rendering of inference outputs on the GPU and write profiles/render_predictions.md.

Workloads: a batch of 16 at 512 x 1024 and one at 1024 x 2048, 19 classes (Cityscapes at the training and at the native size).
For each of the three launches of csrc/render.hip -- labels from logits, unit image, colorize -- the time per launch and the share
of the HBM rate on the bytes it must move (labels: 4 C + 4 per pixel with the id plane; unit image: 5 per value; colorize: two
reads and three floats written, 20 per pixel), for dense NCHW and channels-last logits.  Beside them what the kernels replace: on the
device torch's ``max(1)[1]`` (which only gives the int64 map the reference then copies to the host), on the host a numpy
restatement of ``decode_segmap_tocolor`` plus ``save_image``'s arithmetic for ONE image on one core (the reference does this per
image, so a batch costs B times that), timed in this script.

Every kernel time is a pair of device events around as many back-to-back launches as fill about 100 ms, after a warm-up; median
(min .. max) of the repeats.  Needs a GPU: there is no fallback.

  python tools/render_predictions.py [--out profiles/render_predictions.md] [--repeats 5]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from improving_segmentation_with_selfsupervised_depth_amd import hipops as H  # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd import inference as INF  # noqa: E402

WINDOW_MS = 100.0
HBM_MEASURED_GBS = 6362.5      # bench.py MEASURED_PEAKS["hbm_gbs"]: the streaming rate measured on this GPU model
HBM_NOMINAL_GBS = 8000.0


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


def host_label_image(seg, colours):
    """numpy restatement of Cityscapes.decode_segmap_tocolor + torch.tensor(...).permute + save_image's conversion, one image"""
    r, g, b = seg.copy(), seg.copy(), seg.copy()
    for l in range(len(colours)):
        m = seg == l
        r[m], g[m], b[m] = colours[l][0], colours[l][1], colours[l][2]
    rgb = np.zeros((seg.shape[0], seg.shape[1], 3))
    rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2] = r / 255.0, g / 255.0, b / 255.0
    t = torch.tensor(rgb).permute(2, 0, 1)
    return t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def host_unit_image(img):
    return img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def host_time(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_predictions.md"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/render_predictions.py measures on the GPU"
    dev = "cuda"
    torch.set_num_threads(1)
    C = 19
    r = np.random.default_rng(0)
    pal = torch.from_numpy(r.integers(0, 256, (C, 3)).astype(np.uint8)).to(dev)
    n = 256
    lut = torch.rand((n + 3, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t      # noqa: E731
    share = lambda nbytes, ms: "%.0f GB/s = %.0f %% of %.0f measured, %.0f %% of %.0f nominal" % (      # noqa: E731
        nbytes / ms / 1e6, 100 * nbytes / ms / 1e6 / HBM_MEASURED_GBS, HBM_MEASURED_GBS, 100 * nbytes / ms / 1e6 / HBM_NOMINAL_GBS,
        HBM_NOMINAL_GBS)
    lines = ["# Rendering of inference outputs: times", "",
             "Written by `tools/render_predictions.py` on %s (torch %s)." % (torch.cuda.get_device_name(0), torch.__version__), "",
             "Milliseconds per launch: one pair of device events around as many back-to-back launches as fill about %d ms, after a "
             "warm-up; median (min .. max) of %d windows.  The share of the HBM rate is on the bytes the launch must move (its operands "
             "once each).  Host figures: one image, one core, wall clock, median (min .. max) of %d calls.  One shared machine, one run."
             % (WINDOW_MS, args.repeats, args.repeats), ""]
    for B, Hh, W in ((16, 512, 1024), (16, 1024, 2048)):
        px = B * Hh * W
        logits = torch.randn((B, C, Hh, W), device=dev)
        lcl = logits.contiguous(memory_format=torch.channels_last)
        img = torch.rand((B, 3, Hh, W), device=dev)
        disp = torch.rand((B, 1, Hh, W), device=dev)
        rows = []
        for name, x in (("labels from logits, dense NCHW (+ id plane)", logits), ("labels from logits, channels-last (+ id plane)", lcl)):
            t = timed(lambda: H.render_labels(pal, logits=x, return_ids=True), args.repeats)
            rows.append((name, fmt(t), share(px * (4 * C + 4), t[0])))
        t = timed(lambda: logits.max(1)[1], args.repeats)
        rows.append(("torch `max(1)[1]` on the device (int64 map only)", fmt(t), share(px * (4 * C + 8), t[0])))
        ids = logits.max(1)[1]
        t = timed(lambda: H.render_labels(pal, ids=ids), args.repeats)
        rows.append(("labels from an int64 id map", fmt(t), share(px * 11, t[0])))
        t = timed(lambda: H.render_unit_image(img), args.repeats)
        rows.append(("unit image, 3 channels", fmt(t), share(px * 15, t[0])))
        t = timed(lambda: H.render_unit_image(disp), args.repeats)
        rows.append(("unit image, 1 channel (disparity)", fmt(t), share(px * 5, t[0])))
        t = timed(lambda: H.colorize(disp[:, 0], lut), args.repeats)
        rows.append(("colorize (two launches: min / max, lookup)", fmt(t), share(px * 20, t[0])))
        # what leaves the device per batch
        res = {"image": H.render_unit_image(img), "label": H.render_labels(pal, logits=logits), "depth": H.render_unit_image(disp)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [v.cpu() for v in res.values()]
        t_copy = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref_ids = ids.cpu().numpy()
        t_copy_ref = (time.perf_counter() - t0) * 1e3
        # host restatement, one image
        colours = pal.cpu().tolist()
        seg = ref_ids[0]
        assert np.array_equal(host_label_image(seg, colours), host[1][0].numpy()), "host restatement differs from the kernel"
        img0 = img[0].cpu()
        assert np.array_equal(host_unit_image(img0), host[0][0].numpy())
        th_lab = host_time(lambda: host_label_image(seg, colours), args.repeats)
        th_img = host_time(lambda: host_unit_image(img0), args.repeats)
        lines += ["## %d x %d x %d, %d classes" % (B, Hh, W, C), "", "| launch | ms | bytes it must move / time |", "|---|---|---|"]
        lines += ["| %s | %s | %s |" % row for row in rows]
        lines += ["", "Device to host for the batch: the three uint8 tensors (7 bytes per pixel) %.1f ms, pageable memory, one call each; "
                  "the reference's int64 map alone (8 bytes per pixel) %.1f ms." % (t_copy, t_copy_ref),
                  "Host, one image of the batch on one core: decode + save_image arithmetic of the label %s ms, save_image arithmetic of the "
                  "input image %s ms; the reference runs both per image, %d times per batch." % (fmt(th_lab), fmt(th_img), B), ""]
        del logits, lcl, img, disp, ids, res, host
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
