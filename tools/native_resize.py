#!/usr/bin/env python
"""Time pil_loader's resize on the device (loader/device_batch.pil_resize, csrc/resize.hip) against Pillow on one host core, and
write profiles/native_resize.md.

    python tools/native_resize.py [--repeats 9] [--inner 5] [--cpu-images 4] [--out profiles/native_resize.md]

Two workloads:
  * cityscapes: 16 samples x 3 frames of 1024x2048 (rows x columns) -> 512x1024, the original-Cityscapes reduction;
  * mixed: eight 12-megapixel-class sources of differing sizes -> 768x1024 (Mapillary Vistas at a 768x1024 working size).
GPU: device events around ``--inner`` calls back to back, warm-up first (it also builds and uploads the window tables, which
are cached), then the median and the spread of ``--repeats`` samples.  The bytes that must move are counted from the shapes:
every source byte read once, the uint8 image between the passes written and read once, the result written once; divided by
the time they give the fraction of the HBM peak.  CPU: ``Image.resize(size, Image.LANCZOS)`` of the same images on ONE thread.
Both produce the same bytes; the first call checks that.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from improving_segmentation_with_selfsupervised_depth_amd.loader.device_batch import pil_resize  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s
WORKLOADS = {
    "cityscapes": dict(sources=[(1024, 2048)] * 48, size=(512, 1024), what="16 x 3 frames 1024x2048 -> 512x1024"),
    "mixed": dict(sources=[(3024, 4032), (3000, 4000), (2448, 3264), (3456, 4608), (2988, 5312), (3120, 4160), (2736, 3648), (3024, 4032)],
                  size=(768, 1024), what="8 mixed 8..16-megapixel sources -> 768x1024"),
}


def moved_bytes(sources, size):
    h, w = size
    total = 0
    for hs, ws in sources:
        total += 3 * hs * ws + 3 * h * w
        if hs != h and ws != w:
            total += 2 * 3 * hs * w
    return total


def images(sources, seed):
    rng = np.random.RandomState(seed)
    out = []
    for hs, ws in sources:
        a = rng.randint(0, 256, (hs // 8 + 1, ws // 8 + 1, 3), dtype=np.uint8)           # blocks of noise: cheap to make
        out.append(np.ascontiguousarray(np.kron(a, np.ones((8, 8, 1), dtype=np.uint8))[:hs, :ws] ^ rng.randint(0, 8, (1, ws, 3), dtype=np.uint8)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--cpu-images", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_resize.md"))
    args = ap.parse_args()
    from PIL import Image
    import PIL
    torch.set_num_threads(1)
    dev = torch.device("cuda")
    lines = ["# pil_loader's resize on the device", "",
             "`python tools/native_resize.py` on %s; Pillow %s on one host core.  Times are per call (all samples of the workload)."
             % (torch.cuda.get_device_name(0), PIL.__version__), "",
             "| workload | device, median (min .. max) | bytes that must move | share of the HBM peak (%.0f TB/s) | Pillow, one core | ratio |" % (HBM_PEAK / 1e12),
             "|---|---|---|---|---|---|"]
    for name, wl in WORKLOADS.items():
        host = images(wl["sources"], 7)
        same = all(s == wl["sources"][0] for s in wl["sources"])
        src = torch.from_numpy(np.stack(host)).to(dev) if same else [torch.from_numpy(a).to(dev) for a in host]
        h, w = wl["size"]
        got = pil_resize(src, wl["size"])
        n_cpu = min(args.cpu_images, len(host))
        t0 = time.perf_counter()
        want = [np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS)) for a in host[:n_cpu]]
        cpu_s = (time.perf_counter() - t0) / n_cpu * len(host)
        assert np.array_equal(got[:n_cpu].cpu().numpy(), np.stack(want)), "the device result differs from Pillow"
        for _ in range(2):
            pil_resize(src, wl["size"])
        samples = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                pil_resize(src, wl["size"])
            b.record()
            torch.cuda.synchronize()
            samples.append(a.elapsed_time(b) / args.inner * 1e-3)
        med, nbytes = statistics.median(samples), moved_bytes(wl["sources"], wl["size"])
        lines.append("| %s | %.3f ms (%.3f .. %.3f) | %.1f MB | %.1f %% | %.0f ms | %.0fx |" % (
            wl["what"], med * 1e3, min(samples) * 1e3, max(samples) * 1e3, nbytes / 1e6, 100 * nbytes / med / HBM_PEAK, cpu_s * 1e3, cpu_s / med))
        print(lines[-1], flush=True)
    lines += ["", "The device time is the whole `pil_resize` call: descriptor upload, both passes, allocation of the intermediate image.",
              "Pillow's time is extrapolated from %d images of each workload.  No speed gate is attached to these numbers: the stage" % args.cpu_images,
              "frees loader cores, it is not on the training step's critical path."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
