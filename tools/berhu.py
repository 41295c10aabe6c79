#!/usr/bin/env python
"""Measure the BerHu pseudo-depth loss (loss.loss.berhu / berhu_own_car, csrc/berhu.hip) on the GPU and write profiles/berhu.md.

Workloads: 16 x 1 x 512 x 1024 (a training batch) and 2 x 1 x 1024 x 2048 (the native size); inputs uniform in (0, 1).  Modes:
plain (a mask tensor of ones, as the signature demands), apply_log, and the own-car crop -- berhu_own_car, no mask tensor -- against
the reference's way, the torch formula on a materialised keep tensor built per call as both callers did.  Timed is forward plus
backward of the HIP path and of the torch formula of the reference (loss.py:5-15, its .item() included) on the same device.

Bytes the HIP path must move: two forward passes of 8 bytes per element (input and target read once each) and one backward pass of
12 (both read, the gradient written), plus 4 per pass with a mask tensor.  The share of the HBM rate is those bytes over the time of
forward plus backward, launch gaps included.

Every time is a pair of device events around as many back-to-back calls as fill about 100 ms, after a warm-up; the two versions
alternate, window by window; median (min .. max) of the repeats.  The second part evaluates the error ratios of tests/berhu_cases.py
(error against the float64 oracle over the error of the reference formula in fp32 on the CPU).  Needs a GPU: there is no fallback.

  python tools/berhu.py [--out profiles/berhu.md] [--repeats 5]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import berhu, berhu_own_car  # noqa: E402

WINDOW_MS = 100.0
HBM_MEASURED_GBS = 6362.5      # bench.py MEASURED_PEAKS["hbm_gbs"]: the streaming rate measured on this GPU model
HBM_NOMINAL_GBS = 8000.0


def torch_berhu(input, target, mask, apply_log=False):
    """the reference's formula, loss.py:5-15"""
    threshold = 0.2
    if apply_log:
        input, target = torch.log(1 + input), torch.log(1 + target)
    absdiff = torch.abs(target - input) * mask
    C = threshold * torch.max(absdiff).item()
    return torch.mean(torch.where(absdiff <= C, absdiff, (absdiff * absdiff + C * C) / (2 * C)))


def keep_tensor(x):
    keep = torch.ones(x.shape, device=x.device)
    keep[:, :, int(x.shape[2] * 0.9):, :] = 0
    return keep


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def timed_pair(f, g, repeats, warmup=3):
    """two versions, alternating window by window -> ((median, min, max) of f, the same of g)"""
    inner = []
    for fn in (f, g):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        inner.append(int(min(2000, max(1, round(WINDOW_MS / max(_window(fn, 3), 1e-3))))))
    ms = ([], [])
    for _ in range(repeats):
        ms[0].append(_window(f, inner[0]))
        ms[1].append(_window(g, inner[1]))
    return tuple((float(np.median(m)), float(min(m)), float(max(m))) for m in ms)


def step(loss_of, x):
    x.grad = None
    loss_of(x).backward()


def error_ratios(dev):
    import berhu_cases as C
    rows = []
    for seed, shape, mode in C.GENERATED:
        c, (want_loss, want_grad, _), (ref_loss, ref_grad) = C.generated(seed, shape, mode)
        loss, _, dx = C.run_ops(dev, c)
        e_l, r_l = abs(float(loss[0]) - want_loss), abs(ref_loss - want_loss)
        finite = bool(np.all(np.isfinite(ref_grad)))
        e_g = float(np.abs(dx.astype(np.float64) - want_grad).max())
        r_g = float(np.abs(ref_grad - want_grad).max()) if finite else float("nan")
        ratio = lambda e, r: "%.2f" % (e / r) if r > 0 else ("0" if e == 0 else "inf")      # noqa: E731
        rows.append("| %d | %s | %s | %.2e | %.2e | %s | %.2e | %.2e | %.2e | %s | %.2e |" % (
            seed, C.case_id(shape), mode, r_l, e_l, ratio(e_l, r_l), 4 * C.EPS32 * abs(want_loss), r_g, e_g,
            ratio(e_g, r_g) if finite else "-", 4 * C.EPS32 * float(np.abs(want_grad).max())))
    return rows


MODE_NAMES = ("plain", "apply_log", "own-car crop", "own-car crop, apply_log")
KERNEL_BYTES = {"berhu_max_kernel": 8, "berhu_sum_kernel": 8, "berhu_finish_kernel": 0, "berhu_backward_kernel": 12}


def summarise_trace(path, shape=(16, 512, 1024), steps=10, skip=2):
    """the kernel trace (CSV) of a --kernels-only run -> markdown lines: per mode the median duration of each of the four kernels
    over the steps after the first ``skip``, and the rate on the bytes that kernel must move"""
    import csv
    import re
    rows = [r for r in csv.DictReader(open(path)) if "berhu_" in r["Kernel_Name"]]
    assert len(rows) == len(MODE_NAMES) * steps * 4, "%d berhu dispatches in %s" % (len(rows), path)
    n = shape[0] * shape[1] * shape[2]
    lines = ["## Kernel times, %d x 1 x %d x %d" % shape, "",
             "From `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/berhu.py --kernels-only` (a run of its own; %d "
             "steps per mode, the first %d left out): median microseconds per launch and the rate on the bytes that launch must move.  "
             "The difference between the sum and the time per call above is launch gaps and the host." % (steps, skip), "",
             "| mode | kernel | us | B/element | GB/s | of %.0f measured |" % HBM_MEASURED_GBS, "|---|---|---|---|---|---|"]
    for mi, mode in enumerate(MODE_NAMES):
        chunk = rows[mi * steps * 4 + skip * 4:(mi + 1) * steps * 4]
        per = {}
        for r in chunk:
            k = re.search(r"berhu_\w+_kernel", r["Kernel_Name"]).group(0)
            per.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        total = 0.0
        for k, v in per.items():
            med = float(np.median(v))
            total += med
            bpe = KERNEL_BYTES[k] + (4 if mi < 2 and KERNEL_BYTES[k] else 0)
            gbs = bpe * n / med / 1e3
            lines.append("| %s | `%s` | %.2f | %d | %s | %s |" % (mode, k, med, bpe, "%.0f" % gbs if bpe else "-",
                                                            "%.0f %%" % (100 * gbs / HBM_MEASURED_GBS) if bpe else "-"))
        lines.append("| %s | sum | %.2f | | | |" % (mode, total))
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise-trace", metavar="CSV", help="append the kernel-time table of a --kernels-only trace to --out and exit "
                    "(needs no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "berhu.md"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true",
                    help="ten steps of every mode of the first workload and nothing else: the run to put under a kernel trace "
                         "(rocprofv3 --kernel-trace --stats -- python tools/berhu.py --kernels-only), whose per-kernel times "
                         "separate the kernels from the launch gaps and the host")
    args = ap.parse_args()
    if args.summarise_trace:
        lines = summarise_trace(args.summarise_trace)
        open(args.out, "a").write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    assert torch.cuda.is_available(), "tools/berhu.py measures on the GPU"
    dev = "cuda"
    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t      # noqa: E731
    lines = ["# BerHu pseudo-depth loss: times and errors", "",
             "Written by `python tools/berhu.py` on %s (torch %s)." % (torch.cuda.get_device_name(0), torch.__version__), "",
             "Milliseconds for forward plus backward: one pair of device events around as many back-to-back calls as fill about %d ms, "
             "after a warm-up, the two versions alternating window by window; median (min .. max) of %d windows.  The HIP path is four "
             "launches (block maxima; C and block sums; the fold; the gradient) and never returns to the host; the torch formula is the "
             "reference's (loss.py:5-15), its `.item()` included, with autograd's backward, on the same device.  In the own-car rows the "
             "HIP path is `berhu_own_car` (no mask tensor) and the torch formula builds the keep tensor per call, as both callers did.  "
             "Bytes the HIP path must move: 2 x 8 per element forward, 12 backward, 4 more per pass with a mask tensor; the rate is those "
             "bytes over the whole time, launch gaps included.  One shared machine, one run." % (WINDOW_MS, args.repeats), ""]
    for B, Hh, W in ((16, 512, 1024), (2, 1024, 2048)):
        n = B * Hh * W
        gen = torch.Generator(device=dev).manual_seed(0)
        x = (torch.rand((B, 1, Hh, W), device=dev, generator=gen) * 0.998 + 1e-3).requires_grad_(True)
        t = torch.rand((B, 1, Hh, W), device=dev, generator=gen) * 0.998 + 1e-3
        ones = torch.ones((B, 1, Hh, W), device=dev)
        lines += ["## %d x 1 x %d x %d" % (B, Hh, W), "", "| mode | HIP ms | torch ms | torch / HIP | HIP bytes | GB/s | of %.0f measured | of %.0f "
                  "nominal |" % (HBM_MEASURED_GBS, HBM_NOMINAL_GBS), "|---|---|---|---|---|---|---|---|"]
        modes = (("plain", lambda v: berhu(v, t, ones), lambda v: torch_berhu(v, t, ones), True),
                 ("apply_log", lambda v: berhu(v, t, ones, apply_log=True), lambda v: torch_berhu(v, t, ones, apply_log=True), True),
                 ("own-car crop", lambda v: berhu_own_car(v, t), lambda v: torch_berhu(v, t, keep_tensor(v)), False),
                 ("own-car crop, apply_log", lambda v: berhu_own_car(v, t, apply_log=True),
                  lambda v: torch_berhu(v, t, keep_tensor(v), apply_log=True), False))
        if args.kernels_only:
            for name, hip, ref, has_mask in modes:
                for _ in range(10):
                    step(hip, x)
            torch.cuda.synchronize()
            return
        for name, hip, ref, has_mask in modes:
            a, b = hip(x), ref(x)
            rel = abs(float(a) - float(b)) / abs(float(b))
            assert rel < 1e-5, "the two formulations disagree in %s: %g" % (name, rel)
            t_h, t_t = timed_pair(lambda: step(hip, x), lambda: step(ref, x), args.repeats)
            nbytes = n * (2 * 8 + 12 + (3 * 4 if has_mask else 0))
            gbs = nbytes / t_h[0] / 1e6
            lines.append("| %s | %s | %s | %.2f | %d B/element | %.0f | %.0f %% | %.0f %% |" % (
                name, fmt(t_h), fmt(t_t), t_t[0] / t_h[0], nbytes // n, gbs, 100 * gbs / HBM_MEASURED_GBS, 100 * gbs / HBM_NOMINAL_GBS))
        lines.append("")
        del x, t, ones
        torch.cuda.empty_cache()
    lines += ["## Error ratios of the test cases", "",
              "The cases of `tests/berhu_cases.py` (`GENERATED`), gradient with g = 1: errors against the float64 oracle of the reference "
              "formula in fp32 on the CPU (e_ref) and of the kernels (e_hip), their ratio (the tests allow 3, or the floor), for the loss "
              "and for the gradient's maximum error.", "",
              "| seed | shape | mode | loss e_ref | loss e_hip | ratio | loss floor | grad e_ref | grad e_hip | ratio | grad floor |",
              "|---|---|---|---|---|---|---|---|---|---|---|"] + error_ratios(dev) + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
