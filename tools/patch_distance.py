#!/usr/bin/env python
"""Measure the patch-wise (directed Chamfer) feature distances on the GPU and write profiles/patch_distance.md.

Workloads: the Cityscapes pool (N = 2975) and the CamVid pool (N = 367) with u3 features pooled to C = 256 channels x 4 x 8
positions (P = 32), p = 1 and p = 2.  In the same run, alternating windows:
  (a) the reference's formulation in torch on the same device and bank: chunks of 200 images of torch.cdist over the [N*P, C]
      patch vectors, min over the patches of the other image, mean over the own; with its peak memory;
  (b) hipops.labelsel_distance on the 2975 x 8192 bank: the direct-form kernel of the plain distance matrix, the yardstick of the
      arithmetic rate.
Times are device events around windows of back-to-back calls after a warm-up, median (min .. max) of the repeats.  The rate is
time per term evaluation |x - y|^p, counting the image pairs i <= j only for both kernels (each evaluates a pair once).
Needs a GPU: there is no fallback.

  python tools/patch_distance.py [--out profiles/patch_distance.md] [--repeats 5] [--ref-full-p1]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from improving_segmentation_with_selfsupervised_depth_amd import hipops as H  # noqa: E402

WINDOW_MS = 300.0      # a timed window holds as many back-to-back calls as fill about this much
CHUNK = 200            # images per torch.cdist block in the reference


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def _inner(fn):
    return int(min(2000, max(1, round(WINDOW_MS / max(_window(fn, 1), 1e-3)))))


def alternating(fns, repeats):
    """ms per call of every function: median (min .. max) over `repeats` windows, the functions' windows interleaved"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    inner = [_inner(f) for f in fns]
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, f in enumerate(fns):
            ms[k].append(_window(f, inner[k]))
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def make_bank(N, C, P, seed):
    """low intrinsic dimension + noise, channels of different scale: [N, C*P] float32 on the device"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    latent = torch.rand((N, P, 16), generator=g)
    f = latent @ torch.randn((16, C), generator=g) + 0.1 * torch.randn((N, P, C), generator=g)      # [N, P, C]
    f = f * torch.linspace(0.5, 4.0, C) + 3.0
    return f.permute(0, 2, 1).reshape(N, C * P).contiguous().cuda()


def ref_chunk(v, s, n, N, P, p):
    d = torch.cdist(v[s * P:(s + n) * P], v, p=p).reshape(n, P, N, P).permute(0, 2, 1, 3)
    return d.min(dim=-1).values.mean(dim=-1)


def ref_full(v, N, P, p):
    return torch.cat([ref_chunk(v, s, min(CHUNK, N - s), N, P, p) for s in range(0, N, CHUNK)])


def fmt(t):
    return "%.3f (%.3f .. %.3f)" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_distance.md"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-full-p1", action="store_true", help="time the reference's p = 1 formulation on the whole Cityscapes pool "
                    "(default: one chunk of 200 images, scaled)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/patch_distance.py measures on the GPU"
    C, h = 256, 4
    P = h * 2 * h
    lines = ["# Patch-wise feature distances: times and rates", "",
             "Written by `tools/patch_distance.py` on %s (torch %s)." % (torch.cuda.get_device_name(0), torch.__version__), "",
             "Milliseconds per call; a timed window is one pair of device events around as many back-to-back calls as fill about %d ms "
             "(at least one) after a warm-up; median (min .. max) of %d windows, the windows of one table row interleaved.  One shared "
             "machine, one run: differences below the spread mean nothing.  Terms: |x - y|^p evaluations over the image pairs i <= j, "
             "N (N + 1) / 2 * P^2 * C for the patch kernel and N (N + 1) / 2 * D for `labelsel_distance`." % (WINDOW_MS, args.repeats), ""]
    # ---------------------------------------------------------------- the yardstick: labelsel_distance at 2975 x 8192
    ybank = make_bank(2975, C, P, 1)
    yout = torch.empty((2975, 2975), device="cuda")
    table = ["| workload | p | patch kernel, ms | ps per term | `labelsel_distance` 2975 x 8192, ms | ps per term | ratio | reference formulation "
             "in torch, ms | its peak memory |", "|---|---|---|---|---|---|---|---|---|"]
    checks, ratios = [], []
    for name, N in (("Cityscapes, N = 2975", 2975), ("CamVid, N = 367", 367)):
        bank = make_bank(N, C, P, 2)
        v = bank.reshape(N, C, P).permute(0, 2, 1).reshape(N * P, C).contiguous()
        out = torch.empty((N, N), device="cuda")
        for p in (2, 1):
            whole = N <= CHUNK * 4 or p == 2 or args.ref_full_p1
            ref = (lambda: ref_full(v, N, P, p)) if whole else (lambda: ref_chunk(v, 0, CHUNK, N, P, p))
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ref()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            tk, ty, tr = alternating([lambda: H.labelsel_patch_distance(bank, C, P, p, out=out),
                                      lambda: H.labelsel_distance(ybank, p, out=yout), ref], args.repeats)
            terms_k = N * (N + 1) / 2 * P * P * C
            terms_y = 2975 * 2976 / 2 * C * P
            ps_k, ps_y = tk[0] * 1e9 / terms_k, ty[0] * 1e9 / terms_y
            ref_txt = fmt(tr) if whole else "%s for one chunk of %d images; x %.3f = %.0f for the pool (scaled, not measured)" % (
                fmt(tr), CHUNK, N / CHUNK, tr[0] * N / CHUNK)
            table.append("| %s | %d | %s | %.4f | %s | %.4f | %.2f | %s | %.2f GB |" % (name, p, fmt(tk), ps_k, fmt(ty), ps_y, ps_k / ps_y,
                                                                                  ref_txt, peak / 1e9))
            ratios.append(ps_k / ps_y)
            print(table[-1], flush=True)
            if N <= CHUNK * 4:      # the whole matrix against the reference's formulation and float64 on a sample of rows
                d_k = H.labelsel_patch_distance(bank, C, P, p)
                d_r = ref_full(v, N, P, p)
                d_r.fill_diagonal_(0)
                rows = torch.arange(0, N, 23, device="cuda")
                v64 = v.double().reshape(N, P, C)
                t64 = torch.stack([torch.cdist(v64[i:i + 1].expand(N, P, C), v64, p=p).min(dim=-1).values.mean(dim=-1) for i in rows.tolist()])
                t64[torch.arange(len(rows)), rows] = 0
                e_k, e_r = (d_k[rows].double() - t64).abs(), (d_r[rows].double() - t64).abs()
                checks.append("%s, p = %d: %d rows of the matrix against float64: kernel max %.3e rms %.3e; reference formulation in fp32 "
                              "max %.3e rms %.3e; values around %.2f.  Kernel diagonal exactly 0: %s; two runs equal bit for bit: %s."
                              % (name, p, len(rows), e_k.max(), e_k.pow(2).mean().sqrt(), e_r.max(), e_r.pow(2).mean().sqrt(), t64.mean(),
                                 bool((d_k.diagonal() == 0).all()), bool(torch.equal(d_k, H.labelsel_patch_distance(bank, C, P, p)))))
                if float(e_r.max()) > 1e-2 * float(t64.mean()):
                    checks[-1] += ("  The torch formulation's result is NOT the float64 result here (its error is of the size of the "
                                   "values): its time in the table is not the time of a correct evaluation.")
                print(checks[-1], flush=True)
        del bank, v, out
    lines += table + [""] + checks + [""]
    worst = max(ratios)
    lines += ["Expectation: a per-term time within 1.5x of `labelsel_distance`'s from the same run (the margin for the segmented-minimum "
              "epilogue and the reduction over 256 terms instead of 8192).  Largest ratio measured: %.2f -- %s." %
              (worst, "met" if worst <= 1.5 else "MISSED"), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
