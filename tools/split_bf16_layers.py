"""Per-launch cost and error of the split-bf16 operand mode (segsde_conv_desc.compute = 2) against the fp32 kernels
(compute = 0) on the direct-route geometries of profiles/layers_r06_latest.txt: the 1x1 bottleneck layers, the dilated ASPP
branches and their weight gradients, batch 16 as in the benchmark step.

    python tools/split_bf16_layers.py [--reps 7] [--iters 20] [--no-error] [--out FILE.md]

The modes are timed in the same process on the same random tensors, interleaved (f32, bf16x9, f32, ...), each sample
a device-event window around `iters` back-to-back launches after a warm-up of every mode; the table reports the median over
`reps` samples and the spread of the fp32 samples.  TFLOP/s is executed FLOPs (dead tap rows of the dilated windows are not
counted) over that time: the weight gradient includes its split-K reduce kernel.  Errors are max / rms against a float64
convolution of the same inputs on the CPU.  `taken` is segsde_conv_compute_taken: what the launcher dispatches to."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn   # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H        # noqa: E402

MODES = (("f32", 0), ("bf16x9", 2))
# (C, Cout, k, dil, H, W, batch of the error check)
LAYERS = [(256, 1024, 1, 1, 32, 64, 4), (1024, 256, 1, 1, 32, 64, 4), (512, 2048, 1, 1, 32, 64, 4), (2048, 512, 1, 1, 32, 64, 4),
          (1024, 2048, 1, 1, 32, 64, 4), (2048, 256, 1, 1, 32, 64, 4), (128, 512, 1, 1, 64, 128, 2), (512, 128, 1, 1, 64, 128, 2),
          (64, 256, 1, 1, 128, 256, 1), (256, 64, 1, 1, 128, 256, 1), (64, 64, 1, 1, 512, 1024, 1),
          (2048, 256, 3, 6, 32, 64, 2), (2048, 256, 3, 12, 32, 64, 2), (2048, 256, 3, 18, 32, 64, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-error", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(1)
    lines = ["| geometry | direction | taken | f32 ms (spread) | f32 TF | bf16x9 ms | TF | x f32 | max err f32 / x9 | rms err f32 / x9 |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for C, Co, k, dil, Hh, W, eb in LAYERS:
        pad = dil * (k // 2)
        geoms = {}
        for name, mode in MODES:
            with Fn.conv_compute(name):
                geoms[name] = H.ConvGeom(C, Co, k, 1, dil, pad, False, 0, False)
        B = a.batch
        x = torch.relu(torch.randn(B, Hh, W, C, device=dev))
        dy = torch.randn(B, Hh, W, Co, device=dev)
        w = torch.randn(Co, C, k, k, device=dev) * (2.0 / (k * k * C)) ** 0.5
        wp, wdp = H.pack_weight_both(w)
        flops = 2.0 * B * Hh * W * C * Co * k * k
        calls = {"fwd": lambda g: H.conv_forward(g, x, None, wp, None), "dgrad": lambda g: H.conv_dgrad(g, dy, wdp, w, (Hh, W))[0],
                 "wgrad": lambda g: H.conv_wgrad(g, x, None, dy)}
        err = {}
        if not a.no_error:
            xs, dys = x[:eb], dy[:eb]
            a0 = xs.cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
            wq = w.cpu().double().requires_grad_(True)
            y = F.conv2d(a0, wq, padding=pad, dilation=dil)
            y.backward(dys.cpu().double().permute(0, 3, 1, 2))
            want = {"fwd": y.detach().permute(0, 2, 3, 1), "dgrad": a0.grad.permute(0, 2, 3, 1), "wgrad": wq.grad}
            for name, mode in MODES:
                g = geoms[name]
                got = {"fwd": H.conv_forward(g, xs, None, wp, None), "dgrad": H.conv_dgrad(g, dys, wdp, w, (Hh, W))[0],
                       "wgrad": H.conv_wgrad(g, xs, None, dys)}
                for d in got:
                    e = got[d].cpu().double() - want[d]
                    err[name, d] = (float(e.abs().max()), float(e.pow(2).mean().sqrt()))
        for d, call in calls.items():
            frac = H._live_tap_frac(geoms["f32"], Hh, W, wgrad=(d == "wgrad"))
            tk = [H.conv_compute_taken(geoms[n], B, Hh, W, d) for n, _ in MODES]
            for n, _ in MODES:                                   # warm-up: code objects, workspaces
                for _ in range(3):
                    call(geoms[n])
            torch.cuda.synchronize()
            samples = {n: [] for n, _ in MODES}
            for _ in range(a.reps):
                for n, _ in MODES:
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(a.iters):
                        call(geoms[n])
                    e.record()
                    e.synchronize()
                    samples[n].append(s.elapsed_time(e) / a.iters)
            med = {n: statistics.median(v) for n, v in samples.items()}
            tf = {n: flops * frac / (med[n] * 1e-3) / 1e12 for n in med}
            spread = (max(samples["f32"]) - min(samples["f32"])) / med["f32"]
            row = "| %d->%d k%d d%d %dx%d | %s | %s | %.3f (%.1f%%) | %.1f | %.3f | %.1f | %.2f |" % (
                C, Co, k, dil, Hh, W, d, "/".join(map(str, tk)), med["f32"], 100 * spread, tf["f32"], med["bf16x9"], tf["bf16x9"],
                med["f32"] / med["bf16x9"])
            if err:
                row += " %.2e / %.2e | %.2e / %.2e |" % tuple(err[n, d][i] for i in (0, 1) for n, _ in MODES)
            else:
                row += " - | - |"
            print(row, flush=True)
            lines.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
