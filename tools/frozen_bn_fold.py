"""Frozen-BatchNorm fold (functional.frozen_bn_fold) measured on the GPU: the dilated ResNet-101 encoder in eval mode under
no_grad at 16 x 3 x 512 x 1024, switch off and on in ONE process -- end-to-end time (device events, the two settings alternating),
time per layer class from the bracketed launches (hipops.PROFILE), bytes saved by count, and the error ratios of the test
suite's gate (tests/frozen_bn_cases.py).  Writes a markdown report:

    python tools/frozen_bn_fold.py --out profiles/frozen_bn_fold.md

Needs the MI355X: there is no CPU path."""
import argparse
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn      # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H            # noqa: E402
from improving_segmentation_with_selfsupervised_depth_amd.models.resnet_encoder import ResnetEncoder   # noqa: E402

TAG = re.compile(r"(\d+)\+(\d+)->(\d+) k(\d+) s(\d+) d(\d+) ")


def conv_class(tag):
    if tag.startswith("stem"):
        return "stem 7x7/2"
    m = TAG.match(tag)
    k, s, d = int(m.group(4)), int(m.group(5)), int(m.group(6))
    if k == 1:
        return "1x1"
    if "wino" in tag:
        return "3x3 Winograd"
    if d > 1:
        return "3x3 dilated"
    return "3x3 direct (stride %d)" % s


def out_elems(rec):
    """output elements of a conv_fwd record, from its algorithmic FLOPs and its tag"""
    tag = rec[4]
    if tag.startswith("stem"):
        return rec[1] / (2.0 * int(re.match(r"stem c(\d+)", tag).group(1)) * 49)
    m = TAG.match(tag)
    return rec[1] / (2.0 * (int(m.group(1)) + int(m.group(2))) * int(m.group(4)) ** 2)


def profiled_pass(enc, img, on):
    """one forward with every launch bracketed -> {class: [pairs, conv ms, BatchNorm ms, elements]}"""
    H.PROFILE, H.PROFILE_PERIOD = [], 1
    H.profile_step(0)
    with torch.no_grad(), Fn.frozen_bn_fold(on):
        enc.forward_nhwc(img)
    torch.cuda.synchronize()
    recs, H.PROFILE = H.PROFILE, None
    out, last = {}, None
    for r in recs:
        ms = r[2].elapsed_time(r[3])
        if r[0] == "conv_fwd":
            cls = conv_class(r[4])
            n = out_elems(r)
            if " res" in r[4]:
                cls += " + residual"
            last = [cls, n, ms]
            c = out.setdefault(cls, [0, 0.0, 0.0, 0.0])
            c[0] += 1; c[1] += ms; c[3] += n
        elif r[0] == "hbm_bn_apply" and last is not None:
            cls, n, cms = last
            if r[1] / n > 10.0 and not cls.endswith("residual"):       # 12 B per element: the pass also read a residual
                c = out[cls]
                c[0] -= 1; c[1] -= cms; c[3] -= n
                cls += " + residual"
                c = out.setdefault(cls, [0, 0.0, 0.0, 0.0])
                c[0] += 1; c[1] += cms; c[3] += n
            out[cls][2] += ms
            last = None
    return out


def timed(enc, img, on, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad(), Fn.frozen_bn_fold(on):
        s.record()
        for _ in range(steps):
            enc.forward_nhwc(img)
        e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn_fold.md"))
    ap.add_argument("--size", type=int, nargs=4, default=[16, 3, 512, 1024])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--no-errors", action="store_true", help="skip the error ratios of the test cases")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    import frozen_bn_cases as FC
    lines = ["# Frozen BatchNorm folded into the convolutions of no-grad forward passes", "",
             "Written by `tools/frozen_bn_fold.py` on %s; one process, switch off (the parent's launches) and on alternating." %
             torch.cuda.get_device_name(0), ""]

    enc = FC.randomize(ResnetEncoder(101, False, replace_stride_with_dilation=[False, False, True]), 3).cuda().eval()
    img = torch.rand(*a.size, generator=torch.Generator().manual_seed(1)).cuda()
    for on in (False, True, False, True):                      # warm-up: code objects, allocator, the fold itself
        timed(enc, img, on, 2)
    t = {False: [], True: []}
    for _ in range(a.rounds):
        for on in (False, True):
            t[on].append(timed(enc, img, on, a.steps))
    Fn.fusion_report(reset=True)
    with torch.no_grad(), Fn.frozen_bn_fold():
        f_on = enc.forward_nhwc(img)
    rep = Fn.fusion_report(reset=True)["frozen_bn_folded"]
    with torch.no_grad():
        f_off = enc.forward_nhwc(img)
    dev = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(f_on, f_off)]
    del f_on, f_off
    fmt = lambda v: ", ".join("%.2f" % x for x in v)
    lines += ["## ResNet-101 (dilated layer4) encoder, eval, no_grad, %d x %d x %d x %d" % tuple(a.size), "",
              "End to end, ms per forward (device events around %d forwards, %d rounds each, alternating):" % (a.steps, a.rounds), "",
              "| switch | rounds (ms) | median (ms) |", "|---|---|---|"]
    med = {}
    for on in (False, True):
        v = sorted(t[on])
        med[on] = 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])
        lines.append("| %s | %s | %.2f |" % ("on" if on else "off", fmt(t[on]), med[on]))
    lines += ["", "Folded / unfolded = %.3f.  Pairs folded: %d, left unfused: %d.  Largest difference of a feature between the two "
              "settings, relative to the feature's largest value: %.2e." % (med[True] / med[False], rep["taken"], rep["missed"], max(dev)), ""]

    off, on = profiled_pass(enc, img, False), profiled_pass(enc, img, True)
    for _ in range(2):                                        # three bracketed passes per setting, summed
        for dst, src in ((off, profiled_pass(enc, img, False)), (on, profiled_pass(enc, img, True))):
            for k, v in src.items():
                for i in (1, 2):
                    dst[k][i] += v[i]
    lines += ["Per layer class, one forward (every launch bracketed by events, mean of three passes; the brackets drain the stream, so",
              "the sums are larger than the end-to-end time).  Bytes saved by count: 8 B per output element of a folded pair (the",
              "normalisation pass's read and write of the convolution output).", "",
              "| class | pairs | unfolded: conv + BatchNorm (ms) | folded: conv (ms) | folded / unfolded | bytes saved (MB) |", "|---|---|---|---|---|---|"]
    slower = []
    for cls in sorted(off):
        n, cms, bms, el = off[cls]
        if n == 0:
            continue
        f = on.get(cls)
        if f is None or f[2] > 0.0:
            lines.append("| %s | %d | %.3f + %.3f | not folded | -- | 0 |" % (cls, n, cms / 3, bms / 3))
            continue
        ratio = f[1] / (cms + bms)
        if ratio > 1.0:
            slower.append(cls)
        lines.append("| %s | %d | %.3f + %.3f | %.3f | %.3f | %.1f |" % (cls, n, cms / 3, bms / 3, f[1] / 3, ratio, 8.0 * el / 1e6))
    lines += ["", "Classes slower folded than unfolded: %s." % (", ".join(slower) if slower else "none"), ""]

    if not a.no_errors:
        report = []
        for name in sorted(FC.BLOCKS):
            FC.run_block("cuda", name, report)
        for nl in (18, 50):
            FC.run_encoder("cuda", nl, report=report)
        lines += ["## Error against float64: folded / unfolded (gate: 3.0 for both)", "",
                  "The cases of `tests/frozen_bn_cases.py` (blocks at 2 x 10 x 14, encoders at 2 x 3 x 64 x 128).", "",
                  "| tensor | max error folded | max error unfolded | ratio | rms folded | rms unfolded | ratio |", "|---|---|---|---|---|---|---|"]
        for what, m1, m0, r1, r0 in report:
            lines.append("| %s | %.3e | %.3e | %.2f | %.3e | %.3e | %.2f |" % (what, m1, m0, m1 / m0, r1, r0, r1 / r0))
        lines += ["", "Largest ratio: max %.2f, rms %.2f." % (max(r[1] / r[2] for r in report), max(r[3] / r[4] for r in report)), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
