#!/usr/bin/env python
"""Time the device batch builder (loader/device_batch.py) against the same work done by Pillow on one host core.

    python tools/device_batch.py [--batch 16] [--crop 512 1024] [--sources 512x1024 1024x2048] [--repeats 9] [--cpu-samples 7]
    python tools/device_batch.py --color-aug [--batch 16] [--crop 512 1024]      # the colour-augmentation leg alone

GPU: device events around (a) the kernels alone -- three crop launches, three pyramid launches, the label launch -- and (b) the
whole ``builder(...)`` call, which adds the host's K / inv_K arithmetic and three small copies; warm-up, then the median and the
spread of ``--repeats`` samples, each sample ``--inner`` calls back to back.  The bytes the stage must move are counted from the
shapes (below) and divided by the kernel time.
CPU: flip / crop / three chained LANCZOS resizes / ToTensor per frame, the label table as one full-image comparison per id, K / inv_K per scale -- the
reference's __getitem__ without the decode, which both paths need -- on ONE thread; samples per second, and that times 16 as the
(linear-scaling, so optimistic) rate of 16 loader workers.  Prints one JSON line.
``--color-aug``: the whole ``builder(...)`` call on crop-sized frames without colour augmentation, with every sample augmented and
with the jitter the builder draws itself (about half the samples); the two jitter launches alone (tables already on the device)
against the bytes they must move -- the uint8 level-0 image read by both, the float32 image written once; and the four PIL
operations of ColorJitter on the three frames of a sample on one host core.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from improving_segmentation_with_selfsupervised_depth_amd.loader.device_batch import DeviceBatchBuilder  # noqa: E402

FRAMES = (0, -1, 1)
HBM_PEAK = 8.0e12          # bytes / s
LUT_FILE = os.path.join(ROOT, "tests", "golden", "device_batch.npz")     # "lut": the label table recorded from the reference


def label_table():
    return np.load(LUT_FILE, allow_pickle=False)["lut"].astype(np.int64)


def encode_by_comparisons(mask, lut):
    """the host path's cost model: one full-image comparison + masked assignment per label id that the table changes (34 for the
    Cityscapes table), as a per-id loop does; ids in ascending order, targets written to a second array so no id is hit twice"""
    out = mask.copy()
    for v in np.flatnonzero(lut != np.arange(256)):
        out[mask == v] = lut[v]
    return out


def stage_bytes(B, ch, cw, scales, n_frames, labels):
    """what the stage has to read and write at the least: the crop window of every frame, every uint8 level once as output and
    once as the next level's input, every float level once, the label window in, the int64 map out"""
    px = B * ch * cw
    rd = wr = 0
    for s in range(scales):
        p = px // 4 ** s
        rd += n_frames * 3 * (p if s == 0 else px // 4 ** (s - 1))
        wr += n_frames * 3 * p * (4 + (1 if s < scales - 1 else 0))
    if labels:
        rd += px
        wr += 8 * px
    return rd, wr


def gpu_side(args, H, W):
    dev = torch.device("cuda")
    B, (ch, cw) = args.batch, args.crop
    g = torch.Generator(device="cpu").manual_seed(0)
    frames = {f: torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev) for f in FRAMES}
    lbl = torch.randint(0, 34, (B, H, W), dtype=torch.uint8, generator=g).to(dev)
    lut = label_table()
    b = DeviceBatchBuilder(H, W, ch, cw, label_lut=lut, n_classes=19)
    crops, flips = b.draw(B)
    crop_d = torch.from_numpy(crops).to(dev) if (ch, cw) != (H, W) else None
    from improving_segmentation_with_selfsupervised_depth_amd import hipops
    lut_d = torch.from_numpy(lut).to(dev)

    def kernels():
        b.colors(frames, crop_d, None, {})
        hipops.batchprep_labels(lbl, crop_d, None, ch, cw, lut_d, None, 250, 19, False)

    def whole():
        b(frames, lbl=lbl, crops=crops, flips=flips)

    out = {}
    for name, fn in (("kernels", kernels), ("call", whole)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.inner)
        out[name + "_ms"] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "samples": len(ms)}
    rd, wr = stage_bytes(B, ch, cw, 4, len(FRAMES), True)
    t = out["kernels_ms"]["median"] * 1e-3
    out.update(read_mb=rd / 1e6, write_mb=wr / 1e6, achieved_gbs=(rd + wr) / t / 1e9, frac_of_8tbs=(rd + wr) / t / HBM_PEAK,
               img_per_s_kernels=B / t, img_per_s_call=B / (out["call_ms"]["median"] * 1e-3))
    return out


def cpu_side(args, H, W):
    from PIL import Image
    torch.set_num_threads(1)
    ch, cw = args.crop
    rng = np.random.RandomState(0)
    imgs = [Image.fromarray(rng.randint(0, 256, (H, W, 3), dtype=np.uint8), "RGB") for _ in FRAMES]
    lbl = Image.fromarray(rng.randint(0, 34, (H, W), dtype=np.uint8), "L")
    to_tensor = lambda im: torch.from_numpy(np.ascontiguousarray(np.asarray(im, dtype=np.uint8).reshape(im.size[1], im.size[0], -1)
                                                                 .transpose(2, 0, 1))).to(torch.float32).div(255)
    b = DeviceBatchBuilder(H, W, ch, cw)
    lut = label_table()

    def sample(flip):
        x1, y1 = (W - cw) // 2, (H - ch) // 2
        box = (x1, y1, x1 + cw, y1 + ch)
        out = {}
        for f, im in zip(FRAMES, imgs):
            if flip:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            if (ch, cw) != (H, W):
                im = im.crop(box)
            for s in range(4):
                im = im.resize((cw >> s, ch >> s), Image.LANCZOS)
                out[("color", f, s)] = to_tensor(im)
                if s == 0:
                    out[("color_aug", f, 0)] = to_tensor(im)
        lb = lbl.transpose(Image.FLIP_LEFT_RIGHT) if flip else lbl
        if (ch, cw) != (H, W):
            lb = lb.crop(box)
        out["lbl"] = torch.from_numpy(encode_by_comparisons(np.array(lb, dtype=np.uint8), lut)).long()
        out["K"] = b.intrinsics([(x1, y1)], [flip])
        return out

    sample(False)
    dt = []
    for i in range(args.cpu_samples):
        t0 = time.perf_counter()
        sample(bool(i & 1))
        dt.append(time.perf_counter() - t0)
    med = statistics.median(dt)
    return {"ms_per_sample": {"median": med * 1e3, "min": min(dt) * 1e3, "max": max(dt) * 1e3, "samples": len(dt)},
            "samples_per_s_one_core": 1.0 / med, "samples_per_s_16_cores_linear": 16.0 / med}


def timed(fn, repeats, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "samples": len(ms)}


def color_aug_gpu(args):
    import random
    from improving_segmentation_with_selfsupervised_depth_amd import _lib, hipops
    from improving_segmentation_with_selfsupervised_depth_amd.loader.device_batch import jitter_tables
    dev = torch.device("cuda")
    B, (ch, cw) = args.batch, args.crop
    g = torch.Generator(device="cpu").manual_seed(0)
    frames = {f: torch.randint(0, 256, (B, ch, cw, 3), dtype=torch.uint8, generator=g).to(dev) for f in FRAMES}
    plain = DeviceBatchBuilder(ch, cw)
    aug = DeviceBatchBuilder(ch, cw, color_aug=True)
    random.seed(0)
    crops, flips, drawn = aug.draw_with_jitter(B)
    rng = np.random.RandomState(0)
    every = {"apply": np.ones(B, bool), "factors": np.column_stack([rng.uniform(0.8, 1.2, (B, 3)), rng.uniform(-0.1, 0.1, B)]),
             "order": np.stack([rng.permutation(4) for _ in range(B)]).astype(np.uint8)}
    out = {"samples_augmented_by_the_drawn_jitter": int(drawn["apply"].sum()),
           "call_plain_ms": timed(lambda: plain(frames, crops=crops, flips=flips), args.repeats, args.inner),
           "call_every_sample_ms": timed(lambda: aug(frames, crops=crops, flips=flips, jitter=every), args.repeats, args.inner),
           "call_drawn_jitter_ms": timed(lambda: aug(frames, crops=crops, flips=flips, jitter=drawn), args.repeats, args.inner)}
    # the two launches alone: level-0 uint8 image and tables already on the device
    F = len(FRAMES)
    u8 = torch.randint(0, 256, (F, B, 3, ch, cw), dtype=torch.uint8, generator=g).to(dev)
    alpha, shift = jitter_tables(every["factors"])
    tb = [torch.from_numpy(a).to(dev) for a in (every["apply"].astype(np.uint8), alpha, shift, every["order"])]
    sums = torch.empty(F * B, dtype=torch.int32, device=dev)
    f32 = torch.empty((F, B, 3, ch, cw), dtype=torch.float32, device=dev)
    lib, p = _lib.lib(), lambda t: t.data_ptr()
    stream = hipops._stream(u8)

    def launches():
        _lib.check(lib.segsde_batchprep_color_jitter(p(u8), F * B, B, ch, cw, p(tb[0]), p(tb[1]), p(tb[2]), p(tb[3]), 15, p(sums), p(f32),
                                                     stream), "color_jitter")
    out["launches_ms"] = timed(launches, args.repeats, args.inner)
    rd, wr = 2 * u8.numel(), 4 * f32.numel()
    t = out["launches_ms"]["median"] * 1e-3
    out.update(read_mb=rd / 1e6, write_mb=wr / 1e6, achieved_gbs=(rd + wr) / t / 1e9, frac_of_8tbs=(rd + wr) / t / HBM_PEAK)
    return out


def color_aug_cpu(args):
    """torchvision 0.7.0's PIL ColorJitter (restated: torchvision is not a dependency) on the three level-0 frames of one sample"""
    from PIL import Image, ImageEnhance
    ch, cw = args.crop
    rng = np.random.RandomState(0)
    imgs = [Image.fromarray(rng.randint(0, 256, (ch, cw, 3), dtype=np.uint8)) for _ in FRAMES]

    def hue(im, f):
        h, s, v = im.convert("HSV").split()
        h = Image.fromarray(((np.asarray(h).astype(np.int64) + (int(f * 255) & 255)) & 255).astype(np.uint8))
        return Image.merge("HSV", (h, s, v)).convert("RGB")
    ops = [lambda im: ImageEnhance.Brightness(im).enhance(1.13), lambda im: ImageEnhance.Contrast(im).enhance(0.91),
           lambda im: ImageEnhance.Color(im).enhance(1.07), lambda im: hue(im, -0.06)]

    def sample(i):
        for im in imgs:
            for k in np.random.RandomState(i).permutation(4):
                im = ops[k](im)
    sample(0)
    dt = []
    for i in range(args.cpu_samples):
        t0 = time.perf_counter()
        sample(i)
        dt.append(time.perf_counter() - t0)
    med = statistics.median(dt)
    return {"ms_per_sample": {"median": med * 1e3, "min": min(dt) * 1e3, "max": max(dt) * 1e3, "samples": len(dt)},
            "samples_per_s_one_core": 1.0 / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop", type=int, nargs=2, default=[512, 1024])
    ap.add_argument("--sources", nargs="+", default=["512x1024", "1024x2048"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--cpu-samples", type=int, default=7)
    ap.add_argument("--skip-gpu", action="store_true", help="CPU side only (no rate of the builder is reported)")
    ap.add_argument("--color-aug", action="store_true", help="the colour-augmentation leg instead of the pyramid / label stage")
    args = ap.parse_args()
    if not args.skip_gpu and not torch.cuda.is_available():
        sys.exit("tools/device_batch.py measures on the GPU: no device visible")
    if args.color_aug:
        res = {"batch": args.batch, "crop": args.crop, "frames": len(FRAMES), "color_aug": {"cpu": color_aug_cpu(args)}}
        if not args.skip_gpu:
            res["color_aug"]["gpu"] = color_aug_gpu(args)
        print(json.dumps(res))
        return
    res = {"batch": args.batch, "crop": args.crop, "frames": len(FRAMES), "scales": 4, "sources": {}}
    for src in args.sources:
        H, W = (int(v) for v in src.split("x"))
        res["sources"][src] = {"cpu": cpu_side(args, H, W)}
        if not args.skip_gpu:
            res["sources"][src]["gpu"] = gpu_side(args, H, W)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
