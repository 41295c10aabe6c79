#!/usr/bin/env python
"""tests/golden/color_aug.npz: inputs and expected outputs of the device batch builder's colour augmentation, produced by the
REFERENCE's own ``__getitem__`` / ``preprocess`` (imported from /root/reference with the stand-in recipe of make_device_batch.py;
build container only) with Pillow doing the arithmetic.

On top of that recipe:
  * ``transforms.ColorJitter.get_params`` is a stand-in (torchvision is absent): the draws of torchvision 0.7.0 -- ``random.uniform``
    for brightness, contrast, saturation, hue, then ``random.shuffle`` of the four operations -- and its PIL functional operations:
    ``ImageEnhance.Brightness / Contrast / Color(img).enhance(f)`` and, for hue, ``convert("HSV")``, the uint8 add of
    ``uint8(f * 255)`` to the H plane, ``convert("RGB")``.  Every pixel value is computed by Pillow.
  * the scripted cases answer ``random.uniform`` / ``random.shuffle`` from a script as well (so that every order occurs once); the
    ``draw*`` arrays record what the untouched ``random`` module hands the reference after ``random.seed(7)``.
The expected ``color_aug`` tensors are stored as the uint8 images behind them (asserted: float == uint8 / 255).

Asserted here, on the CPU, before anything is written:
  * the numpy oracle of tests/color_aug_cases.py equals Pillow on every fixture image, on all 2^24 colours for RGB -> HSV, HSV ->
    RGB and L, and on all 65 536 (degenerate, pixel) pairs of ``Image.blend`` at every alpha the fixture and the tests use;
  * coverage by the reference's run alone: all 24 orders, a blend clipped at 255 and one at 0, the hue add wrapping past 255 for a
    positive and for a negative factor, pixels with max == min at a hue step, samples with the coin off.

    python tests/golden/make_color_aug.py            # write the fixture
    python tests/golden/make_color_aug.py --check    # regenerate and compare with the committed file, bit for bit
"""
import itertools
import os
import random
import sys

import numpy as np
import torch
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "color_aug.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_device_batch as MDB  # noqa: E402

FRAMES = MDB.FRAMES


class ColorJitter:
    """stand-in for torchvision 0.7.0's transforms.ColorJitter: only get_params, which is all the reference uses"""
    log = []                                            # (factors, order) of every call

    @staticmethod
    def get_params(brightness, contrast, saturation, hue):
        bf = random.uniform(brightness[0], brightness[1])
        cf = random.uniform(contrast[0], contrast[1])
        sf = random.uniform(saturation[0], saturation[1])
        hf = random.uniform(hue[0], hue[1])

        def adjust_hue(img):
            h, s, v = img.convert("HSV").split()
            np_h = (np.array(h, dtype=np.uint8).astype(np.int64) + (int(hf * 255) & 255)) & 255      # uint8 += uint8(hf * 255)
            return Image.merge("HSV", (Image.fromarray(np_h.astype(np.uint8)), s, v)).convert("RGB")
        ops = [(0, lambda img: ImageEnhance.Brightness(img).enhance(bf)), (1, lambda img: ImageEnhance.Contrast(img).enhance(cf)),
               (2, lambda img: ImageEnhance.Color(img).enhance(sf)), (3, adjust_hue)]
        random.shuffle(ops)
        ColorJitter.log.append(((bf, cf, sf, hf), [i for i, _ in ops]))

        def apply(img):
            for _, fn in ops:
                img = fn(img)
            return img
        return apply


class ScriptedJitter(MDB.Scripted):
    """random.random / randint as MDB.Scripted, and random.uniform / random.shuffle from a script too"""

    def __init__(self, randoms, randints, uniforms, perms):
        super().__init__(randoms, randints)
        self.uniforms, self.perms = list(uniforms), [list(p) for p in perms]

    def __enter__(self):
        super().__enter__()
        self.keep2 = (random.uniform, random.shuffle)

        def uniform(a, b):
            v = self.uniforms.pop(0)
            assert a <= v <= b, (a, v, b)
            return v

        def shuffle(x):
            p = self.perms.pop(0)
            x[:] = [x[i] for i in p]
        random.uniform, random.shuffle = uniform, shuffle

    def __exit__(self, *exc):
        random.uniform, random.shuffle = self.keep2
        super().__exit__(*exc)
        assert not self.uniforms and not self.perms, "the reference drew less than scripted"


def patches(img):
    """saturated and grey patches where every crop of case 1 keeps them: rows 5..14, columns 14..22 (mirrored: 5..13)"""
    n = img.shape[0]
    sat = [(255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (254, 1, 128)]
    for i in range(n):
        for k in range(3):
            img[i, 5 + 2 * k:7 + 2 * k, 14:17] = sat[(i + k) % len(sat)]
            img[i, 5 + 2 * k:7 + 2 * k, 17:20] = sat[(i + k + 4) % len(sat)]
        img[i, 11:15, 14:20] = ((37 * i) % 256,) * 3                                 # grey: max == min
        img[i, 5:15, 20:23, 0] = np.arange(250 - 10 + 1, 250 + 1)[:, None]         # reds with a little blue: H close to 255
        img[i, 5:15, 20:23, 1] = 0
        img[i, 5:15, 20:23, 2] = np.arange(1, 11)[:, None]
    return img


def to_u8(t, unit):
    u8 = torch.round(t * 255).to(torch.uint8).numpy()
    assert torch.equal(unit(u8), t), "ToTensor is not uint8 / 255 here"
    return u8


def check_oracle_against_pillow(CA, alphas):
    i = np.arange(1 << 24, dtype=np.int64)
    rgb = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    im = Image.fromarray(rgb)
    assert np.array_equal(np.asarray(im.convert("L")), CA.luma(rgb[..., 0], rgb[..., 1], rgb[..., 2])), "L"
    hsv = np.asarray(im.convert("HSV"))
    got = CA.rgb_to_hsv(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    for c in range(3):
        assert np.array_equal(hsv[..., c], got[c]), "RGB -> HSV plane %d" % c
    back = np.asarray(Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(rgb[..., c])) for c in range(3)]).convert("RGB"))
    got = CA.hsv_to_rgb(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    for c in range(3):
        assert np.array_equal(back[..., c], got[c]), "HSV -> RGB plane %d" % c
    dd, xx = np.mgrid[0:256, 0:256].astype(np.uint8)
    for a in sorted(alphas):
        pil = np.asarray(Image.blend(Image.fromarray(dd), Image.fromarray(xx), float(a)))
        assert np.array_equal(pil, CA.blend(dd, xx, a)), "blend at %r" % a
    return len(alphas)


def generate():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import color_aug_cases as CA
    import device_batch_cases as DC
    make, _ = MDB._reference()
    sys.modules["torchvision.transforms"].ColorJitter = ColorJitter
    d, trace, alphas = {}, {}, {0.0, 0.8, 1.2, 0.9137, 1.0731, 1.0}

    def check_aug(color_u8, aug_u8, factors, order):
        """the oracle on one sample's frame: equal to what Pillow produced inside the reference"""
        assert np.array_equal(CA.jitter_image(color_u8, factors, order, trace), aug_u8), "the numpy oracle differs from Pillow"
        alphas.update(float(np.float32(v)) for v in factors[:3])

    # ---- case 1: the reference batch ------------------------------------------------------------------------------------
    c = CA.CASE_REF
    h, w, n = c["height"], c["width"], c["n_aug"] + c["n_plain"]
    rng = np.random.RandomState(21)
    images = {f: patches(MDB.half_noise(rng, n, h, w)) for f in FRAMES}
    orders = list(itertools.permutations(range(4)))
    assert len(orders) == c["n_aug"]
    factors = np.column_stack([rng.uniform(0.8, 1.2, (c["n_aug"], 3)), rng.uniform(-0.1, 0.1, c["n_aug"])])
    factors[0], factors[5], factors[11], factors[17] = (1.2, 1.2, 1.2, 0.1), (0.8, 0.8, 0.8, -0.1), (1.2, 0.8, 1.2, -0.05), (0.8, 1.2, 0.8, 0.05)
    crops = np.column_stack([rng.randint(0, w - c["crop_w"] + 1, n), rng.randint(0, h - c["crop_h"] + 1, n)]).astype(np.int32)
    crops[1], crops[2] = (0, 0), (w - c["crop_w"], h - c["crop_h"])
    flips = rng.rand(n) < 0.5
    apply = np.array([True] * c["n_aug"] + [False] * c["n_plain"])
    order_i = np.random.RandomState(22).permutation(c["n_aug"])                # which sample gets which order
    ds = make(images, None, None, [True] * n, split="train", img_size=(h, w), crop_h=c["crop_h"], crop_w=c["crop_w"],
              augmentations={"random_horizontal_flip": 0.5, "color_aug": True}, frame_idxs=list(FRAMES), num_scales=3)
    ColorJitter.log.clear()
    with ScriptedJitter([v for i in range(n) for v in (0.9 if apply[i] else 0.3, 0.1 if flips[i] else 0.9)], crops.reshape(-1).tolist(),
                        factors.reshape(-1).tolist(), [orders[order_i[i]] for i in range(c["n_aug"])]):
        batch = MDB.collate([ds[i] for i in range(n)])
    assert ds.flips_seen[::3] == flips.tolist() and len(ColorJitter.log) == c["n_aug"]
    d["ref_apply"], d["ref_crops"], d["ref_flips"] = apply, crops, flips
    d["ref_factors"] = np.concatenate([np.array([fo[0] for fo in ColorJitter.log], dtype=np.float64), np.tile([1.0, 1.0, 1.0, 0.0], (c["n_plain"], 1))])
    d["ref_order"] = np.concatenate([np.array([fo[1] for fo in ColorJitter.log], dtype=np.uint8), np.tile(np.arange(4, dtype=np.uint8), (c["n_plain"], 1))])
    assert np.array_equal(d["ref_factors"][:c["n_aug"]], factors) and len(set(map(tuple, d["ref_order"][:c["n_aug"]].tolist()))) == 24
    for f in FRAMES:
        d["ref_frame_%d" % f] = images[f]
        for s in range(3):
            d["ref_color_%d_%d" % (f, s)] = to_u8(batch[("color", f, s)], DC.unit)
        aug = d["ref_color_aug_%d" % f] = to_u8(batch[("color_aug", f, 0)], DC.unit)
        col = d["ref_color_%d_0" % f]
        for i in range(n):
            assert np.array_equal(col[i], CA.cut(images[f][i], crops[i], flips[i], c["crop_h"], c["crop_w"]))
            if apply[i]:
                check_aug(col[i], aug[i], d["ref_factors"][i], d["ref_order"][i])
                assert not np.array_equal(col[i], aug[i])
            else:
                assert np.array_equal(col[i], aug[i])
    for s in range(3):
        d["ref_K_%d" % s], d["ref_inv_K_%d" % s] = batch[("K", s)].numpy(), batch[("inv_K", s)].numpy()
    want = {"clip_hi", "clip_lo", "wrap_pos", "wrap_neg", "grey"}
    assert all(trace.get(k) for k in want), "coverage: %r" % {k: trace.get(k) for k in want}

    # ---- case 2: many workgroups; the scalar tail -------------------------------------------------------------------------
    for tag, c, scales in (("wide", CA.CASE_WIDE, 4), ("tail", CA.CASE_TAIL, 1)):
        rng = np.random.RandomState(23 if tag == "wide" else 24)
        h, w = c["height"], c["width"]
        images = {f: MDB.half_noise(rng, 1, h, w) for f in FRAMES}
        x1, y1 = c.get("crop", (0, 0))
        for j, (fac, order) in enumerate(CA.CASE_2_JITTER):
            ds = make(images, None, None, [True], split="train", img_size=(h, w), crop_h=c.get("crop_h"), crop_w=c.get("crop_w"),
                      augmentations={"color_aug": True}, frame_idxs=list(FRAMES), num_scales=scales)
            ColorJitter.log.clear()
            with ScriptedJitter([0.75], [x1, y1], list(fac), [order]):
                batch = MDB.collate([ds[0]])
            assert ColorJitter.log == [(tuple(fac), list(order))]
            for f in FRAMES:
                col = to_u8(batch[("color", f, 0)], DC.unit)
                aug = d["%s_color_aug_%d_%d" % (tag, j, f)] = to_u8(batch[("color_aug", f, 0)], DC.unit)
                assert np.array_equal(col[0], CA.cut(images[f][0], (x1, y1), False, c.get("crop_h", h), c.get("crop_w", w)))
                check_aug(col[0], aug[0], fac, order)
        for f in FRAMES:
            d["%s_frame_%d" % (tag, f)] = images[f]
        if tag == "wide":                                # the model step of the GPU suite is fed from this sample
            for f in FRAMES:
                for s in range(scales):
                    d["wide_color_%d_%d" % (f, s)] = to_u8(batch[("color", f, s)], DC.unit)
            for s in range(scales):
                d["wide_K_%d" % s], d["wide_inv_K_%d" % s] = batch[("K", s)].numpy(), batch[("inv_K", s)].numpy()

    # ---- draw order: the untouched random module, seed 7 ------------------------------------------------------------------
    c = CA.CASE_REF
    h, w = c["height"], c["width"]
    for tag, aug in (("draw", {"random_horizontal_flip": 0.5, "color_aug": True}), ("draw_noflip", {"color_aug": True})):
        nd = 6
        ds = make({f: np.zeros((nd, h, w, 3), np.uint8) for f in FRAMES}, None, None, [True] * nd, split="train", img_size=(h, w),
                  crop_h=c["crop_h"], crop_w=c["crop_w"], augmentations=aug, frame_idxs=list(FRAMES), num_scales=3)
        seen, applied = [], []
        keep = random.randint
        random.randint = lambda a, b: (seen.append(keep(a, b)), seen[-1])[1]
        ColorJitter.log.clear()
        try:
            random.seed(7)
            for i in range(nd):
                before = len(ColorJitter.log)
                ds[i]
                applied.append(len(ColorJitter.log) > before)
            nxt = random.random()
        finally:
            random.randint = keep
        fac, order = np.tile([1.0, 1.0, 1.0, 0.0], (nd, 1)), np.tile(np.arange(4, dtype=np.uint8), (nd, 1))
        for i, fo in zip(np.flatnonzero(applied), ColorJitter.log):
            fac[i], order[i] = fo
        d[tag + "_crops"], d[tag + "_flips"] = np.array(seen, dtype=np.int32).reshape(nd, 2), np.array(ds.flips_seen[::3], dtype=np.bool_)
        d[tag + "_apply"], d[tag + "_factors"], d[tag + "_order"] = np.array(applied, dtype=np.bool_), fac, order
        d[tag + "_next_random"] = np.float64(nxt)
        assert any(applied) and not all(applied)

    n_alpha = check_oracle_against_pillow(CA, alphas)
    print("oracle == Pillow %s: all 2^24 colours (L, RGB -> HSV, HSV -> RGB), all pairs of the blend at %d alphas" % (Image.__version__, n_alpha))
    return d


def main():
    d = generate()
    if "--check" in sys.argv[1:]:
        z = np.load(OUT, allow_pickle=False)
        bad = [k for k in sorted(set(d) | set(z.files))
               if k not in d or k not in z.files or d[k].dtype != z[k].dtype or d[k].shape != z[k].shape or d[k].tobytes() != z[k].tobytes()]
        print("make_color_aug --check:", "OK" if not bad else "arrays differ from the committed fixture: %s" % bad)
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, "%.1f KB, %d arrays" % (os.path.getsize(OUT) / 1024, len(d)))


if __name__ == "__main__":
    main()
