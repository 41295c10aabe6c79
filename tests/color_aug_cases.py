"""Cases shared by the CPU run (kernels under the interpreter, tests/test_color_aug_emu.py) and the GPU run
(tests/test_color_aug_gpu.py) of the device batch builder's colour augmentation (loader/device_batch.py: ``color_aug=True``;
csrc/batchprep.hip: jitter_stats_kernel, jitter_apply_kernel).

Expected values come from tests/golden/color_aug.npz, written by tests/golden/make_color_aug.py from the reference's own
``__getitem__`` with Pillow doing the arithmetic, or from the numpy oracle below, which that generator compares with Pillow on
every fixture image, on all 2^24 colours (RGB -> HSV, HSV -> RGB, L) and on all 65 536 (degenerate, pixel) pairs of the blend
at every alpha used.  Every comparison is exact.  The GPU tests read the fixture and numpy only.

The oracle restates Pillow's 8-bit arithmetic in numpy, array at a time, in the number formats Pillow uses (float32 where it
computes in C float, float64 where in double; numpy never fuses a multiply with an add).
"""
import functools
import os
import random

import numpy as np
import torch

from conftest import GOLDEN
from improving_segmentation_with_selfsupervised_depth_amd import _lib, hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.loader.device_batch import DeviceBatchBuilder
from device_batch_cases import FRAMES, INTRINSICS, unit

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
IDENTITY = (1.0, 1.0, 1.0, 0.0)

# Case 1, the reference batch: 26 samples of a 16x24 crop from 20x28 frames, one per order of the four operations, then two
# whose coin says no
CASE_REF = dict(height=20, width=28, crop_h=16, crop_w=24, n_aug=24, n_plain=2)
# Case 2: one sample at 64x288 -- 18 432 pixels are 18 workgroups of the jitter kernels (1024 pixels each), so the contrast sum
# is put together from many atomics -- and one at 21x37 cropped from 24x45 (777 pixels: the scalar load / store path and a
# partly filled last workgroup); contrast first and contrast last for both
CASE_WIDE = dict(height=64, width=288)
CASE_TAIL = dict(height=24, width=45, crop_h=21, crop_w=37, crop=(5, 2))
CASE_2_JITTER = [((1.2, 0.8, 1.15, -0.07), (CONTRAST, HUE, BRIGHTNESS, SATURATION)),
                 ((0.85, 1.2, 0.8, 0.1), (SATURATION, BRIGHTNESS, HUE, CONTRAST))]


def golden():
    z = np.load(os.path.join(GOLDEN, "color_aug.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---- the numpy oracle -------------------------------------------------------------------------------------------------
def tables(factors):
    """float64 factors [B,4] (brightness, contrast, saturation, hue) -> (alpha float32 [B,3] as the C cast rounds a double,
    hue_shift int32 [B] = uint8(hue_factor * 255): truncated toward zero, then mod 256)"""
    factors = np.asarray(factors, dtype=np.float64).reshape(-1, 4)
    return factors[:, :3].astype(np.float32), (np.trunc(factors[:, 3] * 255).astype(np.int64) & 255).astype(np.int32)


def luma(r, g, b):
    """convert("L")"""
    return (19595 * r.astype(np.int64) + 38470 * g.astype(np.int64) + 7471 * b.astype(np.int64) + 0x8000) >> 16


def blend(d, x, alpha, trace=None):
    """Image.blend(degenerate d, image x, alpha): integer arrays in, uint8 out"""
    a = np.float32(alpha)
    t = d.astype(np.float32) + a * (x.astype(np.int64) - d.astype(np.int64)).astype(np.float32)
    assert t.dtype == np.float32
    if np.float32(0) <= a <= np.float32(1):
        return t.astype(np.int64).astype(np.uint8)
    if trace is not None:
        trace["clip_hi"] = trace.get("clip_hi", False) or bool((t > 255).any())
        trace["clip_lo"] = trace.get("clip_lo", False) or bool((t < 0).any())
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64))).astype(np.uint8)


def rgb_to_hsv(r, g, b):
    """convert("HSV"): uint8 planes in, uint8 planes out"""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    f32 = lambda v: v.astype(np.float32)
    cr = f32(np.where(grey, 1, mx - mn))
    s = cr / f32(np.where(grey, 1, mx))
    rc, gc, bc = f32(mx - r) / cr, f32(mx - g) / cr, f32(mx - b) / cr
    f64 = lambda v: v.astype(np.float64)
    h = np.where(r == mx, bc - gc,
                 np.where(g == mx, ((2.0 + f64(rc)) - f64(bc)).astype(np.float32), ((4.0 + f64(gc)) - f64(rc)).astype(np.float32)))
    assert h.dtype == np.float32 and s.dtype == np.float32
    h = np.fmod(f64(h) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.clip((f64(h) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((f64(s) * 255.0).astype(np.int64), 0, 255)
    return np.where(grey, 0, H).astype(np.uint8), np.where(grey, 0, S).astype(np.uint8), mx.astype(np.uint8)


def _round8(x):
    """round half away from zero (x >= 0), clipped to 0..255"""
    fl = np.floor(x)
    return np.clip(fl.astype(np.int64) + ((x - fl) >= 0.5), 0, 255)


def hsv_to_rgb(H, S, V):
    """HSV -> RGB: uint8 planes in, uint8 planes out"""
    H, S, V = (np.asarray(v).astype(np.int64) for v in (H, S, V))
    x = H.astype(np.float64) * 6.0 / 255.0
    fi = np.floor(x)
    f = (x - fi).astype(np.float32).astype(np.float64)
    fs = (S.astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    v = V.astype(np.float64)
    p = _round8(v * (1.0 - fs))
    q = _round8(v * (1.0 - fs * f))
    t = _round8(v * (1.0 - fs * (1.0 - f)))
    i = fi.astype(np.int64) % 6
    pick = lambda c0, c1, c2, c3, c4, c5: np.where(S == 0, V, np.choose(i, [c0, c1, c2, c3, c4, c5])).astype(np.uint8)
    return pick(V, q, p, p, t, V), pick(t, V, V, q, p, p), pick(p, p, t, V, V, q)


def jitter_image(img, factors, order, trace=None):
    """img uint8 [3,h,w] -> uint8 [3,h,w]: the four operations in `order`, a uint8 image between every two"""
    alpha, shift = tables(factors)
    alpha, shift = alpha[0], int(shift[0])
    r, g, b = img[0], img[1], img[2]
    for op in order:
        if op == BRIGHTNESS:
            zero = np.zeros_like(r)
            r, g, b = (blend(zero, c, alpha[0], trace) for c in (r, g, b))
        elif op == CONTRAST:
            lum = luma(r, g, b)
            mean = (2 * int(lum.sum()) + lum.size) // (2 * lum.size)
            assert mean == int(lum.sum() / lum.size + 0.5)
            m = np.full_like(r, mean)
            r, g, b = (blend(m, c, alpha[1], trace) for c in (r, g, b))
        elif op == SATURATION:
            lum = luma(r, g, b)
            r, g, b = (blend(lum, c, alpha[2], trace) for c in (r, g, b))
        elif op == HUE:
            hh, ss, vv = rgb_to_hsv(r, g, b)
            if trace is not None:
                key = "wrap_pos" if factors[3] > 0 else "wrap_neg"
                if factors[3] != 0:
                    trace[key] = trace.get(key, False) or bool((hh.astype(np.int64) + shift > 255).any())
                trace["grey"] = trace.get("grey", False) or bool((ss == 0).any())
            r, g, b = hsv_to_rgb((hh.astype(np.int64) + shift) & 255, ss, vv)
        else:
            raise ValueError(op)
    return np.stack([r, g, b])


def cut(frames, crop, flip, ch, cw):
    """[H,W,3] -> planar [3,ch,cw]: flip, then crop"""
    a = frames[:, ::-1] if flip else frames
    x1, y1 = crop
    return np.ascontiguousarray(np.moveaxis(a[y1:y1 + ch, x1:x1 + cw], -1, 0))


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _dev(a, device):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(device)


def _jitter(apply, factors, order):
    return dict(apply=np.asarray(apply, dtype=np.bool_), factors=np.asarray(factors, dtype=np.float64).reshape(-1, 4),
                order=np.asarray(order, dtype=np.uint8).reshape(-1, 4))


def _same(got, want_u8, what):
    got, want = got.cpu(), unit(want_u8)
    assert got.dtype == torch.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), "%s: %d of %d values differ" % (what, int((got != want).sum()), want.numel())


def run_jitter(u8, factors, order, device, apply=None, ops=15):
    """hipops.batchprep_color_jitter on planar uint8 images [B,3,h,w] with per-sample factors -> uint8 (exactly: the float
    output must be unit() of a uint8 image)"""
    factors = np.asarray(factors, dtype=np.float64).reshape(-1, 4)
    alpha, shift = tables(factors)
    apply = np.ones(len(factors), bool) if apply is None else apply
    out = H.batchprep_color_jitter(_dev(u8, device), apply, alpha, shift, np.asarray(order, dtype=np.uint8).reshape(-1, 4), ops=ops).cpu()
    back = torch.round(out * 255).to(torch.uint8)
    assert torch.equal(unit(back.numpy()), out), "the output is not uint8 / 255"
    return back.numpy()


# ---- case 1 -----------------------------------------------------------------------------------------------------------------
def run_reference_batch(device):
    """the reference's __getitem__ with color_aug on: 24 orders, flips and crops mixed, two samples with the coin off"""
    g = golden()
    c = CASE_REF
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], intrinsics=INTRINSICS, num_scales=3,
                           random_horizontal_flip=0.5, color_aug=True)
    jit = _jitter(g["ref_apply"], g["ref_factors"], g["ref_order"])
    assert len(set(map(tuple, jit["order"][jit["apply"]].tolist()))) == 24 and int((~jit["apply"]).sum()) == c["n_plain"]
    inputs = b({f: _dev(g["ref_frame_%d" % f], device) for f in FRAMES}, crops=g["ref_crops"], flips=g["ref_flips"], jitter=jit)
    for f in FRAMES:
        _same(inputs[("color_aug", f, 0)], g["ref_color_aug_%d" % f], "color_aug %d" % f)
        for s in range(3):
            _same(inputs[("color", f, s)], g["ref_color_%d_%d" % (f, s)], "color %d scale %d" % (f, s))
        off = ~jit["apply"]
        assert torch.equal(inputs[("color_aug", f, 0)].cpu()[off], inputs[("color", f, 0)].cpu()[off])
        assert not torch.equal(inputs[("color_aug", f, 0)].cpu()[~off], inputs[("color", f, 0)].cpu()[~off])
    for s in range(3):
        for name in ("K", "inv_K"):
            assert torch.equal(inputs[(name, s)].cpu(), torch.from_numpy(g["ref_%s_%d" % (name, s)])), (name, s)


# ---- case 2 -----------------------------------------------------------------------------------------------------------------
def run_reduction_and_tail(device):
    """the contrast sum over many workgroups (64x288) and the scalar tail (21x37 from 24x45); contrast first and last; expected
    values from Pillow (the fixture)"""
    g = golden()
    for tag, c in (("wide", CASE_WIDE), ("tail", CASE_TAIL)):
        for j, (factors, order) in enumerate(CASE_2_JITTER):
            assert order[0 if j == 0 else 3] == CONTRAST
            b = DeviceBatchBuilder(c["height"], c["width"], c.get("crop_h"), c.get("crop_w"), intrinsics=INTRINSICS, num_scales=1,
                                   color_aug=True)
            inputs = b({f: _dev(g["%s_frame_%d" % (tag, f)], device) for f in FRAMES}, crops=np.array([c.get("crop", (0, 0))]),
                       flips=np.array([False]), jitter=_jitter([True], [factors], [order]))
            for f in FRAMES:
                _same(inputs[("color_aug", f, 0)], g["%s_color_aug_%d_%d" % (tag, j, f)], "%s jitter %d frame %d" % (tag, j, f))


# ---- case 3 -----------------------------------------------------------------------------------------------------------------
def run_mean_rounding(device):
    """contrast's mean is int(mean + 0.5): an L mean of exactly 100.5 gives 101, one pixel fewer at 101 gives 100, constant
    images give their own level.  Grey pixels have L = the grey level, so the L planes are set directly.  32x40 = 1280 pixels:
    two workgroups.  Expected values: the oracle; with alpha 0 the blend returns the degenerate image, the mean itself."""
    h, w = 32, 40
    n = h * w
    imgs, means = [], []
    for n_hi, lo in ((n // 2, 100), (n // 2 - 1, 100), (0, 173), (0, 255), (0, 0)):
        lum = np.full(n, lo, dtype=np.uint8)
        lum[np.random.RandomState(n_hi).permutation(n)[:n_hi]] = min(lo + 1, 255)
        imgs.append(np.broadcast_to(lum.reshape(1, h, w), (3, h, w)))
        means.append((2 * int(lum.astype(np.int64).sum()) + n) // (2 * n))
    assert means == [101, 100, 173, 255, 0]
    u8 = np.ascontiguousarray(np.stack(imgs))
    order = [ORDER0] * len(imgs)
    for alpha in (0.8, 1.2, 0.0):
        factors = [(1.0, alpha, 1.0, 0.0)] * len(imgs)
        got = run_jitter(u8, factors, order, device, ops=1 << CONTRAST)
        want = np.stack([jitter_image(u8[i], factors[i], (CONTRAST,)) for i in range(len(imgs))])
        assert np.array_equal(got, want), alpha
    for i, m in enumerate(means):
        assert (got[i] == m).all(), (i, m, np.unique(got[i]))
    # 1.2 tells the means 100 and 101 apart at both levels: 100 + 1.2 * (101 - 100) = 101.2 -> 101, 101 + 1.2 * (100 - 101) = 99.8 -> 99
    a = run_jitter(u8[:2], [(1.0, 1.2, 1.0, 0.0)] * 2, order[:2], device, ops=1 << CONTRAST)
    assert sorted(np.unique(a[0]).tolist()) == [99, 101] and sorted(np.unique(a[1]).tolist()) == [100, 101]


# ---- case 4 -----------------------------------------------------------------------------------------------------------------
def all_colours(subsample):
    """planar [3,h,w]: every 24-bit colour once (4096x4096), or a fixed 1/64 of them (512x512: colour 64 i + (37 i mod 64) for
    i < 2^18: every red and green value with a blue value that moves through all residues)"""
    i = np.arange(1 << 24, dtype=np.int64)
    if subsample:
        i = np.arange(1 << 18, dtype=np.int64)
        i = 64 * i + (37 * i) % 64
    side = int(round(len(i) ** 0.5))
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255]).astype(np.uint8).reshape(3, side, side)


@functools.lru_cache(maxsize=None)
def _colour_oracle(subsample):
    """(the image, its HSV planes, the HSV -> RGB table [256,256,256,3] indexed H, S, V), computed once per process"""
    img = all_colours(subsample)
    hsv = rgb_to_hsv(img[0], img[1], img[2])
    hh, ss, vv = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    table = np.stack(hsv_to_rgb(hh.ravel(), ss.ravel(), vv.ravel()), -1).reshape(256, 256, 256, 3)
    for a in (img,) + hsv + (table,):
        a.setflags(write=False)
    return img, hsv, table


# the ends of the reference's hue range (-0.1, 0.1): uint8(0.1 * 255) = 25 and uint8(-0.1 * 255) = -25 mod 256 = 231
HUE_SHIFTS = {0.1: 25, -0.1: 231, 0.0: 0}
ORDER0 = (BRIGHTNESS, CONTRAST, SATURATION, HUE)


def run_exhaustive_hue(device, subsample):
    img, (hh, ss, vv), table = _colour_oracle(subsample)
    for hf, shift in HUE_SHIFTS.items():
        assert int(tables([(1.0, 1.0, 1.0, hf)])[1][0]) == shift
        want = np.moveaxis(table[(hh.astype(np.int64) + shift) & 255, ss, vv], -1, 0)
        got = run_jitter(img[None], [(1.0, 1.0, 1.0, hf)], [ORDER0], device, ops=1 << HUE)[0]
        assert np.array_equal(got, want), "hue %r: %d colours differ" % (hf, int((got != want).any(0).sum()))
    assert not np.array_equal(want, img)                 # shift 0 alters pixels too: the 8-bit HSV round trip is lossy


def run_exhaustive_saturation(device, subsample):
    img = _colour_oracle(subsample)[0]
    lum = luma(img[0], img[1], img[2])
    for alpha in (0.8, 1.2):
        want = np.stack([blend(lum, img[c], alpha) for c in range(3)])
        got = run_jitter(img[None], [(1.0, 1.0, alpha, 0.0)], [ORDER0], device, ops=1 << SATURATION)[0]
        assert np.array_equal(got, want), "saturation %r: %d colours differ" % (alpha, int((got != want).any(0).sum()))


def run_pairs_brightness_contrast(device):
    """the 256x256 plane of all (y, x) byte pairs (red = y, green = x, blue = 255 - x) through brightness alone and contrast
    alone at the ends of the range and inside it (the alphas at which the generator compared blend() with Pillow on all pairs)"""
    yy, xx = np.mgrid[0:256, 0:256]
    img = np.stack([yy, xx, 255 - xx]).astype(np.uint8)
    for op in (BRIGHTNESS, CONTRAST):
        for alpha in (0.8, 1.2, 0.9137, 1.0731):
            factors = [1.0, 1.0, 1.0, 0.0]
            factors[op] = alpha
            got = run_jitter(img[None], [factors], [ORDER0], device, ops=1 << op)[0]
            assert np.array_equal(got, jitter_image(img, factors, (op,))), (op, alpha)
    # neutral parameters: every blend an exact identity (hue masked out)
    assert np.array_equal(run_jitter(img[None], [IDENTITY], [ORDER0], device, ops=7)[0], img)


# ---- case 5 -----------------------------------------------------------------------------------------------------------------
def run_draw():
    """draw_with_jitter replays the reference's stream: under random.seed(7) it equals what the untouched reference drew"""
    import device_batch_cases as DC
    g = golden()
    c = CASE_REF
    n = 6
    for tag, flip in (("draw", 0.5), ("draw_noflip", 0.0)):
        b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], intrinsics=INTRINSICS, random_horizontal_flip=flip,
                               color_aug=True)
        random.seed(7)
        crops, flips, jit = b.draw_with_jitter(n)
        after = random.random()
        assert np.array_equal(crops, g[tag + "_crops"]) and crops.dtype == np.int32
        assert np.array_equal(flips, g[tag + "_flips"]) and flips.dtype == np.bool_
        assert np.array_equal(jit["apply"], g[tag + "_apply"]) and jit["apply"].dtype == np.bool_
        assert jit["factors"].dtype == np.float64 and jit["factors"].tobytes() == g[tag + "_factors"].tobytes()
        assert np.array_equal(jit["order"], g[tag + "_order"])
        assert after == float(g[tag + "_next_random"])
        assert jit["apply"].any() and not jit["apply"].all()
        assert flips.any() == (flip > 0)
        try:
            b.draw(n)
        except ValueError as e:
            assert "draw_with_jitter" in str(e)
        else:
            raise AssertionError("draw() on a color_aug builder did not raise")
    DC.run_draw()                                        # a plain builder: unchanged


# ---- case 6 -----------------------------------------------------------------------------------------------------------------
def run_unchanged_default(device):
    g = golden()
    c = CASE_REF
    frames = {f: _dev(g["ref_frame_%d" % f][:2], device) for f in FRAMES}
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], intrinsics=INTRINSICS, num_scales=3)
    assert b.color_aug is False
    inputs = b(frames, crops=g["ref_crops"][:2], flips=g["ref_flips"][:2])
    for f in FRAMES:
        assert inputs[("color_aug", f, 0)] is inputs[("color", f, 0)]
    try:
        b(frames, crops=g["ref_crops"][:2], flips=g["ref_flips"][:2], jitter=_jitter([True, False], [IDENTITY] * 2, [ORDER0] * 2))
    except ValueError:
        pass
    else:
        raise AssertionError("jitter accepted by a builder without color_aug")
    # validation path of a color_aug builder: randint(0, 0) twice per sample, nothing else, and no augmentation
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], intrinsics=INTRINSICS, num_scales=3, is_train=False,
                           random_horizontal_flip=0.5, color_aug=True)
    random.seed(11)
    for _ in range(2 * 2):
        random.randint(0, 0)
    want_state = random.getstate()
    random.seed(11)
    inputs = b(frames)
    assert random.getstate() == want_state
    for f in FRAMES:
        assert inputs[("color_aug", f, 0)] is inputs[("color", f, 0)]
        _same(inputs[("color", f, 0)], np.moveaxis(g["ref_frame_%d" % f][:2], -1, 1), "validation path, frame %d" % f)


# ---- case 7 -----------------------------------------------------------------------------------------------------------------
def _raises(fn, exc=ValueError):
    try:
        fn()
    except exc:
        return
    raise AssertionError("accepted")


def run_rejections(device):
    """bad tables stop in Python (ValueError), bad shapes and null pointers in the C entry (-2, -1): nothing reaches a kernel"""
    u8 = torch.zeros((2, 3, 4, 8), dtype=torch.uint8, device=device)
    ok = dict(apply=np.ones(2, bool), alpha=np.ones((2, 3), np.float32), hue_shift=np.zeros(2, np.int32),
              order=np.array([ORDER0, ORDER0[::-1]], np.uint8))
    call = lambda t=u8, **kw: H.batchprep_color_jitter(t, **dict(ok, **kw))
    assert tuple(call().shape) == (2, 3, 4, 8)
    _raises(lambda: call(order=np.array([ORDER0, (0, 1, 2, 2)], np.uint8)))                 # no permutation
    _raises(lambda: call(order=np.array([ORDER0, (0, 1, 2, 4)], np.uint8)))                 # an id out of range
    _raises(lambda: call(order=np.array([ORDER0], np.uint8)))                               # table lengths
    _raises(lambda: call(apply=np.ones(3, bool)))
    _raises(lambda: call(alpha=np.ones((2, 4), np.float32)))
    _raises(lambda: call(hue_shift=np.zeros(1, np.int32)))
    _raises(lambda: call(hue_shift=np.array([0, 256], np.int32)))                           # shifts outside 0..255
    _raises(lambda: call(hue_shift=np.array([-1, 0], np.int32)))
    _raises(lambda: call(ops=16))
    assert H.COLOR_JITTER_MAX_PIXELS == 16843009 and 255 * H.COLOR_JITTER_MAX_PIXELS < 2 ** 32 <= 255 * (H.COLOR_JITTER_MAX_PIXELS + 1)
    big = torch.zeros((1, 3, 1, H.COLOR_JITTER_MAX_PIXELS + 1), dtype=torch.uint8, device=device)
    one = {k: v[:1] for k, v in ok.items()}
    _raises(lambda: H.batchprep_color_jitter(big, **one))                                   # the sum's limit
    del big
    _raises(lambda: call(torch.zeros((2, 4, 4, 8), dtype=torch.uint8, device=device)))      # not three planes
    _raises(lambda: call(u8.float()), TypeError)
    # the C entry
    lib = _lib.lib()
    p = lambda t: t.data_ptr()
    tb = [_dev(ok["apply"].astype(np.uint8), device), _dev(ok["alpha"], device), _dev(ok["hue_shift"], device), _dev(ok["order"], device)]
    sums = torch.zeros(2, dtype=torch.int32, device=device)
    out = torch.zeros((2, 3, 4, 8), dtype=torch.float32, device=device)
    entry = lambda a: lib.segsde_batchprep_color_jitter(*a)
    good = [p(u8), 2, 2, 4, 8, p(tb[0]), p(tb[1]), p(tb[2]), p(tb[3]), 15, p(sums), p(out), None]
    assert entry(good) == 0
    for i in (0, 5, 6, 7, 8, 10, 11):
        assert entry(good[:i] + [None] + good[i + 1:]) == -1, i
    for i, v in ((1, 0), (1, 3), (1, 65536), (2, 0), (3, 0), (4, 0), (4, -8), (9, 16), (9, -1)):
        assert entry(good[:i] + [v] + good[i + 1:]) == -2, (i, v)
    assert entry(good[:3] + [4105, 4104] + good[5:]) == -2                                 # 16 851 . . . pixels: above the limit
    assert 4105 * 4104 > H.COLOR_JITTER_MAX_PIXELS


# ---- case 8 -----------------------------------------------------------------------------------------------------------------
def run_end_to_end(device):
    """a tiny R18 mono model step fed from a color_aug builder with scripted jitter equals, bit for bit, the step fed from the
    fixture's tensors (the construction of device_batch_cases.run_end_to_end; the encoder and the pose network read color_aug)"""
    import model_cases as MC
    from oracle import nets as N
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    g = golden()
    cfg = dict(MC.contract_cfgs()["cfgs"]["r18_mono"])
    Hh, W = CASE_WIDE["height"], CASE_WIDE["width"]
    cfg["height"], cfg["width"] = Hh, W
    sd = N.build_state_dict(cfg, 19, seed=11, randomize_bn=True)
    gen = torch.Generator().manual_seed(3)
    noise = {s: torch.randn(1, 2, Hh, W, generator=gen) for s in range(4)}
    tcfg = {"training": {"batch_size": 1, "monodepth_loss": dict(
        num_scales=4, frame_ids=[0, -1, 1], height=Hh, width=W, min_depth=0.1, max_depth=100, test_min_depth=1e-3,
        test_max_depth=80, disparity_smoothness=1e-3, no_ssim=False, avg_reprojection=False, disable_automasking=False)}}

    def step(inputs):
        model = get_model(cfg, 19)
        model.load_state_dict(sd, strict=True)
        model.to(device).train()
        MC.dropout_eval(model)
        lo = get_monodepth_loss(tcfg, is_train=True)
        lo.tiebreak_noise = noise
        out = model(inputs)
        lo.generate_images_pred(inputs, out)
        loss = lo.compute_losses(inputs, out)["loss"]
        loss.backward()
        return loss.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}

    factors, order = CASE_2_JITTER[0]
    b = DeviceBatchBuilder(Hh, W, intrinsics=INTRINSICS, color_aug=True)
    built = b({f: _dev(g["wide_frame_%d" % f], device) for f in FRAMES}, crops=np.zeros((1, 2), np.int32), flips=np.zeros(1, bool),
              jitter=_jitter([True], [factors], [order]))
    fixed = {}
    for f in FRAMES:
        for s in range(4):
            fixed[("color", f, s)] = unit(g["wide_color_%d_%d" % (f, s)]).to(device)
        fixed[("color_aug", f, 0)] = unit(g["wide_color_aug_0_%d" % f]).to(device)
        assert not torch.equal(fixed[("color_aug", f, 0)], fixed[("color", f, 0)])
    for s in range(4):
        fixed[("K", s)], fixed[("inv_K", s)] = _dev(g["wide_K_%d" % s], device), _dev(g["wide_inv_K_%d" % s], device)
    loss_a, grads_a = step(built)
    loss_b, grads_b = step(fixed)
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b), (loss_a, loss_b)
    assert grads_a.keys() == grads_b.keys() and len(grads_a) > 50
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k
