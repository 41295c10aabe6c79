"""Cases shared by the CPU run (kernels under the interpreter, tests/test_device_batch_emu.py) and the GPU run
(tests/test_device_batch_gpu.py) of the device batch builder (loader/device_batch.py, csrc/batchprep.hip).

Expected values come from tests/golden/device_batch.npz, written by tests/golden/make_device_batch.py from the reference's own
loader code and Pillow.  Every comparison is exact (torch.equal / np.array_equal).  The file keeps the colour pyramids as the
uint8 images behind them (a quarter of the bytes): the generator asserts that the reference's float tensors are exactly
``unit()`` of those, the division ToTensor performs.

``pillow_half`` below is a numpy restatement of Pillow's 8-bit resampler for the Lanczos filter at a reduction by exactly 2,
written output by output straight from Resample.c (no coefficient-row sharing as in the kernel): the fixture generator checks
it against ``Image.resize`` itself, and case C uses its unclipped sums to show that the clip to 0..255 is hit in both passes.
"""
import math
import os
import random

import numpy as np
import torch

from conftest import GOLDEN
from improving_segmentation_with_selfsupervised_depth_amd import _lib, hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.loader.device_batch import DeviceBatchBuilder, lanczos_half_table

FRAMES = (0, -1, 1)
INTRINSICS = (2262.52, 2265.3017905988554, 1096.98, 513.137)      # the Cityscapes loader's fx, fy, u0, v0

# Case A: every border case at once.  48x80 frames, crop 40x72 -> levels 20x36, 10x18, 5x9: level 3 is 9 wide from 18, so every
# horizontal window there is clipped (5 high from 10: every vertical one too).  Offsets (0,0), the maximum (8,8) and (3,5).
CASE_A = dict(height=48, width=80, crop_h=40, crop_w=72, crops=[(0, 0), (8, 8), (3, 5)], flips=[False, True, True])
# Case B: more than one tile in both directions.  The pyramid kernel's tile is 64 x 16 outputs (PYR_W x PYR_H, csrc/batchprep.hip):
# 64x288 frames, no crop -> level 1 is 32x144 = 3 x 2 tiles (the last column of tiles 16 wide), level 2 is 16x72 = 2 x 1 tiles;
# widths 288 and 144 take the 16-byte staging path, 72 the byte path.
CASE_B = dict(height=64, width=288)
# Case C: 0 / 255 checkerboards (and noise, and a smooth ramp) at 32x64
CASE_C = dict(height=32, width=64)
# Case D (not in the golden file's reference run: Pillow directly, one scale): a crop whose width is no multiple of 4, so the
# crop kernel's scalar store path runs; 21x37 from 24x45, B = 2, second sample flipped
CASE_D = dict(height=24, width=45, crop_h=21, crop_w=37, crops=[(8, 3), (1, 0)], flips=[False, True])


def golden():
    z = np.load(os.path.join(GOLDEN, "device_batch.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---- numpy restatement of Pillow's resampler ----------------------------------------------------------------------------
def _lanczos(x):
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def _axis_coeffs(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc: per output (xmin, int weights)"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) / filterscale) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        k = [v / ww for v in w]
        out.append((xmin, np.array([int(v * 4194304.0 - 0.5) if v < 0 else int(v * 4194304.0 + 0.5) for v in k], dtype=np.int64)))
    return out


def _pass(img, out_size, want_raw=False):
    """one pass along the LAST axis of a uint8 array; returns uint8 (and the unclipped sums >> 22)"""
    coeffs = _axis_coeffs(img.shape[-1], out_size)
    raw = np.empty(img.shape[:-1] + (out_size,), dtype=np.int64)
    src = img.astype(np.int64)
    for xx, (xmin, k) in enumerate(coeffs):
        raw[..., xx] = ((1 << 21) + (src[..., xmin:xmin + len(k)] * k).sum(-1)) >> 22
    out = np.clip(raw, 0, 255).astype(np.uint8)
    return (out, raw) if want_raw else out


def pillow_half(img, want_raw=False):
    """img [..., H, W] uint8 -> [..., H/2, W/2] as Image.resize((W/2, H/2), Image.LANCZOS) computes it: horizontal pass, uint8
    image, vertical pass.  want_raw: also the unclipped values of both passes."""
    Hs, Ws = img.shape[-2:]
    assert Hs % 2 == 0 and Ws % 2 == 0
    mid, raw_h = _pass(img, Ws // 2, True)
    out, raw_v = _pass(np.swapaxes(mid, -1, -2), Hs // 2, True)
    out, raw_v = np.swapaxes(out, -1, -2), np.swapaxes(raw_v, -1, -2)
    return (np.ascontiguousarray(out), raw_h, raw_v) if want_raw else np.ascontiguousarray(out)


def unit(u8):
    """ToTensor of a uint8 array: float32 division by 255 (IEEE, correctly rounded)"""
    return torch.from_numpy(np.ascontiguousarray(u8)).to(torch.float32).div(255)


# ---- helpers ------------------------------------------------------------------------------------------------------------
def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _frames(g, prefix, device):
    return {f: _dev(g["%s_frame_%d" % (prefix, f)], device) for f in FRAMES}


def _check_colors(inputs, g, prefix, scales=4):
    for f in FRAMES:
        for s in range(scales):
            got = inputs[("color", f, s)].cpu()
            want = unit(g["%s_color_%d_%d" % (prefix, f, s)])
            assert got.dtype == torch.float32 and got.shape == want.shape, (prefix, f, s, got.shape, want.shape)
            assert torch.equal(got, want), "%s color frame %d scale %d: %d of %d values differ" % (
                prefix, f, s, int((got != want).sum()), want.numel())
        assert torch.equal(inputs[("color_aug", f, 0)].cpu(), unit(g["%s_color_%d_0" % (prefix, f)]))


def _check_K(inputs, g, prefix, scales=4):
    for s in range(scales):
        for name in ("K", "inv_K"):
            got = inputs[(name, s)].cpu()
            want = torch.from_numpy(g["%s_%s_%d" % (prefix, name, s)])
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and torch.equal(got, want), (prefix, name, s)


# ---- cases --------------------------------------------------------------------------------------------------------------
def run_case_a(device):
    """crop + flip + three chained levels whose borders meet, labels (table, crop, flip, an unlabeled sample, one-hot with
    ignore pixels), pseudo_depth, K / inv_K of flipped and unflipped samples -- against the reference's __getitem__"""
    g = golden()
    c = CASE_A
    kw = dict(intrinsics=INTRINSICS, label_lut=g["lut"], n_classes=19, random_horizontal_flip=0.5)
    frames = _frames(g, "a", device)
    args = dict(pseudo_depth=_dev(g["a_pd_u8"], device), is_labeled=g["a_is_labeled"], idx=g["a_idx"], crops=np.array(c["crops"]),
                flips=np.array(c["flips"]))
    inputs = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], **kw)(frames, lbl=_dev(g["a_lbl_u8"], device), **args)
    assert "onehot_lbl" not in inputs
    _check_colors(inputs, g, "a")
    _check_K(inputs, g, "a")
    # the reference's one_hot raises on id 255, which encode_segmap keeps: the one-hot run has a label map without it
    onehot = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], load_onehot=True, **kw)(
        frames, lbl=_dev(g["a_lbl_oh_u8"], device), **args)
    for got, name, dtype in ((inputs["lbl"], "a_lbl", torch.int64), (inputs["pseudo_depth"], "a_pseudo_depth", torch.float32),
                             (onehot["lbl"], "a_lbl_oh", torch.int64), (onehot["onehot_lbl"], "a_onehot_lbl", torch.int64)):
        want = torch.from_numpy(g[name])
        got, want = got.cpu(), (want.to(torch.int64) if dtype == torch.int64 else want)      # label expectations are stored as uint8
        assert got.dtype == dtype and got.shape == want.shape and torch.equal(got, want), name
    labeled = g["a_is_labeled"].tolist()
    assert labeled == [True, False, True]
    assert bool((inputs["lbl"][1] == 250).all()) and int(onehot["onehot_lbl"][1].sum()) == 0           # the unlabeled sample
    lab, oh = onehot["lbl"][2], onehot["onehot_lbl"][2]                                                  # a labeled, flipped one
    assert len(torch.unique(inputs["lbl"][2])) == 21 and bool((inputs["lbl"][2] == 255).any())           # 19 classes, 250 and 255
    assert bool((lab == 250).any()) and bool((oh.sum(0) == (lab != 250)).all()) and int(oh.sum()) > 0     # ignore pixels: all planes zero
    assert inputs["is_labeled"].dtype == torch.bool and inputs["is_labeled"].cpu().tolist() == labeled
    assert inputs["idx"].cpu().tolist() == g["a_idx"].tolist()


def run_label_table():
    """the reference's encode_segmap is a table: applying it to a label map equals indexing encode_segmap(arange(256)) -- recorded
    by the generator for a map with every id 0..33 and 255 (CPU, no kernel)"""
    g = golden()
    assert set(range(34)) | {255} <= set(np.unique(g["a_lbl_u8"]).tolist())
    assert np.array_equal(g["lut"][g["a_lbl_u8"]], g["a_lbl_encoded_full"].astype(np.int64))


def run_case_b(device):
    """tile seams in both directions, both staging paths, no crop and no flip (the validation path: is_train=False)"""
    g = golden()
    c = CASE_B
    b = DeviceBatchBuilder(c["height"], c["width"], crop_h=32, crop_w=64, intrinsics=INTRINSICS, is_train=False)
    assert (b.crop_h, b.crop_w) == (c["height"], c["width"])          # the reference ignores the crop outside training (:81-83)
    random.seed(11)
    for _ in range(2 * g["b_frame_0"].shape[0]):                       # the reference's random_crop: randint(0, 0) for x1 and y1, no coins
        random.randint(0, 0)
    want_state = random.getstate()
    random.seed(11)
    inputs = b(_frames(g, "b", device))
    assert random.getstate() == want_state
    _check_colors(inputs, g, "b")
    _check_K(inputs, g, "b")


def run_case_c(device):
    """saturation: 0 / 255 checkerboards overshoot in both passes and are clipped exactly as Pillow clips"""
    g = golden()
    c = CASE_C
    f0 = g["c_frame_0"]                                                # [B,H,W,3]
    planes = np.ascontiguousarray(np.moveaxis(f0, -1, 1))
    out, raw_h, raw_v = pillow_half(planes, want_raw=True)
    assert raw_h.min() < 0 and raw_h.max() > 255 and raw_v.min() < 0 and raw_v.max() > 255        # both passes overshoot ...
    assert out.min() == 0 and out.max() == 255                                                       # ... and the result holds both ends
    assert np.array_equal(out, g["c_color_0_1"])                                       # the restatement is Pillow
    b = DeviceBatchBuilder(c["height"], c["width"], intrinsics=INTRINSICS, num_scales=3)
    inputs = b(_frames(g, "c", device), crops=np.zeros((f0.shape[0], 2), np.int32), flips=np.zeros(f0.shape[0], bool))
    _check_colors(inputs, g, "c", scales=3)


def run_case_d(device):
    """a crop width that is no multiple of 4 (scalar stores), one scale; expected values: the flip / crop as array slicing"""
    c = CASE_D
    rng = np.random.RandomState(5)
    fr = {f: rng.randint(0, 256, (2, c["height"], c["width"], 3), dtype=np.uint8) for f in FRAMES}
    pd = rng.randint(0, 256, (2, c["height"], c["width"]), dtype=np.uint8)
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], intrinsics=INTRINSICS, num_scales=1)
    inputs = b({f: _dev(v, device) for f, v in fr.items()}, pseudo_depth=_dev(pd, device), crops=np.array(c["crops"]),
               flips=np.array(c["flips"]))

    def cut(a, i):
        x1, y1 = c["crops"][i]
        a = a[i, :, ::-1] if c["flips"][i] else a[i]
        return a[y1:y1 + c["crop_h"], x1:x1 + c["crop_w"]]
    for f in FRAMES:
        want = torch.stack([unit(np.moveaxis(cut(fr[f], i), -1, 0)) for i in range(2)])
        assert torch.equal(inputs[("color", f, 0)].cpu(), want), f
    assert torch.equal(inputs["pseudo_depth"].cpu(), torch.stack([unit(cut(pd, i))[None] for i in range(2)]))


def run_unit_division(device):
    """u8 / 255 of the kernels is the IEEE division for all 256 inputs"""
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 4, 64)
    got = H.batchprep_plane(_dev(ramp, device), None, None, 4, 64).cpu().reshape(-1)
    assert torch.equal(got, torch.arange(256, dtype=torch.float32) / 255)
    fr = np.repeat(ramp[..., None], 3, axis=-1)
    _, f32 = H.batchprep_crop(_dev(fr, device), None, None, 4, 64)
    assert torch.equal(f32.cpu()[0, 1].reshape(-1), torch.arange(256, dtype=torch.float32) / 255)


def run_rejected_shapes(device):
    """levels that are not an exact half: SEGSDE_ERR_SHAPE from the library, RuntimeError in Python"""
    lib = _lib.lib()
    src = torch.zeros((3, 10, 18), dtype=torch.uint8, device=device)
    coef = torch.from_numpy(lanczos_half_table(5, 9)).to(device)
    u8, f32 = torch.zeros((3, 5, 9), dtype=torch.uint8, device=device), torch.zeros((3, 5, 9), device=device)
    p = lambda t: t.data_ptr()
    assert lib.segsde_batchprep_pyramid_level(p(src), 3, 10, 18, p(coef), 5, 9, p(u8), p(f32), None) == 0
    for hs, ws, hd, wd in ((10, 17, 5, 8), (9, 18, 4, 9), (10, 18, 5, 8), (10, 18, 4, 9), (10, 18, 10, 18), (10, 18, 0, 0)):
        assert lib.segsde_batchprep_pyramid_level(p(src), 3, hs, ws, p(coef), hd, wd, p(u8), p(f32), None) == -2, (hs, ws, hd, wd)
    assert lib.segsde_batchprep_pyramid_level(None, 3, 10, 18, p(coef), 5, 9, p(u8), p(f32), None) == -1
    assert lib.segsde_batchprep_crop(p(src), 1, 10, 6, None, None, 8, 6, p(u8), p(f32), None) == -2      # a crop without offsets
    assert lib.segsde_batchprep_crop(p(src), 1, 10, 6, None, None, 12, 6, p(u8), p(f32), None) == -2     # larger than the frame
    try:
        H.batchprep_pyramid_level(torch.zeros((3, 10, 17), dtype=torch.uint8, device=device), coef)
    except RuntimeError as e:
        assert "bad shape" in str(e)
    else:
        raise AssertionError("odd level accepted")
    # through the builder: 20x36 -> 10x18 -> 5x9 is fine, 20x34 reaches an odd width at level 2
    b = DeviceBatchBuilder(20, 34, intrinsics=INTRINSICS, num_scales=3, frame_idxs=(0,))
    try:
        b({0: torch.zeros((1, 20, 34, 3), dtype=torch.uint8, device=device)}, crops=np.zeros((1, 2), np.int32), flips=np.zeros(1, bool))
    except RuntimeError as e:
        assert "bad shape" in str(e)
    else:
        raise AssertionError("odd level accepted by the builder")


def run_draw():
    """draw() replays the reference's draws: with random.seed(7) it equals what the reference's __getitem__ drew (recorded)"""
    g = golden()
    c = CASE_A
    n = len(g["draw_crops"])
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], intrinsics=INTRINSICS, random_horizontal_flip=0.5)
    random.seed(7)
    crops, flips = b.draw(n)
    assert np.array_equal(crops, g["draw_crops"]) and np.array_equal(flips, g["draw_flips"])
    assert flips.any() and not flips.all() and len(np.unique(crops[:, 0])) > 2
    after = random.random()
    assert after == float(g["draw_next_random"])                       # and leaves the generator where the reference leaves it
    # no flip configured: one coin fewer per sample
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], intrinsics=INTRINSICS)
    random.seed(7)
    crops, flips = b.draw(n)
    assert np.array_equal(crops, g["draw_noflip_crops"]) and not flips.any()


def run_end_to_end(device):
    """a tiny R18 mono model step fed from the builder equals, bit for bit, the step fed from the fixture's float tensors: the
    dict is accepted unchanged by model() and MonodepthLoss"""
    import model_cases as MC
    from oracle import nets as N
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    g = golden()
    cfg = dict(MC.contract_cfgs()["cfgs"]["r18_mono"])
    Hh, W = CASE_B["height"], CASE_B["width"]
    cfg["height"], cfg["width"] = Hh, W
    sd = N.build_state_dict(cfg, 19, seed=11, randomize_bn=True)
    B = g["b_frame_0"].shape[0]
    gen = torch.Generator().manual_seed(3)
    noise = {s: torch.randn(B, 2, Hh, W, generator=gen) for s in range(4)}
    tcfg = {"training": {"batch_size": B, "monodepth_loss": dict(
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

    b = DeviceBatchBuilder(Hh, W, intrinsics=INTRINSICS, is_train=False)
    built = b(_frames(g, "b", device))
    fixed = {}
    for f in FRAMES:
        for s in range(4):
            fixed[("color", f, s)] = unit(g["b_color_%d_%d" % (f, s)]).to(device)
        fixed[("color_aug", f, 0)] = fixed[("color", f, 0)]
    for s in range(4):
        fixed[("K", s)], fixed[("inv_K", s)] = _dev(g["b_K_%d" % s], device), _dev(g["b_inv_K_%d" % s], device)
    loss_a, grads_a = step(built)
    loss_b, grads_b = step(fixed)
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b), (loss_a, loss_b)
    assert grads_a.keys() == grads_b.keys() and len(grads_a) > 50
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k
