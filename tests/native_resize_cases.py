"""Cases shared by the CPU run (kernels under the interpreter, tests/test_native_resize_emu.py) and the GPU run
(tests/test_native_resize_gpu.py) of the native-resolution front end of the device batch builder: pil_loader's resize on the
device (loader/device_batch.py ``pil_resize`` and ``DeviceBatchBuilder``; csrc/resize.hip, labels_rgb_kernel of csrc/batchprep.hip).

Expected values come from tests/golden/native_resize.npz, written by tests/golden/make_native_resize.py: seeded images saved as
PNG, loaded and resized by the reference's own ``pil_loader`` / ``_load`` and run through the reference's ``__getitem__``
(Pillow 12.2.0).  Every comparison is exact (torch.equal / np.array_equal).

``pillow_resize`` / ``pillow_nearest`` below are numpy restatements of Pillow's 8-bit Lanczos resampler at ANY ratio (Resample.c,
output by output) and of its nearest resize (Geometry.c ImagingScaleAffine: an accumulated float64 step).  The fixture generator
checks them against ``Image.resize`` on every stored case; the saturation case uses the unclipped sums to show that the clip to
0..255 is hit in both passes.

Tile constants of the kernels (csrc/resize.hip): the horizontal pass makes RSH_W = 64 output pixels of RSH_ROWS = 32 source rows
per block, RSH_R = 8 rows at a time; the vertical pass RSV_H = 16 output rows of RSV_WB = 256 bytes (85.3 pixels) per block.
"""
import math
import os

import numpy as np
import torch

import device_batch_cases as DC
from conftest import GOLDEN
from improving_segmentation_with_selfsupervised_depth_amd import _lib, hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.loader import device_batch as DB
from improving_segmentation_with_selfsupervised_depth_amd.loader.device_batch import DeviceBatchBuilder, pil_resize

FRAMES = DC.FRAMES
INTRINSICS = DC.INTRINSICS
unit = DC.unit

# Border-cut windows: 97x131 -> 48x80, ratios 2.02 and 1.64 (15 and 11 taps); every window within 6 / 5 outputs of a border is cut
# and renormalised.  Then device_batch case A's crop 40x72 with its flips and offsets, four scales, labels, K.
CASE_BORDER = dict(src=(97, 131), height=48, width=80, crop_h=40, crop_w=72, crops=DC.CASE_A["crops"], flips=DC.CASE_A["flips"])
# Exact 2:1 (original Cityscapes) over several blocks: 128x576 -> 64x288 is 4.5 x 4 blocks of the horizontal pass (288 / 64 outputs,
# 128 / 32 rows) and 3.4 x 4 blocks of the vertical pass (864 / 256 bytes, 64 / 16 rows); rows of 3 * 288 = 864 bytes take the
# 16-byte paths, 128x296 -> 64x148 (444-byte rows) the byte paths.  The result must equal device_batch_cases.pillow_half.
CASE_HALF = dict(a=((128, 576), (64, 288)), b=((128, 296), (64, 148)))
# Enlargement: filterscale stays 1, six taps (ksize 7)
CASE_UP = ((20, 30), (32, 48))
# One axis only: the other pass is not launched
CASE_AXIS = dict(w=((48, 160), (48, 80)), h=((96, 80), (48, 80)))
# Many taps: 300 -> 64 has ksize 31 (29 taps in use), 401 -> 128 ksize 21 (19); 123 -> 16 ksize 49 (46), 77 -> 8 ksize 59 (58).  The limit is
# RESIZE_MAX_TAPS = 64 (ksize is odd): 82 -> 8 has ksize 63 and runs, 84 -> 8 has ksize 65 and is refused.
CASE_TAPS = dict(a=((300, 401), (64, 128)), b=((123, 77), (16, 8)), lim=((82, 82), (8, 8)), over=((84, 84), (8, 8)))
# Labels: 97x131 -> 48x80 (with the border case) and the enlargement 20x30 -> 33x47, where int((x + 0.5) * in / out) is not Pillow
CASE_LABELS_UP = dict(src=(20, 30), height=33, width=47, crop_h=29, crop_w=43, crops=[(4, 4), (1, 2)], flips=[True, False])
# Colour-coded labels (Mapillary): 60x100 -> 48x80, crop 40x72
CASE_COLORS = dict(src=(60, 100), height=48, width=80, crop_h=40, crop_w=72, crops=[(8, 0), (3, 8), (0, 5)], flips=[False, True, True])


def golden():
    z = np.load(os.path.join(GOLDEN, "native_resize.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---- numpy restatement of Pillow's resampler at any ratio ---------------------------------------------------------------
def _lanczos(x):
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def axis_coeffs(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc: per output (xmin, int64 weights)"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        k = [v / ww for v in w] if ww != 0.0 else w
        out.append((xmin, np.array([int(v * 4194304.0 - 0.5) if v < 0 else int(v * 4194304.0 + 0.5) for v in k], dtype=np.int64)))
    return out


def _pass(img, axis, out_size):
    """one pass along ``axis`` of a uint8 array: (uint8 result, the unclipped sums >> 22)"""
    src = np.moveaxis(img.astype(np.int64), axis, -1)
    raw = np.empty(src.shape[:-1] + (out_size,), dtype=np.int64)
    for xx, (xmin, k) in enumerate(axis_coeffs(src.shape[-1], out_size)):
        raw[..., xx] = ((1 << 21) + (src[..., xmin:xmin + len(k)] * k).sum(-1)) >> 22
    raw = np.moveaxis(raw, -1, axis)
    return np.clip(raw, 0, 255).astype(np.uint8), raw


def pillow_resize(img, size, want_raw=False):
    """img [..., Hs, Ws, C] uint8 -> [..., height, width, C] as Image.resize((width, height), Image.LANCZOS) computes it: the
    horizontal pass, a uint8 image, the vertical pass; a pass whose axis keeps its size is skipped.  want_raw: also the unclipped
    values of the passes that ran (None for a skipped one)."""
    height, width = size
    raw_h = raw_v = None
    if img.shape[-2] != width:
        img, raw_h = _pass(img, -2, width)
    if img.shape[-3] != height:
        img, raw_v = _pass(img, -3, height)
    img = np.ascontiguousarray(img)
    return (img, raw_h, raw_v) if want_raw else img


def nearest_index(in_size, out_size):
    """ImagingScaleAffine: start at a0 / 2, add a0 per output, truncate"""
    a0 = float(in_size) / out_size
    xo, idx = a0 * 0.5, []
    for _ in range(out_size):
        idx.append(int(xo))
        xo += a0
    return np.array(idx, dtype=np.int64)


def pillow_nearest(img, size):
    """img [Hs, Ws(, C)] -> [height, width(, C)] as Image.resize((width, height), Image.NEAREST)"""
    return np.ascontiguousarray(img[nearest_index(img.shape[0], size[0])][:, nearest_index(img.shape[1], size[1])])


# ---- helpers ------------------------------------------------------------------------------------------------------------
def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), "%s: %d of %d values differ" % (what, int((got != want).sum()), want.size)


class Launches:
    """records which hipops.batchprep_* wrappers run"""

    def __enter__(self):
        self.names, self._keep = [], {}
        for name in dir(H):
            if name.startswith("batchprep_"):
                self._keep[name] = getattr(H, name)
                setattr(H, name, self._wrap(name, self._keep[name]))
        return self

    def _wrap(self, name, fn):
        def call(*a, **kw):
            self.names.append(name[len("batchprep_"):])
            return fn(*a, **kw)
        return call

    def __exit__(self, *exc):
        for name, fn in self._keep.items():
            setattr(H, name, fn)


def _resize_both_ways(src, size, want, device, what):
    """pil_resize on a batch tensor and on a list whose sample starts at an odd address (the byte paths of the staging)"""
    _same(pil_resize(_dev(src[None], device), size), want[None], what)
    buf = torch.zeros((src.size + 16,), dtype=torch.uint8, device=device)
    odd = buf[1:1 + src.size].view(src.shape)
    odd.copy_(_dev(src, device))
    _same(pil_resize([odd], size), want[None], what + " (odd address)")


# ---- cases --------------------------------------------------------------------------------------------------------------
def run_border_case(device):
    """native 97x131 frames and label maps -> 48x80 -> device_batch case A's crop, flips, four scales, labels, one-hot, K: against the
    reference's pil_loader + __getitem__"""
    g = golden()
    c = CASE_BORDER
    assert g["na_frame_0"].shape[1:3] == c["src"]
    kw = dict(intrinsics=INTRINSICS, label_lut=g["lut"], n_classes=19, random_horizontal_flip=0.5)
    frames = {f: _dev(g["na_frame_%d" % f], device) for f in FRAMES}
    args = dict(is_labeled=g["na_is_labeled"], crops=np.array(c["crops"]), flips=np.array(c["flips"]))
    _same(pil_resize(frames[0], (c["height"], c["width"])), g["na_resized_0"], "pil_loader of frame 0")
    _same(pil_resize(_dev(g["na_lbl_u8"], device), (c["height"], c["width"]), "nearest"), g["na_lbl_resized"], "pil_loader of the labels")
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], **kw)
    with Launches() as rec:
        inputs = b(frames, lbl=_dev(g["na_lbl_u8"], device), **args)
    # one launch per pass for all nine images, one nearest launch, then the launches device_batch always made
    assert rec.names == ["resample_rows", "resample_cols"] + ["crop"] * 3 + ["pyramid_level"] * 3 + ["resize_nearest", "labels"], rec.names
    DC._check_colors(inputs, g, "na")
    DC._check_K(inputs, g, "na")
    onehot = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], load_onehot=True, **kw)(
        frames, lbl=_dev(g["na_lbl_oh_u8"], device), **args)
    for got, name in ((inputs["lbl"], "na_lbl"), (onehot["lbl"], "na_lbl_oh"), (onehot["onehot_lbl"], "na_onehot_lbl")):
        assert got.dtype == torch.int64
        _same(got, g[name].astype(np.int64), name)
    assert set(range(34)) | {255} <= set(np.unique(g["na_lbl_resized"]).tolist())           # every id survives the resize
    assert bool((inputs["lbl"][1] == 250).all()) and g["na_is_labeled"].tolist() == [True, False, True]
    assert len(torch.unique(inputs["lbl"][2])) == 21


def run_exact_half(device):
    """2:1 over several blocks of both kernels; the 16-byte and the byte paths; equal to the pyramid's pillow_half; through the
    validation path of a single-frame, single-scale builder (the inference loader's shape)"""
    g = golden()
    for tag in ("a", "b"):
        (hs, ws), (h, w) = CASE_HALF[tag]
        src, want = g["h_src_" + tag], g["h_out_" + tag]
        assert src.shape == (hs, ws, 3) and want.shape == (h, w, 3)
        assert np.array_equal(np.moveaxis(DC.pillow_half(np.ascontiguousarray(np.moveaxis(src, -1, 0))), 0, -1), want)
        _resize_both_ways(src, (h, w), want, device, "half " + tag)
        b = DeviceBatchBuilder(h, w, crop_h=32, crop_w=64, intrinsics=INTRINSICS, is_train=False, frame_idxs=(0,), num_scales=1)
        inputs = b({0: _dev(src[None], device)})
        assert torch.equal(inputs[("color", 0, 0)].cpu(), unit(np.moveaxis(want, -1, 0)[None]))       # the generator: __getitem__'s scale 0
        for name in ("K", "inv_K"):
            assert torch.equal(inputs[(name, 0)].cpu(), torch.from_numpy(g["h_%s_%s" % (name, tag)]))


def run_enlargement(device):
    g = golden()
    (hs, ws), size = CASE_UP
    assert g["up_src"].shape == (hs, ws, 3)
    assert DB.lanczos_taps(ws, size[1]) == 7 and DB.resample_tables(ws, size[1])[0][:, 1].max() == 6
    _resize_both_ways(g["up_src"], size, g["up_out"], device, "enlargement")


def run_one_axis(device):
    """a 0 / 255 checkerboard resized along one axis only: the other pass is not launched"""
    g = golden()
    for tag, ran in (("w", "resample_rows"), ("h", "resample_cols")):
        (hs, ws), size = CASE_AXIS[tag]
        src = g["ax_src_" + tag]
        assert src.shape == (hs, ws, 3) and set(np.unique(src).tolist()) == {0, 255}
        with Launches() as rec:
            _resize_both_ways(src, size, g["ax_out_" + tag], device, "one axis " + tag)
        assert rec.names == [ran, ran], rec.names
        out, raw_h, raw_v = pillow_resize(src, size, want_raw=True)
        assert (raw_h is None) != (raw_v is None) and np.array_equal(out, g["ax_out_" + tag])


def run_many_taps(device):
    g = golden()
    for tag in ("a", "b", "lim"):
        (hs, ws), size = CASE_TAPS[tag]
        assert g["mt_src_" + tag].shape == (hs, ws, 3)
        _resize_both_ways(g["mt_src_" + tag], size, g["mt_out_" + tag], device, "many taps " + tag)
    used = lambda i, o: int(DB.resample_tables(i, o)[0][:, 1].max())
    assert (used(300, 64), used(401, 128), used(123, 16), used(77, 8)) == (29, 19, 46, 58)
    assert DB.lanczos_taps(82, 8) == 63 and DB.lanczos_taps(84, 8) == 65 and DB.RESIZE_MAX_TAPS == 64
    # one builder call at one scale
    (hs, ws), (h, w) = CASE_TAPS["b"]
    b = DeviceBatchBuilder(h, w, intrinsics=INTRINSICS, frame_idxs=(0,), num_scales=1, is_train=False)
    got = b({0: [_dev(g["mt_src_b"], device)]})[("color", 0, 0)]
    assert torch.equal(got.cpu(), unit(np.moveaxis(g["mt_out_b"], -1, 0)[None]))


def run_tap_limit(device):
    """just above the limit: ValueError from the Python layer, SEGSDE_ERR_UNSUPPORTED (-4) from the entry points, nothing launched"""
    (hs, ws), size = CASE_TAPS["over"]
    src = torch.zeros((1, hs, ws, 3), dtype=torch.uint8, device=device)
    for images in (src, torch.zeros((1, hs, 8, 3), dtype=torch.uint8, device=device), torch.zeros((1, 8, ws, 3), dtype=torch.uint8, device=device)):
        try:
            pil_resize(images, size)
        except ValueError as e:
            assert "unsupported" in str(e) and "65 taps" in str(e), e
        else:
            raise AssertionError("a 65-tap window was accepted")
    b = DeviceBatchBuilder(8, 8, intrinsics=INTRINSICS, frame_idxs=(0,), num_scales=1)
    try:
        b({0: src})
    except ValueError as e:
        assert "unsupported" in str(e)
    else:
        raise AssertionError("a 65-tap window was accepted by the builder")
    lib = _lib.lib()
    desc = torch.zeros((1, 8), dtype=torch.int64, device=device)
    p = desc.data_ptr()
    assert lib.segsde_batchprep_resample_rows(p, 1, hs, 8, 65, 700, None) == -4
    assert lib.segsde_batchprep_resample_cols(p, 1, 24, 8, 65, 200, None) == -4
    assert lib.segsde_batchprep_resample_rows(p, 1, hs, 8, 63, 100000, None) == -4           # a stage that does not fit the LDS
    assert lib.segsde_batchprep_resample_cols(p, 1, 24, 8, 63, 1000, None) == -4
    assert lib.segsde_batchprep_resample_rows(None, 1, hs, 8, 63, 700, None) == -1
    assert lib.segsde_batchprep_resample_rows(p, 0, hs, 8, 63, 700, None) == -2
    assert lib.segsde_batchprep_resize_nearest(p, 1, 8, 8, 2, None) == -2
    try:
        H.batchprep_resample_rows(desc, hs, 8, 65, 700)
    except RuntimeError as e:
        assert "unsupported" in str(e)
    else:
        raise AssertionError("65 taps accepted by hipops")


def run_saturation(device):
    """0 / 255 checkerboards and random 0 / 255 pixels overshoot in both passes and are clipped exactly as Pillow clips"""
    g = golden()
    c = CASE_BORDER
    src = g["sat_src"]
    assert src.shape[1:3] == c["src"] and set(np.unique(src).tolist()) == {0, 255}
    size = (c["height"], c["width"])
    for i in range(src.shape[0]):
        out, raw_h, raw_v = pillow_resize(src[i], size, want_raw=True)
        assert raw_h.min() < 0 and raw_h.max() > 255 and raw_v.min() < 0 and raw_v.max() > 255, i
        assert out.min() == 0 and out.max() == 255 and np.array_equal(out, g["sat_out"][i])
    _same(pil_resize(_dev(src, device), size), g["sat_out"], "saturation")


def run_per_sample_sizes(device):
    """three sources of three sizes in one call; the last has the working size and comes out as it went in"""
    g = golden()
    c = CASE_BORDER
    srcs = [g["na_frame_0"][0], g["ps_src_1"], g["ps_src_2"]]
    assert [s.shape[:2] for s in srcs] == [(97, 131), (60, 100), (48, 80)]
    with Launches() as rec:
        got = pil_resize([_dev(s, device) for s in srcs], (c["height"], c["width"]))
    assert rec.names == ["resample_rows", "resample_cols"], rec.names
    _same(got, g["ps_out"], "per-sample sizes")
    assert np.array_equal(g["ps_out"][2], srcs[2]) and np.array_equal(g["ps_out"][0], g["na_resized_0"][0])
    b = DeviceBatchBuilder(c["height"], c["width"], intrinsics=INTRINSICS, frame_idxs=(0,), num_scales=1, is_train=False)
    inputs = b({0: [_dev(s, device) for s in srcs]})
    assert torch.equal(inputs[("color", 0, 0)].cpu(), unit(np.moveaxis(g["ps_out"], -1, 1)))


def run_labels_enlarged(device):
    """20x30 frames and labels -> 33x47 (nearest: Pillow's accumulated step, not the naive rule), then flip, crop, table, one-hot"""
    g = golden()
    c = CASE_LABELS_UP
    naive = lambda i, o: np.array([int((x + 0.5) * i / o) for x in range(o)])
    differ = sum(int((naive(i, o) != DB.nearest_table(i, o)).sum()) for i, o in zip(c["src"], (c["height"], c["width"])))
    assert differ > 0                                                         # the case is one where the naive index rule fails
    for i, o in ((20, 33), (30, 47), (97, 48), (131, 80), (7, 50)):
        assert np.array_equal(DB.nearest_table(i, o), nearest_index(i, o))
    assert set(range(34)) | {255} <= set(np.unique(g["lb_lbl_u8"]).tolist())
    _same(pil_resize(_dev(g["lb_lbl_u8"], device), (c["height"], c["width"]), "nearest"), g["lb_lbl_resized"], "nearest enlargement")
    assert not np.array_equal(g["lb_lbl_u8"][0][naive(20, 33)][:, naive(30, 47)], g["lb_lbl_resized"][0])
    kw = dict(intrinsics=INTRINSICS, label_lut=g["lut"], n_classes=19, random_horizontal_flip=0.5, frame_idxs=(0,), num_scales=1,
              load_onehot=True)
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], **kw)
    inputs = b({0: _dev(g["lb_frame_0"], device)}, lbl=[_dev(m, device) for m in g["lb_lbl_oh_u8"]], crops=np.array(c["crops"]),
               flips=np.array(c["flips"]))
    assert torch.equal(inputs[("color", 0, 0)].cpu(), unit(g["lb_color_0_0"]))
    _same(inputs["lbl"], g["lb_lbl"].astype(np.int64), "lb_lbl")
    _same(inputs["onehot_lbl"], g["lb_onehot_lbl"].astype(np.int64), "lb_onehot_lbl")
    for name in ("K", "inv_K"):
        assert torch.equal(inputs[(name, 0)].cpu(), torch.from_numpy(g["lb_%s_0" % name]))


def run_color_labels(device):
    """Mapillary's colour-coded label maps: nearest resize, flip, crop, then encode_segmap's colour table (a later duplicate wins,
    no match -> 0, id 65 -> ignore_index) -- against MapillaryVistasLoader.__getitem__"""
    g = golden()
    c = CASE_COLORS
    colors, maps = g["cl_colors"], g["cl_lbl_rgb"]
    assert colors.shape == (66, 3) and maps.shape[1:] == c["src"] + (3,)
    triples = [tuple(t) for t in colors.tolist()]
    assert len(set(triples)) == 64                                            # two duplicate colours
    flat = set(map(tuple, maps.reshape(-1, 3).tolist()))
    assert flat - set(triples) and set(triples) <= flat                       # pixels that match no colour, and every colour
    b = DeviceBatchBuilder(c["height"], c["width"], c["crop_h"], c["crop_w"], n_classes=65, random_horizontal_flip=0.5, frame_idxs=(0,),
                           num_scales=1, label_colors=colors, load_onehot=True)
    with Launches() as rec:
        inputs = b({0: _dev(g["cl_frame_0"], device)}, lbl=_dev(maps, device), is_labeled=g["cl_is_labeled"], crops=np.array(c["crops"]),
                   flips=np.array(c["flips"]))
    assert rec.names == ["resample_rows", "resample_cols", "crop", "resize_nearest", "labels_rgb"], rec.names
    assert torch.equal(inputs[("color", 0, 0)].cpu(), unit(g["cl_color_0_0"]))
    _same(inputs["lbl"], g["cl_lbl"].astype(np.int64), "cl_lbl")
    want = g["cl_lbl"].astype(np.int64)
    assert {0, 250} <= set(np.unique(want).tolist()) and len(np.unique(want)) > 60
    oh = inputs["onehot_lbl"].cpu().numpy()
    assert oh.shape == (3, 65) + want.shape[1:] and np.array_equal(oh, (want[:, None] == np.arange(65)[None, :, None, None]).astype(np.int64))
    assert g["cl_is_labeled"].tolist() == [True, True, False] and bool((want[2] == 250).all()) and int(oh[2].sum()) == 0
    # a list of maps of the working size needs no resize; a builder without a colour table refuses colour-coded maps
    small = pil_resize(_dev(maps, device), (c["height"], c["width"]), "nearest")
    again = b({0: _dev(g["cl_frame_0"], device)}, lbl=list(small), is_labeled=g["cl_is_labeled"], crops=np.array(c["crops"]), flips=np.array(c["flips"]))
    _same(again["lbl"], want, "cl_lbl from resized maps")
    try:
        DeviceBatchBuilder(c["height"], c["width"], frame_idxs=(0,), num_scales=1)({0: _dev(g["cl_frame_0"], device)}, lbl=small)
    except ValueError as e:
        assert "label_colors" in str(e)
    else:
        raise AssertionError("colour-coded labels accepted without a table")


def run_unchanged(device):
    """frames that have the working size: the same launches as before this front end existed, and device_batch case A's tensors"""
    with Launches() as rec:
        DC.run_case_a(device)
    per_call = ["crop"] * 3 + ["pyramid_level"] * 3 + ["labels", "plane"]
    assert rec.names == per_call * 2, rec.names
    g = DC.golden()
    t = _dev(g["a_frame_0"], device)
    assert pil_resize(t, (DC.CASE_A["height"], DC.CASE_A["width"])) is t
