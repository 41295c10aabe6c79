"""The training ``inputs`` dict built on the GPU from decoded uint8 frames.

The reference prepares every sample on the CPU (loader/sequence_segmentation_loader.py:203-342): flip and crop three PIL frames,
three chained ``Image.ANTIALIAS`` resizes per frame, twelve ``ToTensor`` calls, ``encode_segmap``, ``K`` / ``inv_K`` for four
scales.  With ``DeviceBatchBuilder`` a DataLoader worker only decodes and hands over uint8 arrays; one batched stage on the
device (csrc/batchprep.hip) then produces exactly -- bit for bit -- what ``__getitem__`` plus collation produce.  This module is
not part of the reference's import surface.

Colour augmentation (``augmentations.color_aug``, on in the ``cityscapes_monodepth_highres_dec*.yml`` configs) is covered with
``color_aug=True``: per sample a coin, then torchvision's PIL ``ColorJitter`` (brightness, contrast, saturation, hue in a shuffled
order, a uint8 image between every two) on the scale-0 image of every frame.  The arithmetic is that of the Pillow the fixtures
were generated with (12.2.0: ``ImageEnhance``'s blend, ``convert("L")``, ``convert("HSV")`` and back), bit for bit.  torchvision
itself is not installed where this was written: the draw order of ``ColorJitter.get_params`` and the PIL functional operations
are restated from torchvision 0.7.0, the version the reference pins.  With ``color_aug=False`` (``cityscapes_joint.yml``)
``("color_aug", f, 0)`` is ``("color", f, 0)``, the same tensor.  There is no CPU path: without the HIP library every call raises.

Frames and label maps need not have the working size.  ``pil_loader(path, width, height)`` (loader/loader_utils.py:23-43) resizes
every decoded frame with ``Image.ANTIALIAS`` and every label map with ``Image.NEAREST``; the builder does the same on the device
(csrc/resize.hip) in front of everything else, so a worker hands over what it decoded: one tensor ``[B, Hs, Ws, 3]`` of any size,
or a list of ``B`` tensors whose sizes differ (Mapillary Vistas).  ``pil_resize`` is that step on its own.  The arithmetic is
Pillow 12.2.0's (Resample.c for the 8-bit Lanczos filter; Geometry.c ``ImagingScaleAffine`` for nearest), bit for bit; window
tables are built here in float64 by Pillow's formula, one per distinct (in, out) pair of an axis, and cached.
"""
import math
import random

import numpy as np
import torch

from .. import hipops as H

_PRECISION_BITS = 32 - 8 - 2          # Pillow, Resample.c
_TAPS, _ROWS = 12, 7


def _lanczos(x):
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def _pillow_window(xx, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for output ``xx`` of an axis reduced from 2 * n_out to n_out pixels with
    the Lanczos filter: (first source pixel, fixed-point weights).  Float64 throughout, the same operations in the same order."""
    in_size = 2 * n_out
    scale = in_size / n_out
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    center = (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), in_size) - xmin
    w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
    ww = 0.0
    for v in w:
        ww += v
    if ww != 0.0:
        w = [v / ww for v in w]
    one = float(1 << _PRECISION_BITS)
    return xmin, [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]


def lanczos_half_rows(n_out):
    """The coefficient rows of one axis as segsde_batchprep_pyramid_level reads them: int32 [7, 12]; tap j of output xx weighs
    source pixel 2 xx - 5 + j (zero outside the image).  Rows 0..2: the first three outputs; the last three rows in use (of
    min(n_out, 7)): the last three outputs; row 3: every interior output (whole windows are all alike)."""
    rows = np.zeros((_ROWS, _TAPS), dtype=np.int32)
    used = min(n_out, _ROWS)
    for r in range(used):
        xx = r if (r <= 3 or n_out < _ROWS) else n_out - (used - r)
        xmin, k = _pillow_window(xx, n_out)
        first = xmin - (2 * xx - 5)
        assert first >= 0 and first + len(k) <= _TAPS
        rows[r, first:first + len(k)] = k
    return rows


def lanczos_half_table(h_out, w_out):
    """int32 [2, 7, 12]: the rows of the y axis, then of the x axis"""
    return np.stack([lanczos_half_rows(h_out), lanczos_half_rows(w_out)])

RESIZE_MAX_TAPS = H.RESAMPLE_MAX_TAPS          # the widest window table (Pillow's ksize) the resampling kernels stage
_ROWS_TILE, _COLS_TILE = 64, 16                # outputs per block of the two passes (RSH_W, RSV_H in csrc/resize.hip)


def resample_tables(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the Lanczos filter, any ratio: (bounds int32 [out, 2] = first source
    pixel and number of taps of every output, weights int32 [out, ksize], zero beyond an output's taps).  Float64 throughout, the
    same operations in the same order; ksize = 2 ceil(support) + 1 with support = 3 max(in / out, 1)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    one = float(1 << _PRECISION_BITS)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    weights = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        weights[xx, :xmax] = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]
    return bounds, weights


def nearest_table(in_size, out_size):
    """The source index of every output of ``Image.resize(..., Image.NEAREST)``: int32 [out].  Pillow (Geometry.c,
    ImagingScaleAffine) starts at a0 * 0.5 with a0 = in / out in float64, ADDS a0 per output and truncates -- the accumulated
    rounding is part of the result, so ``int((x + 0.5) * in / out)`` is not the same on enlargements."""
    a0 = float(in_size) / out_size
    idx = np.zeros((out_size,), dtype=np.int32)
    xo = a0 * 0.5
    for x in range(out_size):
        xin = -1 if xo < 0.0 else int(xo)
        if 0 <= xin < in_size:
            idx[x] = xin
        xo += a0
    return idx


def _tile_span(bounds, tile):
    """source pixels from the first window's start to the last window's end, the most over the groups of ``tile`` outputs"""
    n = len(bounds)
    last = np.minimum(np.arange(0, n, tile) + tile, n) - 1
    return int((bounds[last, 0] + bounds[last, 1] - bounds[0:n:tile, 0]).max())


class ResizeTables:
    """The window / index tables of pil_resize, one per distinct (in, out) pair of an axis, on the host and per device"""

    def __init__(self):
        self._host, self._dev = {}, {}

    def _get(self, kind, n_in, n_out, device):
        key = (kind, int(n_in), int(n_out))
        if key not in self._host:
            if kind == "nearest":
                self._host[key] = (nearest_table(n_in, n_out),)
            else:
                bounds, weights = resample_tables(n_in, n_out)
                self._host[key] = (bounds, weights, _tile_span(bounds, _ROWS_TILE), _tile_span(bounds, _COLS_TILE))
        dkey = key + (str(device),)
        if dkey not in self._dev:
            self._dev[dkey] = tuple(torch.from_numpy(a).to(device) for a in self._host[key] if isinstance(a, np.ndarray))
        return self._host[key], self._dev[dkey]

    def lanczos(self, n_in, n_out, device):
        """(device bounds, device weights, taps, span over 64 outputs, span over 16 outputs)"""
        host, dev = self._get("lanczos", n_in, n_out, device)
        return dev[0], dev[1], host[1].shape[1], host[2], host[3]

    def nearest(self, n_in, n_out, device):
        return self._get("nearest", n_in, n_out, device)[1][0]


_TABLES = ResizeTables()


def lanczos_taps(in_size, out_size):
    """Pillow's ksize for this reduction (the pitch of the window table)"""
    return int(math.ceil(3.0 * max(in_size / out_size, 1.0))) * 2 + 1


def _samples(images, what):
    """a tensor [B, ...] or a list of per-sample tensors -> a list of contiguous uint8 tensors on one device"""
    items = list(images.unbind(0)) if torch.is_tensor(images) else list(images)
    if not items:
        raise ValueError("%s: no samples" % what)
    for t in items:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.device != items[0].device or t.dim() != items[0].dim() or \
                t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3) or min(t.shape) < 1:
            raise ValueError("%s: every sample must be a uint8 [Hs,Ws,3] or [Hs,Ws] tensor on one device, got %s" % (
                what, (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t)))
    return [t.contiguous() for t in items]


def pil_resize(images, size, resample="antialias", tables=None, what="images"):
    """``PIL.Image.resize((width, height), resample)`` of every sample, on the device, bit for bit: ``images`` is a uint8 tensor
    ``[B, Hs, Ws, 3]`` (or ``[B, Hs, Ws]`` for ``"nearest"``), or a list of ``B`` such samples of differing sizes; the result is
    uint8 ``[B, height, width(, 3)]``.  ``"antialias"`` is ``Image.ANTIALIAS`` / ``Image.LANCZOS`` as ``pil_loader`` applies it to
    frames (and ``data_preprocessing/prepare_cityscapes.py`` before its JPEG write), ``"nearest"`` is ``Image.NEAREST`` as it
    applies it to label maps.  One launch per pass covers all samples; a pass whose axis keeps its size is not run for that
    sample, and a sample that already has the size is copied (a tensor whose samples all have it is returned as it is).
    Reductions whose window exceeds RESIZE_MAX_TAPS taps (more than about 10.3 to 1) raise ValueError."""
    height, width = int(size[0]), int(size[1])
    if height < 1 or width < 1:
        raise ValueError("size must be (height, width), got %r" % (size,))
    if resample not in ("antialias", "nearest"):
        raise ValueError("resample must be 'antialias' or 'nearest', got %r" % (resample,))
    if torch.is_tensor(images) and images.dtype == torch.uint8 and images.dim() in (3, 4) and tuple(images.shape[1:3]) == (height, width) \
            and (images.dim() == 3 or images.shape[3] == 3):
        return images
    srcs = _samples(images, what)
    tables = _TABLES if tables is None else tables
    device, chan = srcs[0].device, (3 if srcs[0].dim() == 3 else 1)
    if resample == "antialias" and chan != 3:
        raise ValueError("%s: 'antialias' takes [Hs,Ws,3] samples" % what)
    out = torch.empty((len(srcs), height, width) + ((3,) if chan == 3 else ()), dtype=torch.uint8, device=device)
    todo = []
    for b, s in enumerate(srcs):
        if tuple(s.shape[:2]) == (height, width):
            out[b].copy_(s)
        else:
            todo.append((s, out[b]))
    if not todo:
        return out
    upload = lambda rows: torch.from_numpy(np.array(rows, dtype=np.int64).reshape(-1, 8)).to(device)
    if resample == "nearest":
        # the index tables stay referenced here until the launch has been issued, whatever cache ``tables`` keeps (or does not)
        idx = [(tables.nearest(s.shape[0], height, device), tables.nearest(s.shape[1], width, device)) for s, _ in todo]
        rows = [(s.data_ptr(), d.data_ptr(), ty.data_ptr(), tx.data_ptr(), s.shape[0], s.shape[1], 0, 0)
                for (s, d), (ty, tx) in zip(todo, idx)]
        H.batchprep_resize_nearest(upload(rows), height, width, chan)
        return out
    for s, _ in todo:
        for n_in, n_out in ((s.shape[1], width), (s.shape[0], height)):
            if n_in != n_out and lanczos_taps(n_in, n_out) > RESIZE_MAX_TAPS:
                raise ValueError("%s: unsupported reduction %d -> %d: its Lanczos window has %d taps, the kernels stage at most %d" % (
                    what, n_in, n_out, lanczos_taps(n_in, n_out), RESIZE_MAX_TAPS))
    # the uint8 image between the passes, for the samples that need both (16-byte aligned starts)
    both = [(s.shape[0] * width * 3 + 15) // 16 * 16 if (s.shape[0] != height and s.shape[1] != width) else 0 for s, _ in todo]
    mid = torch.empty((max(sum(both), 1),), dtype=torch.uint8, device=device)
    rows, cols, at = [], [], 0
    rows_arg, cols_arg = [0, 0, 0], [0, 0]               # (max rows, max taps, max span), (max taps, max span)
    for (s, d), nbytes in zip(todo, both):
        hs, ws = int(s.shape[0]), int(s.shape[1])
        between = mid.data_ptr() + at if nbytes else None
        at += nbytes
        if ws != width:
            bounds, weights, taps, span, _ = tables.lanczos(ws, width, device)
            rows.append((s.data_ptr(), between or d.data_ptr(), bounds.data_ptr(), weights.data_ptr(), hs, ws, taps, 0))
            rows_arg = [max(rows_arg[0], hs), max(rows_arg[1], taps), max(rows_arg[2], span)]
        if hs != height:
            bounds, weights, taps, _, span = tables.lanczos(hs, height, device)
            cols.append((between or s.data_ptr(), d.data_ptr(), bounds.data_ptr(), weights.data_ptr(), hs, width, taps, 0))
            cols_arg = [max(cols_arg[0], taps), max(cols_arg[1], span)]
    desc = upload(rows + cols)                           # one copy for both passes
    if rows:
        H.batchprep_resample_rows(desc[:len(rows)], rows_arg[0], width, rows_arg[1], rows_arg[2])
    if cols:
        H.batchprep_resample_cols(desc[len(rows):], 3 * width, height, cols_arg[0], cols_arg[1])
    return out


def pack_colors(label_colors):
    """[n, 3] RGB triples -> int32 [n] = r | g << 8 | b << 16, what segsde_batchprep_labels_rgb compares pixels with"""
    c = np.asarray(label_colors).astype(np.int64).reshape(-1, 3)
    if c.size == 0 or (c < 0).any() or (c > 255).any():
        raise ValueError("label_colors must be [n,3] values in 0..255")
    return (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)).astype(np.int32)


def _no_jitter(batch_size):
    return {"apply": np.zeros((batch_size,), dtype=np.bool_), "factors": np.tile(np.array([1.0, 1.0, 1.0, 0.0]), (batch_size, 1)),
            "order": np.tile(np.arange(4, dtype=np.uint8), (batch_size, 1))}


def jitter_tables(factors):
    """float64 [B,4] factors -> what the kernel reads: alpha float32 [B,3] (Pillow's blend takes a C float: the double is rounded
    once) and hue_shift int32 [B] = ``np.uint8(hue_factor * 255)``, truncated toward zero and wrapped into 0..255"""
    factors = np.asarray(factors, dtype=np.float64).reshape(-1, 4)
    return factors[:, :3].astype(np.float32), (np.trunc(factors[:, 3] * 255.0).astype(np.int64) & 255).astype(np.int32)


class DeviceBatchBuilder:
    """``builder(frames, lbl=..., ...)`` -> the dict a batch of ``SequenceSegmentationLoader.__getitem__`` collates to.

    ``random_horizontal_flip``: a positive probability configures the flip (the reference's
    ``augmentations["random_horizontal_flip"]``); 0.0 means the key is absent, and no flip coin is drawn.

    ``frames[f]`` is a uint8 tensor ``[B, Hs, Ws, 3]`` or a list of ``B`` tensors ``[Hs_b, Ws_b, 3]``: whatever is not ``height x
    width`` is resized first as ``pil_loader`` resizes it (``pil_resize``), then flipped, cropped and so on; frames that have the
    working size take the path they always took, with no extra launch.  ``lbl`` likewise (``[B, Hl, Wl]`` or a list; nearest, the
    reference's ``downsample_gt``), and with ``label_colors`` (``[n, 3]`` RGB triples, Mapillary's ``config.json`` colours) it is a
    colour-coded map ``[.., 3]`` encoded as ``MapillaryVistasLoader.encode_segmap`` encodes it: the last matching colour's index, 0
    for no match, ``label_ignore_id`` (default: the last entry, Mapillary's "unlabeled") -> ``ignore_index``.  ``pseudo_depth`` is
    never resized (the reference loads it with ``(-1, -1)``).  ``K`` / ``inv_K`` do not depend on the source size."""

    def __init__(self, height, width, crop_h=None, crop_w=None, num_scales=4, frame_idxs=(0, -1, 1),
                 intrinsics=(2262.52, 2265.3017905988554, 1096.98, 513.137), full_res_shape=(2048, 1024), label_lut=None,
                 n_classes=None, ignore_index=250, load_onehot=False, is_train=True, random_horizontal_flip=0.0, color_aug=False,
                 brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-0.1, 0.1), label_colors=None,
                 label_ignore_id=None):
        self.height, self.width = int(height), int(width)
        self.is_train = bool(is_train)
        if crop_h is None or crop_w is None or not self.is_train:          # sequence_segmentation_loader.py:81-86
            self.crop_h, self.crop_w = self.height, self.width
        else:
            self.crop_h, self.crop_w = int(crop_h), int(crop_w)
        if self.crop_h > self.height or self.crop_w > self.width:
            raise ValueError("crop %dx%d larger than the %dx%d frames" % (self.crop_h, self.crop_w, self.height, self.width))
        self.num_scales = int(num_scales)
        self.frame_idxs = tuple(frame_idxs)
        self.fx, self.fy, self.u0, self.v0 = intrinsics
        self.full_res_shape = tuple(full_res_shape)
        self.n_classes = n_classes
        self.ignore_index = int(ignore_index)
        self.load_onehot = bool(load_onehot)
        if self.load_onehot and not n_classes:
            raise ValueError("load_onehot needs n_classes")
        self.random_horizontal_flip = float(random_horizontal_flip or 0.0)
        self.color_aug = bool(color_aug)                                   # augmentations["color_aug"]; the ranges: :90-93
        self.jitter_ranges = tuple((float(lo), float(hi)) for lo, hi in (brightness, contrast, saturation, hue))
        self.label_lut = None if label_lut is None else np.asarray(label_lut).astype(np.int64).reshape(256)
        self.label_colors = None if label_colors is None else pack_colors(label_colors)
        if self.label_colors is not None and len(self.label_colors) > 1024:
            raise ValueError("at most 1024 label colours")
        self.label_ignore_id = (-1 if self.label_colors is None else len(self.label_colors) - 1) if label_ignore_id is None \
            else int(label_ignore_id)
        self.resize_tables = ResizeTables()
        self.level_sizes = [(self.crop_h, self.crop_w)]
        for _ in range(1, self.num_scales):
            h, w = self.level_sizes[-1]
            self.level_sizes.append((h // 2, w // 2))       # an odd level is rejected by the kernel when it is reached
        if min(self.level_sizes[-1]) < 1:
            raise ValueError("%d scales do not fit a %dx%d crop" % (self.num_scales, self.crop_h, self.crop_w))
        self._tables = [None] + [lanczos_half_table(*self.level_sizes[s]) for s in range(1, self.num_scales)]
        self._dev = {}

    # ---- host side -------------------------------------------------------------------------------------------------
    def draw(self, batch_size):
        """Crop offsets (int32 [B,2] = x1, y1) and flips (bool [B]) from Python's ``random`` in the reference's order per sample
        (sequence_segmentation_loader.py:210-212, 259-260): the colour-augmentation coin (drawn whenever ``is_train``; its
        result is unused here), the flip coin if a flip is configured, ``randint`` for x1, then for y1.  With ``is_train=False``
        no coin is drawn and both ``randint`` calls are ``randint(0, 0)``, which still advance the generator as in the reference."""
        if self.color_aug:
            raise ValueError("a color_aug builder draws the jitter between the samples' crops: use draw_with_jitter()")
        return self.draw_with_jitter(batch_size)[:2]

    def draw_with_jitter(self, batch_size):
        """``draw`` plus the colour jitter: (crops, flips, jitter).  Per sample the reference draws the coin, the flip coin if a
        flip is configured, x1, y1 and then -- only when the builder has ``color_aug`` and the coin was > 0.5 (:210, :297-299) --
        what torchvision 0.7.0's ``ColorJitter.get_params`` draws: ``random.uniform`` for brightness, contrast, saturation and hue
        in that order, then one ``random.shuffle`` of the four operations.  ``jitter``: ``apply`` bool [B], ``factors`` float64
        [B,4] (1, 1, 1, 0 where not applied) and ``order`` uint8 [B,4], the operation ids (0 brightness, 1 contrast, 2
        saturation, 3 hue) in the order they run."""
        crops = np.zeros((batch_size, 2), dtype=np.int32)
        flips = np.zeros((batch_size,), dtype=np.bool_)
        jitter = _no_jitter(batch_size)
        for b in range(batch_size):
            coin = random.random() if self.is_train else 0.0
            if self.is_train and self.random_horizontal_flip > 0.0:
                flips[b] = random.random() < self.random_horizontal_flip
            crops[b, 0] = random.randint(0, self.width - self.crop_w)
            crops[b, 1] = random.randint(0, self.height - self.crop_h)
            if self.is_train and coin > 0.5 and self.color_aug:
                jitter["apply"][b] = True
                jitter["factors"][b] = [random.uniform(lo, hi) for lo, hi in self.jitter_ranges]
                ops = [0, 1, 2, 3]
                random.shuffle(ops)
                jitter["order"][b] = ops
        return crops, flips, jitter

    def get_K(self, u_offset, v_offset, do_flip):
        """the reference's get_K (:332-342), including its flip of v0"""
        u0, v0 = self.u0, self.v0
        if do_flip:
            u0 = self.full_res_shape[0] - u0
            v0 = self.full_res_shape[1] - v0
        return np.array([[self.fx, 0, u0 - u_offset, 0],
                         [0, self.fy, v0 - v_offset, 0],
                         [0, 0, 1, 0],
                         [0, 0, 0, 1]], dtype=np.float32)

    def intrinsics(self, crops, flips):
        """float32 [2, num_scales, B, 4, 4]: K and inv_K of every scale by the reference's numpy expressions (:277-286)"""
        B = len(crops)
        out = np.empty((2, self.num_scales, B, 4, 4), dtype=np.float32)
        for b in range(B):
            for scale in range(self.num_scales):
                K = self.get_K(int(crops[b][0]), int(crops[b][1]), bool(flips[b]))
                K[0, :] /= (2 ** scale)
                K[1, :] /= (2 ** scale)
                out[0, scale, b] = K
                out[1, scale, b] = np.linalg.pinv(K)
        return out

    # ---- device side -----------------------------------------------------------------------------------------------
    def _cached(self, key, device, make):
        k = (key, str(device))
        if k not in self._dev:
            self._dev[k] = make().to(device)
        return self._dev[k]

    def working_size_frames(self, frames):
        """{frame id: uint8 [B, height, width, 3]}: frames of another size (a tensor, or a list of per-sample tensors) resized as
        pil_loader resizes them, all frames' samples in one launch per pass; tensors that have the size are passed through"""
        out, todo = {}, []
        B = None
        for f in self.frame_idxs:
            v = frames[f]
            n = v.shape[0] if torch.is_tensor(v) else len(v)
            B = n if B is None else B
            if n != B or n < 1:
                raise ValueError("frame %r: %d samples for a batch of %d" % (f, n, B))
            if torch.is_tensor(v) and (v.dim() != 4 or v.shape[3] != 3 or v.dtype != torch.uint8):
                raise ValueError("frame %r: expected uint8 [%d,Hs,Ws,3] or a list of [Hs,Ws,3], got %s %s" % (
                    f, B, v.dtype, tuple(v.shape)))
            if torch.is_tensor(v) and tuple(v.shape[1:3]) == (self.height, self.width):
                out[f] = v
            else:
                todo.append((f, _samples(v, "frame %r" % f)))
        if todo:
            for f, items in todo:
                if items[0].dim() != 3:
                    raise ValueError("frame %r: samples must be [Hs,Ws,3]" % f)
            resized = pil_resize([t for _, items in todo for t in items], (self.height, self.width), "antialias", self.resize_tables,
                                 "frames")
            for i, (f, _) in enumerate(todo):
                out[f] = resized[i * B:(i + 1) * B]
        return out

    def colors(self, frames, crop_d, flip_d, inputs, jitter=None):
        """the colour pyramid of every frame: one crop launch per frame, one launch per level for all frames together; with a
        ``jitter`` that applies to some sample, two more launches for the color_aug images of all frames"""
        first = frames[self.frame_idxs[0]]
        B, device = first.shape[0], first.device
        F = len(self.frame_idxs)
        u8 = torch.empty((F, B, 3, self.crop_h, self.crop_w), dtype=torch.uint8, device=device)
        color = torch.empty((F, B, 3, self.crop_h, self.crop_w), dtype=torch.float32, device=device)
        for i, f in enumerate(self.frame_idxs):
            H.batchprep_crop(frames[f], crop_d, flip_d, self.crop_h, self.crop_w, u8_out=u8[i], f32_out=color[i])
            inputs[("color", f, 0)] = inputs[("color_aug", f, 0)] = color[i]          # one tensor under both keys
        if jitter is not None and jitter["apply"].any():
            alpha, shift = jitter_tables(jitter["factors"])
            aug = H.batchprep_color_jitter(u8, jitter["apply"], alpha, shift, jitter["order"])
            for i, f in enumerate(self.frame_idxs):
                inputs[("color_aug", f, 0)] = aug[i]
        for s in range(1, self.num_scales):
            table = self._cached(("lanczos", s), device, lambda: torch.from_numpy(self._tables[s]))
            u8, color = H.batchprep_pyramid_level(u8, table)
            for i, f in enumerate(self.frame_idxs):
                inputs[("color", f, s)] = color[i]
        return inputs

    def __call__(self, frames, lbl=None, pseudo_depth=None, is_labeled=None, idx=None, crops=None, flips=None, jitter=None):
        """``crops`` / ``flips`` / ``jitter``: what ``draw_with_jitter`` returns; drawn here when neither crops nor flips are given
        (``jitter`` too on a ``color_aug`` builder, unless one is passed).  Crops or flips without a ``jitter`` augment nothing."""
        frames = self.working_size_frames(frames)
        first = frames[self.frame_idxs[0]]
        B, device = first.shape[0], first.device
        if crops is None and flips is None:        # also on the validation path: the reference's random_crop draws randint(0, 0) there
            crops, flips, drawn = self.draw_with_jitter(B)
            jitter = drawn if jitter is None and self.color_aug else jitter
        if jitter is not None:
            if not self.color_aug:
                raise ValueError("jitter passed to a builder without color_aug")
            jitter = {"apply": np.asarray(jitter["apply"]).astype(np.bool_).reshape(B),
                      "factors": np.asarray(jitter["factors"], dtype=np.float64).reshape(B, 4), "order": np.asarray(jitter["order"]).reshape(B, 4)}
            if jitter["apply"].any() and not self.is_train:
                raise ValueError("the validation path never augments (is_train=False)")
        crops = np.zeros((B, 2), np.int32) if crops is None else np.asarray(torch.as_tensor(crops).cpu(), dtype=np.int32).reshape(B, 2)
        flips = np.zeros((B,), np.bool_) if flips is None else np.asarray(torch.as_tensor(flips).cpu()).astype(np.bool_).reshape(B)
        if (crops < 0).any() or (crops[:, 0] > self.width - self.crop_w).any() or (crops[:, 1] > self.height - self.crop_h).any():
            raise ValueError("crop offsets outside the frame")
        cropped = (self.crop_h, self.crop_w) != (self.height, self.width)
        crop_d = torch.from_numpy(crops).to(device, non_blocking=True) if cropped else None
        flip_d = torch.from_numpy(flips.astype(np.uint8)).to(device, non_blocking=True) if flips.any() else None

        inputs = {}
        self.colors(frames, crop_d, flip_d, inputs, jitter)

        kk = torch.from_numpy(self.intrinsics(crops, flips)).to(device, non_blocking=True)     # one copy for all scales
        for s in range(self.num_scales):
            inputs[("K", s)], inputs[("inv_K", s)] = kk[0, s], kk[1, s]

        labeled_d = None
        if is_labeled is not None:
            labeled_d = torch.as_tensor(is_labeled).to(device=device, dtype=torch.uint8)
            inputs["is_labeled"] = labeled_d.bool()
        if lbl is not None:
            lbl = pil_resize(lbl, (self.height, self.width), "nearest", self.resize_tables, "lbl")
            if lbl.shape[0] != B:
                raise ValueError("lbl: %d samples for a batch of %d" % (lbl.shape[0], B))
            if lbl.dim() == 4:
                if self.label_colors is None:
                    raise ValueError("colour-coded labels need label_colors")
                colors = self._cached("colors", device, lambda: torch.from_numpy(self.label_colors))
                inputs["lbl"], onehot = H.batchprep_labels_rgb(lbl, crop_d, flip_d, self.crop_h, self.crop_w, colors, self.label_ignore_id,
                                                               labeled_d, self.ignore_index, self.n_classes or 0, self.load_onehot)
            else:
                if self.label_lut is None:
                    raise ValueError("labels need label_lut (encode_segmap(arange(256)))")
                lut = self._cached("lut", device, lambda: torch.from_numpy(self.label_lut))
                inputs["lbl"], onehot = H.batchprep_labels(lbl, crop_d, flip_d, self.crop_h, self.crop_w, lut, labeled_d,
                                                           self.ignore_index, self.n_classes or 0, self.load_onehot)
            if self.load_onehot:
                inputs["onehot_lbl"] = onehot
        if pseudo_depth is not None:
            inputs["pseudo_depth"] = H.batchprep_plane(pseudo_depth, crop_d, flip_d, self.crop_h, self.crop_w)
        if idx is not None:
            inputs["idx"] = torch.as_tensor(idx).to(device)
        return inputs
