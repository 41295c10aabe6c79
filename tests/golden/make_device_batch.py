#!/usr/bin/env python
"""tests/golden/device_batch.npz: inputs and expected outputs of the device batch builder (loader/device_batch.py), produced by
the REFERENCE's own loader code (imported from /root/reference; build container only) on seeded in-memory images.

How the reference is reached (the stand-in recipe of SURVEY.md 8c):
  * ``CityscapesLoader.__init__`` / ``__getitem__`` / ``get_color`` / ``random_crop`` / ``preprocess`` / ``get_K`` /
    ``Cityscapes.encode_segmap`` run unmodified.  A subclass defined here replaces only what touches the file system
    (``_prepare_filenames``, ``_filter_available_files``, the three path methods), and ``pil_loader`` in the loader module is
    pointed at the in-memory PIL images.
  * torchvision is absent: ``transforms.Resize(size, interpolation)`` -> ``PIL.Image.resize(size[::-1], interpolation)`` and
    ``transforms.ToTensor`` -> uint8 CHW / 255 in float32 (what torchvision does for 8-bit PIL images).  ``Image.ANTIALIAS`` no
    longer exists in this Pillow; it was the same filter as ``Image.LANCZOS`` and is aliased in this process only.
  * the crops and flips of cases A-C are forced by scripting ``random.random`` / ``random.randint`` while ``__getitem__`` runs; the
    ``draw_*`` arrays record what the untouched ``random`` module hands the reference after ``random.seed(7)``.
  * ``torch.utils.data``'s default collation is a stack per key; it is restated here as ``torch.stack``.
  * one-hot: the reference's ``one_hot`` call raises on label 255 (which ``encode_segmap`` leaves untouched), so the one-hot run
    uses the label map ``a_lbl_oh_u8`` without that id; the table / crop / flip run uses the map with every id 0..33 and 255.
The int64 label maps and one-hot planes are stored as uint8 (every value fits; the dtype is asserted here and the tests widen them).
The colour pyramids are stored as the uint8 images behind them; this script asserts that the reference's float tensors are exactly
uint8 / 255 of them, and that tests/device_batch_cases.pillow_half reproduces Pillow on every level.

    python tests/golden/make_device_batch.py            # write the fixture
    python tests/golden/make_device_batch.py --check    # regenerate and compare with the committed file, bit for bit
"""
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "device_batch.npz")
sys.dont_write_bytecode = True
FRAMES = (0, -1, 1)


def _install_standins():
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS

    class Resize:
        def __init__(self, size, interpolation=Image.BILINEAR):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            return img.resize(tuple(self.size)[::-1], self.interpolation)

    class ToTensor:
        def __call__(self, pic):
            a = np.array(pic, dtype=np.uint8)
            if a.ndim == 2:
                a = a[:, :, None]
            return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)

    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    tr.Resize, tr.ToTensor = Resize, ToTensor
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    ut = types.ModuleType("utils")
    ut.__path__ = []
    uu = types.ModuleType("utils.utils")
    uu.np_local_seed = uu.recursive_glob = None          # imported by name, never called here
    ut.utils = uu
    sys.modules["utils"], sys.modules["utils.utils"] = ut, uu
    pkg = types.ModuleType("loader")
    pkg.__path__ = [os.path.join(REF, "loader")]
    sys.modules["loader"] = pkg
    sys.path.insert(0, REF)


def _reference():
    _install_standins()
    import loader.cityscapes_loader as CL
    import loader.sequence_segmentation_loader as SSL
    assert os.path.realpath(CL.__file__).startswith(REF) and os.path.realpath(SSL.__file__).startswith(REF)

    class InMemory(CL.CityscapesLoader):
        """images: {frame id: uint8 [N,H,W,3]}, labels / depths: uint8 [N,H,W] or None"""

        def __init__(self, images, labels, depths, labeled, **kw):
            self._images, self._labels, self._depths = images, labels, depths
            self.flips_seen = []
            super().__init__(root="mem", load_labels=labels is not None, generated_depth_dir="depth" if depths is not None else None,
                             only_sequences_with_segmentation=True, **kw)
            for f, lab in zip(self.files, labeled):
                f["labeled"] = bool(lab)

        def _prepare_filenames(self):
            self.files = ["img/%d/0.jpg" % i for i in range(len(self._images[0]))]

        def _filter_available_files(self):
            pass

        def get_image_path(self, index, offset=0):
            return "img/%d/%d.jpg" % (index, offset)

        def get_segmentation_path(self, index):
            return "lbl/%d/0.png" % index

        def get_color(self, index, offset, do_flip):
            self.flips_seen.append(bool(do_flip))
            return super().get_color(index, offset, do_flip)

        def load(self, path, std_width, std_height, is_segmentation=False, lru_cache=False):
            kind, index, name = path.split(os.sep)[-3:]
            index = int(index)
            if kind == "lbl":
                return Image.fromarray(self._labels[index], "L")
            if name.endswith(".png"):
                return Image.fromarray(self._depths[index], "L")
            return Image.fromarray(self._images[int(name[:-4])][index], "RGB")

    def make(*a, **kw):
        ds = InMemory(*a, **kw)
        SSL.pil_loader = ds.load
        return ds
    return make, CL


class Scripted:
    """random.random / random.randint answer from a script while a reference method runs"""

    def __init__(self, randoms, randints):
        self.randoms, self.randints = list(randoms), list(randints)

    def __enter__(self):
        self.keep = (random.random, random.randint)
        random.random = lambda: self.randoms.pop(0)

        def randint(a, b):
            v = self.randints.pop(0)
            assert a <= v <= b
            return v
        random.randint = randint

    def __exit__(self, *exc):
        random.random, random.randint = self.keep
        assert not self.randoms and not self.randints, "the reference drew less than scripted"


def collate(samples):
    out = {}
    for k in samples[0]:
        v = [s[k] for s in samples]
        if torch.is_tensor(v[0]):
            out[k] = torch.stack(v)
        elif isinstance(v[0], (bool, int)):
            out[k] = torch.tensor(v)
    return out


def smooth(rng, n, h, w, c):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((n, h, w, c), dtype=np.uint8)
    for i in range(n):
        for ch in range(c):
            a, b, p, q = rng.uniform(0.05, 0.4, 4)
            out[i, :, :, ch] = np.clip(127.5 + 80 * np.sin(a * xx + p * 9) + 60 * np.cos(b * yy + q * 9), 0, 255).astype(np.uint8)
    return out


def half_noise(rng, n, h, w):
    """left half noise, right half smooth"""
    img = smooth(rng, n, h, w, 3)
    img[:, :, : w // 2] = rng.randint(0, 256, (n, h, w // 2, 3), dtype=np.uint8)
    return img


def store_colors(d, prefix, batch, scales, pillow_half, unit):
    for f in FRAMES:
        prev = None
        for s in range(scales):
            t = batch[("color", f, s)]
            u8 = torch.round(t * 255).to(torch.uint8).numpy()
            assert torch.equal(unit(u8), t), "ToTensor is not uint8 / 255 here"
            if prev is not None:
                assert np.array_equal(pillow_half(prev), u8), "the numpy restatement differs from Pillow"
            d["%s_color_%d_%d" % (prefix, f, s)] = u8
            prev = u8
        assert torch.equal(batch[("color_aug", f, 0)], batch[("color", f, 0)])
    for s in range(scales):
        d["%s_K_%d" % (prefix, s)] = batch[("K", s)].numpy()
        d["%s_inv_K_%d" % (prefix, s)] = batch[("inv_K", s)].numpy()


def generate():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import device_batch_cases as DC
    make, CL = _reference()
    d = {}
    d["lut"] = CL.Cityscapes.encode_segmap(np.arange(256, dtype=np.uint8)).astype(np.int64)

    # ---- case A -------------------------------------------------------------------------------------------------------
    c = DC.CASE_A
    rng = np.random.RandomState(1)
    n, h, w = len(c["crops"]), c["height"], c["width"]
    images = {f: half_noise(rng, n, h, w) for f in FRAMES}
    ids = np.array(list(range(34)) + [255], dtype=np.uint8)
    lbl = ids[(np.arange(h)[:, None] * 3 + np.arange(w)[None, :] + np.arange(n)[:, None, None] * 5) % len(ids)]   # every id in every crop
    lbl_oh = np.where(lbl == 255, 7, lbl).astype(np.uint8)
    pd = rng.randint(0, 256, (n, h, w), dtype=np.uint8)
    labeled = [True, False, True]
    script = lambda: Scripted([v for fl in c["flips"] for v in (0.0, 0.1 if fl else 0.9)], [v for xy in c["crops"] for v in xy])
    kw = dict(split="train", img_size=(h, w), crop_h=c["crop_h"], crop_w=c["crop_w"], augmentations={"random_horizontal_flip": 0.5},
              frame_idxs=list(FRAMES), num_scales=4)
    ds = make(images, lbl, pd, labeled, **kw)
    with script():
        batch = collate([ds[i] for i in range(n)])
    assert ds.flips_seen[::3] == c["flips"]
    ds = make(images, lbl_oh, pd, labeled, load_onehot=True, **kw)
    with script():
        batch_oh = collate([ds[i] for i in range(n)])
    for f in FRAMES:
        d["a_frame_%d" % f] = images[f]
    d["a_lbl_u8"], d["a_lbl_oh_u8"], d["a_pd_u8"] = lbl, lbl_oh, pd
    d["a_is_labeled"], d["a_idx"] = batch["is_labeled"].numpy(), batch["idx"].numpy()
    assert batch["lbl"].dtype == torch.int64 and batch_oh["onehot_lbl"].dtype == torch.int64 and batch_oh["lbl"].dtype == torch.int64
    narrow = lambda t: (lambda a: (a.astype(np.uint8), np.testing.assert_array_equal(a.astype(np.uint8).astype(np.int64), a))[0])(np.asarray(t))
    d["a_pseudo_depth"] = batch["pseudo_depth"].numpy()
    d["a_lbl"], d["a_lbl_oh"], d["a_onehot_lbl"] = narrow(batch["lbl"]), narrow(batch_oh["lbl"]), narrow(batch_oh["onehot_lbl"])    # int64 in the reference
    d["a_lbl_encoded_full"] = np.stack([CL.Cityscapes.encode_segmap(lbl[i].copy()) for i in range(n)])
    store_colors(d, "a", batch, 4, DC.pillow_half, DC.unit)

    # ---- draw order: the untouched random module, seed 7 ---------------------------------------------------------------
    for tag, aug in (("draw", {"random_horizontal_flip": 0.5}), ("draw_noflip", {})):
        nd = 6
        ds = make({f: np.zeros((nd, h, w, 3), np.uint8) for f in FRAMES}, None, None, [True] * nd, **dict(kw, augmentations=aug))
        seen = []
        keep = random.randint
        random.randint = lambda a, b: (seen.append(keep(a, b)), seen[-1])[1]
        try:
            random.seed(7)
            for i in range(nd):
                ds[i]
            nxt = random.random()
        finally:
            random.randint = keep
        d[tag + "_crops"] = np.array(seen, dtype=np.int32).reshape(nd, 2)
        if tag == "draw":
            d["draw_flips"], d["draw_next_random"] = np.array(ds.flips_seen[::3], dtype=np.bool_), np.float64(nxt)

    # ---- case B: validation path (no crop although one is configured, no flip) ------------------------------------------
    c = DC.CASE_B
    rng = np.random.RandomState(2)
    images = {f: half_noise(rng, 1, c["height"], c["width"]) for f in FRAMES}
    ds = make(images, None, None, [True], split="val", img_size=(c["height"], c["width"]), crop_h=32, crop_w=64,
              augmentations={"random_horizontal_flip": 0.5}, frame_idxs=list(FRAMES), num_scales=4)
    batch = collate([ds[0]])
    assert not any(ds.flips_seen)
    for f in FRAMES:
        d["b_frame_%d" % f] = images[f]
    store_colors(d, "b", batch, 4, DC.pillow_half, DC.unit)

    # ---- case C: checkerboards of 0 / 255 (squares of 1, 2, 3, 4 and 8 pixels), noise, a smooth image ------------------
    c = DC.CASE_C
    rng = np.random.RandomState(3)
    h, w = c["height"], c["width"]
    yy, xx = np.mgrid[0:h, 0:w]
    board = lambda q: (((yy // q + xx // q) & 1) * 255).astype(np.uint8)
    checker = np.stack([np.stack([board(q0), board(q1), board(q2)], -1) for q0, q1, q2 in ((4, 8, 1), (2, 3, 4))])
    images = {0: np.concatenate([checker, rng.randint(0, 256, (1, h, w, 3), dtype=np.uint8), smooth(rng, 1, h, w, 3)]),
              -1: np.concatenate([checker[::-1], smooth(rng, 2, h, w, 3)]), 1: rng.randint(0, 256, (4, h, w, 3), dtype=np.uint8)}
    ds = make(images, None, None, [True] * 4, split="train", img_size=(h, w), augmentations={}, frame_idxs=list(FRAMES), num_scales=3)
    with Scripted([0.0] * 4, [0, 0] * 4):
        batch = collate([ds[i] for i in range(4)])
    for f in FRAMES:
        d["c_frame_%d" % f] = images[f]
    store_colors(d, "c", batch, 3, DC.pillow_half, DC.unit)
    return d


def main():
    d = generate()
    if "--check" in sys.argv[1:]:
        z = np.load(OUT, allow_pickle=False)
        bad = [k for k in sorted(set(d) | set(z.files))
               if k not in d or k not in z.files or d[k].dtype != z[k].dtype or d[k].shape != z[k].shape or d[k].tobytes() != z[k].tobytes()]
        print("make_device_batch --check:", "OK" if not bad else "arrays differ from the committed fixture: %s" % bad)
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, "%.1f KB, %d arrays" % (os.path.getsize(OUT) / 1024, len(d)))


if __name__ == "__main__":
    main()
