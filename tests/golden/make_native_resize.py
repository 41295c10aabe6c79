#!/usr/bin/env python
"""tests/golden/native_resize.npz: inputs and expected outputs of the native-resolution front end of the device batch builder
(loader/device_batch.py ``pil_resize`` / ``DeviceBatchBuilder``), produced by the REFERENCE's own loader code (imported from
/root/reference; build container only) and Pillow 12.2.0 -- the arithmetic of the fixture is that Pillow's.

Seeded images are written as PNG (lossless) into a temporary directory.  Then
  * the reference's ``pil_loader`` (loader/loader_utils.py: ``_load`` opens, converts and resizes with ``Image.ANTIALIAS`` /
    ``Image.NEAREST``) runs on those paths, unmodified, for the stand-alone resize cases;
  * the reference's ``__getitem__`` runs through the stand-in recipe of make_device_batch.py (the torchvision / utils stand-ins,
    scripted ``random``, ``torch.stack`` collation): a ``CityscapesLoader`` subclass that replaces only the file list and the
    three path methods -- here they name the PNG files, so ``get_color`` / ``get_segmentation`` call the reference's
    ``pil_loader`` itself -- and a ``MapillaryVistasLoader`` subclass that replaces only ``_prepare_filenames`` (its
    ``config.json`` is written to the temporary root), for the colour-coded label maps.
This script asserts that the reference's float tensors are exactly uint8 / 255 of the stored images, and that the numpy
restatements of tests/native_resize_cases.py (``pillow_resize``, ``pillow_nearest``) reproduce Pillow on every stored case.

    python tests/golden/make_native_resize.py            # write the fixture
    python tests/golden/make_native_resize.py --check    # regenerate and compare with the committed file, bit for bit
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "native_resize.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_device_batch as MB      # noqa: E402  (the stand-in recipe: _install_standins, Scripted, collate, the image makers)

FRAMES = MB.FRAMES


def save(path, a):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(a, "L" if a.ndim == 2 else "RGB").save(path)
    return path


def patchwork(rng, n, h, w):
    """images that compress well and still meet every regime: a smooth image quantised to eight levels, noise in the top left
    ninth (two borders included), 0 / 255 pixels in the bottom right ninth"""
    img = (MB.smooth(rng, n, h, w, 3) // 32 * 36).astype(np.uint8)
    img[:, : h // 3, : w // 3] = rng.randint(0, 256, (n, h // 3, w // 3, 3), dtype=np.uint8)
    img[:, h - h // 3:, w - w // 3:] = (rng.randint(0, 2, (n, h // 3, w // 3, 3)) * 255).astype(np.uint8)
    return img


def _reference(tmp):
    MB._install_standins()
    import loader.loader_utils as LU
    import loader.cityscapes_loader as CL
    import loader.mapillary_vistas_loader as MV
    import loader.sequence_segmentation_loader as SSL
    for m in (LU, CL, MV, SSL):
        assert os.path.realpath(m.__file__).startswith(MB.REF)
    SSL.pil_loader = LU.pil_loader          # the reference's own, whatever an earlier import of this process left there

    class OnDisk(CL.CityscapesLoader):
        """images: {frame id: list of uint8 [H,W,3]}, labels: list of uint8 [H,W] or None -- written as PNG under ``tag``"""

        def __init__(self, tag, images, labels, labeled, **kw):
            self._dir = os.path.join(tmp, tag)
            self._n = len(images[0])
            for f, items in images.items():
                for i, a in enumerate(items):
                    save(self.get_image_path(i, f), a)
            for i, a in enumerate(labels or []):
                save(self.get_segmentation_path(i), a)
            self.flips_seen = []
            super().__init__(root=self._dir, load_labels=labels is not None, generated_depth_dir=None,
                             only_sequences_with_segmentation=True, **kw)
            for f, lab in zip(self.files, labeled):
                f["labeled"] = bool(lab)

        def _prepare_filenames(self):
            self.files = ["img/%d/0.png" % i for i in range(self._n)]

        def _filter_available_files(self):
            pass

        def get_image_path(self, index, offset=0):
            return os.path.join(self._dir, "img", str(index), "%d.png" % offset)

        def get_segmentation_path(self, index):
            return os.path.join(self._dir, "lbl", str(index), "0.png")

        def get_color(self, index, offset, do_flip):
            self.flips_seen.append(bool(do_flip))
            return super().get_color(index, offset, do_flip)

    class Mapillary(MV.MapillaryVistasLoader):
        def _prepare_filenames(self):
            self.images_base = os.path.join(self.root, self.split, "images")
            self.annotations_base = os.path.join(self.root, self.split, "labels")
            self.files = sorted(os.path.join(self.images_base, n) for n in os.listdir(self.images_base))

    return OnDisk, Mapillary, CL, LU


def generate():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import native_resize_cases as NC
    DC = NC.DC
    with tempfile.TemporaryDirectory() as tmp:
        return _generate(tmp, NC, DC)


def _generate(tmp, NC, DC):
    OnDisk, Mapillary, CL, LU = _reference(tmp)
    d = {}
    d["lut"] = CL.Cityscapes.encode_segmap(np.arange(256, dtype=np.uint8)).astype(np.int64)
    counter = [0]

    def loaded(a, size, seg=False):
        """the reference's pil_loader on a PNG of ``a``; also: the restatement is Pillow"""
        counter[0] += 1
        path = save(os.path.join(tmp, "single", "%d.png" % counter[0]), a)
        out = np.array(LU.pil_loader(path, size[1], size[0], is_segmentation=seg))
        assert out.dtype == np.uint8 and out.shape[:2] == tuple(size)
        again = NC.pillow_nearest(a, size) if seg else NC.pillow_resize(a, size)
        assert np.array_equal(again, out), "the numpy restatement differs from Pillow at %s -> %s" % (a.shape, size)
        return out

    narrow = lambda t: (lambda a: (a.astype(np.uint8), np.testing.assert_array_equal(a.astype(np.uint8).astype(np.int64), a))[0])(np.asarray(t))

    # ---- border case: native 97x131 frames and label maps through __getitem__ -------------------------------------------
    c = NC.CASE_BORDER
    rng = np.random.RandomState(21)
    n, (hs, ws), size = len(c["crops"]), c["src"], (c["height"], c["width"])
    images = {f: patchwork(rng, n, hs, ws) for f in FRAMES}
    ids = np.array(list(range(34)) + [255], dtype=np.uint8)
    lbl = ids[(np.arange(hs)[:, None] * 3 + np.arange(ws)[None, :] + np.arange(n)[:, None, None] * 5) % len(ids)]
    lbl_oh = np.where(lbl == 255, 7, lbl).astype(np.uint8)
    labeled = [True, False, True]
    script = lambda: MB.Scripted([v for fl in c["flips"] for v in (0.0, 0.1 if fl else 0.9)], [v for xy in c["crops"] for v in xy])
    kw = dict(split="train", img_size=size, crop_h=c["crop_h"], crop_w=c["crop_w"], augmentations={"random_horizontal_flip": 0.5},
              frame_idxs=list(FRAMES), num_scales=4)
    ds = OnDisk("na", {f: list(v) for f, v in images.items()}, list(lbl), labeled, **kw)
    with script():
        batch = MB.collate([ds[i] for i in range(n)])
    assert ds.flips_seen[::3] == c["flips"]
    ds = OnDisk("na_oh", {f: list(v) for f, v in images.items()}, list(lbl_oh), labeled, load_onehot=True, **kw)
    with script():
        batch_oh = MB.collate([ds[i] for i in range(n)])
    for f in FRAMES:
        d["na_frame_%d" % f] = images[f]
    d["na_lbl_u8"], d["na_lbl_oh_u8"] = lbl, lbl_oh
    d["na_is_labeled"] = batch["is_labeled"].numpy()
    assert batch["lbl"].dtype == torch.int64 and batch_oh["onehot_lbl"].dtype == torch.int64
    d["na_lbl"], d["na_lbl_oh"], d["na_onehot_lbl"] = narrow(batch["lbl"]), narrow(batch_oh["lbl"]), narrow(batch_oh["onehot_lbl"])
    MB.store_colors(d, "na", batch, 4, DC.pillow_half, DC.unit)
    d["na_resized_0"] = np.stack([loaded(a, size) for a in images[0]])
    d["na_lbl_resized"] = np.stack([loaded(a, size, seg=True) for a in lbl])
    # __getitem__'s scale 0 is the crop of what pil_loader returned
    for i, ((x1, y1), fl) in enumerate(zip(c["crops"], c["flips"])):
        r = d["na_resized_0"][i][:, ::-1] if fl else d["na_resized_0"][i]
        assert np.array_equal(np.moveaxis(r[y1:y1 + c["crop_h"], x1:x1 + c["crop_w"]], -1, 0), d["na_color_0_0"][i])

    # ---- exact 2:1, the validation path of a single-frame, single-scale loader -----------------------------------------
    rng = np.random.RandomState(22)
    for tag in ("a", "b"):
        (hs, ws), size = NC.CASE_HALF[tag]
        src = patchwork(rng, 1, hs, ws)[0]
        ds = OnDisk("half_" + tag, {0: [src]}, None, [True], split="val", img_size=size, crop_h=32, crop_w=64,
                    augmentations={"random_horizontal_flip": 0.5}, frame_idxs=[0], num_scales=1)
        batch = MB.collate([ds[0]])
        t = batch[("color", 0, 0)]
        u8 = torch.round(t * 255).to(torch.uint8).numpy()
        assert torch.equal(DC.unit(u8), t), "ToTensor is not uint8 / 255 here"
        d["h_src_" + tag], d["h_out_" + tag] = src, loaded(src, size)
        d["h_K_" + tag], d["h_inv_K_" + tag] = batch[("K", 0)].numpy(), batch[("inv_K", 0)].numpy()
        assert np.array_equal(np.moveaxis(u8[0], 0, -1), d["h_out_" + tag])

    # ---- stand-alone resizes through pil_loader --------------------------------------------------------------------------
    rng = np.random.RandomState(23)
    (hs, ws), size = NC.CASE_UP
    d["up_src"] = rng.randint(0, 256, (hs, ws, 3), dtype=np.uint8)
    d["up_out"] = loaded(d["up_src"], size)
    board = lambda h, w, q: ((((np.arange(h)[:, None] // q) + (np.arange(w)[None, :] // q)) & 1) * 255).astype(np.uint8)
    for tag in ("w", "h"):
        (hs, ws), size = NC.CASE_AXIS[tag]
        d["ax_src_" + tag] = np.stack([board(hs, ws, 1), board(hs, ws, 3), board(hs, ws, 2)], -1)
        d["ax_out_" + tag] = loaded(d["ax_src_" + tag], size)
    for tag in ("a", "b", "lim"):
        (hs, ws), size = NC.CASE_TAPS[tag]
        src = patchwork(rng, 1, hs, ws)[0]
        d["mt_src_" + tag], d["mt_out_" + tag] = src, loaded(src, size)
    c = NC.CASE_BORDER
    (hs, ws), size = c["src"], (c["height"], c["width"])
    d["sat_src"] = np.stack([np.stack([board(hs, ws, 1), board(hs, ws, 2), board(hs, ws, 3)], -1),
                             (rng.randint(0, 2, (hs, ws, 3)) * 255).astype(np.uint8)])
    d["sat_out"] = np.stack([loaded(a, size) for a in d["sat_src"]])
    d["ps_src_1"], d["ps_src_2"] = patchwork(rng, 1, 60, 100)[0], patchwork(rng, 1, 48, 80)[0]
    d["ps_out"] = np.stack([loaded(a, size) for a in (d["na_frame_0"][0], d["ps_src_1"], d["ps_src_2"])])

    # ---- labels at an enlargement: 20x30 -> 33x47 through __getitem__ (one frame, one scale, one-hot) ------------------
    c = NC.CASE_LABELS_UP
    rng = np.random.RandomState(24)
    n, (hs, ws), size = len(c["crops"]), c["src"], (c["height"], c["width"])
    images = {0: rng.randint(0, 256, (n, hs, ws, 3), dtype=np.uint8)}
    lbl = ids[(np.arange(hs)[:, None] * 7 + np.arange(ws)[None, :] + np.arange(n)[:, None, None] * 5) % len(ids)]
    lbl_oh = np.where(lbl == 255, 7, lbl).astype(np.uint8)
    ds = OnDisk("lb", {0: list(images[0])}, list(lbl_oh), [True] * n, split="train", img_size=size, crop_h=c["crop_h"], crop_w=c["crop_w"],
                augmentations={"random_horizontal_flip": 0.5}, frame_idxs=[0], num_scales=1, load_onehot=True)
    with MB.Scripted([v for fl in c["flips"] for v in (0.0, 0.1 if fl else 0.9)], [v for xy in c["crops"] for v in xy]):
        batch = MB.collate([ds[i] for i in range(n)])
    assert ds.flips_seen == c["flips"]
    t = batch[("color", 0, 0)]
    u8 = torch.round(t * 255).to(torch.uint8).numpy()
    assert torch.equal(DC.unit(u8), t)
    d["lb_frame_0"], d["lb_lbl_u8"], d["lb_lbl_oh_u8"], d["lb_color_0_0"] = images[0], lbl, lbl_oh, u8
    d["lb_lbl"], d["lb_onehot_lbl"] = narrow(batch["lbl"]), narrow(batch["onehot_lbl"])
    d["lb_K_0"], d["lb_inv_K_0"] = batch[("K", 0)].numpy(), batch[("inv_K", 0)].numpy()
    d["lb_lbl_resized"] = np.stack([loaded(a, size, seg=True) for a in lbl])

    # ---- colour-coded label maps: MapillaryVistasLoader ------------------------------------------------------------------
    c = NC.CASE_COLORS
    rng = np.random.RandomState(25)
    n, (hs, ws), size = len(c["crops"]), c["src"], (c["height"], c["width"])
    colors = rng.randint(0, 256, (66, 3)).astype(np.uint8)
    colors[40], colors[65] = colors[3], colors[17]                  # two duplicates: ids 3 and 17 never come out, 40 and 65 do
    assert len(set(map(tuple, colors.tolist()))) == 64
    root = os.path.join(tmp, "mapillary")
    os.makedirs(root)
    with open(os.path.join(root, "config.json"), "w") as fh:
        json.dump({"labels": [{"readable": "class %d" % i, "color": [int(v) for v in col]} for i, col in enumerate(colors)]}, fh)
    pick = (np.arange(hs)[:, None] * 5 + np.arange(ws)[None, :] + np.arange(n)[:, None, None] * 11) % 68       # 66, 67: no colour
    table = np.concatenate([colors, np.array([[1, 2, 3], [254, 0, 77]], dtype=np.uint8)])
    assert not any(tuple(t) in set(map(tuple, colors.tolist())) for t in table[66:].tolist())
    maps = table[pick]
    frames = patchwork(rng, n, hs, ws)
    for i in range(n):
        save(os.path.join(root, "train", "images", "%02d.png" % i), frames[i])
        save(os.path.join(root, "train", "labels", "%02d.png" % i), maps[i])
    labeled = [True, True, False]
    ds = Mapillary(root=root, split="train", img_size=size, crop_h=c["crop_h"], crop_w=c["crop_w"],
                   augmentations={"random_horizontal_flip": 0.5}, load_sequence=False)
    assert ds.n_classes == 65 and ds.ignore_index == 250 and len(ds.class_colors) == 66
    for f, lab in zip(ds.files, labeled):
        f["labeled"] = lab
    with MB.Scripted([v for fl in c["flips"] for v in (0.0, 0.1 if fl else 0.9)], [v for xy in c["crops"] for v in xy]):
        batch = MB.collate([ds[i] for i in range(n)])
    t = batch[("color", 0, 0)]
    u8 = torch.round(t * 255).to(torch.uint8).numpy()
    assert torch.equal(DC.unit(u8), t) and batch["lbl"].dtype == torch.int64
    d["cl_colors"], d["cl_lbl_rgb"], d["cl_frame_0"], d["cl_color_0_0"] = colors, maps, frames, u8
    d["cl_lbl"], d["cl_is_labeled"] = narrow(batch["lbl"]), batch["is_labeled"].numpy()
    for i in range(n):
        assert np.array_equal(NC.pillow_nearest(maps[i], size), np.array(LU.pil_loader(
            os.path.join(root, "train", "labels", "%02d.png" % i), size[1], size[0], is_segmentation=True)))
    return d


def main():
    d = generate()
    if "--check" in sys.argv[1:]:
        z = np.load(OUT, allow_pickle=False)
        bad = [k for k in sorted(set(d) | set(z.files))
               if k not in d or k not in z.files or d[k].dtype != z[k].dtype or d[k].shape != z[k].shape or d[k].tobytes() != z[k].tobytes()]
        print("make_native_resize --check:", "OK" if not bad else "arrays differ from the committed fixture: %s" % bad)
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, "%.1f KB, %d arrays, Pillow %s" % (os.path.getsize(OUT) / 1024, len(d), __import__("PIL").__version__))


if __name__ == "__main__":
    main()
