#!/usr/bin/env python
"""Fixture recipe of the rendering tests (build container only: needs the reference tree and matplotlib).

Feeds the seeded inputs of tests/render_cases.py to the REFERENCE's own functions and writes what they produce to
tests/golden/render.npz (numbers only).  The reference's loaders and train.py import their whole stack at module level, so nothing
is imported: ``decode_segmap_tocolor`` of the Cityscapes, Mapillary and CamVid loaders and ``_colorize`` of train.py are taken out
of the files with ``ast`` when this script runs and executed in a namespace of numpy / matplotlib (make_label_selection.py does
the same).  Nothing of the reference's text is stored here or in the fixture.

  * The Cityscapes class is plain data plus static methods and is executed as a whole; the other two decoders are methods and get
    a stub ``self`` (``n_classes``; for Mapillary ``class_colors`` = the 66 seeded colours of render_cases.mapillary_colors, which
    stand for the dataset's config.json).
  * What ``Inference.run`` does next -- ``torch.tensor(decoded).permute(2, 0, 1)`` into ``save_image`` -- is RESTATED below from
    torchvision 0.7.0 (``utils.make_grid`` for a single image and the conversion line of ``utils.save_image``), the version the
    reference pins: torchvision is not installed here, so this step is a restatement and is not pinned by the reference (the same
    position as tests/golden/_tv_standin.py).  The uint8 array it hands to Pillow is what is recorded.
  * ``pal_<decoder>`` is the decoder's palette, recovered by decoding the ids 0..n-1.
  * ``plasma`` is matplotlib's table (3.10.8 here): ``cm(np.arange(N))``, ``get_under()``, ``get_over()``, ``get_bad()``, three
    columns, float32.  matplotlib's data, not the reference's; with it the GPU machine needs no matplotlib.
  * ``col_*``: ``_colorize(img, "plasma", mask_zero, 100)`` per image, its float64 result rounded to float32.

Asserted on the way: trunc((c / 255.0) * 255 + 0.5) == c in float64 for all 256 values (why the label path needs no float
arithmetic), and that the id maps hold the ids n, 250 and 255.

  --check   recompute everything and compare with the committed fixture, exactly."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SEGSDE_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
for p_ in (REPO, os.path.join(REPO, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
OUT = os.path.join(HERE, "render.npz")


def _nodes(path, want):
    """top-level class / function definitions of a file by name"""
    tree = ast.parse(open(path).read())
    return {n.name: n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in want}


def _method(path, cls, name, ns):
    for sub in _nodes(path, (cls,))[cls].body:
        if isinstance(sub, ast.FunctionDef) and sub.name == name:
            sub.decorator_list = []
            exec(compile(ast.Module([sub], []), path, "exec"), ns)
            return ns[name]
    raise SystemExit("%s.%s not found in %s" % (cls, name, path))


def reference_functions():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import render_cases as C
    ns = {"np": np}
    path = os.path.join(REF, "loader", "cityscapes_loader.py")
    exec(compile(ast.Module([_nodes(path, ("Cityscapes",))["Cityscapes"]], []), path, "exec"), ns)
    city = ns["Cityscapes"].decode_segmap_tocolor
    assert ns["Cityscapes"].n_classes == C.DECODERS["cityscapes"][0]
    fm = _method(os.path.join(REF, "loader", "mapillary_vistas_loader.py"), "MapillaryVistasLoader", "decode_segmap_tocolor", {"np": np})
    fc = _method(os.path.join(REF, "loader", "camvid_loader.py"), "CamvidLoader", "decode_segmap_tocolor", {"np": np})
    self_m = types.SimpleNamespace(n_classes=C.DECODERS["mapillary"][0], class_colors=C.mapillary_colors().tolist())
    self_c = types.SimpleNamespace(n_classes=C.DECODERS["camvid"][0])
    tpath = os.path.join(REF, "train.py")
    tns = {"np": np, "plt": plt}
    exec(compile(ast.Module([_nodes(tpath, ("_colorize",))["_colorize"]], []), tpath, "exec"), tns)
    return {"cityscapes": city, "mapillary": lambda t: fm(self_m, t), "camvid": lambda t: fc(self_c, t)}, tns["_colorize"], plt


# ---- torchvision 0.7.0, restated (see the module docstring)
def tv_make_grid_single(tensor):
    """utils.make_grid(tensor) with its defaults for ONE image: [H,W], [C,H,W] or [1,C,H,W] -> [3,H,W] / [C,H,W]"""
    if tensor.dim() == 2:
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 3:
        if tensor.size(0) == 1:
            tensor = torch.cat((tensor, tensor, tensor), 0)
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 4 and tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    assert tensor.size(0) == 1
    return tensor.squeeze(0)


def tv_save_image_array(tensor):
    """the uint8 [H,W,3] array utils.save_image hands to PIL.Image.fromarray"""
    grid = tv_make_grid_single(tensor)
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def plasma_table(plt):
    cm = plt.get_cmap("plasma")
    rows = [cm(np.arange(cm.N))[:, :3], np.asarray(cm.get_under())[None, :3], np.asarray(cm.get_over())[None, :3],
            np.asarray(cm.get_bad())[None, :3]]
    return np.concatenate(rows).astype(np.float32)


def build():
    import render_cases as C
    decoders, colorize, plt = reference_functions()
    c = np.arange(256)
    assert np.array_equal(np.trunc((c / 255.0) * 255 + 0.5).astype(np.int64), c), "palette identity"
    out = {}
    for name, fn in decoders.items():
        n = C.DECODERS[name][0]
        label = lambda seg: tv_save_image_array(torch.tensor(fn(seg)).permute(2, 0, 1))      # noqa: E731  (inference.py:115-116)
        out["pal_" + name] = label(np.arange(n, dtype=np.int64)[None, :])[0]
        for shape in C.SHAPES:
            ids = C.id_map(name, shape)
            assert all((ids == v).any() for v in (n, 250, 255))
            out["lab_%s_%s" % (name, C.tag(shape))] = np.stack([label(seg) for seg in ids])
    for ch in (1, 3):
        for shape in C.SHAPES:
            x = torch.from_numpy(C.unit_image(ch, shape))
            out["unit_c%d_%s" % (ch, C.tag(shape))] = np.stack([tv_save_image_array(img) for img in x])   # save_image(img, fn) / (depth, ...)
    out["plasma"] = plasma_table(plt)
    for name, imgs in C.colorize_images().items():
        for mz in (False, True):
            res = [colorize(torch.from_numpy(img[None]), "plasma", mz, 100) for img in imgs]
            assert all(r.dtype == np.float64 and r.shape == imgs.shape[1:] + (3,) for r in res)
            out["col_%s_m%d" % (name, mz)] = np.stack(res).astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    out = build()
    if not args.check:
        np.savez_compressed(OUT, **out)
        print("wrote %s (%d bytes), %d arrays" % (OUT, os.path.getsize(OUT), len(out)))
        return 0
    z = np.load(OUT, allow_pickle=False)
    bad = sorted(set(z.files) ^ set(out))
    for k in sorted(set(z.files) & set(out)):
        a, b = z[k], out[k]
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            bad.append(k)
    print("check:", "ok" if not bad else bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
