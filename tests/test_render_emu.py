"""CPU: rendering of inference outputs (inference.py, csrc/render.hip) with the kernels run by the interpreter build of the real
sources -- the cases of render_cases.py against the reference's recorded images (tests/golden/render.npz), every comparison exact --
plus what needs no kernel at all: the prototypes in header and binding, argument validation of the hipcc-built library,
write_predictions on CPU tensors, the operator registrations, the fixture recipe's --check."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu
import render_cases as C
from conftest import GOLDEN, REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

REF = "/root/reference"
NEW = ["segsde_render_labels", "segsde_render_unit_image", "segsde_colorize_workspace", "segsde_colorize"]


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("decoder", sorted(C.DECODERS))
def test_labels_from_ids(interp, decoder):
    """fails without the feature: inference.render_segmentation against the reference decoder's recorded bytes"""
    C.run_labels_from_ids("cpu", decoder)


def test_label_ids_above_255(interp):
    C.run_label_saturation("cpu")


@pytest.mark.parametrize("n_classes", C.LOGIT_C)
def test_labels_from_logits(interp, n_classes):
    C.run_labels_from_logits("cpu", n_classes)


def test_labels_from_channel_contiguous_logits_of_many_classes(interp):
    C.run_labels_wide_rows("cpu")


def test_unit_image(interp):
    C.run_unit_image("cpu")


def test_unit_image_rounding_boundaries(interp):
    """the interpreter build is compiled without contraction: only the GPU run of this case can show a fused multiply-add"""
    C.run_unit_boundaries("cpu")


def test_colorize(interp):
    C.run_colorize("cpu")


def test_predict_batch_end_to_end(interp):
    """predict_batch and the three renders under the interpreter; the model is a stand-in of three torch convolutions (the GPU
    suite runs the tiny ResNet-18 joint model)"""
    C.run_predict_batch("cpu", stand_in=True)


def test_torch_ops(interp):
    C.run_torch_ops("cpu")


def test_new_prototypes_in_header_and_binding():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS
    assert int(re.search(r"#define SEGSDE_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION
    assert int(re.search(r"#define SEGSDE_RENDER_MAX_COLORS (\d+)", txt).group(1)) == C.H.RENDER_MAX_COLORS == 256
    assert int(re.search(r"#define SEGSDE_COLORIZE_MAX_N (\d+)", txt).group(1)) == C.H.COLORIZE_MAX_N >= 256


def test_argument_validation_without_gpu():
    """the codes of include/segsde_hip.h, returned before any launch by the hipcc-built library"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    L = _lib.bind(ctypes.CDLL(ge.LIB))
    assert L.segsde_abi_version() == _lib.ABI_VERSION
    fake = ctypes.c_void_p(4096)
    labels = lambda **k: L.segsde_render_labels(*[k.get(n, d) for n, d in (      # noqa: E731
        ("logits", fake), ("sb", 19 * 64), ("sc", 64), ("sh", 8), ("sw", 1), ("ids", None), ("dtype", 0), ("B", 1), ("C", 19), ("H", 8),
        ("W", 8), ("pal", fake), ("n", 19), ("mode", 0), ("rgb", fake), ("ids_out", None), ("stream", None))])
    assert labels(logits=None) == -1 and labels(pal=None) == -1 and labels(rgb=None) == -1
    assert labels(B=0) == -2 and labels(H=0) == -2 and labels(W=-1) == -2 and labels(n=0) == -2 and labels(C=0) == -2
    assert labels(n=257) == -4 and labels(mode=2) == -4
    assert labels(logits=None, ids=fake, dtype=0) == -4                      # float ids
    assert labels(rgb=ctypes.c_void_p(4097)) == -4 and labels(ids_out=ctypes.c_void_p(4098)) == -4
    unit = lambda **k: L.segsde_render_unit_image(*[k.get(n, d) for n, d in (      # noqa: E731
        ("x", fake), ("sb", 192), ("sc", 64), ("sh", 8), ("sw", 1), ("B", 1), ("C", 3), ("H", 8), ("W", 8), ("out", fake), ("stream", None))])
    assert unit(x=None) == -1 and unit(out=None) == -1
    assert unit(B=0) == -2 and unit(H=-3) == -2 and unit(W=0) == -2
    assert unit(C=2) == -4 and unit(C=4) == -4 and unit(C=0) == -4
    assert unit(out=ctypes.c_void_p(4099)) == -4
    assert L.segsde_colorize_workspace(2, 40, 600) >= 2 * 2 * 4 and L.segsde_colorize_workspace(0, 8, 8) == 0
    col = lambda **k: L.segsde_colorize(*[k.get(n, d) for n, d in (      # noqa: E731
        ("img", fake), ("B", 1), ("H", 8), ("W", 8), ("lut", fake), ("N", 256), ("mz", 0), ("out", fake), ("ws", fake), ("ws_bytes", 1 << 16),
        ("stream", None))])
    assert col(img=None) == -1 and col(lut=None) == -1 and col(out=None) == -1 and col(ws=None) == -1
    assert col(B=0) == -2 and col(H=0) == -2 and col(W=0) == -2 and col(N=0) == -2
    assert col(N=1025) == -4
    assert col(ws_bytes=4) == -3


def test_python_argument_checks():
    """refused in Python, before the library is looked up"""
    from improving_segmentation_with_selfsupervised_depth_amd import inference as INF
    ids = torch.zeros(1, 2, 2, dtype=torch.int64)
    pal = torch.zeros(19, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        INF.render_segmentation(pred=ids)                                     # no palette inside the package
    with pytest.raises(ValueError):
        INF.render_segmentation(label_colors=pal)
    with pytest.raises(NotImplementedError):
        INF.render_segmentation(pred=ids, label_colors=torch.zeros(257, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        INF.render_segmentation(pred=ids, label_colors=pal, unmapped="white")
    with pytest.raises(TypeError):
        INF.render_segmentation(pred=ids.int(), label_colors=pal)
    with pytest.raises(ValueError):
        INF.render_unit_image(torch.zeros(1, 2, 4, 4))
    with pytest.raises(NotImplementedError):
        INF.colorize(torch.zeros(1, 2, 2), torch.zeros(259, 3), max_percentile=80)


def test_write_predictions(tmp_path):
    from PIL import Image
    from improving_segmentation_with_selfsupervised_depth_amd import inference as INF
    r = C.rng(9)
    B, Hh, W = 2, 5, 7
    res = {"image": torch.from_numpy(r.integers(0, 256, (B, Hh, W, 3)).astype(np.uint8)),
           "label": torch.from_numpy(r.integers(0, 256, (B, Hh, W, 3)).astype(np.uint8)),
           "depth": torch.from_numpy(r.integers(0, 256, (B, Hh, W, 1)).astype(np.uint8)), "pred_ids": None, "outputs": {}}
    names = ["frankfurt/a_000.jpg", "munster/deep/er/b_001.jpg"]
    logdir = str(tmp_path / "run2")
    written = INF.write_predictions(res, names, logdir)
    want = []
    for i, n in enumerate(names):
        fn = "%s/%s" % (logdir, n)
        want += [fn, fn.replace(".jpg", "_depth.png"), fn.replace(".jpg", "_label.png")]
        im = Image.open(fn)
        assert im.mode == "RGB" and im.size == (W, Hh)                           # JPEG bytes are Pillow's: only mode and size
        dep = Image.open(fn.replace(".jpg", "_depth.png"))
        lab = Image.open(fn.replace(".jpg", "_label.png"))
        assert dep.mode == "RGB" and lab.mode == "RGB"
        d = np.asarray(dep)
        assert np.array_equal(d[..., 0], d[..., 1]) and np.array_equal(d[..., 0], d[..., 2])
        assert np.array_equal(d[..., 0], res["depth"][i, ..., 0].numpy())
        assert np.array_equal(np.asarray(lab), res["label"][i].numpy())
    assert written == want and os.path.isdir(os.path.join(logdir, "munster", "deep", "er"))
    # without segmentation / depth only the image is written
    only = INF.write_predictions({"image": res["image"], "label": None, "depth": None}, ["x/y.jpg"], str(tmp_path / "run3"))
    assert only == [str(tmp_path / "run3") + "/x/y.jpg"]


def test_torch_ops_registered():
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    for n in ("render_labels", "render_unit_image", "colorize"):
        assert "segsde::" + n in TO.names()
        assert getattr(torch.ops.segsde, n) is not None


@pytest.mark.skipif(not os.path.isdir(REF), reason="the upstream reference tree is not on this machine")
def test_fixture_recipe_check():
    here = os.path.join(GOLDEN, "make_render.py")
    res = subprocess.run([sys.executable, here, "--check"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert os.path.getsize(os.path.join(GOLDEN, "render.npz")) < 200 * 1024
