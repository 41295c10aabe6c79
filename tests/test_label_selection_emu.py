"""CPU: label selection (label_selection.py, csrc/labelsel.hip) with the kernels run by the interpreter build of the real sources --
the cases of label_selection_cases.py, against the reference's recorded results (tests/golden/label_selection.npz: discrete results
bit for bit, everything else by the 3x rule against float64) -- plus what needs no kernel at all: the prototypes in header and
binding, argument validation of the hipcc-built library, the public signatures, the fixture recipe's --check."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import emu
import label_selection_cases as C
from conftest import GOLDEN, REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

REF = "/root/reference"
NEW = ["segsde_labelsel_score_workspace", "segsde_labelsel_score", "segsde_labelsel_pool", "segsde_labelsel_normalize_workspace",
       "segsde_labelsel_normalize", "segsde_labelsel_distance", "segsde_labelsel_farthest_point"]


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_farthest_point_bit_exact(interp):
    """fails without the feature: label_selection.iterative_farthest_point against the reference's indices and distances"""
    C.run_fps("cpu")


def test_farthest_point_above_64k_of_lds(interp):
    """N = 16500: the first size whose LDS layout passes 64 KB (the GPU suite runs 18 000 and the cap)"""
    C.run_fps_large("cpu", 16500, n_new=3)


@pytest.mark.parametrize("N", C.DIST_N)
def test_distances(interp, N):
    for D in C.DIST_D:
        for p in C.DIST_P:
            C.run_distance_case("cpu", N, D, p)


def test_distance_properties(interp):
    C.run_distance_properties("cpu")


def test_calc_feature_distance(interp):
    C.run_calc_feature_distance("cpu")


def test_normalize_over_several_blocks(interp):
    C.run_normalize_blocks("cpu")


@pytest.mark.parametrize("name", sorted(C.SCORE_CASES))
def test_scores(interp, name):
    C.run_score_case("cpu", name)


def test_score_rejections_and_pixel_wise_entropy(interp):
    C.run_score_rejections("cpu")
    C.run_pixel_wise_entropy("cpu")


def test_pooling(interp):
    C.run_pool("cpu")


def test_selection_on_the_fixture_bank(interp):
    """12 additions: one workgroup runs through two barriers per step under the interpreter (the GPU suite adds 30)"""
    C.run_ifp_selection("cpu", C.IFP_ADD_SMALL)


def test_acquire_scores_end_to_end(interp):
    """acquire_scores and every kernel behind it under the interpreter; the model is a stand-in of three torch convolutions (a
    forward pass of even the tiny ResNet takes minutes under the interpreter: the GPU suite runs the real one)"""
    C.run_acquire_scores("cpu", stand_in=True)


def test_torch_ops(interp):
    C.run_torch_ops("cpu")


def test_host_mirrors():
    C.run_choose_from_scores()
    C.run_initial_and_totals()


def test_dilate_mirror():
    g = C.golden()
    for name in ("s23x40_c19", "s64x128_c20_pitched"):
        _, _, ds = C.score_inputs(name)
        m = C.LS.dilate((torch.from_numpy(ds[0]) < 0.07).float(), 7, 3)
        assert torch.equal(m.to(torch.uint8), g["mask_" + name])


def test_new_prototypes_in_header_and_binding():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS
    assert int(re.search(r"#define SEGSDE_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION
    assert int(re.search(r"#define SEGSDE_LABELSEL_FPS_MAX_N (\d+)", txt).group(1)) == C.H.LABELSEL_FPS_MAX_N >= 18000


def test_argument_validation_without_gpu():
    """the codes of include/segsde_hip.h, returned before any launch by the hipcc-built library"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    L = _lib.bind(ctypes.CDLL(ge.LIB))
    fake = ctypes.c_void_p(4096)
    types = (ctypes.c_int * 7)(0, 1, 2, 3, 4, 5, 6)
    score = lambda **k: L.segsde_labelsel_score(*[k.get(n, d) for n, d in (
        ("logits", fake), ("sb", 19 * 64), ("sc", 64), ("sh", 8), ("sw", 1), ("B", 1), ("C", 19), ("H", 8), ("W", 8), ("dp", fake), ("ds", fake),
        ("types", types), ("T", 7), ("table", fake), ("ent", None), ("err", None), ("ws", fake), ("ws_bytes", 1 << 20), ("stream", None))])
    assert score(logits=None) == -1 and score(table=None) == -1 and score(ws=None) == -1 and score(dp=None) == -1
    assert score(H=0) == -2 and score(T=8) == -2 and score(types=(ctypes.c_int * 7)(0, 1, 2, 3, 4, 5, 7)) == -2
    assert score(C=1) == -4 and score(C=161) == -4
    assert score(ws_bytes=8) == -3
    assert L.segsde_labelsel_score_workspace(1, 8, 8, 7) > 0
    pool = lambda **k: L.segsde_labelsel_pool(*[k.get(n, d) for n, d in (
        ("x", fake), ("sb", 192), ("sc", 64), ("sh", 8), ("sw", 1), ("B", 1), ("C", 3), ("H", 8), ("W", 8), ("h", 2), ("is_max", 0), ("tr", 0),
        ("bank", fake), ("ld", 24), ("N", 4), ("row0", 0), ("stream", None))])
    assert pool(x=None) == -1 and pool(bank=None) == -1
    assert pool(ld=23) == -2 and pool(row0=4) == -2 and pool(h=0) == -2
    assert pool(tr=3) == -4
    assert L.segsde_labelsel_normalize_workspace(10, 3, 8) > 0
    assert L.segsde_labelsel_normalize(None, 24, 10, 3, 8, fake, 1 << 20, None) == -1
    assert L.segsde_labelsel_normalize(fake, 23, 10, 3, 8, fake, 1 << 20, None) == -2
    assert L.segsde_labelsel_normalize(fake, 24, 10, 3, 8, fake, 8, None) == -3
    assert L.segsde_labelsel_distance(None, 8, 4, 8, 2, None, fake, 4, None) == -1
    assert L.segsde_labelsel_distance(fake, 7, 4, 8, 2, None, fake, 4, None) == -2
    assert L.segsde_labelsel_distance(fake, 8, 4, 8, 2, None, fake, 3, None) == -2
    assert L.segsde_labelsel_distance(fake, 8, 4, 8, 3, None, fake, 4, None) == -4
    assert L.segsde_labelsel_farthest_point(None, 4, 4, fake, 1, None, 2, fake, fake, fake, None) == -1
    assert L.segsde_labelsel_farthest_point(fake, 4, 4, fake, 0, None, 2, fake, fake, fake, None) == -2
    assert L.segsde_labelsel_farthest_point(fake, 3, 4, fake, 1, None, 2, fake, fake, fake, None) == -2
    big = C.H.LABELSEL_FPS_MAX_N + 1
    assert L.segsde_labelsel_farthest_point(fake, big, big, fake, 1, None, 2, fake, fake, fake, None) == -4


def test_signatures_match_reference():
    """the reference's parameters lead, in order and with their defaults; anything the package adds has a default"""
    import importlib
    ref = json.load(open(os.path.join(GOLDEN, "label_selection_signatures.json")))
    assert len(ref) == 8
    for key, want in ref.items():
        mod, name = key.split(":") if ":" in key else ("label_selection", key)
        fn = getattr(importlib.import_module("improving_segmentation_with_selfsupervised_depth_amd." + mod), name)
        got = list(inspect.signature(fn).parameters.values())
        n_ref = len(inspect.signature(eval("lambda " + want.strip()[1:-1] + ": 0")).parameters)
        assert str(inspect.Signature(got[:n_ref])) == want, (key, want, got)
        assert all(p.default is not inspect.Parameter.empty for p in got[n_ref:]), key
    acq = inspect.signature(C.LS.acquire_scores)
    assert list(acq.parameters)[:7] == ["model", "batches", "samples_to_score", "label_selection_cfg", "depth_teacher", "depth_ifp_w", "amp"]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the upstream reference tree is not on this machine")
def test_fixture_recipe_check():
    here = os.path.join(GOLDEN, "make_label_selection.py")
    res = subprocess.run([sys.executable, here, "--check"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
