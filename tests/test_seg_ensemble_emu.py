"""CPU: segmentation evaluation with test-time ensembling (hipops.seg_eval_ensemble, csrc/segens.hip) with the kernels run by the
interpreter build of the real sources -- the cases of seg_ensemble_cases.py against its float64 torch oracle -- plus what needs no
kernel at all: the prototypes in header and binding, argument validation in Python and of the hipcc-built library, the view sizes.
The model-level cases run around a stand-in head here (ResNet-18 passes take minutes under the interpreter); the ResNet-18 joint
model runs in the -m gpu suite (test_seg_ensemble_gpu.py)."""
import ctypes
import os
import re

import pytest
import torch

import emu
import seg_ensemble_cases as C
from conftest import REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

NEW = ["segsde_seg_ens_workspace", "segsde_seg_ens_plan", "segsde_seg_ens"]


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("seed,bc,sizes,flips,label_size,kind", C.GENERATED, ids=C.case_id)
def test_generated(interp, seed, bc, sizes, flips, label_size, kind):
    """fails without the feature: hipops.seg_eval_ensemble does not exist"""
    C.run_generated("cpu", seed, bc, sizes, flips, label_size, kind)


def test_both_routes_covered(interp):
    C.run_both_routes_covered()


def test_class_limit(interp):
    C.run_class_limit("cpu")


def test_determinism(interp):
    C.run_determinism("cpu")


def test_zero_weight_view_is_not_read(interp):
    C.run_zero_weight("cpu")


def test_weight_scaling(interp):
    C.run_weight_scaling("cpu")


def test_flip_pair_equals_single_view(interp):
    C.run_flip_pair("cpu")


def test_layouts(interp):
    C.run_layouts("cpu")


def test_half_precision_views(interp):
    C.run_half("cpu")


def test_accumulation_and_hist_checks(interp):
    C.run_accumulation("cpu")


def test_inference_form(interp):
    C.run_inference_form("cpu")


def test_running_score(interp):
    C.run_running_score("cpu")


def test_make_views(interp):
    C.run_make_views("cpu")


def test_validate(interp):
    """trainer.validate(tta=...) around a stand-in head: the views, the forwards, the fused pass, the returned dict"""
    C.run_validate("cpu", "tiny")


def test_predict_batch(interp):
    C.run_predict_batch("cpu", "tiny")


def test_view_sizes():
    C.run_view_sizes()


def test_python_argument_checks():
    """refused in Python, before the library is looked up"""
    C.run_python_argument_checks("cpu")


def test_new_prototypes_in_header_and_binding():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    macros = dict(re.findall(r"#define (SEGSDE_SEG_ENS_MAX_\w+) (\d+)", txt))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS
    from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
    assert int(macros["SEGSDE_SEG_ENS_MAX_VIEWS"]) == H.SEG_ENS_MAX_VIEWS == 16
    assert int(macros["SEGSDE_SEG_ENS_MAX_CLASSES"]) == H.SEG_ENS_MAX_CLASSES == C.C_LIMIT
    # the descriptor mirrors the header's struct: a pointer, four longs, three ints, a float
    assert ctypes.sizeof(_lib.SegEnsView) == 56 and _lib.SegEnsView.weight.offset == 52 and _lib.SegEnsView.Hi.offset == 40
    assert int(re.search(r"#define SEGSDE_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION


def test_argument_validation_without_gpu():
    """the codes of include/segsde_hip.h, returned before any launch by the hipcc-built library"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    L = _lib.bind(ctypes.CDLL(ge.LIB))
    fake = ctypes.c_void_p(4096)
    V = _lib.SegEnsView

    def views(*specs):
        """specs: (Hi, Wi, weight) or (Hi, Wi, weight, pointer)"""
        return (V * len(specs))(*[V(s[3] if len(s) > 3 else 4096, 19 * 96, 96, 12, 1, s[0], s[1], 0, s[2]) for s in specs])

    two = views((8, 12, 1.0), (4, 6, 1.0))
    call = lambda **k: L.segsde_seg_ens(*[k.get(n, d) for n, d in (      # noqa: E731
        ("views", two), ("K", 2), ("B", 2), ("C", 19), ("labels", fake), ("Ht", 16), ("Wt", 24), ("ignore", 250), ("hist", fake),
        ("loss", fake), ("ids", fake), ("ws", fake), ("ws_bytes", 1 << 20), ("stream", None))])
    assert call(views=None) == -1 and call(hist=None, loss=None, ids=None) == -1
    assert call(ws=None) == -1                                   # the loss needs the workspace
    assert call(labels=None) == -1 and call(labels=None, loss=None, ws=None) == -1      # hist or loss without labels
    assert call(views=views((8, 12, 1.0, None), (4, 6, 1.0))) == -1                  # a view that takes part has no logits
    assert call(K=0) == -2 and call(K=17) == -2 and call(K=-1) == -2
    for w in (-1.0, float("nan"), float("inf")):
        assert call(views=views((8, 12, 1.0), (4, 6, w))) == -2, w
    assert call(views=views((8, 12, 0.0), (4, 6, 0.0))) == -2    # all weights zero
    assert call(views=views((8, 0, 1.0), (4, 6, 1.0))) == -2 and call(views=views((8, 12, 1.0), (-4, 6, 1.0))) == -2
    for dim in ("B", "C", "Ht", "Wt"):
        assert call(**{dim: 0}) == -2 and call(**{dim: -3}) == -2, dim
    need = L.segsde_seg_ens_workspace(2, 16, 24)
    assert need == 2 * 16 * 1 * 16 and call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert L.segsde_seg_ens_workspace(0, 16, 24) == 0 and L.segsde_seg_ens_workspace(2, 16, 0) == 0
    assert call(C=C.C_LIMIT + 1) == -4 and call(C=300) == -4
    assert call(Ht=65536, Wt=65536, hist=None, loss=None, ws=None) == -4            # Ht * Wt >= 2^32
    assert call(ws=ctypes.c_void_p(4100)) == -4                                     # the partials are doubles
    # the plan: tile rows and the route per view
    staged = (ctypes.c_int * 16)()
    twelve = views(*[(256 + 128 * (i // 2), 512 + 256 * (i // 2), 1.0) for i in range(12)])
    assert L.segsde_seg_ens_plan(twelve, 12, 19, 1024, 2048, staged) == 4 and list(staged[:12]) == [1] * 12
    assert L.segsde_seg_ens_plan(views((1024, 2048, 1.0), (1024, 2048, 1.0)), 2, 19, 1024, 2048, staged) == 4
    assert list(staged[:2]) == [1, 1]
    assert L.segsde_seg_ens_plan(views((512, 1024, 1.0), (1024, 2048, 0.0)), 2, 66, 1024, 2048, staged) == 4
    assert list(staged[:2]) == [1, -1]                           # 66 classes: four rows in the 160 KB a workgroup may have
    assert L.segsde_seg_ens_plan(views((40, 72, 1.0), (5, 7, 1.0)), 2, 19, 9, 13, staged) == 8 and list(staged[:2]) == [0, 1]
    assert L.segsde_seg_ens_plan(views((8, 8, 1.0)), 1, 125, 16, 16, None) in (1, 2)
    assert L.segsde_seg_ens_plan(views((8, 8, 1.0)), 1, C.C_LIMIT, 16, 16, None) == 1
    assert L.segsde_seg_ens_plan(views((8, 8, 1.0)), 1, 0, 16, 16, None) == -2
    assert L.segsde_seg_ens_plan(None, 1, 19, 16, 16, None) == -1
