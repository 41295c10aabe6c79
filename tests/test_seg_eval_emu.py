"""CPU: segmentation validation at label resolution (hipops.seg_eval, csrc/segeval.hip) with the kernels run by the interpreter
build of the real sources -- the cases of seg_eval_cases.py against its float64 torch oracle -- plus what needs no kernel at all:
the prototypes in header and binding, argument validation in Python and of the hipcc-built library, the operator registration, the
meters."""
import ctypes
import os
import re

import pytest
import torch

import emu
import seg_eval_cases as C
from conftest import REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

NEW = ["segsde_seg_eval_workspace", "segsde_seg_eval_plan", "segsde_seg_eval"]


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("seed,shape,route", C.GENERATED, ids=C.case_id)
def test_generated(interp, seed, shape, route):
    """fails without the feature: hipops.seg_eval does not exist"""
    C.run_generated("cpu", seed, shape, route)


def test_ties(interp):
    C.run_ties("cpu")


def test_accumulation_and_optional_outputs(interp):
    C.run_accumulation("cpu")


def test_determinism(interp):
    C.run_determinism("cpu")


def test_strides(interp):
    C.run_strides("cpu")


def test_running_score(interp):
    C.run_running_score("cpu")


def test_validate(interp):
    """trainer.validate around a stand-in head: the loop, the meters, the fused pass, the returned dict"""
    C.run_validate("cpu", "tiny")


@pytest.mark.skipif(not os.environ.get("SEGSDE_SLOW_TESTS"), reason="~11 min under the interpreter (six ResNet-18 passes with the "
                    "monodepth loss); the same case runs in the -m gpu suite (test_seg_eval_gpu.py::test_validate)")
def test_validate_r18(interp):
    C.run_validate("cpu", "r18")


def test_torch_op(interp):
    C.run_torch_op("cpu")


def test_meters():
    C.run_meters("cpu")


def test_python_argument_checks():
    """refused in Python, before the library is looked up"""
    C.run_python_argument_checks("cpu")


def test_torch_op_registered():
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    assert "segsde::seg_eval" in TO.names()
    assert torch.ops.segsde.seg_eval is not None


def test_new_prototypes_in_header_and_binding():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS
    assert int(re.search(r"#define SEGSDE_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION >= 25


def test_argument_validation_without_gpu():
    """the codes of include/segsde_hip.h, returned before any launch by the hipcc-built library"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    L = _lib.bind(ctypes.CDLL(ge.LIB))
    assert L.segsde_abi_version() == _lib.ABI_VERSION
    fake = ctypes.c_void_p(4096)
    call = lambda **k: L.segsde_seg_eval(*[k.get(n, d) for n, d in (      # noqa: E731
        ("logits", fake), ("sb", 19 * 96), ("sc", 96), ("sh", 12), ("sw", 1), ("B", 2), ("C", 19), ("Hi", 8), ("Wi", 12),
        ("labels", fake), ("Ht", 16), ("Wt", 24), ("ignore", 250), ("hist", fake), ("loss", fake), ("ids", fake), ("ws", fake),
        ("ws_bytes", 1 << 20), ("stream", None))])
    assert call(logits=None) == -1 and call(labels=None) == -1
    assert call(hist=None, loss=None, ids=None) == -1
    assert call(ws=None) == -1                                   # the loss needs the workspace
    for dim in ("B", "C", "Hi", "Wi", "Ht", "Wt"):
        assert call(**{dim: 0}) == -2 and call(**{dim: -3}) == -2, dim
    need = L.segsde_seg_eval_workspace(2, 16, 24)
    assert need > 0 and call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert L.segsde_seg_eval_workspace(0, 16, 24) == 0 and L.segsde_seg_eval_workspace(2, 16, 0) == 0
    assert call(C=126) == -4 and call(C=300) == -4               # no room for a tile beside the C x C histogram
    assert call(C=300, hist=None, loss=None, ws=None) == -4      # more than 256 classes with uint8 ids
    assert call(Ht=65536, Wt=65536, loss=None, ws=None) == -4    # Ht * Wt >= 2^32
    assert L.segsde_seg_eval_plan(19, 512, 1024, 1024, 2048) == 16 and L.segsde_seg_eval_plan(66, 512, 1024, 1024, 2048) in (4, 8)
    assert L.segsde_seg_eval_plan(19, 40, 72, 9, 13) == 0 and L.segsde_seg_eval_plan(0, 8, 8, 8, 8) == -2
    assert L.segsde_seg_eval_plan(126, 8, 8, 8, 8) == -4 and L.segsde_seg_eval_plan(125, 8, 8, 16, 16) >= 0
