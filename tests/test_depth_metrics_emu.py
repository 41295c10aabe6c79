"""CPU: depth evaluation (hipops.depth_errors, csrc/depthmetrics.hip) with the kernels run by the interpreter build of the real
sources -- the cases of depth_metrics_cases.py against its numpy oracle -- plus what needs no kernel at all: the prototypes in
header and binding, argument validation in Python and of the hipcc-built library, the operator registration."""
import ctypes
import os
import re

import pytest
import torch

import depth_metrics_cases as C
import emu
from conftest import REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

NEW = ["segsde_depth_errors_workspace", "segsde_depth_errors"]


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("seed,shape", C.GENERATED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_generated(interp, seed, shape):
    """fails without the feature: hipops.depth_errors against the float64 restatement"""
    C.run_generated("cpu", seed, shape)


def test_counts(interp):
    C.run_counts("cpu")


def test_mixed_batch(interp):
    C.run_mixed_batch("cpu")


@pytest.mark.parametrize("name", sorted(C.median_sets()))
def test_median_selection(interp, name):
    C.run_median_selection("cpu", name)


def test_crop(interp):
    C.run_crop("cpu")


def test_no_median_scaling(interp):
    C.run_no_median_scaling("cpu")


def test_lower_clamp(interp):
    C.run_lower_clamp("cpu")


def test_layouts(interp):
    C.run_layouts("cpu")


def test_running_depth_score(interp):
    C.run_running_score("cpu")


def test_compute_depth_metrics(interp):
    C.run_compute_depth_metrics("cpu")


def test_torch_op(interp):
    C.run_torch_op("cpu")


def test_python_argument_checks():
    """refused in Python, before the library is looked up"""
    C.run_python_argument_checks("cpu")


def test_torch_op_registered():
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    assert "segsde::depth_errors" in TO.names()
    assert torch.ops.segsde.depth_errors is not None


def test_new_prototypes_in_header_and_binding():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS
    assert int(re.search(r"#define SEGSDE_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION >= 23
    assert int(re.search(r"#define SEGSDE_DEPTH_ERRORS_COLUMNS (\d+)", txt).group(1)) == len(C.H.DEPTH_ERROR_COLUMNS) == 14
    assert tuple(C.H.DEPTH_ERROR_COLUMNS) == C.COLS


def test_argument_validation_without_gpu():
    """the codes of include/segsde_hip.h, returned before any launch by the hipcc-built library"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    L = _lib.bind(ctypes.CDLL(ge.LIB))
    assert L.segsde_abi_version() == _lib.ABI_VERSION
    fake = ctypes.c_void_p(4096)
    call = lambda **k: L.segsde_depth_errors(*[k.get(n, d) for n, d in (      # noqa: E731
        ("gt", fake), ("pred", fake), ("B", 2), ("H", 8), ("W", 8), ("lo", 1e-3), ("hi", 80.0), ("ms", 1), ("scale", 1.0), ("y0", 0),
        ("y1", 8), ("x0", 0), ("x1", 8), ("table", fake), ("ws", fake), ("ws_bytes", 1 << 20), ("stream", None))])
    assert call(gt=None) == -1 and call(pred=None) == -1 and call(table=None) == -1 and call(ws=None) == -1
    assert call(B=0) == -2 and call(H=0) == -2 and call(W=-1) == -2
    assert call(y1=9) == -2 and call(x1=9) == -2 and call(y0=-1) == -2 and call(x0=-1) == -2
    assert call(y0=8) == -2 and call(y0=3, y1=3) == -2 and call(x0=5, x1=4) == -2
    assert call(lo=-1.0) == -2 and call(lo=80.0) == -2 and call(hi=1e-4) == -2
    assert call(lo=float("nan")) == -2 and call(hi=float("nan")) == -2
    assert call(H=65536, W=65536, y1=65536, x1=65536) == -4
    assert call(ws_bytes=64) == -3
    need = L.segsde_depth_errors_workspace(2, 8, 8)
    assert need > 0 and call(ws_bytes=need - 1) == -3
    assert L.segsde_depth_errors_workspace(0, 8, 8) == 0 and L.segsde_depth_errors_workspace(2, 0, 8) == 0
