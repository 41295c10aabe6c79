"""CPU: patch-wise feature distances (label_selection.patch_feature_distance, section 4b of csrc/labelsel.hip) with the kernel run by
the interpreter build of the real source -- the cases of patch_distance_cases.py against tests/golden/patch_distance.npz -- plus
what needs no kernel: the prototype in header and binding, argument validation of the hipcc-built library, the fixture
recipe's --check.

Thinned under the interpreter: nothing.  The whole grid of cases (9 cases x p in (1, 2) x normalisation off / on) runs here as
on the GPU: the largest case is 640 patch rows and takes about as long as one case of test_label_selection_emu.test_distances."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import emu
import patch_distance_cases as C
from conftest import GOLDEN, REPO
from improving_segmentation_with_selfsupervised_depth_amd import _lib

REF = "/root/reference"
NAME = "segsde_labelsel_patch_distance"


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("k", range(len(C.CASES)), ids=["N%d_C%d_%dx%d" % (n, c, hw[0], hw[1]) for n, c, hw in C.CASES])
def test_error_gate(interp, k):
    """fails without the feature (AttributeError: label_selection.patch_feature_distance)"""
    for kk, p, norm in C.GRID:
        if kk == k:
            C.run_case("cpu", k, p, norm)


def test_discrete_properties(interp):
    C.run_properties("cpu")


def test_refusals(interp):
    C.run_refusals("cpu")


def test_selection_on_the_fixture_bank(interp):
    """12 additions, as test_label_selection_emu does (the GPU suite also adds 30)"""
    C.run_selection("cpu", C.SEL_ADDS[0])


def test_acquire_scores_patch_wise_end_to_end(interp):
    """fails on the parent commit with NotImplementedError("patch_wise feature distances")"""
    C.run_acquire_scores("cpu", stand_in=True)


def test_torch_ops(interp):
    C.run_torch_ops("cpu")


def test_calc_feature_distance_still_refuses_and_names_the_new_function():
    try:
        C.LS._calc_feature_distance([torch.zeros((1, 2, 2, 4))] * 2, [], 0, 2, False, True)
        raise AssertionError("patch_wise accepted")
    except NotImplementedError as e:
        assert "patch_feature_distance" in str(e)


def test_prototype_in_header_and_binding():
    txt = open(os.path.join(REPO, "include", "segsde_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, txt) and NAME in _lib.EXPORTS
    assert int(re.search(r"#define SEGSDE_LABELSEL_PATCH_MAX_P (\d+)", txt).group(1)) == C.H.LABELSEL_PATCH_MAX_P == 128
    assert int(re.search(r"#define SEGSDE_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION


def test_argument_validation_without_gpu():
    """the codes of include/segsde_hip.h, returned before any launch by the hipcc-built library"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    L = _lib.bind(ctypes.CDLL(ge.LIB))
    fake = ctypes.c_void_p(4096)
    call = lambda **k: L.segsde_labelsel_patch_distance(*[k.get(n, d) for n, d in (      # noqa: E731
        ("bank", fake), ("ld", 3 * 32), ("N", 4), ("C", 3), ("P", 32), ("p", 2), ("bias", None), ("out", fake), ("ldo", 4), ("stream", None))])
    assert call(bank=None) == -1 and call(out=None) == -1
    assert call(ld=95) == -2 and call(ldo=3) == -2 and call(N=0) == -2 and call(C=0) == -2
    assert call(p=3) == -4 and call(p=0) == -4
    assert call(P=162, ld=3 * 162) == -4 and call(P=129, ld=3 * 129) == -4 and call(P=0) == -4
    assert call(N=1 << 26, P=32, ldo=1 << 26) == -4          # N * P = 2^31


@pytest.mark.skipif(not os.path.isdir(REF), reason="the upstream reference tree is not on this machine")
def test_fixture_recipe_check():
    here = os.path.join(GOLDEN, "make_patch_distance.py")
    res = subprocess.run([sys.executable, here, "--check"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
