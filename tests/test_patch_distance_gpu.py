"""GPU (-m gpu): patch-wise feature distances (label_selection.patch_feature_distance, section 4b of csrc/labelsel.hip) on the cases
of patch_distance_cases.py against tests/golden/patch_distance.npz: the whole grid by the 3x rule against float64, the discrete
properties bit for bit.  Reads the fixtures and numpy only."""
import pytest

import patch_distance_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(len(C.CASES)), ids=["N%d_C%d_%dx%d" % (n, c, hw[0], hw[1]) for n, c, hw in C.CASES])
def test_error_gate(k):
    """fails without the feature (AttributeError: label_selection.patch_feature_distance)"""
    for kk, p, norm in C.GRID:
        if kk == k:
            C.run_case("cuda", k, p, norm)


def test_discrete_properties():
    C.run_properties("cuda")


def test_refusals():
    C.run_refusals("cuda")


def test_selection_on_the_fixture_bank():
    for n_add in C.SEL_ADDS:
        C.run_selection("cuda", n_add)


def test_acquire_scores_patch_wise_end_to_end():
    """fails on the parent commit with NotImplementedError("patch_wise feature distances")"""
    C.run_acquire_scores("cuda")


def test_torch_ops():
    C.run_torch_ops("cuda")
