"""GPU (-m gpu): label selection (label_selection.py, csrc/labelsel.hip) on the cases of label_selection_cases.py against the
reference's recorded results (tests/golden/label_selection.npz): discrete results bit for bit, everything else by the 3x rule
against float64.  Reads the fixture and numpy only."""
import pytest

import label_selection_cases as C

pytestmark = pytest.mark.gpu


def test_farthest_point_bit_exact():
    """fails without the feature: label_selection.iterative_farthest_point against the reference's indices and distances"""
    C.run_fps("cuda")


@pytest.mark.parametrize("N", [18000, C.H.LABELSEL_FPS_MAX_N])
def test_farthest_point_at_the_pool_sizes_above_64k_of_lds(N):
    """Mapillary's pool (95 KB of LDS) and the stated cap (160 064 B)"""
    C.run_fps_large("cuda", N)


@pytest.mark.parametrize("N", C.DIST_N)
def test_distances(N):
    for D in C.DIST_D:
        for p in C.DIST_P:
            C.run_distance_case("cuda", N, D, p)


def test_distance_properties():
    C.run_distance_properties("cuda")


def test_calc_feature_distance():
    C.run_calc_feature_distance("cuda")


def test_normalize_over_several_blocks():
    C.run_normalize_blocks("cuda")


@pytest.mark.parametrize("name", sorted(C.SCORE_CASES))
def test_scores(name):
    C.run_score_case("cuda", name)


def test_score_rejections_and_pixel_wise_entropy():
    C.run_score_rejections("cuda")
    C.run_pixel_wise_entropy("cuda")


def test_pooling():
    C.run_pool("cuda")


def test_selection_on_the_fixture_bank():
    C.run_ifp_selection("cuda", C.IFP_ADD_SMALL)
    C.run_ifp_selection("cuda", C.IFP_ADD)


def test_acquire_scores_end_to_end():
    C.run_acquire_scores("cuda")


def test_torch_ops():
    C.run_torch_ops("cuda")
