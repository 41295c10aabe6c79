"""GPU (-m gpu): depth evaluation (hipops.depth_errors, csrc/depthmetrics.hip) on the cases of depth_metrics_cases.py against its
numpy oracle.  Reads numpy only."""
import pytest

import depth_metrics_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,shape", C.GENERATED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_generated(seed, shape):
    """fails without the feature: hipops.depth_errors against the float64 restatement"""
    C.run_generated("cuda", seed, shape)


def test_counts():
    C.run_counts("cuda")


def test_mixed_batch():
    C.run_mixed_batch("cuda")


@pytest.mark.parametrize("name", sorted(C.median_sets()))
def test_median_selection(name):
    C.run_median_selection("cuda", name)


def test_crop():
    C.run_crop("cuda")


def test_no_median_scaling():
    C.run_no_median_scaling("cuda")


def test_lower_clamp():
    C.run_lower_clamp("cuda")


def test_layouts():
    C.run_layouts("cuda")


def test_python_argument_checks():
    C.run_python_argument_checks("cuda")


def test_running_depth_score():
    C.run_running_score("cuda")


def test_compute_depth_metrics():
    C.run_compute_depth_metrics("cuda")


def test_torch_op():
    C.run_torch_op("cuda")


def test_offsets_past_2_31_bytes():
    C.run_large_offsets("cuda")


def test_update_does_not_synchronise():
    C.run_no_sync("cuda")
