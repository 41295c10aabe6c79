"""GPU (-m gpu): segmentation validation at label resolution (hipops.seg_eval, csrc/segeval.hip, runningScore.update_from_logits,
trainer.validate) on the cases of seg_eval_cases.py against its float64 torch oracle on the CPU."""
import pytest

import seg_eval_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,shape,route", C.GENERATED, ids=C.case_id)
def test_generated(seed, shape, route):
    """fails without the feature: hipops.seg_eval does not exist"""
    C.run_generated("cuda", seed, shape, route)


def test_ties():
    C.run_ties("cuda")


def test_accumulation_and_optional_outputs():
    C.run_accumulation("cuda")


def test_determinism():
    C.run_determinism("cuda")


def test_strides():
    C.run_strides("cuda")


def test_batch_stride_past_2_31_bytes():
    C.run_large_batch_stride("cuda")


def test_running_score():
    C.run_running_score("cuda")


def test_meters():
    C.run_meters("cuda")


def test_validate():
    C.run_validate("cuda")


def test_validate_loop_does_not_synchronise():
    C.run_validate_no_sync("cuda")


def test_python_argument_checks():
    C.run_python_argument_checks("cuda")


def test_torch_op():
    C.run_torch_op("cuda")
