"""GPU (-m gpu): segmentation evaluation with test-time ensembling (hipops.seg_eval_ensemble, csrc/segens.hip,
runningScore.update_from_views, evaluation/tta.py, trainer.validate(tta=...), inference.predict_batch(tta=...)) on the cases of
seg_ensemble_cases.py against its float64 torch oracle on the CPU; the model-level cases on the ResNet-18 joint model."""
import pytest

import seg_ensemble_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,bc,sizes,flips,label_size,kind", C.GENERATED + [C.RAGGED], ids=C.case_id)
def test_generated(seed, bc, sizes, flips, label_size, kind):
    """fails without the feature: hipops.seg_eval_ensemble does not exist"""
    C.run_generated("cuda", seed, bc, sizes, flips, label_size, kind)


def test_both_routes_covered():
    C.run_both_routes_covered()


def test_class_limit():
    C.run_class_limit("cuda")


def test_determinism():
    C.run_determinism("cuda")


def test_zero_weight_view_is_not_read():
    C.run_zero_weight("cuda")


def test_weight_scaling():
    C.run_weight_scaling("cuda")


def test_flip_pair_equals_single_view():
    C.run_flip_pair("cuda")


def test_layouts():
    C.run_layouts("cuda")


def test_half_precision_views():
    C.run_half("cuda")


def test_accumulation_and_hist_checks():
    C.run_accumulation("cuda")


def test_inference_form():
    C.run_inference_form("cuda")


def test_running_score():
    C.run_running_score("cuda")


def test_make_views():
    C.run_make_views("cuda")


def test_validate():
    C.run_validate("cuda")


def test_predict_batch():
    C.run_predict_batch("cuda")


def test_python_argument_checks():
    C.run_python_argument_checks("cuda")
