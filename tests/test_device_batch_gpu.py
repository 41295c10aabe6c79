"""GPU (-m gpu): the device batch builder (loader/device_batch.py, csrc/batchprep.hip) bit for bit against the reference loader's
outputs (tests/golden/device_batch.npz), and a model step fed from it."""
import pytest

import device_batch_cases as DC

pytestmark = pytest.mark.gpu


def test_case_a_borders_crop_flip_labels_intrinsics():
    DC.run_case_a("cuda")


def test_case_b_tile_seams_validation_path():
    DC.run_case_b("cuda")


def test_case_c_saturation():
    DC.run_case_c("cuda")


def test_case_d_unaligned_crop_width():
    DC.run_case_d("cuda")


def test_division_by_255_is_ieee():
    DC.run_unit_division("cuda")


def test_rejected_shapes():
    DC.run_rejected_shapes("cuda")


def test_model_step_from_the_builder_equals_the_step_from_the_fixture():
    DC.run_end_to_end("cuda")
