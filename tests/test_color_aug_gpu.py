"""GPU (-m gpu): the colour augmentation of the device batch builder (loader/device_batch.py ``color_aug=True``, csrc/batchprep.hip)
bit for bit against the reference loader's outputs with Pillow's arithmetic (tests/golden/color_aug.npz) and the numpy oracle the
fixture generator compared with Pillow; reads the fixture and numpy only."""
import pytest

import color_aug_cases as CA

pytestmark = pytest.mark.gpu


def test_reference_batch_all_orders():
    CA.run_reference_batch("cuda")


def test_reduction_across_workgroups_and_scalar_tail():
    CA.run_reduction_and_tail("cuda")


def test_contrast_mean_rounding():
    CA.run_mean_rounding("cuda")


def test_hue_on_all_colours():
    """the whole domain: the 4096x4096 image of all 2^24 colours at shifts 25, 231 and 0"""
    CA.run_exhaustive_hue("cuda", subsample=False)


def test_saturation_on_all_colours():
    """the whole domain: all 2^24 colours at alpha 0.8 and 1.2"""
    CA.run_exhaustive_saturation("cuda", subsample=False)


def test_brightness_contrast_on_all_pairs():
    CA.run_pairs_brightness_contrast("cuda")


def test_draw_with_jitter_replays_the_reference_order():
    CA.run_draw()


def test_default_builder_unchanged_and_validation_path():
    CA.run_unchanged_default("cuda")


def test_rejections():
    CA.run_rejections("cuda")


def test_model_step_from_a_color_aug_builder_equals_the_step_from_the_fixture():
    CA.run_end_to_end("cuda")
