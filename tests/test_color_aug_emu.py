"""CPU: the colour augmentation of the device batch builder (loader/device_batch.py, ``color_aug=True``) with the kernels of
csrc/batchprep.hip run by the interpreter build of the real sources -- the same cases as test_color_aug_gpu.py, bit for bit against
the reference loader's outputs with Pillow's arithmetic (tests/golden/color_aug.npz) and the numpy oracle that the fixture
generator compared with Pillow."""
import os
import subprocess
import sys

import pytest
import torch

import color_aug_cases as CA
import emu

REF = "/root/reference"


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_reference_batch_all_orders():
    CA.run_reference_batch("cpu")


def test_reduction_across_workgroups_and_scalar_tail():
    CA.run_reduction_and_tail("cpu")


def test_contrast_mean_rounding():
    CA.run_mean_rounding("cpu")


def test_hue_on_a_64th_of_all_colours():
    """under the interpreter the full 2^24-colour image takes minutes per launch: the fixed 1/64 subsample of
    color_aug_cases.all_colours(True) runs here (262 144 colours, three shifts); the GPU suite runs the whole domain"""
    CA.run_exhaustive_hue("cpu", subsample=True)


def test_saturation_on_a_64th_of_all_colours():
    """the same fixed 1/64 subsample as the hue test; the GPU suite runs the whole domain"""
    CA.run_exhaustive_saturation("cpu", subsample=True)


def test_brightness_contrast_on_all_pairs():
    """the whole 256x256 plane"""
    CA.run_pairs_brightness_contrast("cpu")


def test_draw_with_jitter_replays_the_reference_order():
    CA.run_draw()


def test_default_builder_unchanged_and_validation_path():
    CA.run_unchanged_default("cpu")


def test_rejections():
    CA.run_rejections("cpu")


@pytest.mark.skipif(not os.path.isdir(REF), reason="the upstream reference tree is not on this machine")
def test_fixture_recipe_check():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_color_aug.py")
    res = subprocess.run([sys.executable, here, "--check"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
