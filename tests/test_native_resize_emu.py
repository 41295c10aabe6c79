"""CPU: pil_loader's resize on the device (loader/device_batch.py ``pil_resize``, ``DeviceBatchBuilder`` fed native-size frames) with
the kernels of csrc/resize.hip and csrc/batchprep.hip run by the interpreter build of the real sources -- the same cases as
test_native_resize_gpu.py, bit for bit against the reference loader's outputs (tests/golden/native_resize.npz)."""
import os
import subprocess
import sys

import pytest
import torch

import emu

REF = "/root/reference"


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.fixture(scope="module")
def NC():
    import native_resize_cases
    return native_resize_cases


def test_border_cut_windows_crop_flip_labels_intrinsics(NC):
    NC.run_border_case("cpu")


def test_exact_half_over_several_tiles_both_staging_paths(NC):
    NC.run_exact_half("cpu")


def test_enlargement(NC):
    NC.run_enlargement("cpu")


def test_one_axis_only_skips_the_other_pass(NC):
    NC.run_one_axis("cpu")


def test_many_taps(NC):
    NC.run_many_taps("cpu")


def test_tap_limit_is_refused(NC):
    NC.run_tap_limit("cpu")


def test_saturation_in_both_passes(NC):
    NC.run_saturation("cpu")


def test_per_sample_sizes_in_one_call(NC):
    NC.run_per_sample_sizes("cpu")


def test_labels_nearest_enlargement(NC):
    NC.run_labels_enlarged("cpu")


def test_colour_coded_labels(NC):
    NC.run_color_labels("cpu")


def test_working_size_frames_take_the_old_path(NC):
    NC.run_unchanged("cpu")


@pytest.mark.skipif(not os.path.isdir(REF), reason="the upstream reference tree is not on this machine")
def test_fixture_recipe_check():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_native_resize.py")
    res = subprocess.run([sys.executable, here, "--check"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
