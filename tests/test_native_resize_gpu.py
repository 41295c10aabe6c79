"""GPU (-m gpu): pil_loader's resize on the device (loader/device_batch.py ``pil_resize``, ``DeviceBatchBuilder`` fed native-size
frames; csrc/resize.hip, csrc/batchprep.hip) bit for bit against the reference loader's outputs (tests/golden/native_resize.npz)."""
import pytest

import native_resize_cases as NC

pytestmark = pytest.mark.gpu


def test_border_cut_windows_crop_flip_labels_intrinsics():
    NC.run_border_case("cuda")


def test_exact_half_over_several_tiles_both_staging_paths():
    NC.run_exact_half("cuda")


def test_enlargement():
    NC.run_enlargement("cuda")


def test_one_axis_only_skips_the_other_pass():
    NC.run_one_axis("cuda")


def test_many_taps():
    NC.run_many_taps("cuda")


def test_tap_limit_is_refused():
    NC.run_tap_limit("cuda")


def test_saturation_in_both_passes():
    NC.run_saturation("cuda")


def test_per_sample_sizes_in_one_call():
    NC.run_per_sample_sizes("cuda")


def test_labels_nearest_enlargement():
    NC.run_labels_enlarged("cuda")


def test_colour_coded_labels():
    NC.run_color_labels("cuda")


def test_working_size_frames_take_the_old_path():
    NC.run_unchanged("cuda")
