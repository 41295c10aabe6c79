"""CPU: smoothness, pose, SSIM map, projection and disparity-to-depth kernels against the float64 oracle, and the lifetime of the
wrappers' operands, through the interpreter build of the real kernel sources (tests/geometry_cases.py; the -m gpu file runs the
same cases on the real library)."""
import pytest
import torch

import emu
import geometry_cases as GC


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_recorded_seeds_are_the_first_that_fit():
    """float64 only: every seed in GC.SEEDS meets its case's conditions and no smaller one does"""
    for key, seed in GC.SEEDS.items():
        assert GC.seed_fits(key, seed) and not any(GC.seed_fits(key, s) for s in range(seed)), key


def test_operand_lifetime():
    GC.run_operand_lifetime("cpu")


def test_written_buffers_must_be_contiguous():
    GC.run_raw_pointer_contract("cpu")


@pytest.mark.parametrize("name", list(GC.SMOOTH))
def test_smoothness(name):
    GC.run_smoothness("cpu", name)


def test_get_smooth_loss_batch_limits():
    GC.run_get_smooth_loss("cpu")


@pytest.mark.parametrize("invert", [False, True], ids=["forward", "inverted"])
@pytest.mark.parametrize("B", GC.POSE_B)
def test_pose_matrix(B, invert):
    GC.run_pose("cpu", B, invert)


def test_pose_matrix_function():
    GC.run_pose_function("cpu")


@pytest.mark.parametrize("name", list(GC.SSIM_SHAPES) + ["near-equal"])
def test_ssim_map(name):
    GC.run_ssim("cpu", name)


@pytest.mark.parametrize("name", list(GC.PROJ_SHAPES))
def test_backproject_project(name):
    GC.run_projection("cpu", name)


def test_disp_to_depth_upsampled():
    GC.run_disp_to_depth("cpu")
