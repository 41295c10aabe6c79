"""GPU (-m gpu): smoothness, pose, SSIM map, projection and disparity-to-depth kernels against the float64 oracle at ragged, multi-block
and small-angle cases, and the lifetime of the wrappers' operands (tests/geometry_cases.py; the figures of a run are in
profiles/geometry_edges.md)."""
import pytest

import geometry_cases as GC

pytestmark = pytest.mark.gpu


def test_operand_lifetime():
    """every wrapper with all of its pitchable operands strided at once equals the call on held copies bit for bit and leaves its
    inputs alone; SSIM().mean().backward(), Project3D(BackprojectDepth) with expanded K / inv_K and get_smooth_loss on slices
    within the rule"""
    GC.run_operand_lifetime("cuda")


def test_written_buffers_must_be_contiguous():
    GC.run_raw_pointer_contract("cuda")


@pytest.mark.parametrize("name", list(GC.SMOOTH))
def test_smoothness(name):
    """loss, per-image mean and the accumulated disparity gradient, mean-normalised and plain: one block, three blocks per image
    with B = 3, h = 2 / w = 2, exact ties, and 131 200 pixels (above the 512-block cap, 512 partials in the finalize kernel)"""
    GC.run_smoothness("cuda", name)


def test_get_smooth_loss_batch_limits():
    """B = 1 and B = 64 within the rule; B = 65 raises"""
    GC.run_get_smooth_loss("cuda")


@pytest.mark.parametrize("invert", [False, True], ids=["forward", "inverted"])
@pytest.mark.parametrize("B", GC.POSE_B)
def test_pose_matrix(B, invert):
    """|axisangle| from 3.1 down to 1e-5 and exactly 0, an axis-aligned direction, a second block of 64; frame 1 never matters"""
    GC.run_pose("cuda", B, invert)


def test_pose_matrix_function():
    GC.run_pose_function("cuda")


@pytest.mark.parametrize("name", list(GC.SSIM_SHAPES) + ["near-equal"])
def test_ssim_map(name):
    """forward and both adjoints, down to 2x2 (a mirrored pixel enters a window twice), and the clamp-at-0 branch"""
    GC.run_ssim("cuda", name)


@pytest.mark.parametrize("name", list(GC.PROJ_SHAPES))
def test_backproject_project(name):
    """points, grid, d depth, d T; several blocks per image with B = 3; each adjoint of Project3D by itself"""
    GC.run_projection("cuda", name)


def test_disp_to_depth_upsampled():
    GC.run_disp_to_depth("cuda")
