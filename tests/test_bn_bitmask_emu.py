"""CPU: the packed 1-bit ReLU mask of the residual BatchNorms through the interpreter build of the real kernel sources (the lane
exchange that forms a mask word runs there as wave shuffles; the device's DPP form is covered by the -m gpu file)."""
import pytest
import torch

import bn_bitmask_cases as BC
import emu


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("M,C,pitch", BC.EMU_SHAPES)
def test_mask_mode_is_the_saved_output_mode(M, C, pitch):
    BC.run_shape("cpu", M, C, pitch)


def test_unsupported_shapes_keep_the_saved_output():
    BC.run_unsupported("cpu")


def test_bottleneck_blocks_route_on_and_off():
    BC.run_bottleneck("cpu")
