"""GPU (-m gpu): the packed 1-bit ReLU mask of the residual BatchNorms against the saved-output mode, bit for bit."""
import pytest

import bn_bitmask_cases as BC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M,C,pitch", BC.SHAPES)
def test_mask_mode_is_the_saved_output_mode(M, C, pitch):
    """y and the mask words of segsde_bn_apply_mask (against the host packing of y > 0), then dx / dres / dgamma / dbeta of
    segsde_bn_backward_mask for both batch_stats values and with dx / dres switched off once each: planted y == 0, negative
    gammas and a NaN in dy included, every output equals the saved-output mode's bit for bit"""
    BC.run_shape("cuda", M, C, pitch)


def test_unsupported_shapes_keep_the_saved_output():
    BC.run_unsupported("cuda")


def test_bottleneck_blocks_route_on_and_off():
    BC.run_bottleneck("cuda")
