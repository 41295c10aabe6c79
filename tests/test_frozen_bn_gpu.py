"""GPU (-m gpu): frozen BatchNorm folded into the convolutions of no-grad forward passes (functional.frozen_bn_fold)."""
import pytest

import frozen_bn_cases as FC
from improving_segmentation_with_selfsupervised_depth_amd import _lib

pytestmark = pytest.mark.gpu


def test_fold_kernel():
    FC.run_fold_kernel("cuda")


def test_residual_epilogue_is_bit_exact():
    FC.run_residual_epilogue("cuda")


def test_residual_argument_validation():
    FC.run_residual_validation(_lib.lib())


def test_stem_bias_act():
    FC.run_stem_bias_act("cuda")


@pytest.mark.parametrize("name", sorted(FC.BLOCKS))
def test_block_error_gate(name):
    FC.run_block("cuda", name)


@pytest.mark.parametrize("num_layers", [18, 50])
def test_encoder_error_gate_and_coverage(num_layers):
    """ResNet-18 and the dilated ResNet-50 at 2 x 3 x 64 x 128, eval mode under no_grad: every feature within 3 x of the unfused
    path's max and rms error against float64 (measured ratios: profiles/frozen_bn_fold.md), every conv -> BatchNorm pair folded
    but BasicBlock's conv2 / bn2 / residual"""
    FC.run_encoder("cuda", num_layers)


def test_switch_is_inert():
    FC.run_switch_is_inert("cuda")


def test_cache(monkeypatch):
    FC.run_cache("cuda", monkeypatch)
