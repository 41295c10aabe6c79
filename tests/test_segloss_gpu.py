"""GPU (-m gpu): the segmentation loss kernels against float64 at ragged, weighted, offset and saturated cases
(tests/segloss_cases.py; K = 8 and the figures of the run it comes from are in profiles/segloss_edges.md)."""
import pytest

import segloss_cases as SC

pytestmark = pytest.mark.gpu


def test_cross_entropy_sweep():
    """A: C in {1, 3, 19, 20, 64, 65} x M in {1, 255, 256, 257, 700} x dense / pitched / misaligned views, class and pixel weights,
    four target patterns; sum, denominator, gradient, zero rows, untouched padding"""
    SC.run_sweep("cuda")


@pytest.mark.parametrize("shift", SC.SHIFTS, ids=["shift0", "shift+40", "shift+300", "shift-60"])
@pytest.mark.parametrize("spread", SC.SPREADS, ids=["spread1", "spread8", "spread30"])
def test_per_pixel_loss_offset_logits(shift, spread):
    """B: every kept pixel's loss read through a one-hot pixel_weights vector, dense and strided forward kernels"""
    SC.run_pixel_case("cuda", shift, spread)


def test_saturated_rows():
    """B: [1e4, -1e4, 0, ...] towards the high and the low class: finite, exact, zero gradient where exp underflows"""
    SC.run_saturated_rows("cuda")


def test_grid_stride_cross_entropy():
    """C: M = 1024 * 256 + 300, every block takes a second tile"""
    SC.run_grid_stride_ce("cuda")


def test_grid_stride_pseudo_label():
    """C: B * HW = 4096 * 256 + 77, every thread takes a second pixel"""
    SC.run_grid_stride_pseudo_label("cuda")


def test_cross_entropy2d_autograd():
    """D: NCHW and channels-last logits, a target of twice the size, class and pixel weights, a NaN weight, all ignored"""
    SC.run_ce2d("cuda")


def test_pseudo_label_edges():
    """E: the threshold and one ulp below it, zeros of either sign, a tie, the last class, C = 1; HW = 265"""
    SC.run_pseudo_label_edges("cuda")


def test_confusion_update():
    """F: skipped labels and predictions, ties, both layouts, C in {1, 19, 64}, C = 65 refused, two blocks, two calls"""
    SC.run_confusion("cuda")


def test_teacher_softmax():
    """G: four (spread, shift) regimes, C in {1, 19, 160}, an unaligned second image, a pitched slice, C = 161 refused"""
    SC.run_softmax("cuda")


def test_minmax_normalize():
    """G: a constant image (0 / 0 as in the reference) beside ordinary ones, HW below one block"""
    SC.run_minmax("cuda")
