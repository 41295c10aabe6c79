"""GPU (-m gpu): the BatchNorm kernels against float64 at ragged, pitched, offset and degenerate cases
(tests/batchnorm_cases.py; K and the figures of the run it comes from are in profiles/batchnorm_edges.md)."""
import pytest

import batchnorm_cases as BC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("s", BC.APPLY_SHAPES + BC.CAPPED_SHAPES, ids=BC.spec_name)
def test_shape(s):
    """statistics, apply and backward (ELU + residual from the saved output; the four remask configurations bit for bit) at every
    launch shape of the reductions and every index path of the apply kernels; M = 131073: the reductions with 512 capped blocks"""
    BC.run_shape("cuda", s)


def test_remask_nonfinite_gradient():
    """NaN, -Inf and negative gradients on switched-off elements: remask hands on the bits of the saved-output mode"""
    BC.run_remask_nonfinite("cuda")


def test_own_pitches():
    """x, res, y, dy, dx, dres at six different pitches (multiples of 4, then odd ones); guarded slack columns stay untouched"""
    BC.run_own_pitches("cuda")


@pytest.mark.parametrize("s", BC.FLAG_SHAPES, ids=BC.spec_name)
def test_flags(s):
    """act in {none, relu, elu, sigmoid} x residual x gamma / beta None x every (batch_stats, dx, dres)"""
    BC.run_flags("cuda", s)


@pytest.mark.parametrize("s", BC.DROP_SHAPES, ids=BC.spec_name)
def test_dropout(s):
    """p = 0.3 inside apply and backward with real statistics, relu and elu, with and without residual; the keep mask is
    dropout_kernel's draw and the one y implies"""
    BC.run_dropout("cuda", s)


@pytest.mark.parametrize("regime", BC.REGIMES)
def test_regime(regime):
    """R0 .. R3, R5 at (1030, 64) and on the (300, 19) slice"""
    BC.run_regime("cuda", regime)


def test_planted_zeros():
    """R4: ReLU after a residual with exact zeros in y: the derivative there is 0"""
    BC.run_planted_zeros("cuda")


def test_eval_stats():
    BC.run_eval_stats("cuda")


@pytest.mark.parametrize("M,C,VW", BC.TRIP_CASES, ids=["M%d-C%d" % c[:2] for c in BC.TRIP_CASES])
def test_second_trip(M, C, VW):
    """more than 8192 * 256 channel vectors: the grid-stride loops of apply, backward-apply and the mask variant go round again"""
    BC.run_second_trip("cuda", M, C, VW)


def test_end_to_end():
    """functional.BNActFn twice in a row against F.batch_norm in float64 under autograd"""
    BC.run_end_to_end("cuda")
