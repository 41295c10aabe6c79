"""CPU: the BatchNorm kernels against float64 through the interpreter build of the real kernel sources (the launch shapes of the
reductions, the index paths of the apply kernels, pitches and pointer offsets run there as on the device; the -m gpu file adds the
capped reductions of M = 131073 and the second trip of the grid-stride loops on the real library)."""
import pytest
import torch

import batchnorm_cases as BC
import emu


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("s", BC.APPLY_SHAPES, ids=BC.spec_name)
def test_shape(s):
    BC.run_shape("cpu", s)


def test_remask_nonfinite_gradient():
    BC.run_remask_nonfinite("cpu")


def test_own_pitches():
    BC.run_own_pitches("cpu")


@pytest.mark.parametrize("s", BC.FLAG_SHAPES, ids=BC.spec_name)
def test_flags(s):
    BC.run_flags("cpu", s)


@pytest.mark.parametrize("s", BC.DROP_SHAPES, ids=BC.spec_name)
def test_dropout(s):
    BC.run_dropout("cpu", s)


@pytest.mark.parametrize("regime", BC.REGIMES)
def test_regime(regime):
    BC.run_regime("cpu", regime)


def test_planted_zeros():
    BC.run_planted_zeros("cpu")


def test_eval_stats():
    BC.run_eval_stats("cpu")


def test_end_to_end():
    BC.run_end_to_end("cpu")
