"""CPU: the segmentation loss kernels against float64 through the interpreter build of the real kernel sources (LDS staging, ragged
tiles and the dense / strided dispatch run there as on the device; the -m gpu file adds the grid-stride sizes on the real library)."""
import pytest
import torch

import emu
import segloss_cases as SC


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_cross_entropy_sweep():
    SC.run_sweep("cpu")


@pytest.mark.parametrize("shift", SC.SHIFTS, ids=["shift0", "shift+40", "shift+300", "shift-60"])
@pytest.mark.parametrize("spread", SC.SPREADS, ids=["spread1", "spread8", "spread30"])
def test_per_pixel_loss_offset_logits(shift, spread):
    SC.run_pixel_case("cpu", shift, spread)


def test_saturated_rows():
    SC.run_saturated_rows("cpu")


def test_cross_entropy2d_autograd():
    SC.run_ce2d("cpu")


def test_pseudo_label_edges():
    SC.run_pseudo_label_edges("cpu")


def test_confusion_update():
    SC.run_confusion("cpu")


def test_teacher_softmax():
    SC.run_softmax("cpu")


def test_minmax_normalize():
    SC.run_minmax("cpu")
