"""GPU (-m gpu): the BerHu pseudo-depth loss (hipops.berhu_forward / berhu_backward, csrc/berhu.hip, loss.loss.berhu / berhu_own_car,
trainer.train_step / validate) on the cases of berhu_cases.py against its float64 oracle.  Reads the fixture and numpy only."""
import pytest

import berhu_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,shape,mode", C.GENERATED, ids=C.case_id)
def test_generated(seed, shape, mode):
    """fails without the feature: hipops.berhu_forward does not exist"""
    C.run_generated("cuda", seed, shape, mode)


def test_fixture_inputs():
    C.run_fixture_on_device("cuda")


def test_misaligned_base_pointers():
    C.run_misaligned("cuda")


def test_broadcast_mask():
    C.run_broadcast_mask("cuda")


def test_last_element_maximum():
    C.run_last_element_maximum("cuda")


def test_maximum_inside_crop():
    C.run_maximum_inside_crop("cuda")


def test_equal_inputs():
    C.run_equal_inputs("cuda")


def test_autograd_retain_graph():
    C.run_autograd_retain_graph("cuda")


def test_scaled_backward():
    C.run_scaled_backward("cuda")


def test_requires_grad_refused():
    C.run_requires_grad_refused("cuda")


def test_python_argument_checks():
    C.run_python_argument_checks("cuda")


def test_torch_op():
    C.run_torch_op("cuda")


def test_profile_kind(monkeypatch):
    C.run_profile_kind("cuda", monkeypatch)


def test_no_synchronisation():
    """fails on the parent commit: berhu read max(a) with .item()"""
    C.run_no_sync("cuda")


def test_validate():
    C.run_validate("cuda")


def test_train_step():
    C.run_train_step("cuda")
