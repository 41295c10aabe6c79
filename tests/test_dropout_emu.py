"""CPU: the dropout draw of the kernels against its specification (oracle/dropout.py) and the models with dropout on against the
float64 oracle, through the interpreter build of the real kernel sources (tests/dropout_cases.py; the -m gpu file adds the shapes
past the grid caps and runs the whole-model case on the real library)."""
import os

import pytest
import torch

import dropout_cases as DC
import emu


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("case", DC.SPEC_CASES, ids=DC.case_id)
def test_dropout_against_specification(case):
    DC.run_spec_dense("cpu", case)


@pytest.mark.parametrize("case", DC.SPEC_CASES, ids=DC.case_id)
def test_dropout_on_channel_slices(case):
    DC.run_spec_slices("cpu", case)


def test_dropout_identity_and_refusal():
    DC.run_identity_and_refusal("cpu")


@pytest.mark.parametrize("path,s", [(p, s) for p, shapes in DC.FUSED_PATHS.items() for s in shapes],
                         ids=lambda v: v if isinstance(v, str) else DC.BC.spec_name(v))
def test_fused_draw_in_bn_apply(path, s):
    DC.run_fused_apply("cpu", path, s)


@pytest.mark.parametrize("s", DC.BACKWARD_SHAPES, ids=DC.BC.spec_name)
def test_backward_regenerates_the_mask(s):
    DC.run_backward_mask("cpu", s)


def test_dropoutfn_backward():
    DC.run_dropoutfn_backward("cpu")


def test_specification_statistics():
    DC.run_statistics()


def test_window_separation():
    DC.run_window_separation()


def test_aspp_with_dropout():
    DC.run_aspp("cpu")


def test_joint_decoder_with_dropout(golden):
    DC.run_joint_decoder("cpu", golden)


def test_seed_plumbing(golden):
    DC.run_seed_plumbing("cpu", golden)


def test_capture_path():
    DC.run_capture_path("cpu")


@pytest.mark.skipif(not os.environ.get("SEGSDE_SLOW_TESTS"), reason="minutes under the interpreter (a ResNet-18 joint model forward and "
                    "backward); the GPU suite runs it.  SEGSDE_SLOW_TESTS=1 runs it")
def test_full_model_with_dropout(golden):
    DC.run_full_model("cpu", golden)
