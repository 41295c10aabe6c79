"""CPU: cross-replica BatchNorm through the interpreter build of the real kernel sources: the stage-level chunk emulation against
the float64 full-batch oracle, the bit-identity of one gathered row with the single-process kernels, SyncBatchNorm2d in a one-rank
gloo group, and the model conversion (tests/sync_bn_cases.py; the -m gpu file runs the same cases on the real library)."""
import pytest
import torch

import emu
import sync_bn_cases as SC


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("case", SC.CHUNK_CASES, ids=SC.case_name)
def test_chunks(case):
    SC.run_chunks("cpu", case)


@pytest.mark.parametrize("nrows", SC.PARTIAL_ROWS)
@pytest.mark.parametrize("case", SC.PARTIAL_CASES, ids=SC.case_name)
def test_partials_source(case, nrows):
    SC.run_partials_source("cpu", case, nrows)


@pytest.mark.parametrize("s", SC.ONE_RANK_SHAPES, ids=SC.BC.spec_name)
def test_one_rank_changes_nothing(s):
    SC.run_one_rank("cpu", s)


def test_one_rank_partials():
    SC.run_one_rank_partials("cpu")


def test_module_one_rank_gloo():
    SC.run_module_one_rank("cpu", "gloo")


def test_conversion():
    SC.run_conversion()
