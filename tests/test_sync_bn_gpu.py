"""GPU (-m gpu): cross-replica BatchNorm on the real library: the stage-level chunk emulation against the float64 full-batch oracle,
the bit-identity of one gathered row with the single-process kernels, SyncBatchNorm2d and the converted R18 joint model in a
one-rank nccl group (tests/sync_bn_cases.py; the worst ratios of the run are in profiles/sync_bn.md).  The exchange between ranks
itself is shown on the CPU (tests/test_sync_bn_gloo.py)."""
import pytest

import sync_bn_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SC.CHUNK_CASES, ids=SC.case_name)
def test_chunks(case):
    """local stage per row chunk, rows stacked as the all-gather leaves them, global stage and apply per chunk; none / relu / relu +
    residual (bitmask where C % 4 == 0) / elu + residual / dropout / gamma None; guard columns of pitched operands untouched"""
    SC.run_chunks("cuda", case)


@pytest.mark.parametrize("nrows", SC.PARTIAL_ROWS)
@pytest.mark.parametrize("case", SC.PARTIAL_CASES, ids=SC.case_name)
def test_partials_source(case, nrows):
    """a rank whose row comes from a hand-made convolution-epilogue partials table"""
    SC.run_partials_source("cuda", case, nrows)


@pytest.mark.parametrize("s", SC.ONE_RANK_SHAPES, ids=SC.BC.spec_name)
def test_one_rank_changes_nothing(s):
    """W = 1, statistics from x: the bits of segsde_bn_stats / segsde_bn_backward / segsde_bn_backward_mask"""
    SC.run_one_rank("cuda", s)


def test_one_rank_partials():
    """W = 1, statistics from a partials table: the bits of segsde_bn_stats_from_partials at each of its three folds"""
    SC.run_one_rank_partials("cuda")


def test_module_one_rank_nccl():
    """SyncBatchNorm2d with an explicit one-rank RCCL group against BatchNorm2d, bit for bit; collectives counted"""
    SC.run_module_one_rank("cuda", "nccl")


def test_converted_model_one_rank_nccl():
    """the converted R18 joint model with GradAllReducer around it, one train_step-shaped forward and backward: losses, every
    parameter gradient, every buffer and the fusion counters equal those of the unconverted model bit for bit"""
    SC.run_integration("cuda", "nccl")
