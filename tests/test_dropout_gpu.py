"""GPU (-m gpu): the dropout draw of the kernels against its specification (oracle/dropout.py), bit for bit, and the models with
dropout on against the float64 oracle with the masks the kernels drew (tests/dropout_cases.py; figures of the run in
profiles/dropout_draw.md)."""
import pytest

import dropout_cases as DC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", DC.SPEC_CASES + [DC.CAP_CASE], ids=DC.case_id)
def test_dropout_against_specification(case):
    """hipops.dropout == where(keep, x * keep_scale, 0) with the specification's keep; 8193 x 257: past the grid cap"""
    DC.run_spec_dense("cuda", case)


@pytest.mark.parametrize("case", DC.SPEC_CASES, ids=DC.case_id)
def test_dropout_on_channel_slices(case):
    """input and output as channel slices, aligned and not: the mask follows the logical index, the buffers stay intact"""
    DC.run_spec_slices("cuda", case)


def test_dropout_identity_and_refusal():
    DC.run_identity_and_refusal("cuda")


@pytest.mark.parametrize("path,s", [(p, s) for p, shapes in DC.FUSED_PATHS.items() for s in shapes],
                         ids=lambda v: v if isinstance(v, str) else DC.BC.spec_name(v))
def test_fused_draw_in_bn_apply(path, s):
    """the three index paths of bn_apply_kernel, relu / elu, with and without residual, dense and pitched"""
    DC.run_fused_apply("cuda", path, s)


@pytest.mark.parametrize("path", list(DC.FUSED_CAP))
def test_fused_draw_past_the_grid_cap(path):
    """more channel vectors than 8192 blocks of 256 threads: the second trip draws from the right indices"""
    DC.run_fused_apply("cuda", path, DC.FUSED_CAP[path], configs=[("elu", False)])


@pytest.mark.parametrize("s", DC.BACKWARD_SHAPES, ids=DC.BC.spec_name)
def test_backward_regenerates_the_mask(s):
    """bn_backward (batch statistics on and off) and the cross-replica stages on one rank: dz is non-zero exactly where the
    specification keeps"""
    DC.run_backward_mask("cuda", s)


def test_dropoutfn_backward():
    DC.run_dropoutfn_backward("cuda")


def test_aspp_with_dropout():
    """M1"""
    DC.run_aspp("cuda")


def test_joint_decoder_with_dropout(golden):
    """M2"""
    DC.run_joint_decoder("cuda", golden)


def test_full_model_with_dropout(golden):
    """M3"""
    DC.run_full_model("cuda", golden)


def test_seed_plumbing(golden):
    DC.run_seed_plumbing("cuda", golden)


def test_capture_path():
    DC.run_capture_path("cuda")
