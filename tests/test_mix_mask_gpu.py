"""GPU (-m gpu): the batched mix masks (csrc/mixmask.hip, hipops, loader.transformmasks, trainer.generate_mix_mask) on the cases of
mix_mask_cases.py: np.histogram bit for bit, the fused logarithm, ClassMix and "depth" against the per-image formulation of the
parent commit, host traffic, and one unlabeled step per new path."""
import pytest

import mix_mask_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gen,shape,seed", C.HIST_CASES, ids=C.case_id)
def test_histogram_bit_for_bit(gen, shape, seed):
    """fails without the feature: hipops.depth_hist_thresholds does not exist"""
    C.run_hist_case("cuda", gen, shape, seed)


@pytest.mark.parametrize("gen,shape,seed", C.FALLBACK_CASES, ids=C.case_id)
def test_stale_max_depth(gen, shape, seed):
    C.run_fallback_behind_uniform("cuda", gen, shape, seed)


@pytest.mark.parametrize("B", C.BATCHES)
def test_fused_log_and_public_function(B):
    """fails without the feature: "depthhist" raises NotImplementedError"""
    C.run_fused_log("cuda", B)


@pytest.mark.parametrize("B", C.BATCHES)
def test_class_identity(B):
    C.run_class_identity("cuda", B)


def test_class_id_range():
    C.run_class_id_range("cuda")


@pytest.mark.parametrize("B,shape", [(1, (8, 16)), (2, (33, 67)), (5, (33, 67)), (2, (64, 128))], ids=C.case_id)
def test_depth_identity(B, shape):
    C.run_depth_identity("cuda", B, shape)


def test_untouched_modes():
    C.run_untouched_modes("cuda")


def test_python_argument_checks():
    C.run_python_argument_checks("cuda")


def test_no_synchronisation():
    """fails on the parent commit: "depthhist" raises NotImplementedError"""
    C.run_no_sync("cuda")


def test_class_copies_once():
    """fails on the parent commit: torch.unique and the boolean index synchronise twice per image"""
    C.run_class_one_copy("cuda")


@pytest.mark.parametrize("mode", ["depthhist", "class"])
def test_unlabeled_step(mode):
    """"depthhist" fails on the parent commit: NotImplementedError"""
    C.run_unlabeled_step("cuda", mode)
