"""GPU (-m gpu): rendering of inference outputs (inference.py, csrc/render.hip) on the cases of render_cases.py against the
reference's recorded images (tests/golden/render.npz).  Every comparison is exact.  Reads the fixture and numpy only."""
import pytest

import render_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("decoder", sorted(C.DECODERS))
def test_labels_from_ids(decoder):
    """fails without the feature: inference.render_segmentation against the reference decoder's recorded bytes"""
    C.run_labels_from_ids("cuda", decoder)


def test_label_ids_above_255():
    C.run_label_saturation("cuda")


@pytest.mark.parametrize("n_classes", C.LOGIT_C)
def test_labels_from_logits(n_classes):
    C.run_labels_from_logits("cuda", n_classes)


def test_labels_from_channel_contiguous_logits_of_many_classes():
    C.run_labels_wide_rows("cuda")


def test_unit_image():
    C.run_unit_image("cuda")


def test_unit_image_rounding_boundaries():
    """a fused multiply-add in place of the two rounded operations shows here and only here"""
    C.run_unit_boundaries("cuda")


def test_colorize():
    C.run_colorize("cuda")


def test_predict_batch_end_to_end():
    C.run_predict_batch("cuda")


def test_torch_ops():
    C.run_torch_ops("cuda")


def test_offsets_past_2_31_bytes():
    C.run_large_offsets("cuda")
