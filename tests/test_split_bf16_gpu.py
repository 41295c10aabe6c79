"""GPU (-m gpu): the split-bf16 operand mode (segsde_conv_desc.compute = 2: fp32 convolutions on v_mfma_f32_32x32x16_bf16)."""
import pytest
import torch

import model_cases as MC
import split_bf16_cases as SC
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

pytestmark = pytest.mark.gpu


def test_exact_split():
    SC.run_exact_split("cuda")


def test_small_integers_are_bit_exact():
    SC.run_small_integers_exact("cuda")


def test_small_products_reach_the_result():
    SC.run_small_products_reach_result("cuda")


def test_mode_is_taken():
    SC.run_mode_is_taken("cuda")


def test_error_gate_against_float64():
    """The four small geometries, the 1x1 1024 -> 256 @32x64 (batch 16) and the dilated 2048 -> 256 @32x64, rate 12 (batch 4), all
    three directions: bf16x9 within 3 x of the fp32 kernel's max and rms error against float64, the fp32 kernel measured in the same
    run.  (bf16x6 missed its 1.5 x gate with this code -- figures in split_bf16_cases.run_error_gate -- and is not shipped.)"""
    SC.run_error_gate("cuda", fullsize=True)


def _routes():
    return {k: dict(v) for k, v in (("wino", H.WINOGRAD_TAKEN), ("fused", H.WINO_FUSED_TAKEN), ("fold", H.UPFOLD_TAKEN))}


def _delta(a, b):
    return {k: {q: b[k][q] - a[k][q] for q in a[k]} for k in a}


def test_whole_model_switch_on(golden):
    """r18_jsd forward + backward under conv_compute("bf16x9") passes the fp32 run's own criterion (same golden vectors, same
    float64 yardstick, same tolerances), and the Winograd / folded routes are taken exactly as often as with the switch off"""
    r0, t00 = _routes(), dict(H.CONV_COMPUTE_TAKEN)
    MC.run_full_model("cuda", golden, "r18_jsd")
    r1 = _routes()
    Fn.fusion_report(reset=True)
    assert H.CONV_COMPUTE_TAKEN == t00, "the switch was off, nothing may be counted"
    t0 = dict(H.CONV_COMPUTE_TAKEN)
    seen = []
    init = H.ConvGeom.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        seen.append(self.compute)
    H.ConvGeom.__init__ = spy
    try:
        with Fn.conv_compute("bf16x9"):
            MC.run_full_model("cuda", golden, "r18_jsd")
    finally:
        H.ConvGeom.__init__ = init
    r2 = _routes()
    assert seen and all(c == 2 for c in seen), "the convolutions of the model did not see the switch"
    split = {k: H.CONV_COMPUTE_TAKEN[k] - t0[k] for k in t0}
    print("direct launches of r18_jsd that took the split-bf16 loop:", split)
    assert all(v > 0 for v in split.values()), "no launch of the model took the split loop in some direction: %r" % (split,)
    assert _delta(r0, r1) == _delta(r1, r2), (_delta(r0, r1), _delta(r1, r2))
    assert H.CONV_COMPUTE[0] == "f32"


def test_switch_off_is_the_parent():
    SC.run_switch_off("cuda")


def test_non_finite_in_non_finite_out():
    SC.run_non_finite("cuda")
