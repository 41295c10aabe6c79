"""CPU: the split-bf16 operand mode (segsde_conv_desc.compute = 2) through the interpreter build of the real kernel sources.
The bf16 matrix instruction is the host stand-in of csrc/segsde_common.h (eight 2-deep fp32 steps on the widened operands)."""
import pytest
import torch

import emu
import split_bf16_cases as SC


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_exact_split():
    SC.run_exact_split("cpu")


def test_small_integers_are_bit_exact():
    SC.run_small_integers_exact("cpu")


def test_small_products_reach_the_result():
    SC.run_small_products_reach_result("cpu")


def test_mode_is_taken():
    SC.run_mode_is_taken("cpu")


def test_error_gate_against_float64():
    """the four small geometries; the yardstick is the interpreter's own fp32 loop in the same run"""
    SC.run_error_gate("cpu", fullsize=False)


def test_switch_off_is_the_parent():
    SC.run_switch_off("cpu")


def test_non_finite_in_non_finite_out():
    SC.run_non_finite("cpu")


def test_environment_switch():
    """SEGSDE_CONV_COMPUTE is read once at import: a fresh interpreter per value"""
    import os
    import subprocess
    import sys
    from conftest import REPO
    code = "from improving_segmentation_with_selfsupervised_depth_amd import hipops as H; print(H.CONV_COMPUTE[0], H.ConvGeom(64, 64, 1).compute)"
    for val, want in (("bf16x9", "bf16x9 2"), ("f32", "f32 0"), (None, "f32 0")):
        env = {k: v for k, v in os.environ.items() if k != "SEGSDE_CONV_COMPUTE"}
        if val is not None:
            env["SEGSDE_CONV_COMPUTE"] = val
        r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (val, r.stdout, r.stderr[-500:])
    for val in ("bf16", "bf16x6"):          # an unknown value, and the six-product form that is not shipped
        env["SEGSDE_CONV_COMPUTE"] = val
        r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True)
        assert r.returncode != 0 and "ValueError" in r.stderr and all(n in r.stderr for n in ("f32", "bf16x9", "bf16x6"))
