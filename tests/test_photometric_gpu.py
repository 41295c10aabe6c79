"""GPU (-m gpu): the photometric kernels against the float64 oracle at masked, clamped and behind-the-camera regimes
(tests/photometric_cases.py; the figures of a run are in profiles/photometric_edges.md)."""
import os
import subprocess
import sys

import pytest

import photometric_cases as PC

pytestmark = pytest.mark.gpu


def test_structured_selection():
    """A: blocks where the identity, frame 0 or frame 1 wins over whole wave footprints (asserted from the float64 selection) and a
    salt-and-pepper strip; every combination of automask / avg / no_ssim; fused kernels and stage chain within the rule"""
    PC.run_A("cuda")


def test_clamp_states():
    """B: at least 5 % of the pixels clamped in x only, y only, both, and unclamped in the last cell, per frame"""
    PC.run_B("cuda")


def test_behind_the_camera():
    """C: p2 < 0 at a third of the pixels; finite, within the rule, no gradient at pixels clamped on both axes"""
    PC.run_C("cuda")


def test_weighted_accumulate():
    """D: weight = 0.375 as a device scalar, non-zero initial gT0 / gT1, batch of two"""
    PC.run_D("cuda")


@pytest.mark.parametrize("i", range(len(PC.E_SHAPES)), ids=["half", "quarter", "eighth", "full_height"])
def test_pyramid_disparities(i):
    PC.run_E("cuda", i)


@pytest.mark.parametrize("knobs", [{"SEGSDE_PHOTO_TILES": "2"}, {"SEGSDE_PHOTO_PACKED": "0"}, {"SEGSDE_PHOTO_SPLIT": "0"}],
                         ids=["two_tile_strips", "round3_kernels", "unsplit_walkers"])
def test_knob_variants(knobs):
    """A and B under the A/B knobs of the photometric kernels (read once per process: a child process each)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import photometric_cases as PC; "
            "PC.run_knob_cases('cuda'); print('VARIANT OK')" % (os.path.dirname(here), here))
    cp = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **knobs), capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0 and "VARIANT OK" in cp.stdout, cp.stdout[-3000:] + cp.stderr[-2000:]
