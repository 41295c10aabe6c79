"""CPU: the photometric kernels against the float64 oracle through the interpreter build of the real kernel sources (wave votes,
packed lanes and tile strips run there as on the device; the -m gpu file runs the full case list on the real library)."""
import os
import subprocess
import sys

import pytest
import torch

import emu
import photometric_cases as PC


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_nan_guard_comment_matches_aten():
    PC.nan_guard_matches_aten()


def test_structured_selection():
    PC.run_A("cpu")


def test_clamp_states():
    PC.run_B("cpu")


def test_behind_the_camera():
    PC.run_C("cpu")


def test_weighted_accumulate():
    PC.run_D("cpu")


@pytest.mark.parametrize("i", range(len(PC.E_SHAPES)), ids=["half", "quarter", "eighth", "full_height"])
def test_pyramid_disparities(i):
    PC.run_E("cpu", i)


@pytest.mark.parametrize("knobs", [{"SEGSDE_PHOTO_TILES": "2"}, {"SEGSDE_PHOTO_PACKED": "0"}, {"SEGSDE_PHOTO_SPLIT": "0"}],
                         ids=["two_tile_strips", "round3_kernels", "unsplit_walkers"])
def test_knob_variants(knobs):
    """A and B under the A/B knobs of the photometric kernels (read once per process: a child process each)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import emu; emu.install(); import photometric_cases as PC; "
            "PC.run_knob_cases('cpu'); print('VARIANT OK')" % (os.path.dirname(here), here))
    cp = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **knobs), capture_output=True, text=True, timeout=900)
    assert cp.returncode == 0 and "VARIANT OK" in cp.stdout, cp.stdout[-3000:] + cp.stderr[-2000:]
