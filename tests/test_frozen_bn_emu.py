"""CPU: frozen BatchNorm folded into the convolutions of no-grad forward passes, through the interpreter build of the real
kernel sources (the same cases as test_frozen_bn_gpu.py; the encoders at a quarter of the GPU run's image, ResNet-18 only)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import emu
import frozen_bn_cases as FC
from improving_segmentation_with_selfsupervised_depth_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_fold_kernel():
    FC.run_fold_kernel("cpu")


def test_residual_epilogue_is_bit_exact():
    FC.run_residual_epilogue("cpu")


def test_residual_argument_validation_without_gpu():
    """the hipcc-built library, no launch"""
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    FC.run_residual_validation(_lib.bind(ctypes.CDLL(ge.LIB)))
    FC.run_residual_validation(_lib.lib())


def test_stem_bias_act():
    FC.run_stem_bias_act("cpu")


@pytest.mark.parametrize("name", sorted(FC.BLOCKS))
def test_block_error_gate(name):
    FC.run_block("cpu", name)


def test_encoder_r18_error_gate_and_coverage():
    FC.run_encoder("cpu", 18, size=(1, 3, 32, 64))


def test_switch_is_inert():
    FC.run_switch_is_inert("cpu")


def test_cache(monkeypatch):
    FC.run_cache("cpu", monkeypatch)


def test_environment_switch():
    """SEGSDE_FROZEN_BN_FOLD is read once at import: a fresh interpreter per value"""
    from conftest import REPO
    code = "from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn; print(Fn.FROZEN_BN_FOLD[0])"
    for val, want in (("1", "True"), ("0", "False"), (None, "False")):
        env = {k: v for k, v in os.environ.items() if k != "SEGSDE_FROZEN_BN_FOLD"}
        if val is not None:
            env["SEGSDE_FROZEN_BN_FOLD"] = val
        r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (val, r.stdout, r.stderr[-500:])
