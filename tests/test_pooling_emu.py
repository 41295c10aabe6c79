"""CPU: max-pool, nearest x2 upsampling, bilinear resize, global average pool, gate, axpby, channel copies and the NCHW <-> NHWC
edges against the float64 oracle, and the operand contract of their wrappers, through the interpreter build of the real kernel
sources (tests/pooling_cases.py; the -m gpu file runs the same cases on the real library).  The interpreter finishes each of the
grid-stride cases (more than 8192 x 256 threads) in about a second, so all of them run here too."""
import pytest
import torch

import emu
import pooling_cases as PC


@pytest.fixture(scope="module", autouse=True)
def _emu():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


def test_recorded_seeds_are_the_first_that_fit():
    """float64 only: every seed in PC.SEEDS gives its lattice input the asserted share of tied windows and no smaller one does"""
    for key, seed in PC.SEEDS.items():
        assert PC.seed_fits(key, seed) and not any(PC.seed_fits(key, s) for s in range(seed)), key


def test_operand_contract():
    PC.run_operand_contract("cpu")


@pytest.mark.parametrize("kind", PC.MAXPOOL_KINDS)
@pytest.mark.parametrize("shape", PC.MAXPOOL_SHAPES, ids=PC._name)
def test_maxpool(shape, kind):
    PC.run_maxpool("cpu", shape, kind)


def test_maxpool_nonfinite():
    PC.run_maxpool_nonfinite("cpu")


@pytest.mark.parametrize("shape", PC.UPSAMPLE_SHAPES, ids=PC._name)
def test_upsample2x(shape):
    PC.run_upsample2x("cpu", shape)


@pytest.mark.parametrize("C", PC.RESIZE_C)
@pytest.mark.parametrize("index", range(len(PC.RESIZE_CASES)), ids=["%dx%d-%dx%d-%s" % (s + d + ("ac" if a else "hp",)) for s, d, a in PC.RESIZE_CASES])
def test_resize(index, C):
    PC.run_resize("cpu", index, C)


@pytest.mark.parametrize("shape", PC.GAP_SHAPES, ids=PC._name)
def test_global_avgpool(shape):
    PC.run_gap("cpu", shape)


def test_global_avgpool_pitched():
    PC.run_gap("cpu", PC.GAP_PITCHED, pitched=True)


@pytest.mark.parametrize("n", PC.GATE_N)
def test_gate(n):
    PC.run_gate("cpu", n)


def test_gate_function():
    PC.run_gate_function("cpu")


@pytest.mark.parametrize("C,pad_to", PC.LAYOUT_CP)
def test_nchw_to_nhwc(C, pad_to):
    PC.run_nchw_to_nhwc("cpu", C, pad_to)


@pytest.mark.parametrize("shape", PC.STEM_SHAPES, ids=PC._name)
def test_stem_input(shape):
    PC.run_stem_input("cpu", shape)


@pytest.mark.parametrize("shape", PC.TO_NCHW_SHAPES, ids=PC._name)
def test_nhwc_to_nchw(shape):
    PC.run_nhwc_to_nchw("cpu", shape)


@pytest.mark.parametrize("n", PC.AXPBY_N)
def test_axpby(n):
    PC.run_axpby("cpu", n)


@pytest.mark.parametrize("C", PC.COPY_C)
def test_copy_channels(C):
    PC.run_copy_channels("cpu", C)


@pytest.mark.parametrize("name", list(PC.GRID_STRIDE))
def test_grid_stride(name):
    PC.run_grid_stride("cpu", name)
