"""GPU (-m gpu): max-pool, nearest x2 upsampling, bilinear resize, global average pool, gate, axpby, channel copies and the
NCHW <-> NHWC edges against the float64 oracle at ragged, degenerate, misaligned and grid-stride shapes, and the operand contract of
their wrappers (tests/pooling_cases.py; the figures of a run are in profiles/pooling_edges.md)."""
import pytest

import pooling_cases as PC

pytestmark = pytest.mark.gpu


def test_operand_contract():
    """every wrapper with all read operands strided at once equals the call on held contiguous clones bit for bit and leaves the
    operands and the buffers around them alone; a float64 read operand raises TypeError; a strided written buffer raises ValueError
    and nothing is written"""
    PC.run_operand_contract("cuda")


@pytest.mark.parametrize("kind", PC.MAXPOOL_KINDS)
@pytest.mark.parametrize("shape", PC.MAXPOOL_SHAPES, ids=PC._name)
def test_maxpool(shape, kind):
    """strictly negative, normal, lattice (exact ties) and constant inputs: forward, backward with integer-valued dy and the
    accumulating backward bit-equal to float64 F.max_pool2d and its autograd gradient; bit-identical again with x / dy 4 bytes off
    16-byte alignment and idx one byte off 4-byte alignment (the scalar kernels)"""
    PC.run_maxpool("cuda", shape, kind)


def test_maxpool_nonfinite():
    """one NaN, one +inf, a whole -inf channel: compared after nan_to_num with three distinct sentinels"""
    PC.run_maxpool_nonfinite("cuda")


@pytest.mark.parametrize("shape", PC.UPSAMPLE_SHAPES, ids=PC._name)
def test_upsample2x(shape):
    """the C entry points as _UpsampleFn calls them, channel slices of wider buffers, and upsample() on NCHW under autograd"""
    PC.run_upsample2x("cuda", shape)


@pytest.mark.parametrize("C", PC.RESIZE_C)
@pytest.mark.parametrize("index", range(len(PC.RESIZE_CASES)), ids=["%dx%d-%dx%d-%s" % (s + d + ("ac" if a else "hp",)) for s, d, a in PC.RESIZE_CASES])
def test_resize(index, C):
    """3 -> 17, 64 -> 3, one row, one column, an output of 1 with align_corners, one axis only, the 1x1 source (both sum kernels)"""
    PC.run_resize("cuda", index, C)


@pytest.mark.parametrize("shape", PC.GAP_SHAPES, ids=PC._name)
def test_global_avgpool(shape):
    """|y - f64| <= 2^-23 |f64|, |dx - f64| <= 2^-22 |f64|; 11 slices, 256 slices with the last one empty, ragged 64-channel slabs"""
    PC.run_gap("cuda", shape)


def test_global_avgpool_pitched():
    PC.run_gap("cuda", PC.GAP_PITCHED, pitched=True)


@pytest.mark.parametrize("n", PC.GATE_N)
def test_gate(n):
    """+-20 and +-90 planted in the gate's argument (expf overflows at 90)"""
    PC.run_gate("cuda", n)


def test_gate_function():
    PC.run_gate_function("cuda")


@pytest.mark.parametrize("C,pad_to", PC.LAYOUT_CP)
def test_nchw_to_nhwc(C, pad_to):
    """both code paths; the padded channels are +0.0 on an allocation poisoned beforehand"""
    PC.run_nchw_to_nhwc("cuda", C, pad_to)


@pytest.mark.parametrize("shape", PC.STEM_SHAPES, ids=PC._name)
def test_stem_input(shape):
    """interior bit-equal to nchw_to_nhwc, the border (3 above / below, 3 left, 5 right) exactly zero on a poisoned allocation"""
    PC.run_stem_input("cuda", shape)


@pytest.mark.parametrize("shape", PC.TO_NCHW_SHAPES, ids=PC._name)
def test_nhwc_to_nchw(shape):
    PC.run_nhwc_to_nchw("cuda", shape)


@pytest.mark.parametrize("n", PC.AXPBY_N)
def test_axpby(n):
    """axpby and axpby_dev with and without y, out= written in place; device scalars that do not start their allocation"""
    PC.run_axpby("cuda", n)


@pytest.mark.parametrize("C", PC.COPY_C)
def test_copy_channels(C):
    PC.run_copy_channels("cuda", C)


@pytest.mark.parametrize("name", list(PC.GRID_STRIDE))
def test_grid_stride(name):
    """one case per kernel whose thread count is just above 8192 x 256 and no multiple of 256: the grid-stride loop runs"""
    PC.run_grid_stride("cuda", name)
