"""GPU (-m gpu): the convolution routes, the glue kernels and the three concat sites of the models on channel-slice operands, real
libsegsde_hip.so against float64 torch (tests/pitched_cases.py).  With SEGSDE_PITCHED_REPORT=<path> the per-call records (route
taken, errors, bit identity) are written there as JSON at the end of the module: the source of profiles/pitched_operands.md."""
import os

import pytest
import torch

import pitched_cases as P
from improving_segmentation_with_selfsupervised_depth_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _real_lib():
    assert torch.cuda.is_available()
    L = _lib.lib()   # raises if libsegsde_hip.so is missing: there is no fallback
    assert not _lib.HOST_POINTERS_OK
    maps = open("/proc/self/maps").read()
    assert "libsegsde_hip.so" in maps, "native library not loaded"
    yield L
    path = os.environ.get("SEGSDE_PITCHED_REPORT")
    if path:
        P.dump(path)


@pytest.mark.parametrize("name", P.IGEMM + P.STENCIL)
def test_named_case(name):
    P.run_named_case(name, "cuda")


@pytest.mark.parametrize("shape", P.UPFOLD_SHAPES, ids=str)
def test_upfold(shape):
    P.run_upfold_case(shape, "cuda")


@pytest.mark.parametrize("shape", P.FUSED_SHAPES, ids=str)
def test_winograd_fused(shape):
    P.run_fused_case(shape, "cuda")


@pytest.mark.parametrize("shape", P.FUSED_REFLECT_SHAPES, ids=str)
def test_winograd_fused_mirrored_dgrad(shape):
    P.run_fused_reflect_case(shape, "cuda")


def test_winograd_fused_two_sources():
    P.run_fused2_case("cuda")


@pytest.mark.parametrize("shape", P.FUSED_WGRAD_SHAPES, ids=str)
def test_winograd_fused_wgrad(shape):
    P.run_fused_wgrad_case(shape, "cuda")


@pytest.mark.parametrize("shape", P.GROUPED_SHAPES, ids=str)
def test_winograd_grouped(shape):
    P.run_grouped_case(shape, "cuda")


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("which", ["fast_3x3", "wino"])
def test_operand_mode(which, mode):
    P.run_mode_case(which, mode, "cuda")


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("src,dst", P.RESIZES, ids=lambda s: "%dx%d" % s)
def test_resize(src, dst, ac):
    for C in P.GLUE_C:
        P.run_resize_case(src, dst, ac, C, "cuda")


@pytest.mark.parametrize("shape", P.GAP_SHAPES, ids=str)
def test_global_avgpool(shape):
    P.run_gap_case(shape, "cuda")


@pytest.mark.parametrize("C", P.GLUE_C)
def test_pointwise(C):
    P.run_pointwise_case(C, "cuda")


@pytest.mark.parametrize("widths", P.WIDTHS, ids=str)
@pytest.mark.parametrize("site", ["pose", "joint", "aspp"])
def test_site(site, widths, monkeypatch):
    """a .contiguous() in functional._c would make this fail: what reaches the kernels here must stay a slice.  At the ASPP site
    the slices arrive at bn_backward only (every branch ends in BatchNorm + ReLU): see pitched_cases.SPIED"""
    seen = P.install_spy(monkeypatch)
    sliced = P.run_site(site, widths, "cuda", seen)
    if widths == (8, 6, 3):
        assert any(s[2] != 0 for s in sliced), "no gradient slice off a 16-byte boundary: %s" % (sliced,)
