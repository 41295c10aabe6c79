"""CPU: channel-slice operands (tests/pitched_cases.py) with the kernels run by the interpreter build of the real sources: one case
per convolution route at the two placements whose base is off a 16-byte boundary (P2: pitch a multiple of 4, base at 8 mod 16; P3:
odd pitch, base at 12 mod 16), all operands sliced together, the glue kernels, and the three concat sites of the models end to end.
The interpreter runs 16-byte accesses, LDS staging and LDS-DMA as plain loads: this file checks the index arithmetic and the
dispatch; what the code objects do with such addresses is test_pitched_gpu.py's subject (every placement, every case)."""
import pytest
import torch

import emu
import pitched_cases as P

FEW = dict(placements=("P2", "P3"), together_only=True)


@pytest.fixture(scope="module")
def interp():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the -m gpu suite exercises the real library instead")
    emu.install()


@pytest.mark.parametrize("name", ["3x3_zero", "1x1", "fast_3x3", "disp_c128_tiny", "head_c64_19"])
def test_named_case(interp, name):
    """scalar gather, float4 gather, LDS-DMA fast path, stencil, skinny"""
    P.run_named_case(name, "cpu", **FEW)


def test_upfold(interp):
    """the shape whose weight gradient takes the folded route too (parity-class rows 32 pixels wide)"""
    P.run_upfold_case(P.UPFOLD_SHAPES[2], "cpu", **FEW)


def test_winograd_fused(interp):
    P.run_fused_case(P.FUSED_SHAPES[0], "cpu", **FEW)


def test_winograd_fused_mirrored_dgrad(interp):
    P.run_fused_reflect_case(P.FUSED_REFLECT_SHAPES[0], "cpu", **FEW)


@pytest.mark.parametrize("mode", P.MODES)
def test_operand_mode(interp, mode):
    P.run_mode_case("fast_3x3", mode, "cpu", **FEW)


def test_winograd_fused_two_sources(interp):
    P.run_fused2_case("cpu", **FEW)


def test_winograd_fused_wgrad(interp):
    P.run_fused_wgrad_case(P.FUSED_WGRAD_SHAPES[0], "cpu", **FEW)


def test_winograd_grouped(interp):
    P.run_grouped_case(P.GROUPED_SHAPES[0], "cpu", **FEW)


def test_glue(interp):
    for src, dst in P.RESIZES:
        for ac in (False, True):
            P.run_resize_case(src, dst, ac, 8 if src == (1, 1) else 5, "cpu")
    for shape in P.GAP_SHAPES:
        P.run_gap_case(shape, "cpu")
    for C in P.GLUE_C:
        P.run_pointwise_case(C, "cpu")


@pytest.mark.parametrize("widths", P.WIDTHS, ids=str)
@pytest.mark.parametrize("site", ["pose", "joint", "aspp"])
def test_site(interp, site, widths, monkeypatch):
    """a .contiguous() in functional._c would make this fail: what reaches the kernels here must stay a slice.  At the ASPP site
    the slices arrive at bn_backward only (every branch ends in BatchNorm + ReLU): see pitched_cases.SPIED"""
    seen = P.install_spy(monkeypatch)
    sliced = P.run_site(site, widths, "cpu", seen)
    if widths == (8, 6, 3):
        assert any(s[2] != 0 for s in sliced), "no gradient slice off a 16-byte boundary: %s" % (sliced,)


def test_slab_and_rule():
    """the helper itself: poison scale, bit-exact guard, and that the sweep notices a stray read, a write into the buffer and a
    route that fell back (no kernel involved)"""
    t = torch.randn(2, 3, 4, 5)
    s = P.slab(t, 3, 2)
    buf = s._slab[0]
    assert buf.shape == (2, 3, 4, 10) and torch.equal(s, t) and s.data_ptr() == buf.data_ptr() + 12 and P.intact(s)
    rest = torch.cat([buf[..., :3], buf[..., 8:]], -1)
    assert bool(torch.isfinite(rest).all()) and 300 < float(rest.abs().mean()) / float(t.abs().mean()) < 3000
    buf[0, 0, 0, 0] = -buf[0, 0, 0, 0]
    assert not P.intact(s)
    assert P.placement("P4", 19) == (19, 19) and P.placement("P2", 19) == (2, 2)
    want = [t.double().sum(-1)]
    P.sweep("selftest", "sum", lambda o, n: (o["x"].sum(-1),), dict(x=t), ("x",), want)
    with pytest.raises(AssertionError, match="max error"):
        P.sweep("selftest", "stray read", lambda o, n: ((o["x"] + (o["x"]._slab[0][..., :1] if hasattr(o["x"], "_slab") else 0)).sum(-1),),
                dict(x=t), ("x",), want)
    with pytest.raises(AssertionError, match="was written"):
        def writes(o, n):
            if hasattr(o["x"], "_slab"):
                o["x"]._slab[0][..., -1] = 0.0
            return (o["x"].sum(-1),)
        P.sweep("selftest", "write", writes, dict(x=t), ("x",), want)
    with pytest.raises(AssertionError, match="route record"):
        def falls_back(o, n):
            if o["x"].is_contiguous():
                P.H.UPFOLD_TAKEN["fwd"] += 1
            return (o["x"].sum(-1),)
        P.sweep("selftest", "fallback", falls_back, dict(x=t), ("x",), want)
    with pytest.raises(AssertionError, match="did not take its route"):
        P.sweep("selftest", "named route", lambda o, n: (o["x"].sum(-1),), dict(x=t), ("x",), want, expect=("upfold.wgrad",))
    with pytest.raises(AssertionError, match="not bit-identical"):
        P.sweep("selftest", "identical", lambda o, n: ((o["x"] * (1.0 if o["x"].is_contiguous() else 1.0 + 2.0 ** -23)).sum(-1),),
                dict(x=t), ("x",), want, identical=("P1",))
    del P.RECORDS[[i for i, r in enumerate(P.RECORDS) if r["case"] == "selftest"][0]:]
