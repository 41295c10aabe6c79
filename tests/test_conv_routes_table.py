"""The convolution route plan (hipops.forward_routes / backward_routes) on a fixed table of layers: every plan field, the public
gate predicates that are views of the plan (forward and dgrad=True) and the two shape-free pre-pack predicates, under the default
gate constants and with the size floors WINOGRAD_MIN_MACS, UPFOLD_MIN_SAVED_MACS and WINO_FUSED_REFLECT_DGRAD_MIN_PIX at 0.  Host
only: nothing is launched, no GPU needed.  EXPECTED was recorded from the predicates of commit 17f834c, the last one where
functional.py, hipops.py and models/layers.py each asked them on their own; `python tests/test_conv_routes_table.py` prints the
table of the checked-out code."""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script; under pytest conftest.py has done it)
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H  # noqa: E402

FLOORS = ("WINOGRAD_MIN_MACS", "UPFOLD_MIN_SAVED_MACS", "WINO_FUSED_REFLECT_DGRAD_MIN_PIX")

# name -> (ConvGeom arguments, ConvGeom.compute, (B, H, W) of the virtual input)
CASES = {
    "3x3 64->64 zero-padded @1x8x16": (dict(C0=64, Cout=64, k=3, pad=1), 0, (1, 8, 16)),
    "3x3 64->64 mirrored @1x8x16": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True), 0, (1, 8, 16)),
    "3x3 512->512 @1x8x8": (dict(C0=512, Cout=512, k=3, pad=1), 0, (1, 8, 8)),
    "3x3 256->256 @1x8x8": (dict(C0=256, Cout=256, k=3, pad=1), 0, (1, 8, 8)),
    "dilated 3x3 256->256 d=2 @1x8x8": (dict(C0=256, Cout=256, k=3, dil=2, pad=2), 0, (1, 8, 8)),
    "two sources [128|128]->256 mirrored @1x8x16": (dict(C0=128, Cout=256, k=3, pad=1, reflect=True, C1=128), 0, (1, 8, 16)),
    "[up(64)|64]->64 mirrored @1x16x32": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True, C1=64, up0=True), 0, (1, 16, 32)),
    "[up(64)|0]->64 mirrored @1x16x32": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True, up0=True), 0, (1, 16, 32)),
    "[up(64)|32]->64 mirrored @1x16x32": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True, C1=32, up0=True), 0, (1, 16, 32)),
    "[up(256)|256]->256 mirrored @16x64x128": (dict(C0=256, Cout=256, k=3, pad=1, reflect=True, C1=256, up0=True), 0, (16, 64, 128)),
    "3x3 64->64 zero-padded, odd map @1x7x16": (dict(C0=64, Cout=64, k=3, pad=1), 0, (1, 7, 16)),
    "3x3 64->64 mirrored @1x6x4": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True), 0, (1, 6, 4)),
    "1x1 64->128 @1x8x16": (dict(C0=64, Cout=128, k=1), 0, (1, 8, 16)),
    "stride-2 3x3 64->128 @1x8x16": (dict(C0=64, Cout=128, k=3, stride=2, pad=1), 0, (1, 8, 16)),
    "7x7 s2 stem, 4 channels carrying 3 @1x16x32": (dict(C0=4, Cout=64, k=7, stride=2, pad=3, cin_alg=3), 0, (1, 16, 32)),
    "3x3 64->1 mirrored @1x8x16": (dict(C0=64, Cout=1, k=3, pad=1, reflect=True), 0, (1, 8, 16)),
    "3x3 64->64 mirrored, fp16 operands @16x64x128": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True), 1, (16, 64, 128)),
    "3x3 64->64 mirrored, split bf16 @16x64x128": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True), 2, (16, 64, 128)),
    "[up(64)|64]->64 mirrored, fp16 operands @1x16x32": (dict(C0=64, Cout=64, k=3, pad=1, reflect=True, C1=64, up0=True), 1, (1, 16, 32)),
}

FORWARD = ("fused", "grouped", "upfold", "dgrad2", "kn_pack")
BACKWARD = ("dgrad_fused", "dgrad_grouped", "dgrad2", "wgrad_fused", "wgrad_grouped", "wgrad_upfold")
PREDICATES = ("winograd_ok", "winograd_ok dgrad", "winograd_fused_ok", "winograd_fused_ok dgrad", "winograd_fused_dgrad2_ok",
              "winograd_fused_wgrad_ok", "upfold_ok",
              # (the same seven asked without a map: the shape-free halves)
              "winograd_ok -", "winograd_ok dgrad -", "winograd_fused_ok -", "winograd_fused_ok dgrad -", "winograd_fused_dgrad2_ok -",
              "winograd_fused_wgrad_ok -", "upfold_ok -", "winograd_static_ok", "winograd_fused_static_ok")
COLUMNS = tuple("forward." + f for f in FORWARD) + tuple("backward." + f for f in BACKWARD) + PREDICATES

# name -> (answers under the default constants, answers with the size floors at 0), one character per entry of COLUMNS
EXPECTED = {
    '3x3 64->64 zero-padded @1x8x16': ('000000000000000000001101001', '100011001000011010001101001'),
    '3x3 64->64 mirrored @1x8x16': ('000000000000000000001101001', '100011001000011010001101001'),
    '3x3 512->512 @1x8x8': ('010000100101100000110000010', '010000100101100000110000010'),
    '3x3 256->256 @1x8x8': ('000000000000000000111101011', '110011101101111010111101011'),
    'dilated 3x3 256->256 d=2 @1x8x8': ('000000000000000000110000010', '010000100101100000110000010'),
    'two sources [128|128]->256 mirrored @1x8x16': ('000000000000000000100000011', '010000000101000000100000011'),
    '[up(64)|64]->64 mirrored @1x16x32': ('000000000000000000001011101', '101110011010010111001011101'),
    '[up(64)|0]->64 mirrored @1x16x32': ('000000000000000000000001101', '001000001010000011000001101'),
    '[up(64)|32]->64 mirrored @1x16x32': ('000000000000000000000001100', '001000001010000011000001100'),
    '[up(256)|256]->256 mirrored @16x64x128': ('101110011010010111001011111', '101110011010010111001011111'),
    '3x3 64->64 zero-padded, odd map @1x7x16': ('000000000000000000001101001', '000000000000000000001101001'),
    '3x3 64->64 mirrored @1x6x4': ('000000000000000000001101001', '100011001000011010001101001'),
    '1x1 64->128 @1x8x16': ('000000000000000000000000000', '000000000000000000000000000'),
    'stride-2 3x3 64->128 @1x8x16': ('000000000000000000000000000', '000000000000000000000000000'),
    '7x7 s2 stem, 4 channels carrying 3 @1x16x32': ('000000000000000000000000000', '000000000000000000000000000'),
    '3x3 64->1 mirrored @1x8x16': ('000000000000000000000000000', '000000000000000000000000000'),
    '3x3 64->64 mirrored, fp16 operands @16x64x128': ('000000000000000000000000001', '000000000000000000000000001'),
    '3x3 64->64 mirrored, split bf16 @16x64x128': ('100011001000011010001101001', '100011001000011010001101001'),
    '[up(64)|64]->64 mirrored, fp16 operands @1x16x32': ('000000000000000000000000101', '001000000010000001000000101'),
}


def geom(name):
    kw, compute, _ = CASES[name]
    g = H.ConvGeom(**kw)
    g.compute = compute
    return g


def module_like(g):
    """what the shape-free predicates read of the nn.Conv2d that owns convolution g"""
    return types.SimpleNamespace(kernel_size=(g.k, g.k), stride=(g.stride, g.stride), padding=(g.pad, g.pad), dilation=(g.dil, g.dil),
                                 in_channels=g.CinAlg, out_channels=g.Cout, reflect=g.reflect)


def predicate_row(name):
    g, (B, Hh, W) = geom(name), CASES[name][2]
    m = module_like(g)
    return (H.winograd_ok(g, B, Hh, W), H.winograd_ok(g, B, Hh, W, dgrad=True), H.winograd_fused_ok(g, B, Hh, W),
            H.winograd_fused_ok(g, B, Hh, W, dgrad=True), H.winograd_fused_dgrad2_ok(g, B, Hh, W), H.winograd_fused_wgrad_ok(g, B, Hh, W),
            H.upfold_ok(g, B * Hh * W), H.winograd_ok(g), H.winograd_ok(g, dgrad=True), H.winograd_fused_ok(g),
            H.winograd_fused_ok(g, dgrad=True), H.winograd_fused_dgrad2_ok(g), H.winograd_fused_wgrad_ok(g), H.upfold_ok(g),
            H.winograd_static_ok(m), H.winograd_fused_static_ok(m))


def plan_row(name):
    g, (B, Hh, W) = geom(name), CASES[name][2]
    f, b = H.forward_routes(g, B, Hh, W), H.backward_routes(g, B, Hh, W)
    return tuple(getattr(f, n) for n in FORWARD) + tuple(getattr(b, n) for n in BACKWARD)


def table(row):
    """name -> (row under the default constants, row with the floors at 0) as strings of 0 / 1"""
    out = {}
    old = {n: getattr(H, n) for n in FLOORS}
    try:
        for name in CASES:
            both = []
            for zero in (False, True):
                for n in FLOORS:
                    setattr(H, n, 0 if zero else old[n])
                r = row(name)
                assert all(v is True or v is False for v in r), (name, r)
                both.append("".join("01"[v] for v in r))
            out[name] = tuple(both)
    finally:
        for n in FLOORS:
            setattr(H, n, old[n])
    return out


def _lib_ready():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()


def test_conv_routes_table():
    _lib_ready()       # (the one-kernel routes ask the library which maps its tiling takes: segsde_winograd_fused_ok)
    assert set(EXPECTED) == set(CASES)
    got = table(lambda name: plan_row(name) + predicate_row(name))
    for name in CASES:
        for which, g_, e_ in zip(("default constants", "floors at 0"), got[name], EXPECTED[name]):
            assert len(e_) == len(COLUMNS)
            wrong = [c for c, a, b in zip(COLUMNS, g_, e_) if a != b]
            assert not wrong, (name, which, wrong, g_, e_)
    # a forward without gradients (skip_grad=False) asks no backward gate: no dgrad2, the pack layout follows the forward alone,
    # the forward's own answers are unchanged
    for zero in (False, True):
        saved = {n: getattr(H, n) for n in FLOORS}
        try:
            for n in FLOORS:
                setattr(H, n, 0 if zero else saved[n])
            for name in CASES:
                g, (B, Hh, W) = geom(name), CASES[name][2]
                full, nograd = H.forward_routes(g, B, Hh, W), H.forward_routes(g, B, Hh, W, skip_grad=False)
                assert nograd.dgrad2 is False and nograd.kn_pack is nograd.fused, (name, nograd)
                assert nograd[:3] == full[:3], (name, full, nograd)
        finally:
            for n in FLOORS:
                setattr(H, n, saved[n])
    # the table does exercise both answers of every plan field
    for i, c in enumerate(COLUMNS[:len(FORWARD) + len(BACKWARD)]):
        assert {r[i] for rows in EXPECTED.values() for r in rows} == {"0", "1"}, c


if __name__ == "__main__":
    _lib_ready()
    for name_, rows_ in table(lambda name: plan_row(name) + predicate_row(name)).items():
        print("    %r: %r," % (name_, rows_))
