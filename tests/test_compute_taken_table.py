"""segsde_conv_compute_taken on a fixed table of descriptors: the answers of the launchers' dispatch (host only, nothing is launched,
no GPU needed).  EXPECTED was recorded from the library built at commit 458f705, before the decided experiment variants were
removed from the dispatch; `python tests/test_compute_taken_table.py [path/to/libsegsde_hip.so]` prints the table of a library."""
import ctypes
import os
import sys

from improving_segmentation_with_selfsupervised_depth_amd import _lib

ZERO, REFLECT, ADJOINT = 0, 1, 2
FWD, DGRAD, WGRAD, FOLD = 0, 1, 2, 4


def desc(B, H, W, C0, Cout, k, pad, pad_mode=ZERO, C1=0, up0=0, dil=1, in_div=1, sum2x2=0, Ho=None, Wo=None):
    Ho, Wo = H if Ho is None else Ho, W if Wo is None else Wo
    return dict(B=B, H=H, W=W, C0=C0, C1=C1, ld0=C0, ld1=C1, up0=up0, Ho=Ho, Wo=Wo, Cout=Cout, ldy=Cout, ldy2=0, nsplit=0, KH=k, KW=k,
                stride=1, dil=dil, pad=pad, pad_mode=pad_mode, in_div=in_div, act=0, sum2x2=sum2x2, accumulate=0)


# name -> (descriptor, directions asked)
CASES = {
    "plain 3x3 64->64": (desc(2, 16, 32, 64, 64, 3, 1), (FWD, DGRAD, WGRAD)),
    "1x1 64->128": (desc(2, 16, 32, 64, 128, 1, 0), (FWD, DGRAD, WGRAD)),
    "reflect 3x3 64->64": (desc(2, 16, 32, 64, 64, 3, 1, REFLECT), (FWD, WGRAD)),
    "dilated 3x3 rate 6 256->256 (dead tap rows)": (desc(2, 32, 64, 256, 256, 3, 6, dil=6), (FWD, DGRAD, WGRAD)),
    "reflect adjoint, small map (in-kernel for fp32)": (desc(2, 16, 32, 64, 64, 3, 1, ADJOINT), (DGRAD,)),
    "reflect adjoint, 2^21 pixels (border launches)": (desc(16, 256, 512, 64, 32, 3, 1, ADJOINT), (DGRAD,)),
    "reflect adjoint, 2 rows (in-kernel only)": (desc(2, 2, 32, 64, 64, 3, 1, ADJOINT), (DGRAD,)),
    "reflect adjoint + 2x2 sum (in-kernel only)": (desc(2, 16, 32, 64, 64, 3, 1, ADJOINT, sum2x2=1), (DGRAD,)),
    "stride-2 data-gradient (parity classes)": (desc(2, 8, 16, 64, 64, 3, 1, in_div=2, Ho=16, Wo=32), (DGRAD,)),
    "upsample-folded [up(64) | 32] -> 64": (desc(2, 16, 32, 64, 64, 3, 1, REFLECT, C1=32, up0=1),
                                            (FWD, WGRAD, FWD | FOLD, DGRAD | FOLD, WGRAD | FOLD)),
    "two sources [64 | 64] -> 64": (desc(2, 16, 32, 64, 64, 3, 1, C1=64), (FWD, WGRAD)),
    "two sources [48 | 32] -> 64 (concat boundary off the chunk grid)": (desc(2, 16, 32, 48, 64, 3, 1, C1=32), (FWD, WGRAD)),
    "24 -> 40 (not a fast-path shape)": (desc(2, 16, 32, 24, 40, 3, 1), (FWD, DGRAD, WGRAD)),
    "6 -> 10 (scalar gathers)": (desc(2, 16, 32, 6, 10, 3, 1), (FWD, DGRAD, WGRAD)),
    "64 -> 64 on 24-pixel rows (weight gradient off the table loader)": (desc(2, 16, 24, 64, 64, 3, 1), (FWD, WGRAD)),
    "disparity head 64 -> 1 (stencil route)": (desc(2, 16, 32, 64, 1, 3, 1, REFLECT), (FWD, WGRAD)),
    "7x7 64->64 (49 taps: off the tap table)": (desc(2, 16, 32, 64, 64, 7, 3), (FWD, WGRAD)),
}

# name -> {direction: [answer for compute = 0, 1, 2]}
EXPECTED = {
    'plain 3x3 64->64': {0: [0, 1, 2], 1: [0, 1, 2], 2: [0, 1, 2]},
    '1x1 64->128': {0: [0, 1, 2], 1: [0, 1, 2], 2: [0, 1, 2]},
    'reflect 3x3 64->64': {0: [0, 1, 2], 2: [0, 1, 2]},
    'dilated 3x3 rate 6 256->256 (dead tap rows)': {0: [0, 1, 2], 1: [0, 1, 2], 2: [0, 1, 2]},
    'reflect adjoint, small map (in-kernel for fp32)': {1: [0, 1, 2]},
    'reflect adjoint, 2^21 pixels (border launches)': {1: [0, 1, 2]},
    'reflect adjoint, 2 rows (in-kernel only)': {1: [0, 0, 0]},
    'reflect adjoint + 2x2 sum (in-kernel only)': {1: [0, 0, 0]},
    'stride-2 data-gradient (parity classes)': {1: [0, 1, 2]},
    'upsample-folded [up(64) | 32] -> 64': {0: [0, 1, 2], 2: [0, 1, 2], 4: [0, 1, 2], 5: [0, 0, 0], 6: [0, 0, 0]},
    'two sources [64 | 64] -> 64': {0: [0, 1, 2], 2: [0, 1, 2]},
    'two sources [48 | 32] -> 64 (concat boundary off the chunk grid)': {0: [0, 0, 0], 2: [0, 1, 2]},
    '24 -> 40 (not a fast-path shape)': {0: [0, 0, 0], 1: [0, 0, 0], 2: [0, 1, 2]},
    '6 -> 10 (scalar gathers)': {0: [0, 0, 0], 1: [0, 0, 0], 2: [0, 0, 0]},
    '64 -> 64 on 24-pixel rows (weight gradient off the table loader)': {0: [0, 1, 2], 2: [0, 0, 0]},
    'disparity head 64 -> 1 (stencil route)': {0: [0, 0, 0], 2: [0, 0, 0]},
    '7x7 64->64 (49 taps: off the tap table)': {0: [0, 0, 0], 2: [0, 1, 2]},
}


def compute_table(cdll):
    out = {}
    for name, (fields, dirs) in CASES.items():
        out[name] = {}
        for direction in dirs:
            row = []
            for compute in (0, 1, 2):
                d = _lib.ConvDesc(compute=compute, **fields)
                row.append(int(cdll.segsde_conv_compute_taken(ctypes.byref(d), direction)))
            out[name][direction] = row
    return out


def test_compute_taken_table():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    got = compute_table(_lib.bind(ctypes.CDLL(ge.LIB)))
    assert set(EXPECTED) == set(CASES)
    for name in CASES:
        assert got[name] == EXPECTED[name], (name, got[name], EXPECTED[name])
    # the table does exercise every answer
    assert {v for rows in EXPECTED.values() for r in rows.values() for v in r} == {0, 1, 2}


if __name__ == "__main__":
    import pprint
    pprint.pprint(compute_table(_lib.bind(ctypes.CDLL(os.path.abspath(sys.argv[1])))), width=140, sort_dicts=False)
