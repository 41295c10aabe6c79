"""The plumbing kernels of csrc/elementwise.hip that sit between the layers of both networks -- max-pool 3x3 / 2 / 1, nearest x2
upsampling, bilinear resize, global average pool, the attention gate, axpby, channel-slice copies and the NCHW <-> NHWC edges --
against a float64 evaluation of the same operation, at the shapes and values where such kernels go wrong (negative and non-finite
inputs under the pool's padding, exact ties, maps of one or two pixels, strongly non-integer resize ratios, an empty last slice of
the sliced average pool, the 16- and 4-byte alignment fall-backs, more than 8192 x 256 threads: the grid-stride loop), and the
operand contract of their Python wrappers (``run_operand_contract``).  Shared by tests/test_pooling_gpu.py (real library) and
tests/test_pooling_emu.py (interpreter build of the same sources).

References are plain torch on the CPU and call nothing of the package: F.max_pool2d, F.interpolate, mean and sigmoid under float64
autograd (the truth) and, where a comparison is not exact, the same expression in float32 (what plain fp32 arithmetic achieves).
One rule for the inexact comparisons (tests/photometric_cases.py)

    max|kernel - f64| <= 3 * max|fp32 oracle - f64| + 1e-6 * max|f64|

plus the two derived bounds of the average pool: the forward sums in double and rounds once, |got - f64| <= 2^-23 |f64| (half a unit
of rounding, doubled for the re-associated double sum); the backward computes dy * (1.f / HW), two roundings,
|got - f64| <= 2^-22 |f64|.  Everything else is compared bit for bit: selections, copies, and sums of integer-valued gradients,
which are exact in any order."""
import functools

import torch
import torch.nn.functional as F

from improving_segmentation_with_selfsupervised_depth_amd import _lib, functional as Fn, hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.models import monodepth_layers as ML

RECORDS = []            # (kernel, case, tensor, e_kernel, bound, share of the bound, ok)
NOTES = []              # (kind, text)

# ---------------------------------------------------------------------------------------------------------------- the cases
MAXPOOL_SHAPES = [(2, 9, 11, 8), (2, 9, 11, 6), (1, 1, 1, 4), (1, 1, 7, 4), (2, 5, 1, 6), (1, 2, 2, 8), (1, 8, 8, 4), (3, 7, 10, 12)]   # B,H,W,C
MAXPOOL_KINDS = ("negative", "randn", "lattice", "constant")
TIE_SHARE = 0.30        # lattice inputs: share of the windows of more than one pixel whose maximum is attained twice
# found by find_seeds() from float64 alone: the first seed at which the lattice input of the shape has that share of tied windows
# (1x1x1x4 has no window of more than one pixel: nothing to tie, any seed fits)
SEEDS = {"2x9x11x8": 0, "2x9x11x6": 0, "1x1x1x4": 0, "1x1x7x4": 67, "2x5x1x6": 227, "1x2x2x8": 4, "1x8x8x4": 0, "3x7x10x12": 0}
UPSAMPLE_SHAPES = [(1, 1, 1, 1), (2, 3, 7, 5), (1, 4, 2, 8)]            # B,h,w,C
RESIZE_CASES = [((3, 5), (17, 9), False), ((7, 3), (64, 5), True), ((64, 48), (3, 5), False), ((1, 6), (4, 13), False),
                ((6, 1), (5, 1), True), ((2, 2), (1, 1), True), ((5, 9), (5, 20), False), ((9, 9), (1, 1), False),
                ((33, 17), (16, 8), True), ((4, 8), (8, 16), False), ((1, 1), (6, 9), False), ((1, 1), (6, 9), True)]
RESIZE_C = (5, 8)
GAP_SHAPES = [(3, 70, 5, 6), (1, 20, 37, 41), (3, 72, 5, 6), (1, 4, 200, 200), (1, 3, 200, 200), (2, 130, 3, 3), (2, 132, 3, 3),
              (1, 1, 1, 1), (2, 8, 1, 1)]                               # B,C,H,W
GAP_PITCHED = (3, 72, 5, 6)                                             # C % 4 == 0 behind a pitch of C + 3
GATE_N = (1, 255, 257)
GATE_PLANTED = (20.0, -20.0, 90.0, -90.0)                               # expf overflows at 90
LAYOUT_CP = [(3, 4), (6, 8), (4, 4), (8, 1), (5, 1), (5, 4), (9, 4), (1, 1)]    # (C, pad_to) at (B,H,W) = (2,5,7)
LAYOUT_NORM = [(0.45, 0.225), (0.0, 1.0)]
STEM_SHAPES = [(1, 3, 2, 2), (2, 6, 5, 7)]
TO_NCHW_SHAPES = [(1, 1, 1, 1), (2, 7, 3, 5)]                           # B,H,W,C
AXPBY_N = (1, 1000)
COPY_C = (1, 3, 4, 6)
EW_CAP = 8192 * 256     # ew_blocks() caps the grid at 8192 blocks of 256: above this many threads the grid-stride loop runs


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(gen, shape, lo=-8, hi=8):
    """integer-valued float32 in [lo, hi]: sums of a few of them are exact in any order"""
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _name(shape):
    return "x".join(str(int(s)) for s in shape)


# ----------------------------------------------------------------------------------------------------------------- comparison
def _record(kernel, case, name, e_k, e_o, sc, bound, ok):
    share = e_k / bound if bound > 0 else 0.0
    RECORDS.append((kernel, case, name, e_k, bound, share, ok))
    print("POOL-EDGE | %s | %s | %s | %.3e | %.3e | %.3e | %.3f | %s" % (kernel, case, name, e_k, e_o, sc, share, "ok" if ok else "MISSES"))
    return ok


def check(kernel, case, name, got, r32, r64):
    """the rule; -> whether the kernel is bit-identical to the fp32 oracle"""
    g, a, b = got.detach().double().cpu().reshape(r64.shape), r32.detach().double().cpu(), r64.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), (case, name, "not finite")
    e_k, e_o, sc = float((g - b).abs().max()), float((a - b).abs().max()), float(b.abs().max())
    bound = 3 * e_o + 1e-6 * sc
    _record(kernel, case, name, e_k, e_o, sc, bound, e_k <= bound)
    return bool(torch.equal(g, a))


def exact(kernel, case, name, got, r64):
    """bit for bit against float64 (selections, copies, sums of integers)"""
    g, b = got.detach().double().cpu().reshape(r64.shape), r64.detach().double().cpu()
    ok = bool(torch.equal(g, b))
    _record(kernel, case, name + " (exact)", float((g - b).abs().nan_to_num(nan=float("inf")).max()) if g.numel() else 0.0, 0.0,
            float(b.abs().max()) if b.numel() else 0.0, 0.0, ok)
    return ok


def relative(kernel, case, name, got, r64, rel):
    """|got - f64| <= rel * |f64| element by element (the derived bounds of the average pool)"""
    g, b = got.detach().double().cpu().reshape(r64.shape), r64.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), (case, name, "not finite")
    err, lim = (g - b).abs(), rel * b.abs()
    share = float((err / lim.clamp_min(1e-300)).max())
    ok = bool((err <= lim).all())
    RECORDS.append((kernel, case, name, float(err.max()), float(lim.max()), share, ok))
    print("POOL-EDGE | %s | %s | %s | %.3e | 2^%d relative | %.3e | %.3f | %s" % (
        kernel, case, name, float(err.max()), round(torch.log2(torch.tensor(rel)).item()), float(b.abs().max()), share, "ok" if ok else "MISSES"))
    return ok


def finish(first):
    bad = [r for r in RECORDS[first:] if not r[-1]]
    assert not bad, "outside the bound (kernel, case, tensor, error, bound, share, ok): %s" % (bad,)


def note(kind, text):
    NOTES.append((kind, text))
    print("POOL-EDGE-SET | %s | %s" % (kind, text))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _off16(t, elements=1):
    """a contiguous copy of t that starts ``elements`` elements into a longer buffer: 4 bytes off 16-byte alignment for float32,
    one byte off 4-byte alignment for uint8"""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[elements:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == elements * t.element_size()
    return v


# -------------------------------------------------------------------------------------------------------------------- max-pool
def maxpool_input(shape, kind, seed):
    gen = _gen(seed)
    if kind == "negative":
        return -0.5 - torch.rand(shape, generator=gen)
    if kind == "randn":
        return torch.randn(shape, generator=gen)
    if kind == "lattice":
        return torch.randint(-4, 5, shape, generator=gen).float() / 4
    return torch.full(shape, -2.0)


def tie_share(x_nhwc):
    """float64: of the 3x3 / 2 / 1 windows that hold more than one pixel, the share whose maximum is attained more than once
    -> (share, windows counted)"""
    x = nchw(x_nhwc).double()
    B, C, Hh, W = x.shape
    Ho, Wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    cols = torch.stack([xp[:, :, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2] for kh in range(3) for kw in range(3)], 2)    # [B,C,9,Ho,Wo]
    live = (cols > float("-inf")).sum(2)
    tied = (cols == cols.max(2, keepdim=True).values).sum(2) > 1
    n = int((live > 1).sum())
    return (float(tied[live > 1].double().mean()) if n else 1.0), n


def seed_fits(key, seed):
    shape = tuple(int(s) for s in key.split("x"))
    return tie_share(maxpool_input(shape, "lattice", seed))[0] >= TIE_SHARE


def find_seeds(tries=1000):
    return {key: next(s for s in range(tries) if seed_fits(key, s)) for key in SEEDS}


def maxpool_reference(x_nhwc, dy_nhwc):
    """float64 F.max_pool2d and its autograd gradient, NHWC"""
    x = nchw(x_nhwc).double().requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    y.backward(nchw(dy_nhwc).double())
    return nhwc(y.detach()), nhwc(x.grad)


@functools.lru_cache(maxsize=None)
def _maxpool_case(shape, kind):
    B, Hh, W, C = shape
    x = maxpool_input(shape, kind, SEEDS[_name(shape)] if kind == "lattice" else 1 + MAXPOOL_SHAPES.index(shape))
    gen = _gen(77)
    dy = _ints(gen, (B, (Hh - 1) // 2 + 1, (W - 1) // 2 + 1, C))
    base = _ints(gen, shape)
    y64, dx64 = maxpool_reference(x, dy)
    return x, dy, base, y64, dx64


def _maxpool_compare(device, case, x, dy, base, y64, dx64, transform=lambda t: t):
    shape = tuple(x.shape)
    C = shape[-1]
    xd, dyd = x.to(device), dy.to(device)
    y, idx = H.maxpool_forward(xd)
    assert idx.dtype == torch.uint8 and int(idx.max()) <= 8
    exact("maxpool_fwd", case, "y", transform(y), transform(y64))
    dx = H.maxpool_backward(dyd, idx, shape)
    exact("maxpool_bwd", case, "d x", dx, dx64)
    acc = base.clone().to(device)
    out = H.maxpool_backward(dyd, idx, shape, accumulate_into=acc)
    assert out.data_ptr() == acc.data_ptr(), (case, "accumulate_into: another storage came back")
    exact("maxpool_bwd", case, "base + d x", out, base.double() + dx64)
    if C % 4 == 0:
        # contiguous but 4 bytes off 16-byte alignment: the four-channel kernels cannot take it, the scalar ones run instead
        y1, idx1 = H.maxpool_forward(_off16(xd))
        assert _same_bits(y1, y) and torch.equal(idx1, idx), (case, "forward on an operand 4 bytes off 16-byte alignment differs")
        assert _same_bits(H.maxpool_backward(_off16(dyd), idx, shape), dx), (case, "backward, dy 4 bytes off 16-byte alignment, differs")
    # the window taps one byte off 4-byte alignment: the scalar backward kernel
    idx_off = _off16(idx)
    assert _same_bits(H.maxpool_backward(dyd, idx_off, shape), dx), (case, "backward, idx one byte off 4-byte alignment, differs")
    acc = base.clone().to(device)
    out = H.maxpool_backward(dyd, idx_off, shape, accumulate_into=acc)
    assert out.data_ptr() == acc.data_ptr() and _same_bits(out.cpu(), (base.double() + dx64).float())
    return y, idx, dx


def run_maxpool(device, shape, kind):
    first = len(RECORDS)
    x, dy, base, y64, dx64 = _maxpool_case(shape, kind)
    case = "maxpool %s %s" % (_name(shape), kind)
    if kind == "lattice":
        share, n = tie_share(x)
        note(case, "seed %d | exact ties for the maximum in %.1f %% of the %d windows of more than one pixel" % (SEEDS[_name(shape)], 100 * share, n))
        assert share >= TIE_SHARE, (case, "tie share at the recorded seed", share)
    _maxpool_compare(device, case, x, dy, base, y64, dx64)
    finish(first)


def nonfinite_input():
    """(1,7,7,4): one NaN, one +inf (no window holds both NaN and another NaN: there is only one), channel 3 all -inf"""
    x = torch.randn(1, 7, 7, 4, generator=_gen(3))
    x[0, 2, 3, 0] = float("nan")
    x[0, 5, 1, 1] = float("inf")
    x[0, :, :, 3] = float("-inf")
    return x


def run_maxpool_nonfinite(device):
    first = len(RECORDS)
    x = nonfinite_input()
    gen = _gen(78)
    dy, base = _ints(gen, (1, 4, 4, 4)), _ints(gen, (1, 7, 7, 4))
    y64, dx64 = maxpool_reference(x, dy)
    assert int(torch.isnan(y64).sum()) >= 1 and int((y64 == float("inf")).sum()) >= 1 and bool((y64[..., 3] == float("-inf")).all())
    sentinels = lambda t: torch.nan_to_num(t, nan=12345.0, posinf=23456.0, neginf=-34567.0)
    _maxpool_compare(device, "maxpool 1x7x7x4 non-finite", x, dy, base, y64, dx64, transform=sentinels)
    finish(first)


# ------------------------------------------------------------------------------------------------------------------ upsample2x
def upsample2x_forward(x):
    """the C entry point as monodepth_layers._UpsampleFn.forward calls it (x: NHWC, channel slices allowed)"""
    B, h, w, C = x.shape
    y = torch.empty((B, 2 * h, 2 * w, C), dtype=torch.float32, device=x.device)
    H.check(_lib.lib().segsde_upsample2x_forward(H._p(H._f32(x)), H.nhwc_ld(x), B, h, w, C, H._p(y), C, H._stream(x)), "upsample2x_forward")
    return y


def upsample2x_backward(g):
    B, H2, W2, C = g.shape
    dx = torch.empty((B, H2 // 2, W2 // 2, C), dtype=torch.float32, device=g.device)
    H.check(_lib.lib().segsde_upsample2x_backward(H._p(H._f32(g)), H.nhwc_ld(g), B, H2 // 2, W2 // 2, C, H._p(dx), C, H._stream(g)), "upsample2x_backward")
    return dx


def upsample_reference(dtype, x_nhwc, dy_nhwc):
    x = nchw(x_nhwc).to(dtype).requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode="nearest")
    y.backward(nchw(dy_nhwc).to(dtype))
    return nhwc(y.detach()), nhwc(x.grad)


def _channel_slice(t, left=1, right=2, fill=-77.0):
    """t as channels [left, left + C) of a wider NHWC buffer"""
    wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + left + right,), fill, dtype=t.dtype, device=t.device)
    wide[..., left:left + t.shape[-1]] = t
    return wide[..., left:left + t.shape[-1]], wide


def run_upsample2x(device, shape):
    first = len(RECORDS)
    B, h, w, C = shape
    case = "upsample2x " + _name(shape)
    gen = _gen(B + h + w + C)
    x, dyi, dyr = torch.randn(shape, generator=gen), _ints(gen, (B, 2 * h, 2 * w, C)), torch.randn(B, 2 * h, 2 * w, C, generator=gen)
    y64, dxi64 = upsample_reference(torch.float64, x, dyi)
    _, dxr64 = upsample_reference(torch.float64, x, dyr)
    _, dxr32 = upsample_reference(torch.float32, x, dyr)
    xd = x.to(device)
    y = upsample2x_forward(xd)
    exact("upsample2x_fwd", case, "y", y, y64)
    exact("upsample2x_bwd", case, "d x, integer dy", upsample2x_backward(dyi.to(device)), dxi64)
    check("upsample2x_bwd", case, "d x, random dy", upsample2x_backward(dyr.to(device)), dxr32, dxr64)
    # each operand once as a channel slice of a wider buffer
    xs, xwide = _channel_slice(xd)
    snap = xwide.clone()
    assert _same_bits(upsample2x_forward(xs), y) and _same_bits(xwide, snap), (case, "forward of a channel slice")
    gs, gwide = _channel_slice(dyi.to(device))
    snap = gwide.clone()
    exact("upsample2x_bwd", case, "d x, integer dy as a channel slice", upsample2x_backward(gs), dxi64)
    assert _same_bits(gwide, snap)
    # the public layer on NCHW under autograd
    xn = nchw(x).to(device).requires_grad_(True)
    yn = ML.upsample(xn)
    yn.backward(nchw(dyi).to(device))
    exact("upsample2x_fwd", case, "upsample() y", yn, nchw(y64))
    exact("upsample2x_bwd", case, "upsample() d x", xn.grad, nchw(dxi64))
    finish(first)


# ---------------------------------------------------------------------------------------------------------------------- resize
def resize_reference(dtype, x_nhwc, dy_nhwc, out_hw, ac):
    x = nchw(x_nhwc).to(dtype).requires_grad_(True)
    y = F.interpolate(x, size=out_hw, mode="bilinear", align_corners=ac)
    y.backward(nchw(dy_nhwc).to(dtype))
    return nhwc(y.detach()), nhwc(x.grad)


def run_resize(device, index, C):
    first = len(RECORDS)
    (hi, wi), (ho, wo), ac = RESIZE_CASES[index]
    case = "resize %dx%d -> %dx%d %s c%d" % (hi, wi, ho, wo, "ac" if ac else "half-pixel", C)
    gen = _gen(100 * index + C)
    x, dy = torch.randn(2, hi, wi, C, generator=gen), torch.randn(2, ho, wo, C, generator=gen)
    (y32, dx32), (y64, dx64) = (resize_reference(dt, x, dy, (ho, wo), ac) for dt in (torch.float32, torch.float64))
    check("resize_fwd", case, "y", H.resize_bilinear(x.to(device), (ho, wo), ac), y32, y64)
    one = (hi, wi) == (1, 1)
    check("resize_bwd (sum)" if one else "resize_bwd", case, "d x", H.resize_bilinear_backward(dy.to(device), (hi, wi), ac), dx32, dx64)
    if one:
        # a pitch that is no multiple of 4 takes the scalar sum kernel instead of the four-channel one
        gs, _ = _channel_slice(dy.to(device))
        assert C % 4 != 0 or H.nhwc_ld(gs) % 4 != 0
        check("resize_bwd (sum)", case, "d x, dy behind a pitch of %d" % H.nhwc_ld(gs), H.resize_bilinear_backward(gs, (1, 1), ac), dx32, dx64)
    finish(first)


# ---------------------------------------------------------------------------------------------------------- global average pool
def gap_slices(B, HW, C):
    """pixel slices of the forward launch, from the workspace the library asks for (0 bytes: one slice)"""
    nbytes = int(_lib.lib().segsde_global_avgpool_workspace(B, HW, C))
    assert nbytes % (B * C * 8) == 0
    return max(1, nbytes // (B * C * 8))


def run_gap(device, shape, pitched=False):
    first = len(RECORDS)
    B, C, Hh, W = shape
    HW = Hh * W
    case = "gap %s%s" % (_name(shape), " pitched" if pitched else "")
    gen = _gen(C + HW)
    x = torch.randn(B, Hh, W, C, generator=gen) + 2
    dy = torch.randn(B, 1, 1, C, generator=gen)
    nz = gap_slices(B, HW, C)
    per = -(-HW // nz)
    note(case, "%d slice(s) of %d pixels%s" % (nz, per, ", the last %d empty" % (nz - -(-HW // per)) if per * (nz - 1) >= HW else ""))
    if HW == 40000:
        assert nz > 1, (case, "takes one slice")
        if C <= 64:
            assert nz == 256 and per * (nz - 1) >= HW, (case, "the last slice is not empty", nz, per)
    xd = x.to(device)
    if pitched:
        xd, _ = _channel_slice(xd, 1, 2)
        assert C % 4 == 0 and H.nhwc_ld(xd) % 4 != 0
    y64 = x.double().mean((1, 2), keepdim=True)
    relative("gap_fwd4" if C % 4 == 0 and not pitched else "gap_fwd", case, "y", H.global_avgpool(xd), y64, 2.0 ** -23)
    if not pitched:
        dx64 = (dy.double() / HW).expand(B, Hh, W, C)
        relative("gap_bwd", case, "d x", H.global_avgpool_backward(dy.to(device), (B, Hh, W, C)), dx64, 2.0 ** -22)
    finish(first)


# ------------------------------------------------------------------------------------------------------------------------ gate
def gate_inputs(n, seed=0):
    gen = _gen(seed + n)
    f, a, dy = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    if n >= 4:
        for i, v in enumerate(GATE_PLANTED):
            a[(i * n) // 4] = v
    return f, a, dy


def gate_reference(dtype, f, a, dy):
    f, a = f.detach().clone().to(dtype).requires_grad_(True), a.detach().clone().to(dtype).requires_grad_(True)
    y = f * torch.sigmoid(a)
    y.backward(dy.to(dtype))
    return y.detach(), f.grad, a.grad


def run_gate(device, n):
    first = len(RECORDS)
    f, a, dy = gate_inputs(n)
    case = "gate n=%d" % n
    r32, r64 = gate_reference(torch.float32, f, a, dy), gate_reference(torch.float64, f, a, dy)
    fd, ad = f.to(device), a.to(device)
    check("gate_fwd", case, "y", H.gate_forward(fd, ad), r32[0], r64[0])
    df, da = H.gate_backward(dy.to(device), fd, ad)
    check("gate_bwd", case, "d f", df, r32[1], r64[1])
    check("gate_bwd", case, "d a", da, r32[2], r64[2])
    finish(first)


def run_gate_function(device):
    """once through the autograd function the models use, on permuted (non-contiguous) operands"""
    first = len(RECORDS)
    f, a, dy = (t.reshape(2, 4, 8, 4) for t in gate_inputs(256, seed=1))
    r32, r64 = gate_reference(torch.float32, f, a, dy), gate_reference(torch.float64, f, a, dy)
    fw, aw = f.permute(0, 3, 1, 2).contiguous().to(device).requires_grad_(True), a.permute(0, 3, 1, 2).contiguous().to(device).requires_grad_(True)
    fv, av = fw.permute(0, 2, 3, 1), aw.permute(0, 2, 3, 1)
    assert not fv.is_contiguous() and not av.is_contiguous()
    y = Fn.GateFn.apply(fv, av)
    y.backward(dy.permute(0, 3, 1, 2).contiguous().to(device).permute(0, 2, 3, 1))
    check("gate_fwd", "GateFn 2x4x8x4 permuted", "y", y, r32[0], r64[0])
    check("gate_bwd", "GateFn 2x4x8x4 permuted", "d f", fw.grad.permute(0, 2, 3, 1), r32[1], r64[1])
    check("gate_bwd", "GateFn 2x4x8x4 permuted", "d a", aw.grad.permute(0, 2, 3, 1), r32[2], r64[2])
    finish(first)


# ---------------------------------------------------------------------------------------------------------------------- layout
def _twice_on_poison(call, poison=7.0):
    """the result of ``call`` on an allocation that was filled with ``poison`` beforehand: run, poison the result, release it, run
    again (the caching allocator hands the block straight back)"""
    out = call()
    out.fill_(poison)
    del out
    return call()


def run_nchw_to_nhwc(device, C, pad_to):
    first = len(RECORDS)
    B, Hh, W = 2, 5, 7
    Cp = -(-C // pad_to) * pad_to
    x = torch.rand(B, C, Hh, W, generator=_gen(10 * C + pad_to))
    xd = x.to(device)
    for mean, std in LAYOUT_NORM:
        case = "nchw_to_nhwc c%d pad_to %d (%g, %g)" % (C, pad_to, mean, std)
        y = _twice_on_poison(lambda: H.nchw_to_nhwc(xd, mean, std, pad_to=pad_to))
        assert tuple(y.shape) == (B, Hh, W, Cp)
        vec = Cp <= 8 and Cp % 4 == 0
        bit = check("nchw_to_nhwc (4/8 channels)" if vec else "nchw_to_nhwc (generic)", case, "present channels", y[..., :C],
                    nhwc((x - mean) / std), nhwc((x.double() - mean) / std))
        note(case, "present channels %s the fp32 oracle" % ("bit-identical to" if bit else "NOT bit-identical to"))
        if Cp > C:
            assert _same_bits(y[..., C:].cpu(), torch.zeros(B, Hh, W, Cp - C)), (case, "padded channels are not +0.0")
    finish(first)


def run_stem_input(device, shape):
    B, C, Hh, W = shape
    x = torch.rand(shape, generator=_gen(C + W)).to(device)
    cp = 4 if C <= 4 else 8
    for mean, std in LAYOUT_NORM:
        case = "stem_input %s (%g, %g)" % (_name(shape), mean, std)
        y = _twice_on_poison(lambda: H.stem_input(x, mean, std))
        assert tuple(y.shape) == (B, Hh + 6, W + 8, cp)
        inner = H.nchw_to_nhwc(x, mean, std, pad_to=cp)
        assert _same_bits(y[:, 3:3 + Hh, 3:3 + W], inner), (case, "the interior differs from nchw_to_nhwc")
        border = y.clone()
        border[:, 3:3 + Hh, 3:3 + W] = 0.0
        assert _same_bits(border.cpu(), torch.zeros(B, Hh + 6, W + 8, cp)), (case, "the border is not +0.0")
        assert bool((y[:, :3] == 0).all()) and bool((y[:, 3 + Hh:] == 0).all()) and bool((y[:, :, :3] == 0).all()) and bool((y[:, :, 3 + W:] == 0).all())
        assert y.shape[1] - (3 + Hh) == 3 and y.shape[2] - (3 + W) == 5
        print("POOL-EDGE | nchw_to_nhwc_border | %s | interior and border (exact) | 0.000e+00 | 0.000e+00 | - | 0.000 | ok" % case)


def run_nhwc_to_nchw(device, shape):
    first = len(RECORDS)
    x = torch.randn(shape, generator=_gen(sum(shape)))
    exact("nhwc_to_nchw", "nhwc_to_nchw " + _name(shape), "y", H.nhwc_to_nchw(x.to(device)), nchw(x).double())
    finish(first)


# --------------------------------------------------------------------------------------------------- axpby / copy_channels
def run_axpby(device, n):
    first = len(RECORDS)
    gen = _gen(n)
    x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    alpha, beta = 0.99, -0.37
    af, bf = float(torch.tensor(alpha)), float(torch.tensor(beta))      # the float32 scalars the kernel receives, as doubles
    xd, yd = x.to(device), y.to(device)
    scal = torch.tensor([7.0, alpha, beta]).to(device)
    a_t, b_t = scal[1:2], scal[2:3]                                     # device scalars that do not start their allocation
    for with_y in (True, False):
        r32 = alpha * x + beta * y if with_y else alpha * x
        r64 = af * x.double() + bf * y.double() if with_y else af * x.double()
        tag = "a x + b y" if with_y else "a x"
        for kernel, call in (("axpby", lambda out: H.axpby(alpha, xd, beta, yd if with_y else None, out=out)),
                             ("axpby_dev", lambda out: H.axpby_dev(a_t, xd, b_t if with_y else None, yd if with_y else None, out=out))):
            case = "%s n=%d" % (kernel, n)
            got = call(None)
            bit = check(kernel, case, tag, got, r32, r64)
            note(case + " " + tag, "%s the fp32 oracle" % ("bit-identical to" if bit else "NOT bit-identical to"))
            buf = torch.full((n,), -5.0).to(device)
            back = call(buf)
            assert back is buf and _same_bits(buf, got), (case, tag, "out= is not written in place and returned")
    finish(first)


def run_copy_channels(device, C):
    """ragged widths between channel slices of different pitch"""
    gen = _gen(C)
    x = torch.randn(2, 3, 5, C, generator=gen).to(device)
    src, swide = _channel_slice(x, 2, 3)
    dst, dwide = _channel_slice(torch.zeros_like(x), 1, 2, fill=-3.0)
    ssnap, want = swide.clone(), dwide.clone()
    want[..., 1:1 + C] = x
    assert H.nhwc_ld(src) != H.nhwc_ld(dst) or C == 1
    back = H.copy_channels(src, dst)
    assert back is dst and _same_bits(dwide, want) and _same_bits(swide, ssnap), ("copy_channels c%d" % C, "slice to slice")
    print("POOL-EDGE | copy_channels | copy_channels c%d pitch %d -> %d | dst and its surroundings (exact) | 0.000e+00 | 0.000e+00 | - | 0.000 | ok" % (
        C, swide.shape[-1], dwide.shape[-1]))


# -------------------------------------------------------------------------------------------------------- the grid-stride loop
def _threads(n):
    assert n > EW_CAP and n % 256 != 0, (n, "not just above the cap of 8192 x 256 threads, or a multiple of 256")
    return n


def _gs_maxpool_fwd(device, shape, kernel):
    gen = _gen(1)
    x = _ints(gen, shape, -100, 100)
    B, Hh, W, C = shape
    _threads(B * ((Hh - 1) // 2 + 1) * ((W - 1) // 2 + 1) * (C // 4 if C % 4 == 0 else C))
    y64 = nhwc(F.max_pool2d(nchw(x).double(), 3, 2, 1))
    y, idx = H.maxpool_forward(x.to(device))
    exact(kernel, "grid-stride " + _name(shape), "y", y, y64)
    # the taps select the maximum: gathering through them reproduces y
    xp = F.pad(nchw(x), (1, 1, 1, 1), value=float("-inf"))
    i = nchw(idx.cpu()).long()
    ho, wo = torch.arange(i.shape[2]).view(1, 1, -1, 1), torch.arange(i.shape[3]).view(1, 1, 1, -1)
    rows, cols = 2 * ho + i // 3, 2 * wo + i % 3
    picked = xp[torch.arange(B).view(-1, 1, 1, 1), torch.arange(C).view(1, -1, 1, 1), rows, cols]
    assert torch.equal(nhwc(picked).double(), y64), (kernel, "idx does not point at the maximum")


def _gs_maxpool_bwd(device, shape, kernel):
    B, Hh, W, C = shape
    _threads(B * Hh * W * (C // 4 if C % 4 == 0 else C))
    gen = _gen(2)
    x = _ints(gen, shape, -3, 3)                     # many ties: first maximum wins
    dy = _ints(gen, (B, (Hh - 1) // 2 + 1, (W - 1) // 2 + 1, C))
    _, dx64 = maxpool_reference(x, dy)
    xd = x.to(device)
    _, idx = H.maxpool_forward(xd)
    exact(kernel, "grid-stride " + _name(shape), "d x", H.maxpool_backward(dy.to(device), idx, shape), dx64)


def _gs_upsample_fwd(device):
    shape = (1, 725, 724, 1)
    _threads(4 * 725 * 724)
    x = _ints(_gen(3), shape, -100, 100)
    exact("upsample2x_fwd", "grid-stride " + _name(shape), "y", upsample2x_forward(x.to(device)),
          nhwc(F.interpolate(nchw(x).double(), scale_factor=2, mode="nearest")))


def _gs_upsample_bwd(device):
    shape = (1, 1449, 1448, 1)
    _threads(1449 * 1448)
    dy = _ints(_gen(4), (1, 2898, 2896, 1))
    want = nhwc(F.avg_pool2d(nchw(dy).double(), 2) * 4)       # the adjoint of nearest x2: the sum of each 2x2 block (exact on integers)
    exact("upsample2x_bwd", "grid-stride " + _name(shape), "d x", upsample2x_backward(dy.to(device)), want)


def _gs_resize(device, backward):
    small, large = (725, 724), (1449, 1448)
    _threads(1449 * 1448)
    gen = _gen(5)
    if backward:        # one thread per source pixel: the large map is the source
        src, dst, kernel = large, small, "resize_bwd"
    else:
        src, dst, kernel = small, large, "resize_fwd"
    x, dy = torch.randn(1, src[0], src[1], 1, generator=gen), torch.randn(1, dst[0], dst[1], 1, generator=gen)
    (y32, dx32), (y64, dx64) = (resize_reference(dt, x, dy, dst, False) for dt in (torch.float32, torch.float64))
    case = "grid-stride %dx%d -> %dx%d" % (src + dst)
    if backward:
        check(kernel, case, "d x", H.resize_bilinear_backward(dy.to(device), src, False), dx32, dx64)
    else:
        check(kernel, case, "y", H.resize_bilinear(x.to(device), dst, False), y32, y64)


def _gs_gap_bwd(device):
    shape = (1, 837, 836, 3)
    _threads(837 * 836 * 3)
    dy = torch.randn(1, 1, 1, 3, generator=_gen(6))
    relative("gap_bwd", "grid-stride " + _name(shape), "d x", H.global_avgpool_backward(dy.to(device), shape),
             (dy.double() / (837 * 836)).expand(shape), 2.0 ** -22)


def _gs_gate(device, backward):
    n = _threads(EW_CAP + 77)
    f, a, dy = gate_inputs(n, seed=7)
    r32, r64 = gate_reference(torch.float32, f, a, dy), gate_reference(torch.float64, f, a, dy)
    case = "grid-stride n=%d" % n
    if backward:
        df, da = H.gate_backward(dy.to(device), f.to(device), a.to(device))
        check("gate_bwd", case, "d f", df, r32[1], r64[1])
        check("gate_bwd", case, "d a", da, r32[2], r64[2])
    else:
        check("gate_fwd", case, "y", H.gate_forward(f.to(device), a.to(device)), r32[0], r64[0])


def _gs_axpby(device):
    n = _threads(EW_CAP + 77)
    gen = _gen(8)
    x, y = _ints(gen, (n,), -100, 100), _ints(gen, (n,), -100, 100)
    exact("axpby", "grid-stride n=%d" % n, "2 x + 3 y", H.axpby(2.0, x.to(device), 3.0, y.to(device)), 2 * x.double() + 3 * y.double())


def _gs_copy_channels(device, C):
    M = (EW_CAP + 79) // 3 if C == 3 else EW_CAP + 77
    _threads(M * C // 4 if C % 4 == 0 else M * C)
    x = _ints(_gen(9), (M, C), -100, 100).to(device)
    wide = torch.full((M, 2 * C), -3.0, device=device)
    dst = wide[:, C:]
    H.copy_channels(x, dst)
    ok = bool(torch.equal(dst, x)) and bool((wide[:, :C] == -3.0).all())
    _record("copy_channels<%d>" % (4 if C % 4 == 0 else 1), "grid-stride %dx%d" % (M, C), "dst and its neighbours (exact)", 0.0 if ok else float("inf"), 0.0, 100.0, 0.0, ok)


def _gs_scale_channels(device):
    shape = (2, 591, 592, 3)
    _threads(2 * 591 * 592 * 3)
    gen = _gen(10)
    x, s = _ints(gen, shape, -100, 100), _ints(gen, (2, 3), -8, 8)
    exact("scale_channels", "grid-stride " + _name(shape), "y", H.scale_channels(x.to(device), s.to(device)), x.double() * s.double().view(2, 1, 1, 3))


def _gs_nchw_to_nhwc(device, vec):
    shape = (1, 3, 1449, 1448) if vec else (1, 3, 837, 836)         # 4 / 8 channels: one thread per pixel; generic: one per element
    _threads(shape[2] * shape[3] * (1 if vec else 3))
    x = 1 + 2 * _ints(_gen(11), shape, -50, 50)                     # odd integers: (x - 1) / 2 is exact
    y = H.nchw_to_nhwc(x.to(device), 1.0, 2.0, pad_to=4 if vec else 1)
    kernel = "nchw_to_nhwc (4/8 channels)" if vec else "nchw_to_nhwc (generic)"
    exact(kernel, "grid-stride " + _name(shape), "present channels", y[..., :3], nhwc((x.double() - 1) / 2))
    if vec:
        assert y.shape[-1] == 4 and bool((y[..., 3] == 0).all())


def _gs_stem_input(device):
    shape = (1, 3, 1443, 1440)
    _threads(1449 * 1448)
    x = 1 + 2 * _ints(_gen(12), shape, -50, 50)
    y = H.stem_input(x.to(device), 1.0, 2.0)
    exact("nchw_to_nhwc_border", "grid-stride " + _name(shape), "interior", y[:, 3:-3, 3:-5, :3], nhwc((x.double() - 1) / 2))
    total = float(y.double().abs().sum())
    assert total == float(((x.double() - 1) / 2).abs().sum()), "the border or the padded channel is not zero"


def _gs_nhwc_to_nchw(device):
    shape = (1, 837, 836, 3)
    _threads(837 * 836 * 3)
    x = _ints(_gen(13), shape, -100, 100)
    exact("nhwc_to_nchw", "grid-stride " + _name(shape), "y", H.nhwc_to_nchw(x.to(device)), nchw(x).double())


# thread counts (not elements: the four-channel kernels count channel quads) just above 8192 x 256 and no multiple of 256
GRID_STRIDE = {
    "maxpool_fwd": lambda d: _gs_maxpool_fwd(d, (1, 1183, 1181, 6), "maxpool_fwd"),                 # 592 x 591 x 6 outputs
    "maxpool_fwd4": lambda d: _gs_maxpool_fwd(d, (1, 1, 2 * (EW_CAP + 77) - 1, 4), "maxpool_fwd4"),  # one row: 16 floats read per thread
    "maxpool_bwd": lambda d: _gs_maxpool_bwd(d, (1, 592, 591, 6), "maxpool_bwd"),
    "maxpool_bwd4": lambda d: _gs_maxpool_bwd(d, (1, 1449, 1448, 4), "maxpool_bwd4"),
    "upsample2x_fwd": _gs_upsample_fwd,
    "upsample2x_bwd": _gs_upsample_bwd,
    "resize_fwd": lambda d: _gs_resize(d, False),
    "resize_bwd": lambda d: _gs_resize(d, True),
    "gap_bwd": _gs_gap_bwd,
    "gate_fwd": lambda d: _gs_gate(d, False),
    "gate_bwd": lambda d: _gs_gate(d, True),
    "axpby": _gs_axpby,
    "copy_channels<1>": lambda d: _gs_copy_channels(d, 3),
    "copy_channels<4>": lambda d: _gs_copy_channels(d, 4),
    "scale_channels": _gs_scale_channels,
    "nchw_to_nhwc generic": lambda d: _gs_nchw_to_nhwc(d, False),
    "nchw_to_nhwc 4-channel": lambda d: _gs_nchw_to_nhwc(d, True),
    "nchw_to_nhwc_border": _gs_stem_input,
    "nhwc_to_nchw": _gs_nhwc_to_nchw,
}


def run_grid_stride(device, name):
    first = len(RECORDS)
    GRID_STRIDE[name](device)
    finish(first)


# ------------------------------------------------------------------------------------------------------------ operand contract
CONTRACT_FAILED = []        # (call, what) of the last run_operand_contract


class _Strided:
    """read operands in the non-contiguous forms callers produce, each inside a wider buffer whose other elements are watched"""

    def __init__(self, device, seed):
        self.dev, self.gen, self.watch = device, _gen(seed), []

    def channels(self, t, left=4, right=4):
        """NHWC / [M, C] tensor as a channel slice: a pitch, the form the pitched kernels take in place"""
        v, wide = _channel_slice(t.to(self.dev), left, right)
        self.watch.append((wide, wide.clone()))
        return v

    def columns(self, t):
        """NCHW tensor as a W-slice: not expressible as a pitch"""
        wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), -77, dtype=t.dtype).to(self.dev)
        wide[..., 1:1 + t.shape[-1]] = t.to(self.dev)
        self.watch.append((wide, wide.clone()))
        return wide[..., 1:1 + t.shape[-1]]

    def untouched(self):
        return all(_same_bits(w, s) for w, s in self.watch)


def _fail(call, what):
    CONTRACT_FAILED.append((call, what))
    print("POOL-EDGE-CONTRACT | %s | %s" % (call, what))


def _contract(name, call, strided, fixed=None, store=None):
    """``call(**operands) -> tuple of tensors``, once on the strided operands and once on contiguous clones held in locals: the
    results are bit-identical, float32, and the operands and the buffers around them are untouched"""
    for k, t in strided.items():
        assert not t.is_contiguous(), (name, k, "the test's operand is contiguous")
    held = {k: t.clone(memory_format=torch.contiguous_format) for k, t in strided.items()}
    fixed = fixed or {}
    try:
        got = call(**strided, **fixed)
    except Exception as e:
        _fail(name, "strided operands: raised %s: %s" % (type(e).__name__, e))
        return None
    want = call(**held, **fixed)
    for i, (g, w) in enumerate(zip(got, want)):
        if not _same_bits(g, w):
            diff = " (max diff %.3g)" % float((g.double() - w.double()).abs().max()) if g.shape == w.shape and g.is_floating_point() else ""
            _fail(name, "strided operands: output %d differs from the call on held contiguous clones%s" % (i, diff))
    if store is not None and not store.untouched():
        _fail(name, "strided operands: an operand or the buffer around it was modified")
    return want


def _raises(name, what, exc, call, watched=()):
    snaps = [t.clone() for t in watched]
    try:
        out = call()
    except exc:
        pass
    except Exception as e:
        _fail(name, "%s: raised %s (%s), not %s" % (what, type(e).__name__, e, exc.__name__))
    else:
        if isinstance(out, tuple):
            out = out[0]
        _fail(name, "%s: no %s; returned %s %s" % (what, exc.__name__, getattr(out, "dtype", None), tuple(getattr(out, "shape", ()))))
    for t, s in zip(watched, snaps):
        if not _same_bits(t, s):
            _fail(name, "%s: the buffer or its neighbours were written" % what)


def run_operand_contract(device):
    """every wrapper of the family with all of its read operands strided at once against the same call on held contiguous clones,
    a float64 read operand (TypeError), a strided written buffer (ValueError, nothing written)"""
    del CONTRACT_FAILED[:]
    o = _Strided(device, 5)
    gen = o.gen
    d = lambda t: t.to(device)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    B, Hh, W, C = 2, 5, 7, 8
    Ho, Wo = 3, 4
    run = lambda name, call, strided, fixed=None: _contract(name, call, strided, fixed, o)

    # max-pool
    x = rnd(B, Hh, W, C)
    fwd = run("maxpool_forward", lambda x: H.maxpool_forward(x), dict(x=o.channels(x)))
    _raises("maxpool_forward", "float64 x", TypeError, lambda: H.maxpool_forward(d(x).double()))
    y, idx = H.maxpool_forward(d(x))
    dy = _ints(gen, (B, Ho, Wo, C))
    want = H.maxpool_backward(d(dy), idx, (B, Hh, W, C))
    idx_w = torch.full((B, Ho, Wo + 2, C), 9, dtype=torch.uint8, device=device)      # the taps as a view of a wider buffer
    idx_w[:, :, 1:1 + Wo] = idx
    o.watch.append((idx_w, idx_w.clone()))
    got = run("maxpool_backward", lambda dy, idx: (H.maxpool_backward(dy, idx, (B, Hh, W, C)),), dict(dy=o.channels(dy), idx=idx_w[:, :, 1:1 + Wo]))
    if got is not None and not _same_bits(got[0], want):
        _fail("maxpool_backward", "held clones differ from the dense call")
    _raises("maxpool_backward", "float64 dy", TypeError, lambda: H.maxpool_backward(d(dy).double(), idx, (B, Hh, W, C)))
    _raises("maxpool_backward", "int64 idx", TypeError, lambda: H.maxpool_backward(d(dy), idx.long(), (B, Hh, W, C)))
    # a strided accumulator is not written: the result comes back in a fresh tensor (the gradient collector looks at the address)
    acc_w = torch.full((B, Hh, W, C + 2), 0.5, device=device)
    acc, snap = acc_w[..., 1:1 + C], acc_w.clone()
    out = H.maxpool_backward(d(dy), idx, (B, Hh, W, C), accumulate_into=acc)
    if not (_same_bits(acc_w, snap) and _same_bits(out, want) and out.data_ptr() != acc.data_ptr()):
        _fail("maxpool_backward", "strided accumulate_into: written, or the fresh result differs")

    # resize
    xr, gr = rnd(B, Hh, W, C), rnd(B, 9, 4, C)
    run("resize_bilinear", lambda x: (H.resize_bilinear(x, (9, 4), False),), dict(x=o.channels(xr)))
    run("resize_bilinear_backward", lambda dy: (H.resize_bilinear_backward(dy, (Hh, W), False),), dict(dy=o.channels(gr)))
    run("resize_bilinear_backward to 1x1", lambda dy: (H.resize_bilinear_backward(dy, (1, 1), False),), dict(dy=o.channels(gr, 3, 2)))
    _raises("resize_bilinear", "float64 x", TypeError, lambda: H.resize_bilinear(d(xr).double(), (9, 4), False))
    _raises("resize_bilinear_backward", "float64 dy", TypeError, lambda: H.resize_bilinear_backward(d(gr).double(), (Hh, W), False))

    # global average pool
    gg = rnd(B, 1, 1, C)
    run("global_avgpool", lambda x: (H.global_avgpool(x),), dict(x=o.channels(xr)))
    run("global_avgpool_backward", lambda dy: (H.global_avgpool_backward(dy, (B, Hh, W, C)),), dict(dy=o.channels(gg)))
    _raises("global_avgpool", "float64 x", TypeError, lambda: H.global_avgpool(d(xr).double()))
    _raises("global_avgpool_backward", "float64 dy", TypeError, lambda: H.global_avgpool_backward(d(gg).double(), (B, Hh, W, C)))

    # gate
    f, a, g = rnd(B, Hh, W, C), rnd(B, Hh, W, C), rnd(B, Hh, W, C)
    run("gate_forward", lambda f, a: (H.gate_forward(f, a),), dict(f=o.channels(f), a=o.channels(a)))
    run("gate_backward", lambda dy, f, a: H.gate_backward(dy, f, a), dict(dy=o.channels(g), f=o.channels(f), a=o.channels(a)))
    _raises("gate_forward", "float64 f", TypeError, lambda: H.gate_forward(d(f).double(), d(a)))
    _raises("gate_forward", "float64 a", TypeError, lambda: H.gate_forward(d(f), d(a).double()))
    _raises("gate_backward", "float64 dy", TypeError, lambda: H.gate_backward(d(g).double(), d(f), d(a)))
    _raises("gate_backward", "float64 f", TypeError, lambda: H.gate_backward(d(g), d(f).double(), d(a)))
    _raises("gate_backward", "float64 a", TypeError, lambda: H.gate_backward(d(g), d(f), d(a).double()))

    # axpby / axpby_dev
    xa, ya = rnd(6, 8), rnd(6, 8)
    scal = d(torch.tensor([7.0, 2.0, 3.0]))
    a_t, b_t = scal[1:2], scal[2:3]
    run("axpby", lambda x, y: (H.axpby(2.0, x, 3.0, y),), dict(x=o.channels(xa), y=o.channels(ya)))
    run("axpby_dev", lambda x, y: (H.axpby_dev(a_t, x, b_t, y),), dict(x=o.channels(xa), y=o.channels(ya)))
    _raises("axpby", "float64 x", TypeError, lambda: H.axpby(2.0, d(xa).double(), 3.0, d(ya)))
    _raises("axpby", "float64 y", TypeError, lambda: H.axpby(2.0, d(xa), 3.0, d(ya).double()))
    _raises("axpby_dev", "float64 alpha_t", TypeError, lambda: H.axpby_dev(a_t.double(), d(xa), b_t, d(ya)))
    _raises("axpby_dev", "float64 x", TypeError, lambda: H.axpby_dev(a_t, d(xa).double(), b_t, d(ya)))
    _raises("axpby_dev", "float64 beta_t", TypeError, lambda: H.axpby_dev(a_t, d(xa), b_t.double(), d(ya)))
    _raises("axpby_dev", "float64 y", TypeError, lambda: H.axpby_dev(a_t, d(xa), b_t, d(ya).double()))
    for name, call in (("axpby", lambda out: H.axpby(2.0, d(xa), 3.0, d(ya), out=out)), ("axpby_dev", lambda out: H.axpby_dev(a_t, d(xa), b_t, d(ya), out=out))):
        buf = torch.full((6, 16), -1.0, device=device)
        _raises(name, "out= a column slice of a wider buffer", ValueError, lambda: call(buf[:, 4:12]), watched=(buf,))

    # copy_channels / scale_channels
    src = rnd(B, Hh, W, C)
    run("copy_channels", lambda src: (H.copy_channels(src, torch.empty(B, Hh, W, C, device=device)),), dict(src=o.channels(src)))
    _raises("copy_channels", "float64 src", TypeError, lambda: H.copy_channels(d(src).double(), torch.empty(B, Hh, W, C, device=device)))
    buf = torch.full((B, Hh, W, 2 * C), -1.0, device=device)
    _raises("copy_channels", "dst with a channel stride of 2", ValueError, lambda: H.copy_channels(d(src), buf[..., ::2]), watched=(buf,))
    sc = rnd(B, C)
    run("scale_channels", lambda x, scale: (H.scale_channels(x, scale),), dict(x=o.channels(xr), scale=o.channels(sc, 1, 1)))
    _raises("scale_channels", "float64 x", TypeError, lambda: H.scale_channels(d(xr).double(), d(sc)))
    _raises("scale_channels", "float64 scale", TypeError, lambda: H.scale_channels(d(xr), d(sc).double()))

    # layout edges
    img = torch.rand(B, 3, Hh, W, generator=gen)
    run("nchw_to_nhwc", lambda x: (H.nchw_to_nhwc(x, 0.45, 0.225, pad_to=4),), dict(x=o.columns(img)))
    run("nhwc_to_nchw", lambda x: (H.nhwc_to_nchw(x),), dict(x=o.channels(xr)))
    _raises("nchw_to_nhwc", "float64 x", TypeError, lambda: H.nchw_to_nhwc(d(img).double(), 0.45, 0.225))
    _raises("nhwc_to_nchw", "float64 x", TypeError, lambda: H.nhwc_to_nchw(d(xr).double()))

    # column sums: a pitch is taken in place, a column stride is not expressible
    wm = rnd(50, 24)
    run("colsum", lambda x: (H.colsum(x),), dict(x=o.channels(wm, 8, 8)))
    _raises("colsum", "float64 x", TypeError, lambda: H.colsum(d(wm).double()))
    _raises("colsum", "a transposed matrix (column stride 24)", ValueError, lambda: H.colsum(d(wm).t()))

    note("operand contract", "%d calls break the contract%s" % (len(CONTRACT_FAILED), "".join("; %s: %s" % c for c in CONTRACT_FAILED)))
    assert not CONTRACT_FAILED, CONTRACT_FAILED


# ------------------------------------------------------------------------------------------------------------------- the page
def render_table(log_lines):
    """markdown for profiles/pooling_edges.md from the ``POOL-EDGE`` lines a ``pytest -s`` run printed"""
    rows = [[f.strip() for f in l[l.index("POOL-EDGE"):].split("|")] for l in log_lines if "POOL-EDGE" in l]
    worst = {}
    for r in rows:
        if r[0] == "POOL-EDGE" and len(r) == 9 and "(exact)" not in r[3]:
            worst[r[1]] = max(worst.get(r[1], 0.0), float(r[7]))
    out = ["| kernel | largest share of the bound |", "|---|---|"] + ["| %s | %.3f |" % kv for kv in sorted(worst.items())]
    out += ["", "| kernel | case | tensor | e_kernel | e_oracle | scale | share | ok |", "|---|---|---|---|---|---|---|---|"]
    out += ["| %s |" % " | ".join(r[1:9]) for r in rows if r[0] == "POOL-EDGE" and len(r) == 9]
    out += ["", "Conditions:", ""] + ["* %s: %s" % (r[1], " | ".join(r[2:])) for r in rows if r[0] == "POOL-EDGE-SET"]
    return "\n".join(out)


if __name__ == "__main__":      # no argument: the seed search; python tests/pooling_cases.py run.log: the tables of the figures page
    import sys
    print(render_table(open(sys.argv[1]).read().splitlines()) if len(sys.argv) > 1 else find_seeds())
