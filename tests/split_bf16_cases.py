"""Split-bf16 operand mode of the implicit-GEMM convolutions (segsde_conv_desc.compute = 2, hipops.CONV_COMPUTE "bf16x9"; the
six-product form, compute = 3 / "bf16x6", missed its error gate on the MI355X and is refused): shared case functions, run on the GPU (test_split_bf16_gpu.py) and through the CPU interpreter
(test_split_bf16_emu.py).  Every case takes the device."""
import torch
import torch.nn.functional as F

from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

MODE_NAME = {0: "f32", 2: "bf16x9"}
# (H, W, C, Cout, k, dil, pad, reflect): the four geometries of kernel_cases.run_f16_operand_convolutions (batch 2)
GEOMS = [(16, 32, 64, 128, 1, 1, 0, False), (16, 32, 64, 64, 3, 1, 1, False), (16, 32, 64, 64, 3, 1, 1, True),
         (24, 32, 128, 64, 3, 6, 6, False)]
# (H, W, C0 upsampled, C1 skip, Cout): mirrored 3x3 on [upsample(x0) | x1], the folded route in all three directions
FOLDED = (8, 64, 64, 32, 64)
# full-size launches of the error gate (batch, H, W, C, Cout, k, dil, pad, reflect): the 1x1 bottleneck 1024 -> 256 and the
# dilated ASPP branch 2048 -> 256, rate 12, on the 32 x 64 map
FULLSIZE = [(16, 32, 64, 1024, 256, 1, 1, 0, False), (4, 32, 64, 2048, 256, 3, 12, 12, False)]
B = 2


def geom(mode, *args):
    with Fn.conv_compute(MODE_NAME[mode]):
        g = H.ConvGeom(*args)
    assert g.compute == mode
    return g


def run_three(mode, case, x0, x1, w, dy, folded=False):
    """forward, data-gradient(s), weight gradient of one geometry in one operand mode -> dict of tensors"""
    if folded:
        Hh, W, C0, C1, Co = case
        g = geom(mode, C0, Co, 3, 1, 1, 1, True, C1, True)
        wp, wdp = H.pack_weight_both(w)
        wf, wdf = H.upfold_pack(w, C0)
        old = H.UPFOLD_MIN_SAVED_MACS
        H.UPFOLD_MIN_SAVED_MACS = 0.0            # small test shapes take the folded weight gradient too
        t0 = dict(H.UPFOLD_TAKEN)
        try:
            y = H.conv_forward(g, x0, x1, wp, None, wfold=wf)
            dx0, dx1 = H.conv_dgrad(g, dy, wdp, w, (Hh, W), fold=(wf, wdf))
            dw = H.conv_wgrad(g, x0, x1, dy)
        finally:
            H.UPFOLD_MIN_SAVED_MACS = old
        assert all(H.UPFOLD_TAKEN[k] == t0[k] + 1 for k in t0), (t0, H.UPFOLD_TAKEN)
        return {"forward": y, "data-gradient": dx0, "data-gradient (skip)": dx1, "weight gradient": dw}
    Hh, W, C, Co, k, dil, pad, refl = case
    g = geom(mode, C, Co, k, 1, dil, pad, refl, 0, False)
    wp, wdp = H.pack_weight_both(w)
    t0 = dict(H.CONV_COMPUTE_TAKEN)
    out = {"forward": H.conv_forward(g, x0, None, wp, None), "data-gradient": H.conv_dgrad(g, dy, wdp, w, (Hh, W))[0],
           "weight gradient": H.conv_wgrad(g, x0, None, dy)}
    # what the launches themselves reported, from the descriptors they were made with, agrees with the query on the geometry
    B_ = x0.shape[0]
    want = [int(mode >= 2 and t == mode) for t in (H.conv_compute_taken(g, B_, Hh, W, d) for d in ("fwd", "dgrad", "wgrad"))]
    assert [H.CONV_COMPUTE_TAKEN[k] - t0[k] for k in ("fwd", "dgrad", "wgrad")] == want, (t0, H.CONV_COMPUTE_TAKEN, want)
    return out


def reference64(case, x0, x1, w, dy, folded=False):
    """the same three directions as a float64 convolution on the CPU"""
    a0 = x0.cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
    wq = w.cpu().double().requires_grad_(True)
    if folded:
        a1 = x1.cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
        xin = torch.cat([F.interpolate(a0, scale_factor=2, mode="nearest"), a1], 1)
        y = F.conv2d(F.pad(xin, (1, 1, 1, 1), mode="reflect"), wq)
    else:
        Hh, W, C, Co, k, dil, pad, refl = case
        y = F.conv2d(F.pad(a0, (1, 1, 1, 1), mode="reflect") if refl else a0, wq, padding=0 if refl else pad, dilation=dil)
    y.backward(dy.cpu().double().permute(0, 3, 1, 2))
    out = {"forward": y.detach().permute(0, 2, 3, 1), "data-gradient": a0.grad.permute(0, 2, 3, 1), "weight gradient": wq.grad}
    if folded:
        out["data-gradient (skip)"] = a1.grad.permute(0, 2, 3, 1)
    return out


def taken(mode, case, folded=False, batch=B, f16=False):
    """segsde_conv_compute_taken of the three directions, for the entry points run_three calls"""
    if folded:
        Hh, W, C0, C1, Co = case
        g = geom(mode, C0, Co, 3, 1, 1, 1, True, C1, True)
    else:
        Hh, W, C, Co, k, dil, pad, refl = case
        if f16:
            H.COMPUTE_F16[0] = True
            try:
                with Fn.conv_compute(MODE_NAME[mode]):
                    g = H.ConvGeom(C, Co, k, 1, dil, pad, refl, 0, False)
            finally:
                H.COMPUTE_F16[0] = False
        else:
            g = geom(mode, C, Co, k, 1, dil, pad, refl, 0, False)
    return [H.conv_compute_taken(g, batch, Hh, W, d, fold=folded) for d in ("fwd", "dgrad", "wgrad")]


def _ints(gen, shape, lo, hi, device):
    return torch.randint(lo, hi + 1, shape, generator=gen).float().to(device)


# ---------------------------------------------------------------------------------------------
# 1. h + m + l == x, bit for bit
# ---------------------------------------------------------------------------------------------
def run_exact_split(device):
    gen = torch.Generator().manual_seed(11)
    n = 1 << 17
    mant = torch.rand(n, generator=gen) + 1.0                                 # [1, 2): random 24-bit significands
    expo = torch.randint(-60, 61, (n,), generator=gen)                        # 121 binades
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    x = torch.ldexp(mant, expo) * sign
    # the corners: powers of two, all-ones significands, rounding ties of the first and the second split, zero
    one = torch.tensor([1.0, -1.0, 0.0, 2.0 - 2.0 ** -23, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -17,
                        1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 255.0, 255.5, 256.0 - 2.0 ** -15, -7.0 / 3.0])
    x = torch.cat([x, one, one * 2.0 ** 40, one * 2.0 ** -40, torch.tensor([3.0e38, -1e-30, 2.0 ** -100])]).float()
    assert x.numel() >= 1 << 16
    h, m, l = [t.cpu() for t in H.split_bf16(x.to(device))]
    for name, t in (("h", h), ("m", m), ("l", l)):
        assert torch.equal(t.to(torch.bfloat16).float(), t), name + " is not a bf16 number"
    s = h.double() + m.double() + l.double()                                  # exact in float64 (the three parts span < 53 bits)
    bad = s != x.double()
    assert not bool(bad.any()), "h + m + l != x for %d of %d values, first %r" % (int(bad.sum()), x.numel(), x[bad][:4].tolist())
    # and they are the round-to-nearest-even splits, not just any three terms
    assert torch.equal(h, x.to(torch.bfloat16).float())
    assert torch.equal(m, (x - h).to(torch.bfloat16).float())
    assert torch.equal(l, (x - h - m).to(torch.bfloat16).float())


# ---------------------------------------------------------------------------------------------
# 2. small integers: every product and partial sum is exact, the result must equal float64 bit for bit
# ---------------------------------------------------------------------------------------------
def small_integer_inputs(case, device, folded=False):
    gen = torch.Generator().manual_seed(23)
    if folded:
        Hh, W, C0, C1, Co = case
        x0 = _ints(gen, (B, Hh // 2, W // 2, C0), -3, 3, device)
        x1 = _ints(gen, (B, Hh, W, C1), -3, 3, device)
        w = _ints(gen, (Co, C0 + C1, 3, 3), -2, 2, device)
    else:
        Hh, W, C, Co, k = case[:5]
        x0, x1 = _ints(gen, (B, Hh, W, C), -3, 3, device), None
        w = _ints(gen, (Co, C, k, k), -2, 2, device)
    dy = _ints(gen, (B, Hh, W, Co), -3, 3, device)
    return x0, x1, w, dy


def run_small_integers_exact(device):
    for case, folded in [(c, False) for c in GEOMS] + [(FOLDED, True)]:
        x0, x1, w, dy = small_integer_inputs(case, device, folded)
        want = reference64(case, x0, x1, w, dy, folded)
        assert all(float(v.abs().max()) < 2 ** 24 for v in want.values())
        for mode in (2,):
            got = run_three(mode, case, x0, x1, w, dy, folded)
            for name in want:
                assert torch.equal(got[name].cpu(), want[name].float()), "compute=%d %s %s: not bit-exact on small integers (max diff %g)" % (
                    mode, case, name, float((got[name].cpu().double() - want[name]).abs().max()))


# ---------------------------------------------------------------------------------------------
# 3. the small products reach the result
# ---------------------------------------------------------------------------------------------
# Operands a = 1.5 pa + 1.5 qa 2^-9 + ra 2^-18, b likewise, with pa, qa, ra, pb, qb, rb = +-1: the split is h = 1.5 p,
# m = 1.5 q 2^-9, l = r 2^-18 (each residual is below half an ulp of the term before it and the 1.5 keeps every partial value
# inside its binade: no rounding ties, no borrow across a power of two).  Along the reduction index the six sign sequences
# have period 4 and are rows of the 4 x 4 Hadamard matrix, chosen so that over every aligned group of four
#   sum pa pb = sum pa qb = sum qa pb = sum pa rb = sum ra pb = sum qa qb = 0      (h.h, h.m, m.h, h.l, l.h, m.m)
#   sum qa rb = 4,  sum ra qb = 4,  sum ra rb = 0                                   (m.l, l.m, l.l)
# Every product class is a sum of equal-magnitude terms, so each MFMA instruction's own products add up exactly in any order,
# to zero for the six large classes; what is left is m.l + l.m = 1.5 * 2^-24 per four reduction steps, and the kernel must
# return exactly that times the row / column scales: it shows that the m.l and l.m instructions are issued on the right
# operands (a kernel with only the six large products returns exactly zero here).  What the expectation assumes of the matrix
# core, and what was seen when it did not hold, is recorded in profiles/split_bf16_layers.md ("How the matrix core adds").
_E = torch.tensor([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=torch.float64)
_PA, _QA, _RA, _PB, _QB, _RB = _E[0], _E[3], _E[2], _E[1], _E[2], _E[3]


def _crafted(n, along_a, along_b, pairs=False):
    """a [n, along_a], b [n, along_b] float64: the pattern along n, rows scaled by signed powers of two.  pairs: the pattern
    advances every second step -- the weight-gradient loop hands the instruction pixels 2 q + (lane half) in k slot q of that
    half, so the four slots of a float4 of either half then see one whole period"""
    k = (torch.arange(n) // 2) % 4 if pairs else torch.arange(n) % 4
    a = 1.5 * _PA[k] + 1.5 * _QA[k] * 2.0 ** -9 + _RA[k] * 2.0 ** -18
    b = 1.5 * _PB[k] + 1.5 * _QB[k] * 2.0 ** -9 + _RB[k] * 2.0 ** -18
    sa = 2.0 ** (torch.arange(along_a) % 5).double() * (1 - 2 * (torch.arange(along_a) % 2)).double()
    sb = 2.0 ** (torch.arange(along_b) % 3).double() * (1 - 2 * ((torch.arange(along_b) // 2) % 2)).double()
    return a[:, None] * sa[None, :], b[:, None] * sb[None, :], sa, sb


def run_small_products_reach_result(device):
    Hh, W, C = 4, 32, 32                       # 128 pixels, 32 -> 32 channels, 1x1: LDS-DMA loops in all three directions
    unit = 1.5 * 2.0 ** -24                    # m.l + l.m per four reduction steps
    case = (Hh, W, C, C, 1, 1, 0, False)
    assert taken(2, case, batch=1) == [2, 2, 2]
    P = Hh * W
    zx = torch.zeros(1, Hh, W, C)
    for direction in ("forward", "data-gradient", "weight gradient"):
        if direction == "forward":             # y[p, n] = sum_c x[p, c] w[n, c]
            a, b, sa, sb = _crafted(C, P, C)
            x, w, dy = a.t().reshape(1, Hh, W, C), b.t().reshape(C, C, 1, 1), zx
            want = (C // 4) * unit * sa[:, None] * sb[None, :]
            want = want.reshape(1, Hh, W, C)
        elif direction == "data-gradient":     # dx[p, c] = sum_n dy[p, n] w[n, c]
            a, b, sa, sb = _crafted(C, P, C)
            dy, w, x = a.t().reshape(1, Hh, W, C), b.reshape(C, C, 1, 1), zx
            want = ((C // 4) * unit * sa[:, None] * sb[None, :]).reshape(1, Hh, W, C)
        else:                                  # dw[n, c] = sum_p dy[p, n] x[p, c]
            a, b, sa, sb = _crafted(P, C, C, pairs=True)
            x, dy, w = a.reshape(1, Hh, W, C), b.reshape(1, Hh, W, C), torch.zeros(C, C, 1, 1)
            want = ((P // 4) * unit * sb[:, None] * sa[None, :]).reshape(C, C, 1, 1)
        x, w, dy = x.float().contiguous(), w.float().contiguous(), dy.float().contiguous()
        ref = reference64(case, x, None, w, dy)[direction]
        assert torch.equal(ref, want.double()) and float(want.abs().min()) > 0, "the crafted case is not what it claims (" + direction + ")"
        xd, wd, dyd = x.to(device), w.to(device), dy.to(device)
        nine = run_three(2, case, xd, None, wd, dyd)[direction].cpu()
        assert torch.equal(nine, want.float()), "compute=2 %s: the small-product sum %g came out as %g" % (
            direction, float(want.flatten()[0]), float(nine.flatten()[0]))


# ---------------------------------------------------------------------------------------------
# 4. the mode is taken
# ---------------------------------------------------------------------------------------------
def random_inputs(case, device, seed=5, batch=B):
    gen = torch.Generator().manual_seed(seed)
    Hh, W, C, Co, k = case[:5]
    x = torch.relu(torch.randn(batch, Hh, W, C, generator=gen)).to(device)
    dy = torch.randn(batch, Hh, W, Co, generator=gen).to(device)
    w = (torch.randn(Co, C, k, k, generator=gen) * (2.0 / (k * k * C)) ** 0.5).to(device)
    return x, None, w, dy


def run_mode_is_taken(device):
    import ctypes
    from improving_segmentation_with_selfsupervised_depth_amd import _lib
    for mode in (2,):
        for case in GEOMS:
            assert taken(mode, case) == [mode] * 3, (mode, case, taken(mode, case))
            assert taken(mode, case, f16=True) == [1, 1, 1], "autocast's fp16 operand mode keeps precedence"
        assert taken(mode, FOLDED, folded=True) == [mode] * 3, (mode, taken(mode, FOLDED, folded=True))
    assert taken(0, GEOMS[0]) == [0, 0, 0]
    # the six-product form is refused at every level: by name, and as a descriptor value before anything is launched
    try:
        Fn.conv_compute("bf16x6")
    except ValueError as e:
        assert "error gate" in str(e)
    else:
        raise AssertionError("bf16x6 was accepted")
    d = _lib.ConvDesc(B=2, H=16, W=32, C0=64, C1=0, ld0=64, Ho=16, Wo=32, Cout=64, ldy=64, KH=1, KW=1, stride=1, dil=1, pad=0,
                      in_div=1, compute=3)
    L, fake = _lib.lib(), ctypes.c_void_p(4096)
    assert L.segsde_conv2d_forward(ctypes.byref(d), fake, None, fake, None, fake, None, None) == -4
    assert L.segsde_conv2d_wgrad(ctypes.byref(d), fake, None, fake, 64, fake, fake, 1 << 30, None) == -4
    assert all(L.segsde_conv_compute_taken(ctypes.byref(d), k) == 0 for k in (0, 1, 2))
    d.compute = 2
    assert all(L.segsde_conv_compute_taken(ctypes.byref(d), k) == 2 for k in (0, 1, 2))
    # channels not a multiple of 32: off the LDS-DMA loops, fp32 whatever the descriptor says, and bit for bit the compute = 0 result
    odd = (16, 32, 6, 10, 3, 1, 1, False)
    x0, x1, w, dy = random_inputs(odd, device)
    base = run_three(0, odd, x0, x1, w, dy)
    for mode in (2,):
        assert taken(mode, odd) == [0, 0, 0]
        got = run_three(mode, odd, x0, x1, w, dy)
        assert all(torch.equal(got[k], base[k]) for k in base)
    # (24 -> 40 channels: forward and data-gradient are off the LDS-DMA loop; the weight gradient's loop only needs float4 rows)
    assert taken(2, (16, 32, 24, 40, 3, 1, 1, False)) == [0, 0, 2]
    # random data: the split kernel re-associates, so somewhere a last bit differs from the fp32 kernel's
    x0, x1, w, dy = random_inputs(GEOMS[1], device)
    base, nine = run_three(0, GEOMS[1], x0, x1, w, dy), run_three(2, GEOMS[1], x0, x1, w, dy)
    for k in base:
        assert not torch.equal(base[k], nine[k]), "compute=2 %s is bit-identical to compute=0: another kernel did not run" % k


# ---------------------------------------------------------------------------------------------
# 5. error against float64, the fp32 kernel of the same run as the yardstick
# ---------------------------------------------------------------------------------------------
def run_error_gate(device, fullsize):
    """mode 2 <= 3 x the fp32 kernel's error, max and rms (the rule of every re-associated route of this package).  The six-product
    form (mode 3, gate 1.5 x) was measured with the same code before it was withdrawn: identical errors to mode 2 on every line
    (the three small products never reach the result's bits on random data), rms 0.81 - 1.29 x, max 0.81 - 1.37 x the fp32 kernel's
    except the full-size 1x1 forward at max 1.66 x (8.10e-06 against 4.87e-06): over its gate, hence refused.
    fullsize: also the two full-size launches (8.6 / 19 GMAC per direction, sixteen times that through the interpreter: the GPU only)"""
    cases = [((B,) + c) for c in GEOMS] + (FULLSIZE if fullsize else [])
    report, failed = [], []
    for full in cases:
        batch, case = full[0], full[1:]
        x0, x1, w, dy = random_inputs(case, device, batch=batch)
        want = reference64(case, x0, x1, w, dy)

        def run(mode):
            Hh, W, C, Co, k, dil, pad, refl = case
            g = geom(mode, C, Co, k, 1, dil, pad, refl, 0, False)
            wp, wdp = H.pack_weight_both(w)
            return {"forward": H.conv_forward(g, x0, None, wp, None), "data-gradient": H.conv_dgrad(g, dy, wdp, w, (Hh, W))[0],
                    "weight gradient": H.conv_wgrad(g, x0, None, dy)}
        err = {}
        for mode in (0, 2):
            got = run(mode)
            for name in want:
                d = got[name].cpu().double() - want[name]
                err[mode, name] = (float(d.abs().max()), float(d.pow(2).mean().sqrt()))
        for name in want:
            (m0, r0), (m2, r2) = err[0, name], err[2, name]
            line = "%s %-16s max/rms  f32 %.3e %.3e | bf16x9 %.3e %.3e (x%.2f x%.2f)" % (full, name, m0, r0, m2, r2, m2 / m0, r2 / r0)
            print(line)
            report.append(line)
            if not (m2 <= 3.0 * m0 and r2 <= 3.0 * r0):
                failed.append(line)
    assert not failed, "error gate missed:\n" + "\n".join(failed)
    return report


# ---------------------------------------------------------------------------------------------
# 7. switch off is the parent / no leaked state
# ---------------------------------------------------------------------------------------------
def run_switch_off(device):
    assert H.CONV_COMPUTE[0] == "f32" and H.ConvGeom(64, 64, 3, 1, 1, 1).compute == 0
    case = GEOMS[1]
    x0, x1, w, dy = random_inputs(case, device)
    Hh, W, C, Co, k, dil, pad, refl = case

    def plain():
        g = H.ConvGeom(C, Co, k, 1, dil, pad, refl, 0, False)
        assert g.compute == 0
        wp, wdp = H.pack_weight_both(w)
        return (H.conv_forward(g, x0, None, wp, None), H.conv_dgrad(g, dy, wdp, w, (Hh, W))[0], H.conv_wgrad(g, x0, None, dy))
    before = plain()
    with Fn.conv_compute("bf16x9"):
        assert H.CONV_COMPUTE[0] == "bf16x9" and H.ConvGeom(C, Co, k).compute == 2
        with Fn.conv_compute("f32"):
            assert H.ConvGeom(C, Co, k).compute == 0
        assert H.ConvGeom(C, Co, k).compute == 2
        run_three(2, case, x0, x1, w, dy)
    try:
        with Fn.conv_compute("bf16x9"):
            raise KeyError("leave through an exception")
    except KeyError:
        pass
    assert H.CONV_COMPUTE[0] == "f32"
    after = plain()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    for bad in ("bf16", "f16", ""):
        try:
            Fn.conv_compute(bad)
        except ValueError as e:
            assert all(n in str(e) for n in ("f32", "bf16x9", "bf16x6"))
        else:
            raise AssertionError("conv_compute(%r) was accepted" % bad)


# ---------------------------------------------------------------------------------------------
# 8. non-finite in => non-finite out
# ---------------------------------------------------------------------------------------------
def run_non_finite(device):
    case = GEOMS[0]
    Hh, W, C, Co = case[:4]
    for mode in (2,):
        x0, x1, w, dy = random_inputs(case, device)
        x0[1, 3, 5, 7] = float("inf")
        w[9, 11, 0, 0] = float("nan")
        got = run_three(mode, case, x0, x1, w, dy)
        y = got["forward"]
        assert not bool(torch.isfinite(y[1, 3, 5, :]).any()), "an inf operand must reach every output it feeds as a non-finite value"
        assert not bool(torch.isfinite(y[:, :, :, 9]).any()), "a NaN weight must reach every output it feeds"
        rest = torch.ones_like(y, dtype=torch.bool)
        rest[1, 3, 5, :] = False
        rest[:, :, :, 9] = False
        assert bool(torch.isfinite(y[rest]).all()), "non-finite values leaked into outputs the operand does not feed"
        assert not bool(torch.isfinite(got["data-gradient"][:, :, :, 11]).any())       # through the NaN weight
        assert not bool(torch.isfinite(got["weight gradient"][:, 7, 0, 0]).any())      # through the inf activation
