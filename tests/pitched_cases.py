"""Convolution routes and the glue kernels next to them on CHANNEL-SLICE operands: an NHWC tensor that is channels [off, off + C)
of a wider buffer (pixel pitch above the channel count, base pointer at a channel offset), the form in which ConcatFn.backward,
functional._c and the three concat sites of the models hand gradients and features to the kernels.  Shared by
tests/test_pitched_gpu.py (real library) and tests/test_pitched_emu.py (interpreter build of the same sources).

Reference: torch.nn.functional in float64 on the CPU; nothing of the package is called for it.  Every compared tensor obeys the
project's rule for re-associated routes (photometric_cases.py)

    max|pitched - f64| <= 3 * max|dense - f64| + 1e-6 * max|f64|

where "dense" is the same call, at the same route settings, on .contiguous() copies of the operands.

Operands: ``slab(t, off, extra)`` puts t into a fresh [B, H, W, off + C + extra] buffer whose other channels hold finite poison,
i.i.d. normal at 1e3 times the data's scale -- a stray read moves the result far outside the tolerance, while a neighbour lane
that is legitimately loaded and multiplied by a zero weight stays finite.  After every call each buffer must be bit-identical to
its state before the call: inputs are never written.

Route record: around every call the counters WINOGRAD_TAKEN, WINO_FUSED_TAKEN, UPFOLD_TAKEN, CONV_COMPUTE_TAKEN and the
``note`` flags of conv_dgrad are read.  For the placements P1 and P4 (16-byte aligned base, pitch a multiple of 4: what the models
produce) the record must equal the dense call's, so that the file cannot pass because every route quietly fell back; for P0, P2
and P3 a route may decline -- the record goes into RECORDS and the result must still obey the rule."""
import contextlib
import json

import torch
import torch.nn.functional as F

import kernel_cases as KC
from oracle import dropout as OD
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

# name -> (off, extra); P4 = (C, C): one branch of a concat of equal branches, the models' own placement
PLACEMENTS = {"P0": (0, 4), "P1": (4, 4), "P2": (2, 2), "P3": (3, 2), "P4": None}
STRICT = ("P1", "P4")          # the route record must equal the dense call's
ALL_PLACEMENTS = tuple(PLACEMENTS)
POISON = 1e3

RECORDS = []                   # one dict per (case, direction, placement, operand set, tensor)


def placement(name, C):
    p = PLACEMENTS[name]
    return (C, C) if p is None else p


def slab(t, off, extra, seed=0):
    """the NHWC tensor t as channels [off, off + C) of a fresh [B, H, W, off + C + extra] buffer; the slice carries its buffer and
    a bit-exact snapshot of it (``_slab``) for intact()"""
    B, Hh, W, C = t.shape
    scale = float(t.abs().mean()) if t.numel() else 1.0
    gen = torch.Generator().manual_seed(7919 * seed + 13 * off + extra + C)
    buf = (torch.randn(B, Hh, W, off + C + extra, generator=gen) * (POISON * max(scale, 1e-3))).to(t.device)
    buf[..., off:off + C] = t
    s = buf[..., off:off + C]
    s._slab = (buf, buf.clone())
    return s


def intact(s):
    """the buffer around a slab is bit-identical to its state at construction"""
    buf, snap = s._slab
    return bool(torch.equal(buf.view(torch.int32), snap.view(torch.int32)))


@contextlib.contextmanager
def gates(**kw):
    """assign module-level gate constants of hipops for the duration of a case, restored afterwards"""
    old = {k: getattr(H, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(H, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(H, k, v)


_COUNTERS = (("wino", "WINOGRAD_TAKEN"), ("fused", "WINO_FUSED_TAKEN"), ("upfold", "UPFOLD_TAKEN"), ("compute", "CONV_COMPUTE_TAKEN"))


def _counters():
    return {p + "." + k: v for p, name in _COUNTERS for k, v in getattr(H, name).items()}


def recorded(fn, ops):
    """fn(ops, note) -> tuple of tensors; returns (outputs, route record): the counters that moved and the note flags that are set"""
    c0 = _counters()
    note = {}
    outs = fn(ops, note)
    c1 = _counters()
    rec = {k: c1[k] - c0[k] for k in c1 if c1[k] != c0[k]}
    rec.update({"note." + k: True for k in ("actgrad_fused", "skip_accumulated") if note.get(k)})
    return outs, rec


def route_name(rec):
    return "direct" if not rec else " ".join("%s=%d" % (k, int(v)) for k, v in sorted(rec.items()))


def _err(t, want):
    return float((t.detach().double().cpu() - want).abs().max())


def sweep(case, direction, fn, ops, pitchable, wants, placements=ALL_PLACEMENTS, together_only=False, expect=(), extra_bound=None,
          identical=()):
    """One call form on every placement.  fn(ops, note) -> tuple of tensors compared with ``wants`` (float64, CPU, same layout).
    pitchable: the operand names made a slab, one at a time and all together (together_only: just the latter).
    expect: keys the DENSE call's route record must hold -- the route the case is named for; without it the equality of the
    records at P1 / P4 would hold between two fallbacks.
    extra_bound(i, want) -> an absolute error bound every result must also meet (operand modes), or None.
    identical: placements at which every result must be bit-identical to the dense call's (where the record cannot see a
    fallback: CONV_COMPUTE_TAKEN is counted from the launch descriptor, which holds no pointer)."""
    ops = {k: (None if v is None else v.contiguous()) for k, v in ops.items()}
    pitchable = [n for n in pitchable if ops.get(n) is not None]
    dense, rec_d = recorded(fn, ops)
    missing = [k for k in expect if k not in rec_d]
    assert not missing, "%s %s: the dense call did not take its route: %s missing from %s" % (case, direction, missing, route_name(rec_d))
    e_d = [_err(t, w) for t, w in zip(dense, wants)]
    sc = [float(w.abs().max()) for w in wants]
    sets = [tuple(pitchable)] if (together_only or len(pitchable) == 1) else [(n,) for n in pitchable] + [tuple(pitchable)]
    failures = []
    for pname in placements:
        for names in sets:
            o2 = dict(ops)
            for i, n in enumerate(names):
                off, extra = placement(pname, ops[n].shape[3])
                o2[n] = slab(ops[n], off, extra, seed=i)
            outs, rec = recorded(fn, o2)
            what = "%s %s %s [%s]" % (case, direction, pname, "+".join(names))
            for n in names:
                if not intact(o2[n]):
                    failures.append(what + ": the buffer around operand %s was written" % n)
            for i, (t, w) in enumerate(zip(outs, wants)):
                e_p = _err(t, w)
                ok = e_p <= 3.0 * e_d[i] + 1e-6 * sc[i]
                if ok and extra_bound is not None:
                    b = extra_bound(i, w)
                    ok = b is None or e_p <= b
                RECORDS.append(dict(case=case, direction=direction, placement=pname, operands="+".join(names), tensor=i,
                                    route=route_name(rec), dense_route=route_name(rec_d), e_pitched=e_p, e_dense=e_d[i], scale=sc[i],
                                    bit_identical=bool(torch.equal(t, dense[i])), ok=bool(ok)))
                if pname in identical and not torch.equal(t, dense[i]):
                    failures.append("%s: tensor %d is not bit-identical to the dense call's" % (what, i))
                if not ok:
                    failures.append("%s: tensor %d max error %.3e, dense %.3e, scale %.3e (route %s)" % (what, i, e_p, e_d[i], sc[i],
                                                                                                       route_name(rec)))
            if pname in STRICT and rec != rec_d:
                failures.append("%s: route record %s, the dense call's %s" % (what, route_name(rec), route_name(rec_d)))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------ references
_ACT = {"none": lambda t: t, "relu": F.relu, "elu": F.elu, "sigmoid": torch.sigmoid}


def act_derivative(y, act):
    """d act / d pre-activation from the activation's OUTPUT y (float64)"""
    if act == "relu":
        return (y > 0).to(y.dtype)
    if act == "elu":
        return torch.where(y > 0, torch.ones_like(y), y + 1.0)
    if act == "sigmoid":
        return y * (1.0 - y)
    return torch.ones_like(y)


def conv_reference64(x0, x1, w, b, dz, k, stride, dil, pad, reflect, up0, act):
    """float64 convolution of [up2x?(x0) | x1] (NHWC in, NHWC out) and the gradients of its PRE-activation for the upstream dz"""
    a0 = KC.nchw(x0).double().requires_grad_(True)
    a1 = KC.nchw(x1).double().requires_grad_(True) if x1 is not None else None
    wq = w.double().requires_grad_(True)
    xin = F.interpolate(a0, scale_factor=2, mode="nearest") if up0 else a0
    if a1 is not None:
        xin = torch.cat([xin, a1], 1)
    if reflect:
        z = F.conv2d(F.pad(xin, (1, 1, 1, 1), mode="reflect"), wq, None, stride, 0, dil)
    else:
        z = F.conv2d(xin, wq, None, stride, pad, dil)
    z.backward(KC.nchw(dz).double())
    y = _ACT[act](z.detach() + (0 if b is None else b.double().view(1, -1, 1, 1)))
    p = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous()
    return dict(y=p(y), dx0=p(a0.grad), dx1=p(None if a1 is None else a1.grad), dw=wq.grad, dbias=KC.nchw(dz).double().sum((0, 2, 3)))


class ConvData:
    """random operands of one geometry (CPU generator, fixed seed), its float64 reference, and the operands on the device"""

    def __init__(self, device, seed, B, Hh, W, C0, C1, up0, Cout, k=3, stride=1, dil=1, pad=1, reflect=False, bias=False, act="none",
                 scale_w=None):
        gen = torch.Generator().manual_seed(seed)
        H0, W0 = (Hh // 2, W // 2) if up0 else (Hh, W)
        self.hw = (Hh, W)
        x0 = torch.randn(B, H0, W0, C0, generator=gen)
        x1 = torch.randn(B, Hh, W, C1, generator=gen) if C1 else None
        w = torch.randn(Cout, C0 + C1, k, k, generator=gen) * (scale_w if scale_w else (2.0 / (k * k * (C0 + C1))) ** 0.5)
        b = torch.randn(Cout, generator=gen) if bias else None
        e = dil * (k - 1) + 1
        Ho, Wo = (Hh + 2 * pad - e) // stride + 1, (W + 2 * pad - e) // stride + 1
        dz = torch.randn(B, Ho, Wo, Cout, generator=gen)
        ag = F.elu(torch.randn(B, H0, W0, C0, generator=gen))            # x0 as the saved output of a producing ELU
        ysaved = _ACT[act if act != "none" else "elu"](torch.randn(B, Ho, Wo, Cout, generator=gen))
        base0 = torch.randn(B, Hh, W, C0, generator=gen)
        base1 = torch.randn(B, Hh, W, C1, generator=gen) if C1 else None
        self.act, self.bias_on = act, bias
        self.ref = conv_reference64(x0, x1, w, b, dz, k, stride, dil, pad, reflect, up0, act)
        self.ref["dx0_ag"] = self.ref["dx0"] * act_derivative(ag.double(), "elu")
        self.ref["base0"], self.ref["base1"] = base0.double(), None if base1 is None else base1.double()
        self.ref["dz_act"] = dz.double() * act_derivative(ysaved.double(), act if act != "none" else "elu")
        self.ref["colsum"] = dz.double().reshape(-1, Cout).sum(0)
        self.ref["dbias_act"] = self.ref["dz_act"].reshape(-1, Cout).sum(0)
        d = lambda t: None if t is None else t.to(device)
        self.x0, self.x1, self.w, self.b, self.dz, self.ag, self.ysaved = d(x0), d(x1), d(w), d(b), d(dz), d(ag), d(ysaved)
        self.base0, self.base1 = d(base0), d(base1)
        self.geom = (C0, Cout, k, stride, dil, pad, reflect, C1, up0)

    def g(self):
        return H.ConvGeom(*self.geom)       # (built at call time: ConvGeom reads the operand mode when it is constructed)


def conv_sweeps(case, D, placements=ALL_PLACEMENTS, together_only=False, wino=None, fold=False, directions=None, expect=None,
                extra_bound=None, identical=()):
    """forward / data-gradient (plain and through a saved activation output) / weight gradient / colsum / act_backward of one
    geometry.  wino: None, "kn" (one-kernel Winograd packs) or "grouped"; fold: the upsample-folded packs are handed over.
    expect: {direction: record keys of the dense call}, identical: placements (see sweep)."""
    expect = expect or {}
    g = D.g()
    wp, wd = H.pack_weight_both(D.w)
    uf = ud = None
    if wino == "kn":
        uf, ud = H.winograd_fused_pack(D.w, False), H.winograd_fused_pack(D.w, True)
    elif wino == "grouped":
        uf, ud = H.winograd_pack(D.w)
    fd = H.upfold_pack(D.w, g.C0) if fold else None
    wfp = wp if g.reflect else None
    kw = dict(placements=placements, together_only=together_only, identical=identical)
    want = lambda *names: [D.ref[n] for n in names if D.ref[n] is not None]
    some = lambda ts: tuple(t for t in ts if t is not None)
    run = lambda name: directions is None or name in directions
    bound = (lambda name: None if extra_bound is None else (lambda i, w: extra_bound(name, i, w)))

    if run("fwd"):
        sweep(case, "fwd", lambda o, n: (H.conv_forward(g, o["x0"], o["x1"], wp, D.b, D.act, wfold=None if fd is None else fd[0], wino=uf),),
              dict(x0=D.x0, x1=D.x1), ("x0", "x1"), want("y"), expect=expect.get("fwd", ()), extra_bound=bound("fwd"), **kw)
    if run("dgrad"):
        sweep(case, "dgrad", lambda o, n: some(H.conv_dgrad(g, o["dy"], wd, D.w, D.hw, fold=fd, wino=ud, wfpack=wfp, note=n)),
              dict(dy=D.dz), ("dy",), want("dx0", "dx1"), expect=expect.get("dgrad", ()), extra_bound=bound("dgrad"), **kw)
    if run("dgrad_actgrad"):
        sweep(case, "dgrad_actgrad",
              lambda o, n: some(H.conv_dgrad(g, o["dy"], wd, D.w, D.hw, actgrad=(o["ag"], "elu"), fold=fd, wino=ud, wfpack=wfp, note=n)),
              dict(dy=D.dz, ag=D.ag), ("ag", "dy"), want("dx0_ag", "dx1"), expect=expect.get("dgrad_actgrad", ()),
              extra_bound=bound("dgrad"), **kw)
    if run("wgrad"):
        sweep(case, "wgrad", lambda o, n: (H.conv_wgrad(g, o["x0"], o["x1"], o["dy"]),),
              dict(x0=D.x0, x1=D.x1, dy=D.dz), ("x0", "x1", "dy"), want("dw"), expect=expect.get("wgrad", ()),
              extra_bound=bound("wgrad"), **kw)
    if run("colsum"):
        sweep(case, "colsum", lambda o, n: (H.colsum(o["dz"]),), dict(dz=D.dz), ("dz",), want("colsum"), **kw)
    if run("act_backward"):
        a = D.act if D.act != "none" else "elu"
        sweep(case, "act_backward", lambda o, n: H.act_backward(o["dy"], o["y"], a, need_dbias=True),
              dict(dy=D.dz, y=D.ysaved), ("dy", "y"), want("dz_act", "dbias_act"), **kw)


# ------------------------------------------------------------------------------------------- 2. convolution routes: the cases
_BY_NAME = {c[0]: c for c in KC.CONV_CASES}
IGEMM = ["3x3_zero", "7x7_s2_c3",                                                    # scalar gather
         "1x1", "refl_up_cat",                                                       # float4 gather
         "fast_3x3", "fast_refl_up_cat", "fast_refl_cat", "fast_s2", "fast_1x1",     # LDS-DMA fast path
         "lin_1x1_multi", "xtab_w128", "aspp_d6_h16", "w32_refl_up_cat"]
STENCIL = ["disp_c64", "disp_c128_tiny", "disp_strip_c64", "disp_strip_c256", "head_c64_19", "head_c128_22"]
# B, H, W, C0 (upsampled), C1 (skip), Cout.  The folded WEIGHT gradient runs on the table-driven loader only, whose rows -- here
# the rows of one parity class, W / 2 pixels -- must be a multiple of 32 wide (conv_igemm.hip wgrad_mode): of the first two shapes
# (kernel_cases._run_winograd_fused_cases) the launch declines the weight gradient, dense or sliced, so the third
# (kernel_cases.run_upfold_cases), 64 pixels wide, is the one that runs it
UPFOLD_SHAPES = [(1, 8, 16, 64, 64, 64), (1, 20, 12, 128, 64, 128), (1, 8, 64, 32, 32, 64)]
FUSED_SHAPES = [(1, 8, 16, 64, 64), (2, 12, 20, 64, 128)]                             # B, H, W, C, Cout
FUSED_REFLECT_SHAPES = [(2, 12, 24, 64, 64), (1, 10, 36, 64, 64)]
FUSED2_SHAPE = (1, 8, 16, 64, 64, 64)
# the 1st, 5th and 9th row of kernel_cases.run_winograd_fused_wgrad_cases: one source; [upsample | skip]; interior tile blocks
FUSED_WGRAD_SHAPES = [(1, 8, 16, 64, 0, 64, False, False), (2, 8, 16, 64, 32, 64, True, True), (1, 40, 64, 32, 0, 64, False, True)]
GROUPED_SHAPES = [(2, 16, 32, 64, 64, 1), (2, 16, 32, 64, 64, 2)]                     # B, H, W, C, Cout, dilation


def named_data(name, device):
    _, B, Hh, W, C0, C1, up0, Cout, k, stride, dil, pad, reflect, bias, act = _BY_NAME[name]
    return ConvData(device, 100 + KC.CONV_CASES.index(_BY_NAME[name]), B, Hh, W, C0, C1, up0, Cout, k, stride, dil, pad, reflect, bias,
                    act, scale_w=0.2)


def run_named_case(name, device, **kw):
    """an implicit-GEMM, stencil or skinny case of kernel_cases.CONV_CASES, default gates (no Winograd at these sizes)"""
    conv_sweeps(name, named_data(name, device), **kw)


def run_upfold_case(shape, device, **kw):
    B, Hh, W, C0, C1, Co = shape
    D = ConvData(device, 200 + Hh, B, Hh, W, C0, C1, True, Co, reflect=True, bias=True, act="elu")
    with gates(UPFOLD_MIN_SAVED_MACS=0.0):
        assert H.upfold_ok(D.g(), B * Hh * W)
        expect = {"fwd": ("upfold.fwd",), "dgrad": ("upfold.dgrad",), "dgrad_actgrad": ("upfold.dgrad", "note.actgrad_fused")}
        if (W // 2) % 32 == 0:
            expect["wgrad"] = ("upfold.wgrad",)
        conv_sweeps("upfold_%dx%d_%d+%d_%d" % (Hh, W, C0, C1, Co), D, fold=True,
                    directions=("fwd", "dgrad", "dgrad_actgrad", "wgrad"), expect=expect, **kw)


def run_fused_case(shape, device, **kw):
    """one-kernel Winograd, zero padding: forward, forward with statistics, bias + ELU, data-gradient, accumulate"""
    B, Hh, W, C, Co = shape
    case = "wino_fused_%dx%dx%d_%d_%d" % (B, Hh, W, C, Co)
    D = ConvData(device, 300 + Hh, B, Hh, W, C, 0, False, Co)
    Db = ConvData(device, 301 + Hh, B, Hh, W, C, 0, False, Co, bias=True, act="elu")
    with gates(WINOGRAD_MIN_MACS=0.0, WINO_FUSED_REFLECT_DGRAD_MIN_PIX=0):
        g = D.g()
        assert H.winograd_fused_ok(g, B, Hh, W) and H.winograd_fused_ok(g, B, Hh, W, dgrad=True)
        conv_sweeps(case, D, wino="kn", directions=("fwd", "dgrad", "dgrad_actgrad"), **kw,
                    expect={"fwd": ("fused.fwd",), "dgrad": ("fused.dgrad",), "dgrad_actgrad": ("fused.dgrad_actgrad", "note.actgrad_fused")})
        conv_sweeps(case + "_bias_elu", Db, wino="kn", directions=("fwd",), expect={"fwd": ("fused.fwd",)}, **kw)
        wp, wd = H.pack_weight_both(D.w)
        uf, ud = H.winograd_fused_pack(D.w, False), H.winograd_fused_pack(D.w, True)

        def fwd_stats(o, n):
            y, part = H.conv_forward(g, o["x0"], None, wp, None, "none", want_stats=True, wino=uf)
            return y, part[:, 0].sum(0), part[:, 1].sum(0)
        yy = D.ref["y"].reshape(-1, Co)
        sweep(case, "fwd_stats", fwd_stats, dict(x0=D.x0), ("x0",), [D.ref["y"], yy.sum(0), (yy * yy).sum(0)],
              expect=("fused.fwd",), **kw)

        def accumulate(o, n):
            acc = D.base0.clone()                   # the accumulator stays dense, as the binding requires
            r, _ = H.conv_dgrad(g, o["dy"], wd, D.w, D.hw, accumulate_into=acc, wino=ud, note=n)
            if r is None:                           # this operand cannot accumulate in an epilogue: the caller adds
                return (D.base0 + H.conv_dgrad(g, o["dy"], wd, D.w, D.hw, wino=ud, note=n)[0],)
            assert r is acc
            return (acc,)
        sweep(case, "dgrad_accumulate", accumulate, dict(dy=D.dz), ("dy",), [D.ref["base0"] + D.ref["dx0"]],
              expect=("fused.dgrad",), **kw)


def run_fused_reflect_case(shape, device, **kw):
    """mirrored data-gradient on the one-kernel route: with the forward pack (border kernel), without it (direct reflection
    adjoint), and through a saved activation output"""
    B, Hh, W, C, Co = shape
    case = "wino_fused_refl_%dx%dx%d_%d_%d" % (B, Hh, W, C, Co)
    D = ConvData(device, 400 + Hh, B, Hh, W, C, 0, False, Co, reflect=True)
    with gates(WINOGRAD_MIN_MACS=0.0, WINO_FUSED_REFLECT_DGRAD_MIN_PIX=0):
        conv_sweeps(case, D, wino="kn", directions=("fwd", "dgrad", "dgrad_actgrad"), **kw,
                    expect={"fwd": ("fused.fwd",), "dgrad": ("fused.dgrad_refl",),
                            "dgrad_actgrad": ("fused.dgrad_refl", "fused.dgrad_actgrad", "note.actgrad_fused")})
        g = D.g()
        _, wd = H.pack_weight_both(D.w)
        ud = H.winograd_fused_pack(D.w, True)
        sweep(case, "dgrad_no_wfpack", lambda o, n: (H.conv_dgrad(g, o["dy"], wd, D.w, D.hw, wino=ud, note=n)[0],),
              dict(dy=D.dz), ("dy",), [D.ref["dx0"]], **kw)


def run_fused2_case(device, **kw):
    """[up(x0) | x1] forward on the one-kernel route; the skip source's data-gradient on it (dgrad2), also accumulated onto a
    collector (accumulate_skip_into)"""
    B, Hh, W, C0, C1, Co = FUSED2_SHAPE
    case = "wino_fused2_%dx%d_%d+%d_%d" % (Hh, W, C0, C1, Co)
    D = ConvData(device, 500, B, Hh, W, C0, C1, True, Co, reflect=True, bias=True, act="elu")
    with gates(WINOGRAD_MIN_MACS=0.0, WINO_FUSED_REFLECT_DGRAD_MIN_PIX=0, WINO_FUSED2_MIN_FOLD=0.0, UPFOLD_MIN_SAVED_MACS=0.0):
        g = D.g()
        assert H.winograd_fused_ok(g, B, Hh, W) and H.winograd_fused_dgrad2_ok(g, B, Hh, W)
        conv_sweeps(case, D, wino="kn", directions=("fwd",), expect={"fwd": ("fused.fwd2",)}, **kw)
        wp, wd = H.pack_weight_both(D.w)
        ud = H.winograd_fused_pack(D.w, True)
        fd = H.upfold_pack(D.w, C0)
        sweep(case, "dgrad2", lambda o, n: H.conv_dgrad(g, o["dy"], wd, D.w, D.hw, fold=fd, wino=ud, wfpack=wp, note=n),
              dict(dy=D.dz), ("dy",), [D.ref["dx0"], D.ref["dx1"]], expect=("fused.dgrad2", "upfold.dgrad"), **kw)

        def skip_acc(o, n):
            acc = D.base1.clone()
            _, a1 = H.conv_dgrad(g, o["dy"], wd, D.w, D.hw, fold=fd, wino=ud, wfpack=wp, accumulate_skip_into=acc, need0=False, note=n)
            if not n["skip_accumulated"]:           # no route that accumulates took this operand: the caller adds
                return (D.base1 + a1,)
            assert a1 is acc
            return (acc,)
        sweep(case, "dgrad2_accumulate_skip", skip_acc, dict(dy=D.dz), ("dy",), [D.ref["base1"] + D.ref["dx1"]],
              expect=("fused.dgrad2", "note.skip_accumulated"), **kw)


def run_fused_wgrad_case(shape, device, **kw):
    B, Hh, W, C0, C1, Co, up, refl = shape
    D = ConvData(device, 600 + Hh, B, Hh, W, C0, C1, up, Co, reflect=refl)
    with gates(WINOGRAD_MIN_MACS=0.0, WINO_FUSED_WGRAD_MIN_FOLD=0.0):
        assert H.winograd_fused_wgrad_ok(D.g(), B, Hh, W)
        conv_sweeps("wino_fused_wgrad_%dx%dx%d_%d+%d_%d%s%s" % (B, Hh, W, C0, C1, Co, "_up" if up else "", "_refl" if refl else ""), D,
                    directions=("wgrad",), expect={"wgrad": ("fused.wgrad",)}, **kw)


def run_grouped_case(shape, device, **kw):
    B, Hh, W, C, Co, dil = shape
    D = ConvData(device, 700 + dil, B, Hh, W, C, 0, False, Co, dil=dil, pad=dil)
    with gates(WINOGRAD_MIN_CH=32, WINOGRAD_MIN_MACS=0.0, WINO_FUSED=False):
        g = D.g()
        assert H.winograd_ok(g, B, Hh, W) and H.winograd_ok(g, B, Hh, W, dgrad=True)
        conv_sweeps("wino_grouped_%dx%dx%d_%d_%d_d%d" % (B, Hh, W, C, Co, dil), D, wino="grouped", directions=("fwd", "dgrad", "wgrad"),
                    expect={"fwd": ("wino.fwd",), "dgrad": ("wino.dgrad",), "wgrad": ("wino.wgrad",)}, **kw)


# operand modes: the yardstick is the mode's own dense result (the rule above), and the mode's tolerance holds for the pitched
# result as for the dense one -- half precision: 1.5e-3 of the result's maximum (kernel_cases.run_f16_operand_convolutions);
# split bf16: 3 x the fp32 kernel's error (split_bf16_cases.run_error_gate).  The route record of these cases cannot see a launch
# that left the mode's loop (CONV_COMPUTE_TAKEN is counted from the descriptor, and the half-precision mode has no counter), so at
# P0, P1 and P4 the results must be bit-identical to the dense call's.  Dense route per mode: split bf16 -- the split loop forward
# and data-gradient of fast_3x3 (its weight gradient, rows 11 pixels wide, has no table-driven loader and hence no split loop), the
# one-kernel Winograd launches, fp32 kernels that the mode keeps, for the Winograd shape
MODES = ("bf16x9", "f16")


def _fp32_errors(D, wino):
    """errors of the dense fp32 launches of the three directions (the split-bf16 gate's yardstick)"""
    g = D.g()
    assert g.compute == 0
    wp, wd = H.pack_weight_both(D.w)
    uf = ud = None
    if wino == "kn":
        uf, ud = H.winograd_fused_pack(D.w, False), H.winograd_fused_pack(D.w, True)
    return {"fwd": _err(H.conv_forward(g, D.x0, None, wp, D.b, D.act, wino=uf), D.ref["y"]),
            "dgrad": _err(H.conv_dgrad(g, D.dz, wd, D.w, D.hw, wino=ud)[0], D.ref["dx0"]),
            "wgrad": _err(H.conv_wgrad(g, D.x0, None, D.dz), D.ref["dw"])}


def run_mode_case(which, mode, device, **kw):
    """which: "fast_3x3" (implicit GEMM, LDS-DMA loop) or "wino" (the first one-kernel Winograd shape)"""
    if which == "wino":
        B, Hh, W, C, Co = FUSED_SHAPES[0]
        D, wino = ConvData(device, 300 + Hh, B, Hh, W, C, 0, False, Co), "kn"
    else:
        D, wino = named_data(which, device), None
    with gates(WINOGRAD_MIN_MACS=0.0 if wino else H.WINOGRAD_MIN_MACS):
        e32 = _fp32_errors(D, wino)

        def bound(direction, i, w):
            if i > 0:
                return None
            return 1.5e-3 * float(w.abs().max()) if mode == "f16" else 3.0 * e32[direction]
        H.COMPUTE_F16[0] = mode == "f16"
        try:
            with Fn.conv_compute("bf16x9" if mode == "bf16x9" else "f32"):
                assert D.g().compute == (1 if mode == "f16" else 2)
                expect = {}
                if mode == "f16":       # (as run_f16_operand_convolutions: the half-precision kernel shows in the error)
                    g16 = D.g()
                    e16 = _err(H.conv_forward(g16, D.x0, None, H.pack_weight(D.w), D.b, D.act), D.ref["y"])
                    assert e16 > 10 * e32["fwd"], "the dense call did not take the half-precision kernel (%g vs %g)" % (e16, e32["fwd"])
                if mode == "bf16x9":
                    expect = ({"fwd": ("fused.fwd",), "dgrad": ("fused.dgrad",), "wgrad": ("fused.wgrad",)} if wino else
                              {"fwd": ("compute.fwd",), "dgrad": ("compute.dgrad",)})
                conv_sweeps("%s_%s" % (which, mode), D, wino=wino, directions=("fwd", "dgrad", "wgrad"), extra_bound=bound,
                            expect=expect, identical=("P0", "P1", "P4"), **kw)
        finally:
            H.COMPUTE_F16[0] = False


# --------------------------------------------------------------------------------------------------------- 3. glue kernels
RESIZES = [((5, 7), (10, 14)), ((8, 12), (4, 6)), ((1, 1), (6, 9)), ((13, 9), (5, 4))]
GLUE_C = (5, 8, 19)
GAP_SHAPES = [(3, 70, 5, 6), (1, 20, 37, 41), (3, 72, 5, 6)]          # B, C, H, W


def run_resize_case(src, dst, ac, C, device, **kw):
    gen = torch.Generator().manual_seed(31 * src[0] + dst[1] + C)
    x = torch.randn(2, src[0], src[1], C, generator=gen)
    dy = torch.randn(2, dst[0], dst[1], C, generator=gen)
    xr = KC.nchw(x).double().requires_grad_(True)
    y = F.interpolate(xr, size=dst, mode="bilinear", align_corners=ac)
    y.backward(KC.nchw(dy).double())
    case = "resize_%dx%d_%dx%d_ac%d_c%d" % (src + dst + (int(ac), C))
    sweep(case, "fwd", lambda o, n: (H.resize_bilinear(o["x"], dst, ac),), dict(x=x.to(device)), ("x",),
          [y.detach().permute(0, 2, 3, 1).contiguous()], **kw)
    sweep(case, "bwd", lambda o, n: (H.resize_bilinear_backward(o["dy"], src, ac),), dict(dy=dy.to(device)), ("dy",),
          [xr.grad.permute(0, 2, 3, 1).contiguous()], **kw)


def run_gap_case(shape, device, **kw):
    B, C, Hh, W = shape
    gen = torch.Generator().manual_seed(C + W)
    x = torch.randn(B, Hh, W, C, generator=gen) + 1.0
    sweep("gap_%dx%dx%dx%d" % shape, "fwd", lambda o, n: (H.global_avgpool(o["x"]),), dict(x=x.to(device)), ("x",),
          [x.double().mean((1, 2), keepdim=True)], **kw)


def run_pointwise_case(C, device, **kw):
    """scale_channels and nhwc_to_nchw against float64 (both exact: one rounding of a product / a copy), dropout bit-identical to
    the dense call with the same seed, copy_channels into and out of P2 / P3 slices"""
    gen = torch.Generator().manual_seed(C)
    x = (torch.randn(2, 5, 7, C, generator=gen) + 3.0)
    s = torch.rand(2, C, generator=gen) * 2
    xd, sd = x.to(device), s.to(device)
    case = "pointwise_c%d" % C
    sweep(case, "scale_channels", lambda o, n: (H.scale_channels(o["x"], sd),), dict(x=xd), ("x",),
          [x.double() * s.double().view(2, 1, 1, C)], **kw)
    sweep(case, "nhwc_to_nchw", lambda o, n: (H.nhwc_to_nchw(o["x"]),), dict(x=xd), ("x",), [KC.nchw(x).double()], **kw)
    y = H.dropout(xd, 0.3, 12345)
    kept = torch.from_numpy(OD.keep(12345, tuple(x.shape), 0.3)).double()      # the specification's mask (oracle/dropout.py);
    assert torch.equal((y != 0).double().cpu(), kept), (case, "dropout_kernel's mask is not the specification's")      # a witness
    assert 0.5 < float(kept.mean()) < 0.9
    sweep(case, "dropout", lambda o, n: (H.dropout(o["x"], 0.3, 12345),), dict(x=xd), ("x",), [x.double() * kept / (1.0 - 0.3)], **kw)
    for r in RECORDS:
        if r["case"] == case and r["direction"] in ("nhwc_to_nchw", "dropout"):
            assert r["bit_identical"], r
    for pname in ("P2", "P3"):
        off, extra = placement(pname, C)
        src = slab(xd, off, extra, seed=1)
        out = H.copy_channels(src, torch.empty_like(xd))
        assert torch.equal(out, xd) and intact(src), (case, pname, "copy out of a slice")
        dst = slab(torch.zeros_like(xd), off, extra, seed=2)
        H.copy_channels(xd, dst)
        buf, snap = dst._slab
        assert torch.equal(dst, xd), (case, pname, "copy into a slice")
        snap[..., off:off + C] = xd
        assert intact(dst), (case, pname, "copy into a slice wrote outside it")
        dst2 = slab(torch.zeros_like(xd), 3, 2, seed=3)
        H.copy_channels(src, dst2)
        dst2._slab[1][..., 3:3 + C] = xd
        assert torch.equal(dst2, xd) and intact(dst2) and intact(src), (case, pname, "slice to slice")


# ------------------------------------------------------------------------------------------- 4. the three model sites, end to end
WIDTHS = [(64, 64, 64), (8, 6, 3)]
SITE_HW, SITE_B, SITE_CIN = (6, 10), 2, 16
# entry point -> position of dy.  bn_backward is watched besides the four entry points that take gradients from ConvFn, ResizeFn and
# ActGradFn: at the ASPP site every branch ends in BatchNorm + ReLU, so the slices of ConcatFn.backward arrive at bn_backward and at
# none of the other four -- there the "at least one slice" requirement is met by bn_backward alone, as in the model.
SPIED = {"conv_dgrad": 1, "conv_wgrad": 3, "resize_bilinear_backward": 0, "act_backward": 0, "bn_backward": 0}


def install_spy(monkeypatch):
    """wrap the kernels' entry points that receive gradients; returns the list that collects (name, contiguous, data_ptr % 16)"""
    seen = []
    for name, pos in SPIED.items():
        orig = getattr(H, name)

        def wrapper(*a, _orig=orig, _name=name, _pos=pos, **k):
            dy = a[_pos]
            seen.append((_name, bool(dy.is_contiguous()), int(dy.data_ptr() % 16)))
            return _orig(*a, **k)
        monkeypatch.setattr(H, name, wrapper)
    return seen


def _site_modules(site, widths, device):
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
    torch.manual_seed(11)
    tot = sum(widths)
    if site == "pose":
        w = widths[1:]
        m = dict(sq0=L.Conv2d(SITE_CIN, w[0], 1), sq1=L.Conv2d(SITE_CIN, w[1], 1), out=L.Conv2d(sum(w), 32, 3, padding=1))
    elif site == "joint":
        m = dict(p0=L.Conv2d(SITE_CIN, widths[0], 1, bias=False), p1=L.Conv2d(SITE_CIN, widths[1], 1, bias=False),
                 p2=L.Conv2d(SITE_CIN, widths[2], 1, bias=False), out=L.Conv2d(tot, 32, 3, padding=1, bias=False), bn=L.BatchNorm2d(32))
    else:
        m = dict(c0=L.Conv2d(SITE_CIN, widths[0], 1, bias=False), b0=L.BatchNorm2d(widths[0]),
                 c1=L.Conv2d(SITE_CIN, widths[1], 3, padding=2, dilation=2, bias=False), b1=L.BatchNorm2d(widths[1]),
                 c2=L.Conv2d(SITE_CIN, widths[2], 3, padding=3, dilation=3, bias=False), b2=L.BatchNorm2d(widths[2]),
                 out=L.Conv2d(tot, 32, 1))
    for mod in m.values():
        mod.to(device).train()
        if isinstance(mod, torch.nn.BatchNorm2d):
            with torch.no_grad():
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_()
    return m


def _site_inputs(site, gen):
    Hh, W = SITE_HW
    if site == "joint":
        sizes = [(Hh, W), (Hh // 2, W // 2), (2 * Hh, 2 * W)]
    else:
        sizes = [(Hh, W)] * (2 if site == "pose" else 1)
    return [torch.randn(SITE_B, h, w, SITE_CIN, generator=gen) for h, w in sizes]


def _site_forward(site, m, xs):
    """the graph on the package's modules (NHWC)"""
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
    if site == "pose":
        cat = Fn.ConcatFn.apply(m["sq0"](xs[0], act="relu"), m["sq1"](xs[1], act="relu"))
        return m["out"](cat)
    if site == "joint":
        cat = Fn.ConcatFn.apply(*[Fn.resize_bilinear(m["p%d" % i](x), SITE_HW, False) for i, x in enumerate(xs)])
        return m["bn"](m["out"](cat), act="relu")
    res = [L.conv_bn(m["c%d" % i], m["b%d" % i], xs[0], act="relu") for i in range(3)]
    return m["out"](Fn.ConcatFn.apply(*res))


def _site_reference(site, m, xs):
    """the same graph in float64 torch (NCHW), on copies of the parameters"""
    p = {k: {n: t.detach().double().cpu().requires_grad_(True) for n, t in mod.named_parameters()} for k, mod in m.items()}
    conv = lambda k, x, **kw: F.conv2d(x, p[k]["weight"], p[k].get("bias"), **kw)
    bn = lambda k, x: F.batch_norm(x, None, None, p[k]["weight"], p[k]["bias"], training=True, eps=m[k].eps)
    if site == "pose":
        y = conv("out", torch.cat([F.relu(conv("sq0", xs[0])), F.relu(conv("sq1", xs[1]))], 1), padding=1)
    elif site == "joint":
        cat = torch.cat([F.interpolate(conv("p%d" % i, x), size=SITE_HW, mode="bilinear", align_corners=False) for i, x in enumerate(xs)], 1)
        y = F.relu(bn("bn", conv("out", cat, padding=1)))
    else:
        res = [F.relu(bn("b0", conv("c0", xs[0]))), F.relu(bn("b1", conv("c1", xs[0], padding=2, dilation=2))),
               F.relu(bn("b2", conv("c2", xs[0], padding=3, dilation=3)))]
        y = conv("out", torch.cat(res, 1))
    return y, p


def run_site(site, widths, device, seen):
    """output, input gradients and every parameter gradient of one concat site against float64 autograd (rtol 1e-3, atol 1e-4 of
    the tensor's maximum, as the glue check of kernel_cases.run_winograd_cases); ``seen``: install_spy's list, which must hold a
    non-contiguous gradient"""
    gen = torch.Generator().manual_seed(17)
    m = _site_modules(site, widths, device)
    xs = _site_inputs(site, gen)
    xd = [x.to(device).clone().requires_grad_(True) for x in xs]
    y = _site_forward(site, m, xd)
    gy = torch.randn(y.shape, generator=gen)
    del seen[:]
    y.backward(gy.to(device))
    sliced = [s for s in seen if not s[1]]
    assert sliced, "%s %s: no kernel entry point saw a non-contiguous gradient (%s)" % (site, widths, seen)
    xr = [KC.nchw(x).double().requires_grad_(True) for x in xs]
    yr, p = _site_reference(site, m, xr)
    yr.backward(KC.nchw(gy).double())
    close = lambda a, b, what: KC.assert_close(a, b, rtol=1e-3, atol=1e-4 * float(b.abs().max()) / max(1.0, float(b.abs().max())),
                                               what="%s %s: %s" % (site, widths, what))
    close(KC.nchw(y), yr.detach(), "output")
    for i, (a, b) in enumerate(zip(xd, xr)):
        close(KC.nchw(a.grad), b.grad, "gradient of input %d" % i)
    for k, mod in m.items():
        for n, t in mod.named_parameters():
            close(t.grad, p[k][n].grad, "gradient of %s.%s" % (k, n))
    return sliced


# ------------------------------------------------------------------------------------------------------------------ the report
def render_table(records=None):
    """markdown rows for profiles/pitched_operands.md: one per (case, direction, placement) -- the all-operands call's route, the
    worst tensor's errors, and whether every result of that placement was bit-identical to the dense call's"""
    records = RECORDS if records is None else records
    rows, order = {}, []
    for r in records:
        key = (r["case"], r["direction"], r["placement"])
        if key not in rows:
            rows[key] = []
            order.append(key)
        rows[key].append(r)
    out = ["| case | direction | placement | route, all operands sliced | dense route | other routes seen | error pitched | error dense | f64 scale | bit-identical |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for key in order:
        rs = rows[key]
        widest = max(rs, key=lambda r: r["operands"].count("+"))["operands"]
        full = [r for r in rs if r["operands"] == widest]
        worst = max(full, key=lambda r: r["e_pitched"] / max(r["scale"], 1e-30))
        others = sorted({"%s: %s" % (r["operands"], r["route"]) for r in rs if r["route"] != worst["route"]})
        out.append("| %s | %s | %s | %s | %s | %s | %.2e | %.2e | %.2e | %s |" % (
            key + (worst["route"], "=" if worst["dense_route"] == worst["route"] else worst["dense_route"], "; ".join(others) or "-",
                   worst["e_pitched"], worst["e_dense"], worst["scale"], "yes" if all(r["bit_identical"] for r in rs) else "no")))
    return "\n".join(out)


def dump(path):
    with open(path, "w") as f:
        json.dump(RECORDS, f)


if __name__ == "__main__":      # python tests/pitched_cases.py records.json [...]: the table of profiles/pitched_operands.md
    import sys
    print(render_table([r for p in sys.argv[1:] for r in json.load(open(p))]))
