"""Thin tensor-level wrappers over the C ABI (include/segsde_hip.h).

PyTorch is used here for device memory (``torch.empty``), the current HIP stream and dtype/shape checks only;
every arithmetic step is a call into libsegsde_hip.so.  Activations are NHWC fp32 tensors ``[B, H, W, C]`` whose
last dimension is contiguous (a channel slice of a wider buffer is fine: its pixel pitch ``ld`` is passed on).

Which kernel family a convolution runs on is decided in one place, the route plan (forward_routes / backward_routes); by-products
of a call (a kept Winograd transform, an epilogue fusion that was applied) come back in the ``note`` dict the caller passes.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, check

ACT = {"none": 0, "relu": 1, "elu": 2, "sigmoid": 3}


# Optional live kernel timing (bench.py): when set to a list, every implicit-GEMM launch -- and every launch (group) of the
# HBM-bound kernel families, kind "hbm_*" -- is bracketed by HIP events recorded on the stream the kernel is launched on;
# entries are (kind, algorithmic flops (conv_*) or algorithmic bytes (hbm_*: the operands once each), start, end, tag).
PROFILE = None


# Sampled timing: a HIP event pair around a launch drains the stream on both sides (the next kernel's launch latency is
# no longer hidden behind the previous kernel: ~5 us per event, ~2 000 events = 9 ms of a 320 ms cfg3 step when EVERY launch
# is bracketed).  With PROFILE_PERIOD = P the launch with sequence number q of step i is bracketed iff (q + i) % P == 0:
# every launch site is timed in one step out of P, every step carries 1/P of the events; the launches that are not
# bracketed are still recorded (events = None) so that the consumer knows the population.  bench.py sets these.
PROFILE_PERIOD = 1
_profile_state = [0, 0]      # [sequence number inside the step, step index]


def profile_step(i):
    _profile_state[0], _profile_state[1] = 0, int(i)


def _timed(kind, flops, like, launch, tag="", executed=None):
    """executed: the multiply-add work the launch really issues when that is less than the algorithmic figure (the
    upsample-folded convolutions); defaults to ``flops``"""
    if PROFILE is None or not like.is_cuda:
        return launch()
    q = _profile_state[0]
    _profile_state[0] = q + 1
    if PROFILE_PERIOD > 1 and (q + _profile_state[1]) % PROFILE_PERIOD:
        PROFILE.append((kind, flops, None, None, tag, flops if executed is None else executed))
        return launch()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = launch()
    e.record()
    PROFILE.append((kind, flops, s, e, tag, flops if executed is None else executed))
    return r


def _taken(what, kind, flops, like, launch, tag="", executed=None, may_decline=True):
    """one route attempt, timed: True when the launch ran, False when it declined the shape (-4: the caller goes on to its next
    route; an error too where the caller has none, may_decline = False); any other code raises"""
    rc = _timed(kind, flops, like, launch, tag, executed)
    if rc == -4 and may_decline:
        return False
    check(rc, what)
    return True


# Upsample-folded route of the decoder's Conv3x3 on [upsample(x) | skip] (csrc/conv_igemm.hip, "Upsample-folded 3x3
# convolutions"): SEGSDE_UPFOLD=0 keeps the plain 9-tap route (A/B measurements, debugging)
UPFOLD = os.environ.get("SEGSDE_UPFOLD", "1") != "0"
UPFOLD_TAKEN = {"fwd": 0, "dgrad": 0, "wgrad": 0}    # diagnostics / tests: launches that took the folded route


UPFOLD_MIN_SAVED_MACS = float(os.environ.get("SEGSDE_UPFOLD_MIN_MACS", "1e10"))


def upfold_pack(w_oihw, C0):
    """(wfold [4][Cout][2][2][C0], wdfold [C0][4][4][Cout]) of an OIHW 3x3 weight whose first C0 input channels see a
    nearest-upsampled source: the pre-summed 2x2 taps of the four output parity classes / the 4x4 stride-2 kernel of the
    low-resolution data-gradient"""
    w = _f32(w_oihw.detach()).contiguous()
    Cout, Ctot, KH, KW = w.shape
    assert KH == 3 and KW == 3 and 0 < C0 <= Ctot
    wf = torch.empty((4, Cout, 2, 2, C0), dtype=torch.float32, device=w.device)
    wd = torch.empty((C0, 4, 4, Cout), dtype=torch.float32, device=w.device)
    check(_lib.lib().segsde_upfold_pack(_p(w), Cout, C0, Ctot, _p(wf), _p(wd), _stream(w)), "upfold_pack")
    return wf, wd


# Winograd F(2x2,3x3) route of the stride-1 3x3 convolutions with many channels (csrc/winograd.hip, segsde_conv2d_winograd):
# SEGSDE_WINOGRAD=0 keeps the direct implicit GEMM (A/B measurements; the exactness tests of the direct kernels use it)
WINOGRAD = os.environ.get("SEGSDE_WINOGRAD", "1") != "0"
WINOGRAD_MIN_CH = int(os.environ.get("SEGSDE_WINOGRAD_MIN_CH", "256"))
WINOGRAD_MIN_MACS = float(os.environ.get("SEGSDE_WINOGRAD_MIN_MACS", "1e8"))
WINOGRAD_TAKEN = {"fwd": 0, "dgrad": 0, "wgrad": 0}


def winograd_pack(w_oihw, kn=False):
    """(forward pack [16][Cout][Cin], data-gradient pack [16][Cin][Cout]) = G g G^T of an OIHW 3x3 weight; kn: the [16][K][N]
    packs of the one-kernel route instead ([16][Cin][Cout], [16][Cout][Cin])"""
    if kn:
        return winograd_fused_pack(w_oihw, False), winograd_fused_pack(w_oihw, True)
    w = _f32(w_oihw.detach()).contiguous()
    O, I, KH, KW = w.shape
    assert KH == 3 and KW == 3
    uf = torch.empty((16, O, I), dtype=torch.float32, device=w.device)
    ud = torch.empty((16, I, O), dtype=torch.float32, device=w.device)
    check(_lib.lib().segsde_winograd_pack(_p(w), O, I, _p(uf), _p(ud), _stream(w)), "winograd_pack")
    return uf, ud


_WINO_MULTI = {}


def winograd_packs_multi(weights, kn=False):
    """[(forward pack, data-gradient pack)] of many 3x3 weights in ONE launch; the packs are views into a flat buffer that the
    next call with the same weights rewrites (what a training step needs, like pack_weights_multi)"""
    ws = [_f32(w.detach()) for w in weights]
    assert ws and all(w.is_contiguous() and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) for w in ws)
    dev = ws[0].device
    key = (dev, bool(kn), tuple((w.data_ptr(), tuple(w.shape)) for w in ws))
    hit = _WINO_MULTI.get(key)
    if hit is None:
        if len(_WINO_MULTI) > 8:
            _WINO_MULTI.clear()
        total = sum(16 * w.shape[0] * w.shape[1] for w in ws)
        flat = torch.empty(2 * total, dtype=torch.float32, device=dev)
        jobs = (_lib.WinoJob * len(ws))()
        views, off, blk = [], 0, 0
        for i, w in enumerate(ws):
            O, I = w.shape[0], w.shape[1]
            n = 16 * O * I
            if kn:
                uf, ud = _kn(flat[off:off + n].view(16, I, O)), _kn(flat[off + n:off + 2 * n].view(16, O, I))
            else:
                uf, ud = flat[off:off + n].view(16, O, I), flat[off + n:off + 2 * n].view(16, I, O)
            off += 2 * n
            assert not kn or (O % 64 == 0 and I % 64 == 0), "the one-kernel route's pack layout has whole 64-filter blocks only"
            jobs[i] = _lib.WinoJob(w.data_ptr(), uf.data_ptr(), ud.data_ptr(), O, I, blk, 1 if kn else 0)
            blk += 2 * ((O * I + 255) // 256)
            views.append((uf, ud))
        raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
        hit = _WINO_MULTI[key] = (raw, flat, views, len(ws), blk)
    raw, flat, views, n, blk = hit
    check(_lib.lib().segsde_winograd_pack_multi(_p(raw), n, blk, _stream(flat)), "winograd_pack_multi")
    return views


def _winograd(kind, d, x0, x1, upack, want_stats, flops, tag, bias=None, keep_v=False):
    """one grouped-GEMM Winograd convolution [x0 | x1] [B,H,W,C] -> [B,H,W,d.Cout] (descriptor d: ConvGeom.desc for the forward,
    ConvGeom.dgrad_desc for the data-gradient as the convolution of dy with the flipped pack; normalised below); returns (y, partials or None, the
    transformed input if keep_v), or None when the kernel declines"""
    # the route's own copy: its position GEMMs run on the implicit-GEMM kernel, which reads these three fields -- always the fp32
    # loop (compute 0: "fp32 arithmetic either way", also in the split-bf16 mode), no column split, no input divisor
    d = ConvDesc.from_buffer_copy(d)
    d.compute, d.nsplit, d.in_div = 0, 0, 1
    B, H, W, Cout = d.B, d.H, d.W, d.Cout
    L = _lib.lib()
    nbytes = L.segsde_conv2d_winograd_workspace(ctypes.byref(d))
    if not nbytes:
        return None
    y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x0.device)
    part = None
    if want_stats:
        part = torch.empty((int(L.segsde_conv2d_winograd_stats_rows(ctypes.byref(d))), 2, Cout), dtype=torch.float64, device=x0.device)
    ws = _ws(nbytes, x0)
    Tp = (B * (H // 2) * (W // 2) + 127) // 128 * 128          # rows per position plane: whole 128-row GEMM tiles
    vk = torch.empty((16, Tp, d.C0 + d.C1), dtype=torch.float32, device=x0.device) if keep_v else None
    if not _taken("conv2d_winograd", kind, flops, x0, lambda: L.segsde_conv2d_winograd(
            ctypes.byref(d), _p(_f32(x0)), _p(x1), _p(upack), _p(bias), _p(y), _p(part), _p(vk), _p(ws), nbytes, _stream(x0)),
            tag + " wino", executed=flops * 16.0 / 36.0):
        return None
    WINOGRAD_TAKEN["fwd" if kind == "conv_fwd" else "dgrad"] += 1
    return y, part, vk


# ---- Winograd with the transforms inside the kernel (csrc/winograd_fused.hip): 3x3 / stride 1 / padding 1, one source,
# 64 .. 256 channels.  Measured (profiles/probe_r04_winograd_fused.log, B = 16): 1.6-1.7x the direct kernel forward, 1.55x
# data-gradient from 64 channels on, 1.3x the grouped-GEMM route of winograd.hip at 256 channels (168 against 217 us), equal to
# it at 512 (where the grouped route also hands its transformed input to the weight gradient).  SEGSDE_WINO_FUSED=0: off.
WINO_FUSED = os.environ.get("SEGSDE_WINO_FUSED", "1") != "0"
WINO_FUSED_MAX_CH = int(os.environ.get("SEGSDE_WINO_FUSED_MAX_CH", "256"))
# round 5: the decoder's Conv3x3 on [upsample(x) | skip] (mirrored padding) through the same kernel -- upsampling and concat are
# index arithmetic of its patch loader -- instead of the upsample-folded direct route, when the layer's folded multiply-add share
# (4/9 on the upsampled channels, 9/9 on the skip) is above WINO_FUSED2_MIN_FOLD: the route runs all channels at 16/36 but at
# ~0.75 of the direct kernel's multiply-add rate (profiles/probe_r05_*.log)
WINO_FUSED2_MAX_CIN = int(os.environ.get("SEGSDE_WINO_FUSED2_MAX_CIN", "768"))
WINO_FUSED2_MIN_FOLD = float(os.environ.get("SEGSDE_WINO_FUSED2_MIN_FOLD", "0.6"))
# round 5: data-gradients of the mirrored-padding Conv3x3 (zero-padded one-kernel launch + border launches) and data-gradients
# with the activation-derivative epilogue on the one-kernel route.
# the mirrored convolution's data-gradient takes the route from this many pixels on (measured, profiles/probe_r05_winograd_dgrad_*.log:
# 1.35-1.6x from 16 x 64 x 128 pixels; at 16 x 32 x 64 the two border launches -- 64 workgroups with long reductions -- cost more
# than the Winograd launch saves: 395 vs 338 us)
WINO_FUSED_REFLECT_DGRAD_MIN_PIX = int(os.environ.get("SEGSDE_WINO_FUSED_REFLECT_DGRAD_MIN_PIX", str(1 << 17)))
# the skip-source gradient of the decoder's two-source layers (dy -> the C1 encoder channels, mirrored padding, accumulated onto the
# feature's gradient collector) on the one-kernel route -- a column slice of the flipped pack -- while the upsampled source's
# low-resolution gradient stays on the folded route's 4x4 / stride-2 launch.
WINO_FUSED_TAKEN = {"fwd": 0, "dgrad": 0, "fwd2": 0, "dgrad_refl": 0, "dgrad_actgrad": 0, "dgrad2": 0, "wgrad": 0}


class _KnPack(torch.Tensor):
    """a transformed weight pack of the one-kernel route: 16 K N floats, logical shape [16][K][N] (N % 64 == 0), stored in the blocked
    order the kernel reads (include/segsde_hip.h, segsde_winograd_fused_pack) -- a plain tensor with a type the dispatch can see;
    only the library's pack and convolution kernels interpret its contents"""


def _kn(t):
    return t.as_subclass(_KnPack)


def winograd_fused_pack(w_oihw, flip):
    """OIHW 3x3 -> U (logical [16][K][N], see _KnPack for the storage order): flip False = forward pack (K = Cin, N = Cout), True =
    data-gradient pack"""
    O, I = w_oihw.shape[0], w_oihw.shape[1]
    w = _f32(w_oihw.detach()).contiguous()
    u = torch.empty((16, O, I) if flip else (16, I, O), dtype=torch.float32, device=w.device)
    check(_lib.lib().segsde_winograd_fused_pack(_p(w), O, I, 1 if flip else 0, _p(u), _stream(w)), "winograd_fused_pack")
    return _kn(u)


def winograd_fused(kind, x, u_kn, bias=None, act="none", want_stats=False, tag=None, reflect=False, accumulate_into=None, x1=None,
                   up0=False, actgrad=None, adjoint=None, cols=None):
    """[up2x?(x) | x1] [B,H,W,C] NHWC -> act(conv3x3(.) + bias) [B,H,W,N] with u_kn [16][C][N]; (y, statistics partials or None).
    accumulate_into: a dense [B,H,W,N] tensor the result is added onto (and which is returned).
    Data-gradient extras: actgrad = (saved activation output [B,H,W,N], kind): the result is multiplied by the activation's
    derivative; adjoint = the FORWARD pack [Cout][3][3][Cin]: the convolution was mirror-padded -- the gradient of the padding
    cells is added by segsde_reflect_adjoint_borders2 after the zero-padded launch."""
    B, H0, W0, C0 = x.shape
    H, W = (2 * H0, 2 * W0) if up0 else (H0, W0)
    C1 = 0 if x1 is None else x1.shape[3]
    C = C0 + C1
    ldu = u_kn.shape[2]
    n_off, N = (0, ldu) if cols is None else cols       # cols = (first column, count): the gradient of ONE source of a two-source convolution
    assert u_kn.shape[1] == C and n_off + N <= ldu and (cols is None or (actgrad is not None or adjoint is not None or kind == "conv_dgrad"))
    L = _lib.lib()
    if accumulate_into is not None:
        y = accumulate_into
        if tuple(y.shape) != (B, H, W, N) or not y.is_contiguous() or bias is not None or act != "none" or want_stats:
            return None
    else:
        y = torch.empty((B, H, W, N), dtype=torch.float32, device=x.device)
    part = None
    if want_stats:
        part = torch.empty((int(L.segsde_winograd_fused_stats_rows(B, H, W)), 2, N), dtype=torch.float64, device=x.device)
    flops = 2.0 * B * H * W * C * N * 9
    tagf = (tag or "%d+%d->%d k3 s1 d1 %dx%d" % (C0, C1, N, H, W)) + " wino-fused"
    if x1 is not None or up0:
        assert accumulate_into is None and actgrad is None and adjoint is None
        if not _taken("conv2d_winograd_fused2", kind, flops, x, lambda: L.segsde_conv2d_winograd_fused2(
            _p(_f32(x)), nhwc_ld(x), C0, 1 if up0 else 0, _p(x1), nhwc_ld(x1) if x1 is not None else 0, C1, B, H, W, 1 if reflect else 0,
            _p(u_kn), N, _p(bias), ACT[act], _p(y), N, _p(part), _stream(x)), tagf,
            # issued multiply-adds: 16 / 36 of the algorithmic count, 9 / 36 on the channels of a nearest-upsampled source (seven of
            # the sixteen positions are identically zero there and skipped: csrc/winograd_fused.hip, UPSKIP)
                executed=flops * ((9.0 * C0 + 16.0 * C1) / (36.0 * (C0 + C1)) if up0 else 16.0 / 36.0)):
            return None
        WINO_FUSED_TAKEN["fwd2"] += 1
        return y, part
    if actgrad is not None or adjoint is not None or cols is not None:
        assert bias is None and act == "none" and not want_stats and not reflect
        ag_y, ag_kind = (actgrad[0], ACT[actgrad[1]]) if actgrad is not None else (None, 0)
        ag_ld = nhwc_ld(ag_y) if ag_y is not None else 0
        acc = 1 if accumulate_into is not None else 0
        wfpack = adjoint       # (the FORWARD pack of a mirrored convolution, or None)

        def launch():
            u_off = 4 * (n_off // 64) * 256      # a column slice starts n_off / 64 blocks of 256 floats into the blocked layout
            rc = L.segsde_conv2d_winograd_fused_dgrad(_p(_f32(x)), nhwc_ld(x), B, H, W, C, ctypes.c_void_p(u_kn.data_ptr() + u_off), ldu,
                                                      N, _p(y), N, acc, _p(ag_y), ag_ld, ag_kind, _stream(x))
            if rc == 0 and wfpack is not None:
                # the border kernel of csrc/winograd_fused.hip (two launches), forward pack (its channel slice)
                rc = L.segsde_reflect_adjoint_borders2(_p(x), nhwc_ld(x), ctypes.c_void_p(wfpack.data_ptr() + 4 * n_off), wfpack.shape[3],
                                                       _p(y), N, _p(ag_y), ag_ld, ag_kind, B, H, W, N, C, _stream(x))
                if rc == -4:
                    raise RuntimeError("the mirrored-padding launches declined a shape the one-kernel data-gradient took: "
                                       "the zero-padded part is already in dx (hipops.conv_dgrad must gate this)")
            return rc
        if not _taken("conv2d_winograd_fused_dgrad", kind, flops, x, launch, tagf, executed=flops * 16.0 / 36.0):
            return None
        WINO_FUSED_TAKEN["dgrad"] += 1
        WINO_FUSED_TAKEN["dgrad_refl"] += adjoint is not None
        WINO_FUSED_TAKEN["dgrad_actgrad"] += actgrad is not None
        return y, None
    if not _taken("conv2d_winograd_fused", kind, flops, x, lambda: L.segsde_conv2d_winograd_fused(
            _p(_f32(x)), nhwc_ld(x), B, H, W, C, 1 if reflect else 0, _p(u_kn), N, _p(bias), ACT[act], _p(y), N,
            1 if accumulate_into is not None else 0, _p(part), _stream(x)), tagf, executed=flops * 16.0 / 36.0):
        return None
    WINO_FUSED_TAKEN["fwd" if kind == "conv_fwd" else "dgrad"] += 1
    return y, part


def _reflect_borders2_ok(dy, H, W, Cin, Cout):
    """the argument checks of segsde_reflect_adjoint_borders2 (csrc/winograd_fused.hip) on the gradient dy [B,H,W,Cout] -> dx
    [B,H,W,Cin] that conv_dgrad is about to hand it (dx dense, the activation output checked by the caller): asked BEFORE the
    zero-padded launch writes dx"""
    return (H >= 4 and W >= 4 and Cin % 32 == 0 and Cout % 32 == 0 and Cout <= 1024 and nhwc_ld(dy) % 4 == 0
            and dy.data_ptr() % 16 == 0)


# round 5: the weight gradient on the one-kernel Winograd scheme (csrc/winograd_wgrad.hip): every 3x3 / stride-1 layer below 512
# channels whose forward leaves no transformed input behind, incl. the decoder's two-source / upsampled layers when the folded
# route's multiply-add share is above WINO_FUSED_WGRAD_MIN_FOLD.  SEGSDE_WINO_FUSED_WGRAD=0: off
WINO_FUSED_WGRAD = os.environ.get("SEGSDE_WINO_FUSED_WGRAD", "1") != "0"
WINO_FUSED_WGRAD_MAX_CH = int(os.environ.get("SEGSDE_WINO_FUSED_WGRAD_MAX_CH", "256"))
WINO_FUSED_WGRAD_MAX_CIN2 = int(os.environ.get("SEGSDE_WINO_FUSED_WGRAD_MAX_CIN2", "768"))
# (round 6: 0.6 -> 0.4 -- with the zero positions of an upsampled source skipped, the pure upsampled layer 64 -> 64 @512x1024, share
# 4/9, runs 1.23x the folded route: 2272 -> 1849 us, profiles/probe_r06_upskip_wgrad.log)
WINO_FUSED_WGRAD_MIN_FOLD = float(os.environ.get("SEGSDE_WINO_FUSED_WGRAD_MIN_FOLD", "0.4"))


def _fold_frac(g):
    return (4.0 * g.C0 + 9.0 * g.C1) / (9.0 * (g.C0 + g.C1))


# ----------------------------------------------------------------------------------------------
# Route plan: which kernel families a convolution may run on, as a function of its geometry and the [B, H, W] of its virtual input
# (after up0).  This is the one place that holds the policy: ConvFn asks forward_routes once per forward and backward_routes once
# per backward and hands the record to conv_forward / conv_dgrad / conv_wgrad (routes=...), which ask on their own only when
# called without one.  What depends on tensors -- contiguity, pitches and pointer alignment, which packs the caller has, statistics
# together with a bias or an activation, a kernel's own "declined" (-4) -- stays with those three.  The gate constants above are
# read at call time (tests and probes assign them).
# ----------------------------------------------------------------------------------------------
ForwardRoutes = collections.namedtuple("ForwardRoutes", "fused grouped upfold dgrad2 kn_pack")
BackwardRoutes = collections.namedtuple("BackwardRoutes", "dgrad_fused dgrad_grouped dgrad2 wgrad_fused wgrad_grouped wgrad_upfold")
_NO_FORWARD_ROUTE, _NO_BACKWARD_ROUTE = ForwardRoutes(*[False] * 5), BackwardRoutes(*[False] * 6)


def forward_routes(g, B=None, H=None, W=None, skip_grad=True):
    """fused: the one-kernel Winograd forward, incl. its [up(x0) | x1] form; grouped: the grouped-GEMM Winograd forward; upfold: the
    upsample-folded direct forward; dgrad2: the skip-source data-gradient will want the flipped [16][K][N] pack (a backward gate: not
    asked with skip_grad = False); kn_pack: the transformed packs to build are [16][K][N] ones.  B = None: shape-free answers."""
    if g.k != 3 or g.stride != 1:
        return _NO_FORWARD_ROUTE
    # the Winograd routes are fp32 kernels: not taken in the half-precision operand mode (ConvGeom.compute 1; the split-bf16 mode, 2,
    # keeps them: fp32 arithmetic either way), nor with the zero pad channels of a stem
    wino = bool(WINOGRAD) and g.compute != 1 and g.cin_alg is None
    fused = wino and _fused_route(g, False, B, H, W)
    dgrad2 = wino and skip_grad and _dgrad2_route(g, B, H, W)
    return ForwardRoutes(fused, wino and _grouped_route(g, False, B, H, W), _upfold_route(g, None if B is None else B * H * W), dgrad2,
                         fused or dgrad2)


def backward_routes(g, B=None, H=None, W=None):
    """The routes of the data-gradient (one-kernel, grouped, one-kernel for the skip source of a two-source layer whose upsampled
    source stays on the folded route) and of the weight gradient (one-kernel, grouped, upsample-folded), tried in that order"""
    if g.k != 3 or g.stride != 1:
        return _NO_BACKWARD_ROUTE
    upfold = _upfold_route(g, None if B is None else B * H * W)
    if not WINOGRAD or g.compute == 1 or g.cin_alg is not None:          # (as in forward_routes)
        return BackwardRoutes(False, False, False, False, False, upfold)
    return BackwardRoutes(_fused_route(g, True, B, H, W), _grouped_route(g, True, B, H, W), _dgrad2_route(g, B, H, W),
                          _wgrad_fused_route(g, B, H, W), _grouped_route(g, False, B, H, W), upfold)


def _upfold_route(g, pixels):
    """pixels = B * H * W of the output (None: shape test only).  The folded route issues ~10 more launches per direction than
    the plain one (pack, class launches, border launches): it is taken when the multiply-adds it saves -- 5 of 9 taps on the
    C0 upsampled channels -- outweigh ~100 us of launches at ~130 TFLOP/s (cfg1's 2 x 256 x 512 layers stay on the plain route:
    measured 28.9 vs 31.7 ms/step)."""
    if not (UPFOLD and g.up0 and g.reflect and g.dil == 1 and g.pad == 1 and g.C0 % 32 == 0 and g.C1 % 32 == 0 and g.Cout % 32 == 0):
        return False
    return pixels is None or 5.0 * pixels * g.C0 * g.Cout >= UPFOLD_MIN_SAVED_MACS


def _grouped_route(g, dgrad, B, H, W):
    """Shape gate of the grouped-GEMM Winograd route.  Measured (profiles/probe_r04_winograd_gate.log, probe_r04_winograd_route.log):
    with the transforms as separate passes the route wins from 256 channels on (1.4x at 256 channels, 1.8x at 512); at 128 channels
    the transforms' traffic eats the 2.25x fewer multiply-adds.  The multiply-add floor keeps tiny launches (and the small-shape
    golden tests of the direct kernels) on the direct route.  Forward and weight gradient: one or two sources, zero / mirrored
    padding (mirrored: dilation 1), any dilation that divides the map into even sub-lattices.  Data-gradient: one source, zero
    padding."""
    cin, cout = (g.Cout, g.C0) if dgrad else (g.Cin, g.Cout)      # the data-gradient is the convolution Cout -> C0
    if not (g.pad == g.dil and not g.up0 and g.C0 % 4 == 0 and cin % 32 == 0 and cout % 64 == 0
            and min(g.Cin, g.Cout) >= WINOGRAD_MIN_CH and not (g.reflect and g.dil != 1)):
        return False
    if dgrad and (g.C1 or g.reflect):
        return False
    if B is None:
        return True
    if H % (2 * g.dil) or W % (2 * g.dil) or H < 4 * g.dil or W < 4 * g.dil:
        return False
    return 9.0 * B * H * W * g.Cin * g.Cout >= WINOGRAD_MIN_MACS


_FUSED_SHAPE_OK = {}


def _fused_shape_ok(B, H, W, cin, cout):
    """segsde_winograd_fused_ok, remembered per shape (a foreign-function call per convolution and direction shows on the
    launch-bound small workloads)"""
    key = (B, H, W, cin, cout)
    r = _FUSED_SHAPE_OK.get(key)
    if r is None:
        r = _FUSED_SHAPE_OK[key] = bool(_lib.lib().segsde_winograd_fused_ok(B, H, W, cin, cout))
    return r


def _fused_route(g, dgrad, B, H, W):
    """the shapes csrc/winograd_fused.hip takes: 3x3 / stride 1 / padding 1 / dilation 1, channel counts multiples of 64.
    One source at output resolution: up to WINO_FUSED_MAX_CH channels, zero or mirrored padding, forward and data-gradient
    (mirrored: + segsde_reflect_adjoint_borders2).  Forward on [upsample(x0) | x1] (g.up0): C0 % 64 == 0, up to
    WINO_FUSED2_MAX_CIN input channels, when the folded route's multiply-add share is above WINO_FUSED2_MIN_FOLD."""
    cin, cout = (g.Cout, g.C0) if dgrad else (g.Cin, g.Cout)
    if not (WINO_FUSED and g.dil == 1 and g.pad == 1 and cin % 64 == 0 and cout % 64 == 0):
        return False
    if g.up0 or g.C1:
        # two sources without upsampling (the bottleneck-resolution layer) stay on the grouped route, which takes them
        if dgrad or not (g.up0 and g.C0 % 64 == 0 and cin <= WINO_FUSED2_MAX_CIN and cout <= WINO_FUSED_MAX_CH
                         and _fold_frac(g) >= WINO_FUSED2_MIN_FOLD):
            return False
    elif max(cin, cout) > WINO_FUSED_MAX_CH:
        return False
    if B is None:
        return True
    return _fused_shape_ok(B, H, W, cin, cout) and 9.0 * B * H * W * cin * cout >= WINOGRAD_MIN_MACS


def _dgrad2_route(g, B, H, W):
    """the skip-source data-gradient of a [upsample(x0) | x1] -> Cout mirrored 3x3 convolution as the one-kernel Winograd
    convolution Cout -> C1 (+ border kernel)"""
    if not (WINO_FUSED and g.dil == 1 and g.pad == 1 and g.reflect and g.up0 and g.C1 and g.C1 % 64 == 0 and g.Cout % 64 == 0
            and g.C0 % 64 == 0       # (the slice starts on a 64-filter block of the blocked pack layout)
            and g.Cout <= WINO_FUSED_MAX_CH and g.Cin <= WINO_FUSED2_MAX_CIN):
        return False
    if B is None:
        return True
    return (B * H * W >= WINO_FUSED_REFLECT_DGRAD_MIN_PIX and _fused_shape_ok(B, H, W, g.Cout, g.C1)
            and 9.0 * B * H * W * g.C1 * g.Cout >= WINOGRAD_MIN_MACS)


def _wgrad_fused_route(g, B, H, W):
    """the weight gradient on the one-kernel scheme (csrc/winograd_wgrad.hip)"""
    if not (WINO_FUSED and WINO_FUSED_WGRAD and g.dil == 1 and g.pad == 1 and g.C0 % 32 == 0 and g.C1 % 32 == 0 and g.Cout % 64 == 0
            and g.Cout <= WINO_FUSED_WGRAD_MAX_CH):
        return False
    if g.up0 or g.C1:
        if not (g.up0 and g.Cin <= WINO_FUSED_WGRAD_MAX_CIN2 and _fold_frac(g) >= WINO_FUSED_WGRAD_MIN_FOLD):
            return False
    elif g.Cin > WINO_FUSED_WGRAD_MAX_CH:
        return False
    if B is None:
        return True
    return H % 2 == 0 and W % 2 == 0 and H >= 4 and W >= 4 and 9.0 * B * H * W * g.Cin * g.Cout >= WINOGRAD_MIN_MACS


# the gates by name: views of the plan (tests, tools and probes ask these; the package itself asks the plan)
def winograd_ok(g, B=None, H=None, W=None, dgrad=False):
    return backward_routes(g, B, H, W).dgrad_grouped if dgrad else forward_routes(g, B, H, W).grouped


def winograd_fused_ok(g, B=None, H=None, W=None, dgrad=False):
    return backward_routes(g, B, H, W).dgrad_fused if dgrad else forward_routes(g, B, H, W).fused


def winograd_fused_dgrad2_ok(g, B=None, H=None, W=None):
    return backward_routes(g, B, H, W).dgrad2


def winograd_fused_wgrad_ok(g, B=None, H=None, W=None):
    return backward_routes(g, B, H, W).wgrad_fused


def upfold_ok(g, pixels=None):
    """(asked by pixel count, B * H * W of the output, where the plans take a map: their own helper)"""
    return g.k == 3 and g.stride == 1 and _upfold_route(g, pixels)


# the shape-free questions weight_pack_scope asks of an nn.Conv2d before any input is seen
def winograd_static_ok(conv):
    """could this nn.Conv2d ever take the grouped route"""
    return (WINOGRAD and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == conv.dilation
            and conv.in_channels % 32 == 0 and conv.out_channels % 64 == 0
            and min(conv.in_channels, conv.out_channels) >= WINOGRAD_MIN_CH)


def winograd_fused_static_ok(conv):
    """could this nn.Conv2d ever take the one-kernel route"""
    if not (WINOGRAD and WINO_FUSED and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0):
        return False
    if max(conv.in_channels, conv.out_channels) <= WINO_FUSED_MAX_CH:
        return True
    # the decoder's two-source layers ([upsample(x) | skip], mirrored padding)
    return bool(getattr(conv, "reflect", False) and conv.out_channels <= WINO_FUSED_MAX_CH and conv.in_channels <= WINO_FUSED2_MAX_CIN)


def winograd_prepack_layout(conv):
    """the transformed packs weight_pack_scope(model) builds up front: True the one-kernel route's layout, False the grouped, None no pack"""
    return True if winograd_fused_static_ok(conv) else (False if winograd_static_ok(conv) else None)


def _live_tap_frac(g, H, W, wgrad=False):
    """Executed share of a dilated, zero-padded window (csrc/conv_igemm.hip, ConvP::tapskip): tap rows that only see padding
    for a whole 128-pixel tile (forward / data-gradient) or a whole output row (weight gradient, 128-column reduction tiles
    inside one tap row) are not multiplied.  Mirrors the kernels' tile-uniform rule for the reported 'executed' FLOPs; 1.0
    where the rule does not apply."""
    if g.reflect or g.dil <= 1 or g.k <= 1 or g.stride != 1 or g.up0:
        return 1.0
    if wgrad:
        if g.C1 or g.C0 % 128 or W % 32:
            return 1.0
        live = sum(max(0, min(H - 1, H - 1 + g.pad - kh * g.dil) - max(0, g.pad - kh * g.dil) + 1) for kh in range(g.k))
        return live / float(g.k * H)
    if (H * W) % 128 or (128 % W and W % 128):
        return 1.0
    rows = max(1, 128 // W)
    live = total = 0
    for r0 in range(0, H, rows):
        r1 = r0 + rows - 1
        live += sum(1 for kh in range(g.k) if r1 + kh * g.dil - g.pad >= 0 and r0 + kh * g.dil - g.pad <= H - 1)
        total += g.k
    return live / float(total)


def _tag(g, H, W):
    return "%d+%d->%d k%d s%d d%d %dx%d%s%s" % (g.C0, g.C1, g.Cout, g.k, g.stride, g.dil, H, W, " up" if g.up0 else "",
                                                " refl" if g.reflect else "")
PAD_ZERO, PAD_REFLECT, PAD_REFLECT_ADJOINT = 0, 1, 2
COMPUTE_F16 = [False]      # see ConvGeom.compute
# Operand arithmetic of the fp32 convolutions that run on the direct (implicit-GEMM) kernels, read once at import from
# SEGSDE_CONV_COMPUTE and switched by functional.conv_compute: "f32" (default) exact fp32 products on v_mfma_f32_32x32x2_f32;
# "bf16x9": every operand split into three bf16 numbers that sum to it exactly, nine bf16 products per fp32 product on
# v_mfma_f32_32x32x16_bf16 with fp32 accumulation (segsde_conv_desc.compute = 2): fp32 re-associated, not reduced precision.
# The Winograd routes stay taken as with "f32".  "bf16x6" (six products, terms <= 2^-24 of a product dropped; compute = 3) is
# a known name that is refused: measured 0.96-1.34x the fp32 launches, but it missed its error gate (profiles/split_bf16_layers.md).
CONV_COMPUTE_MODES = {"f32": 0, "bf16x9": 2}


def conv_compute_mode(name):
    if name == "bf16x6":
        raise ValueError("SEGSDE_CONV_COMPUTE / conv_compute: 'bf16x6' missed its error gate on the MI355X (max error 1.66x the "
                         "fp32 kernel's, gate 1.5x) and is not shipped; of 'f32', 'bf16x9', 'bf16x6' use 'f32' or 'bf16x9'")
    if name not in CONV_COMPUTE_MODES:
        raise ValueError("SEGSDE_CONV_COMPUTE / conv_compute: %r is not one of 'f32', 'bf16x9', 'bf16x6'" % (name,))
    return name


CONV_COMPUTE = [conv_compute_mode(os.environ.get("SEGSDE_CONV_COMPUTE", "f32"))]
# diagnostics / tests: direct launches made in the split-bf16 mode whose descriptor -- the one handed to the launch -- takes
# the split loop (segsde_conv_compute_taken); nothing is counted, or asked, with the switch off
CONV_COMPUTE_TAKEN = {"fwd": 0, "dgrad": 0, "wgrad": 0}


def _note_compute(d, code, kind):
    if d.compute >= 2 and _lib.lib().segsde_conv_compute_taken(ctypes.byref(d), code) == d.compute:
        CONV_COMPUTE_TAKEN[kind] += 1


# the current stream's handle straight from the C binding (torch.cuda.current_stream(device).cuda_stream builds a Stream object
# per call: 5.4 us x ~600 calls per step showed as 1.4 ms of cfg1's 20 ms step in each of the two host threads)
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    if t.is_cuda:
        if _RAW_STREAM is not None:
            return ctypes.c_void_p(_RAW_STREAM(t.device.index))
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    if not _lib.HOST_POINTERS_OK:
        raise RuntimeError("segsde HIP kernels need tensors on a ROCm device (got %s); there is no CPU path" % t.device)
    return ctypes.c_void_p(0)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _f32(t, name="tensor"):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    return t


# Operand lifetime: ``_p`` hands the C call a bare address, so the tensor behind it must be referenced by a local name of the
# wrapper until ``check`` / ``_timed`` has returned.  Taking the address of ``t.contiguous()`` inline does not do that: for a
# strided ``t`` the copy is released as soon as ``_p`` returns, before the launch, and a second copy of the same size may be given
# its block.  The wrappers therefore bind ``x = _cf32(x)`` / ``x = _c(x)`` on the lines before the call (a contiguous operand is
# returned as it is: no copy on the training path), and buffers a kernel writes or accumulates into go through ``_dense``.
def _c(t):
    return None if t is None else t.contiguous()


def _cf32(t, name="tensor"):
    return _f32(t, name).contiguous()


def _dense(t, name):
    """an operand read or written in place through its address: never with the wrong strides"""
    if t is not None and not t.is_contiguous():
        raise ValueError("%s must be contiguous, got strides %s for shape %s" % (name, t.stride(), tuple(t.shape)))
    return t


def nhwc_ld(t):
    """pixel pitch of an NHWC tensor (validates that it is a dense-row channel slice)"""
    B, H, W, C = t.shape
    sb, sh, sw, sc = t.stride()
    if C > 1 and sc != 1:
        raise ValueError("NHWC tensor must be channel-contiguous")
    ld = sw if W > 1 else (sh if H > 1 else (sb if B > 1 else C))
    if W > 1 and H > 1 and sh != W * ld or (B > 1 and H * W > 1 and sb != H * W * ld) or ld < C:
        raise ValueError("unsupported NHWC strides %s for shape %s" % (t.stride(), tuple(t.shape)))
    return int(ld)


def _ws(nbytes, like):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


# ----------------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------------
class ConvGeom:
    """Static description of one convolution of the reference model (shared by fwd / dgrad / wgrad)."""

    def __init__(self, C0, Cout, k, stride=1, dil=1, pad=0, reflect=False, C1=0, up0=False, cin_alg=None):
        """cin_alg: input channels of the convolution as the REFERENCE defines it when the launch carries zero pad channels
        (network stems: 3 -> 4, 6 -> 8): the algorithmic FLOP count of the bench uses it, the executed count the padded width"""
        self.C0, self.C1, self.Cout, self.k = int(C0), int(C1), int(Cout), int(k)
        self.Cin = self.C0 + self.C1       # (a plain attribute, not a property: the route plan reads it ~10 times per call, and
        #                                    C0 / C1 are fixed at construction -- nothing reassigns them)
        self.cin_alg = int(cin_alg) if cin_alg else None
        self.stride, self.dil, self.pad, self.reflect, self.up0 = int(stride), int(dil), int(pad), bool(reflect), bool(up0)
        # segsde_conv_desc.compute of every launch of this convolution (forward, data-gradient, weight gradient): 1 under the
        # half-precision operand mode of `amp: True` (COMPUTE_F16, set by functional.fp32_region), where the Winograd routes --
        # fp32 kernels, and 16 / 36 of the multiply-adds at 1 / 16 of the fp16 matrix rate -- are not taken; else 2 in the
        # split-bf16 mode (CONV_COMPUTE), 0 by default
        self.compute = 1 if COMPUTE_F16[0] else CONV_COMPUTE_MODES[CONV_COMPUTE[0]]
        if reflect and (self.k != 3 or self.stride != 1 or self.dil != 1 or self.pad != 1):
            raise NotImplementedError("reflection padding is implemented for the reference's 3x3/s1/p1 Conv3x3 only")

    @property
    def CinAlg(self):
        return self.cin_alg if self.cin_alg else self.C0 + self.C1

    def out_hw(self, H, W):
        e = self.dil * (self.k - 1) + 1
        return (H + 2 * self.pad - e) // self.stride + 1, (W + 2 * self.pad - e) // self.stride + 1

    def desc(self, B, H, W, Ho=None, Wo=None, ld0=None, ld1=None, act=0):
        """the launch descriptor as the forward sees the convolution (forward, weight gradient, every upsample-folded entry) on a
        [B, H, W] virtual input; Ho, Wo: of the output (default out_hw), ld0 / ld1: the sources' pixel pitches (default dense)"""
        if Ho is None:
            Ho, Wo = self.out_hw(H, W)
        return ConvDesc(B=B, H=H, W=W, C0=self.C0, C1=self.C1, ld0=self.C0 if ld0 is None else ld0, ld1=self.C1 if ld1 is None else ld1,
                        up0=int(self.up0), Ho=Ho, Wo=Wo, Cout=self.Cout, ldy=self.Cout, ldy2=0, nsplit=0, KH=self.k, KW=self.k,
                        stride=self.stride, dil=self.dil, pad=self.pad, pad_mode=PAD_REFLECT if self.reflect else PAD_ZERO, in_div=1,
                        act=act, sum2x2=0, compute=self.compute)

    def dgrad_desc(self, B, H, W, Ho=None, Wo=None, ld0=None, sum2x2=0, accumulate=0):
        """the data-gradient's: the stride-1 convolution of dy [B,Ho,Wo,Cout] (pitch ld0) with the flipped pack, output columns split
        into dx0 | dx1; sum2x2: the upsample adjoint's 2x2 sum in the epilogue, accumulate: the result is added onto dx0"""
        if Ho is None:
            Ho, Wo = self.out_hw(H, W)
        return ConvDesc(B=B, H=Ho, W=Wo, C0=self.Cout, C1=0, ld0=self.Cout if ld0 is None else ld0, ld1=0, up0=0, Ho=H, Wo=W,
                        Cout=self.Cin, ldy=self.C0, ldy2=self.C1, nsplit=self.C0, KH=self.k, KW=self.k, stride=1, dil=self.dil,
                        pad=(self.k - 1) * self.dil - self.pad, pad_mode=PAD_REFLECT_ADJOINT if self.reflect else PAD_ZERO,
                        in_div=self.stride, act=0, sum2x2=sum2x2, accumulate=accumulate, compute=self.compute)


def pack_weight(w_oihw, for_dgrad=False):
    """OIHW -> [O][KH][KW][I] (forward) or [I][KH][KW][O] flipped (data-gradient)."""
    w = _f32(w_oihw.detach()).contiguous()
    O, I, KH, KW = w.shape
    out = torch.empty((I, KH, KW, O) if for_dgrad else (O, KH, KW, I), dtype=torch.float32, device=w.device)
    check(_lib.lib().segsde_pack_weight(_p(w), _p(out), O, I, KH, KW, int(for_dgrad), _stream(w)), "pack_weight")
    return out


def pack_weight_both(w_oihw):
    """(forward pack, data-gradient pack) of one OIHW weight in a single launch"""
    w = _f32(w_oihw.detach()).contiguous()
    O, I, KH, KW = w.shape
    outf = torch.empty((O, KH, KW, I), dtype=torch.float32, device=w.device)
    outd = torch.empty((I, KH, KW, O), dtype=torch.float32, device=w.device)
    check(_lib.lib().segsde_pack_weight_both(_p(w), _p(outf), _p(outd), O, I, KH, KW, _stream(w)), "pack_weight_both")
    return outf, outd


_MULTI_PACK = {}     # (device, weight pointers / shapes) -> (job table on the device, flat pack buffer, [(fwd view, dgrad view)])


def pack_weights_multi(weights):
    """[(forward pack, data-gradient pack)] of many OIHW weights in ONE launch.  The packs are views into one flat buffer
    that is reused by the next call with the same weights (same storage, same shapes): valid until then -- what a training
    step needs (models/layers.weight_pack_scope), not something to keep."""
    ws = [_f32(w.detach()) for w in weights]
    assert ws and all(w.is_contiguous() and w.dim() == 4 for w in ws)
    dev = ws[0].device
    key = (dev, tuple((w.data_ptr(), tuple(w.shape)) for w in ws))
    hit = _MULTI_PACK.get(key)
    if hit is None:
        if len(_MULTI_PACK) > 8:            # weights were re-allocated (load_state_dict into new storage ...): start over
            _MULTI_PACK.clear()
        total = sum(w.numel() for w in ws)
        flat = torch.empty(2 * total, dtype=torch.float32, device=dev)
        jobs = (_lib.PackJob * (len(ws) + 1))()
        views, off, blk = [], 0, 0
        for i, w in enumerate(ws):
            O, I, KH, KW = w.shape
            n = w.numel()
            f, d = flat[off:off + n].view(O, KH, KW, I), flat[off + n:off + 2 * n].view(I, KH, KW, O)
            off += 2 * n
            tiled = KH * KW <= 9                              # one block per 32 x 32 channel block, transposed through LDS
            jobs[i] = _lib.PackJob(w.data_ptr(), f.data_ptr(), d.data_ptr(), O, I, KH, KW, blk, 1 if tiled else 0)
            blk += ((O + 31) // 32) * ((I + 31) // 32) if tiled else max(1, min(2048, (n + 1023) // 1024))
            views.append((f, d))
        jobs[len(ws)] = _lib.PackJob(None, None, None, 0, 0, 0, 0, blk, 0)
        raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
        hit = _MULTI_PACK[key] = [raw, flat, views, len(ws), blk, 0]
    raw, flat, views, n, blk, gen = hit
    hit[5] = gen = gen + 1
    for f, d in views:       # a graph that still holds the previous contents must not run its data-gradients (ConvFn.backward checks)
        d._segsde_gen = gen
    check(_lib.lib().segsde_pack_weight_both_multi(_p(raw), n, blk, _stream(flat)), "pack_weight_both_multi")
    return views


def conv_forward(g, x0, x1, wpack, bias, act="none", want_stats=False, wfold=None, wino=None, keep_v=False, residual=None,
                 routes=None, note=None):
    """y = act(conv(cat[up?(x0), x1]) + bias).  x0: [B,H0,W0,C0] (H0 = H/2 if g.up0), x1: [B,H,W,C1] or None.
    want_stats: also return the per-tile statistics partials of y for the BatchNorm that follows ([rows,2,Cout] doubles,
    or None when this shape cannot fuse them) -> (y, partials).
    residual: [B,Ho,Wo,Cout] added before the activation, y = act((conv + bias) + residual), on the direct route only
    (segsde_conv2d_forward_residual; no statistics, no Winograd / folded route) -> y, or None when the launch declines the shape
    (the caller then runs the unfused sequence).
    routes: forward_routes(g, B, H, W), if the caller has asked already.  note: a dict that receives "wino_v": the transformed input
    a grouped Winograd launch kept for the weight gradient (keep_v), None on every other route."""
    B, H0, W0, C0 = x0.shape
    H, W = (2 * H0, 2 * W0) if g.up0 else (H0, W0)
    assert C0 == g.C0 and (g.C1 == 0) == (x1 is None)
    if x1 is not None:
        assert tuple(x1.shape) == (B, H, W, g.C1), (tuple(x1.shape), (B, H, W, g.C1))
    Ho, Wo = g.out_hw(H, W)
    y = torch.empty((B, Ho, Wo, g.Cout), dtype=torch.float32, device=x0.device)
    d = g.desc(B, H, W, Ho, Wo, nhwc_ld(x0), nhwc_ld(x1) if x1 is not None else 0, ACT[act])
    L = _lib.lib()
    flops = 2.0 * B * Ho * Wo * g.Cout * g.CinAlg * g.k * g.k
    flops_x = flops * g.Cin / g.CinAlg * _live_tap_frac(g, H, W)   # executed: zero pad channels of a stem are multiplied too, dead tap rows are not
    if note is not None:
        note["wino_v"] = None
    if residual is not None:
        assert not want_stats and wfold is None and wino is None and tuple(residual.shape) == tuple(y.shape)
        if not _taken("conv2d_forward_residual", "conv_fwd", flops, x0, lambda: L.segsde_conv2d_forward_residual(
                ctypes.byref(d), _p(_f32(x0)), _p(x1), _p(wpack), _p(bias), _p(_f32(residual)), nhwc_ld(residual), _p(y), _stream(x0)),
                _tag(g, H, W) + " res", executed=flops_x):
            return None
        _note_compute(d, 0, "fwd")
        return y
    if wino is not None and (not want_stats or (bias is None and act == "none")):
        if routes is None:
            routes = forward_routes(g, B, H, W, skip_grad=False)
        r = None
        if isinstance(wino, _KnPack):
            if routes.fused:
                r = winograd_fused("conv_fwd", x0, wino, bias=bias, act=act, want_stats=want_stats, tag=_tag(g, H, W), reflect=g.reflect,
                                   x1=x1, up0=g.up0)
        elif routes.grouped:
            r = _winograd("conv_fwd", d, x0, x1, wino, want_stats, flops, _tag(g, H, W), bias=bias, keep_v=keep_v)
            if r is not None and note is not None:
                note["wino_v"] = r[2]
        if r is not None:
            return r[:2] if want_stats else r[0]
    if wfold is not None and not want_stats:
        if _taken("conv2d_forward_upfold", "conv_fwd", flops, x0, lambda: L.segsde_conv2d_forward_upfold(
                ctypes.byref(d), _p(_f32(x0)), _p(x1), _p(wpack), _p(wfold), _p(bias), _p(y), _stream(x0)), _tag(g, H, W) + " fold",
                executed=flops * _fold_frac(g)):
            UPFOLD_TAKEN["fwd"] += 1
            _note_compute(d, 4, "fwd")
            return y
    part = None
    if want_stats and bias is None and act == "none":
        rows = int(L.segsde_conv2d_stats_rows(ctypes.byref(d)))
        if rows > 0:
            part = torch.empty((rows, 2, g.Cout), dtype=torch.float64, device=x0.device)
    _timed("conv_fwd", flops, x0, lambda: check(L.segsde_conv2d_forward_stats(
        ctypes.byref(d), _p(_f32(x0)), _p(x1), _p(wpack), _p(bias), _p(y), None, _p(part), _stream(x0)), "conv2d_forward"),
        _tag(g, H, W), executed=flops_x)
    _note_compute(d, 0, "fwd")
    return (y, part) if want_stats else y


def conv_dgrad(g, dy, wdpack, w_oihw, in_hw, need0=True, need1=True, accumulate_into=None, actgrad=None, fold=None, wino=None,
               accumulate_skip_into=None, wfpack=None, routes=None, note=None):
    """Data gradient(s) of conv_forward w.r.t. (x0, x1).  dy: [B,Ho,Wo,Cout]; in_hw = (H, W) of the virtual input.
    wfpack: the FORWARD pack, if the caller has it (the mirrored-padding border kernel of the one-kernel Winograd route reads it;
    without it a mirrored convolution's data-gradient runs on the direct reflection-adjoint kernel).
    Returns (dx0, dx1); dx0 is at the *stored* resolution of x0 (2x2-summed when g.up0).
    accumulate_into: a dense [B,H,W,C0] tensor that already holds another gradient of x0 (single-source, non-upsampled
    convs): the result is ADDED to it in the kernel epilogue and that tensor is returned as dx0 (None is returned instead
    when this shape cannot accumulate in place -- the caller then adds).
    actgrad = (x0_saved, kind): x0 is the OUTPUT of an activation ("relu" / "elu" / "sigmoid"); dx0 is returned already
    multiplied by its derivative, i.e. as the gradient w.r.t. the PRE-activation (fused into the kernel epilogue where the
    shape allows, otherwise by a separate pass).
    routes: backward_routes(g, B, H, W), if the caller has asked already.  note: a dict that receives "actgrad_fused" (actgrad's
    derivative was applied in a kernel epilogue) and "skip_accumulated" (dx1 is accumulate_skip_into, holding the sum), else False."""
    B, Ho, Wo, Cout = dy.shape
    H, W = in_hw
    assert Cout == g.Cout
    note = {} if note is None else note
    note["actgrad_fused"] = note["skip_accumulated"] = False
    if routes is None and wino is not None:
        routes = backward_routes(g, B, H, W)
    dx1 = torch.empty((B, H, W, g.C1), dtype=torch.float32, device=dy.device) if g.C1 else None
    L = _lib.lib()
    flops = 2.0 * B * Ho * Wo * Cout * g.CinAlg * g.k * g.k
    ag_y, ag_ld, ag_kind = None, 0, 0
    if actgrad is not None:
        ag_y, ag_kind = actgrad[0], ACT[actgrad[1]]
        ag_ld = nhwc_ld(ag_y)

    def desc(sum2x2=0, accumulate=0):
        return g.dgrad_desc(B, H, W, Ho, Wo, nhwc_ld(dy), sum2x2, accumulate)

    if isinstance(wino, _KnPack):
        # (a mirrored convolution: the border kernel reads the FORWARD pack; without one the direct reflection-adjoint kernel below)
        if (routes.dgrad_fused and (Ho, Wo) == (H, W)
                and (not g.reflect or (wfpack is not None and B * H * W >= WINO_FUSED_REFLECT_DGRAD_MIN_PIX
                                       and _reflect_borders2_ok(dy, H, W, g.C0, Cout)))
                and (actgrad is None or (ag_ld % 4 == 0 and ag_y.data_ptr() % 16 == 0))):
            r = winograd_fused("conv_dgrad", dy, wino, tag=_tag(g, H, W), accumulate_into=accumulate_into, actgrad=actgrad,
                               adjoint=wfpack if g.reflect else None)
            if r is not None:
                note["actgrad_fused"] = actgrad is not None
                return r[0], None
    elif wino is not None and accumulate_into is None and actgrad is None and routes.dgrad_grouped and (Ho, Wo) == (H, W):
        # zero-padded 3x3 / stride 1, one source: dX is the same convolution of dY with the flipped, transposed kernel
        r = _winograd("conv_dgrad", desc(), dy, None, wino, False, flops, _tag(g, H, W))
        if r is not None:
            return r[0], None

    def launch(d, y, y2, fuse):
        return L.segsde_conv2d_dgrad_actgrad(ctypes.byref(d), _p(_f32(dy)), None, _p(wdpack), None, _p(y), _p(y2), None,
                                             _p(ag_y) if fuse else None, ag_ld if fuse else 0, ag_kind if fuse else 0,
                                             _stream(dy))

    def finish_unfused(dx0):
        """the activation derivative as its own pass (shapes whose epilogue cannot take it)"""
        if actgrad is None or dx0 is None:
            return dx0
        dz, _ = act_backward(dx0, ag_y, actgrad[1])
        return dz

    if accumulate_into is not None:
        acc = accumulate_into
        if g.up0 or g.C1 or tuple(acc.shape) != (B, H, W, g.C0) or not acc.is_contiguous():
            return None, None
        d = desc(0, 1)
        if not _taken("conv2d dgrad (accumulate)", "conv_dgrad", flops, dy, lambda: launch(d, acc, None, actgrad is not None),
                      _tag(g, H, W), executed=flops * _live_tap_frac(g, H, W)):
            return None, None
        _note_compute(d, 1, "dgrad")
        note["actgrad_fused"] = actgrad is not None
        return acc, None
    if g.up0 and fold is not None and accumulate_into is None:
        # upsample-folded route: low-resolution gradient as a 4x4 stride-2 convolution of dy (+ clamp adjoint on the border),
        # skip-channel gradient as the ordinary reflection adjoint over its own channels
        wfold, wdfold = fold
        dx0 = torch.empty((B, H // 2, W // 2, g.C0), dtype=torch.float32, device=dy.device) if need0 else None
        dx1f = dx1 if need1 else None
        # accumulate_skip_into: a dense [B,H,W,C1] tensor that already holds another consumer's gradient of the skip source (the
        # encoder feature both decoders read): the skip launch adds onto it in its epilogue instead of producing a tensor that
        # autograd would add with a 12-byte-per-element pass
        acc1 = accumulate_skip_into
        if dx1f is not None and acc1 is not None and tuple(acc1.shape) == (B, H, W, g.C1) and acc1.is_contiguous():
            dx1f = acc1
        else:
            acc1 = None
        if dx0 is None and dx1f is None:
            return None, None
        # round 5: the skip-source gradient on the one-kernel Winograd route (flipped pack's columns [C0, C0 + C1), border kernel on
        # the forward pack's same channels); the folded call below then computes the upsampled source's gradient only
        w1 = None
        # (a gradient slice off a 16-byte boundary: the border kernel would decline it AFTER the zero-padded launch wrote dx1 -- asked
        # first, as on the single-source route above; such a slice stays on the folded route)
        if (dx1f is not None and isinstance(wino, _KnPack) and wfpack is not None and routes.dgrad2 and (Ho, Wo) == (H, W)
                and _reflect_borders2_ok(dy, H, W, g.C1, Cout)):
            r = winograd_fused("conv_dgrad", dy, wino, tag="%d+0->%d k3 s1 d1 %dx%d refl skip-of-%d+%d" % (Cout, g.C1, H, W, g.C0, g.C1),
                               accumulate_into=acc1, adjoint=wfpack, cols=(g.C0, g.C1))
            if r is not None:
                w1 = r[0]
                WINO_FUSED_TAKEN["dgrad2"] += 1
        if w1 is not None:
            if dx0 is None:
                note["skip_accumulated"] = acc1 is not None
                return None, w1
            dx1f = None
        df = g.desc(B, H, W, Ho, Wo)
        fr = ((4.0 * g.C0 if dx0 is not None else 0.0) + (9.0 * g.C1 if dx1f is not None else 0.0)) / (9.0 * g.Cin)
        if w1 is not None:
            flops = flops * g.C0 / g.Cin          # the skip channels' multiply-adds were counted (and timed) with the Winograd launch
            fr = 4.0 / 9.0
        # (with the skip gradient already in place the folded launch has to take the upsampled source: no decline then)
        if _taken("conv2d_dgrad_upfold" + (" (upsampled source only)" if w1 is not None else ""), "conv_dgrad", flops, dy,
                  lambda: L.segsde_conv2d_dgrad_upfold(
                      ctypes.byref(df), _p(_f32(dy)), nhwc_ld(dy), _p(wdpack), _p(wfold), _p(wdfold), _p(dx0), _p(dx1f),
                      1 if acc1 is not None else 0, _p(ag_y) if dx0 is not None else None, ag_ld, ag_kind, _stream(dy)),
                  _tag(g, H, W) + " fold", executed=flops * fr, may_decline=w1 is None):
            UPFOLD_TAKEN["dgrad"] += 1
            _note_compute(df, 5, "dgrad")
            note["skip_accumulated"] = acc1 is not None
            note["actgrad_fused"] = actgrad is not None and dx0 is not None
            return dx0, (w1 if w1 is not None else dx1f)
    if g.up0:
        # fused: the 2x2 sum of the upsample adjoint happens in the GEMM epilogue (no full-resolution gradient tensor)
        dx0 = torch.empty((B, H // 2, W // 2, g.C0), dtype=torch.float32, device=dy.device)
        d = desc(1)
        if _taken("conv2d dgrad (fused upsample adjoint)", "conv_dgrad", flops, dy, lambda: launch(d, dx0, dx1, actgrad is not None),
                  _tag(g, H, W)):
            note["actgrad_fused"] = actgrad is not None
            _note_compute(d, 1, "dgrad")
            return dx0, dx1
        if actgrad is not None:          # declined with the derivative in its epilogue: once more without (not timed again)
            rc = launch(d, dx0, dx1, False)
            if rc == 0:
                _note_compute(d, 1, "dgrad")
                return finish_unfused(dx0), dx1
            if rc != -4:
                check(rc, "conv2d dgrad (fused upsample adjoint)")
    full0 = torch.empty((B, H, W, g.C0), dtype=torch.float32, device=dy.device)
    d = desc(0)
    fused = actgrad is not None and not g.up0
    if not _taken("conv2d dgrad", "conv_dgrad", flops, dy, lambda: launch(d, full0, dx1, fused), _tag(g, H, W),
                  executed=flops * _live_tap_frac(g, H, W), may_decline=fused):
        fused = False                    # (as above)
        check(launch(d, full0, dx1, False), "conv2d dgrad")
    _note_compute(d, 1, "dgrad")
    if g.up0:
        dx0 = torch.empty((B, H // 2, W // 2, g.C0), dtype=torch.float32, device=dy.device)
        check(L.segsde_upsample2x_backward(_p(full0), g.C0, B, H // 2, W // 2, g.C0, _p(dx0), g.C0, _stream(dy)),
              "upsample2x_backward")
    else:
        dx0 = full0
    note["actgrad_fused"] = fused
    return (dx0 if fused else finish_unfused(dx0)), dx1


def conv_wgrad(g, x0, x1, dy, wino_v=None, out=None, routes=None):
    """dW in OIHW layout.  wino_v: the transformed input the forward's grouped Winograd launch kept (conv_forward's note["wino_v"]),
    if any.  out: a dense [Cout, Cin, k, k] tensor to write into (the parameter's slice of a gradient bucket, ddp.grad_destination).
    routes: backward_routes(g, B, H, W), if the caller has asked already."""
    B, H0, W0, _ = x0.shape
    H, W = (2 * H0, 2 * W0) if g.up0 else (H0, W0)
    _, Ho, Wo, Cout = dy.shape
    assert Cout == g.Cout
    if routes is None:
        routes = backward_routes(g, B, H, W)
    d = g.desc(B, H, W, Ho, Wo, nhwc_ld(x0), nhwc_ld(x1) if x1 is not None else 0)
    L = _lib.lib()
    if out is not None and tuple(out.shape) == (Cout, g.Cin, g.k, g.k) and out.is_contiguous() and out.dtype == torch.float32:
        dw = out
    else:
        dw = torch.empty((Cout, g.Cin, g.k, g.k), dtype=torch.float32, device=dy.device)
    flops = 2.0 * B * Ho * Wo * Cout * g.CinAlg * g.k * g.k
    flops_x = flops * g.Cin / g.CinAlg * _live_tap_frac(g, H, W, wgrad=True)
    same_map = (Ho, Wo) == (H, W)

    def attempt(workspace, launch, what, suffix, executed, x0p, *extra):
        """one route: its workspace size (0: it does not take this descriptor), then the launch"""
        nbytes = workspace(ctypes.byref(d))
        if not nbytes:
            return False
        ws = _ws(nbytes, dy)
        return _taken(what, "conv_wgrad", flops, dy, lambda: launch(
            ctypes.byref(d), x0p, _p(x1), _p(_f32(dy)), nhwc_ld(dy), *extra, _p(dw), _p(ws), nbytes, _stream(dy)),
            _tag(g, H, W) + suffix, executed=executed)

    # (one-kernel: 9 / 36 on the upsampled source's channels where the launch skips its zero positions -- that source carries at
    # least half of the channels, csrc/winograd_wgrad.hip)
    if wino_v is None and routes.wgrad_fused and same_map and attempt(
            L.segsde_conv2d_wgrad_winograd_fused_workspace, L.segsde_conv2d_wgrad_winograd_fused, "conv2d_wgrad_winograd_fused",
            " wino-fused", flops * ((9.0 * g.C0 + 16.0 * g.C1) / (36.0 * g.Cin) if (g.up0 and 2 * g.C0 >= g.Cin) else 16.0 / 36.0),
            _p(_f32(x0))):
        WINO_FUSED_TAKEN["wgrad"] += 1
        return dw
    if routes.wgrad_grouped and same_map and attempt(L.segsde_conv2d_wgrad_winograd_workspace, L.segsde_conv2d_wgrad_winograd,
                                                     "conv2d_wgrad_winograd", " wino", flops * 16.0 / 36.0, _p(x0), _p(wino_v)):
        WINOGRAD_TAKEN["wgrad"] += 1
        return dw
    if routes.wgrad_upfold and attempt(L.segsde_conv2d_wgrad_upfold_workspace, L.segsde_conv2d_wgrad_upfold, "conv2d_wgrad_upfold",
                                       " fold", flops * _fold_frac(g), _p(x0)):
        UPFOLD_TAKEN["wgrad"] += 1
        _note_compute(d, 6, "wgrad")
        return dw
    nbytes = L.segsde_conv2d_wgrad_workspace(ctypes.byref(d))
    ws = _ws(nbytes, dy)
    _timed("conv_wgrad", flops, dy, lambda: check(L.segsde_conv2d_wgrad(
        ctypes.byref(d), _p(x0), _p(x1), _p(_f32(dy)), nhwc_ld(dy), _p(dw), _p(ws), nbytes, _stream(dy)), "conv2d_wgrad"),
        _tag(g, H, W), executed=flops_x)
    _note_compute(d, 2, "wgrad")
    return dw


def conv_compute_taken(g, B, H, W, direction, fold=False):
    """The operand arithmetic (0 fp32, 1 fp16, 2 split bf16) the DIRECT kernels will run convolution g in on a [B, H, W] virtual
    input with dense tensors (segsde_conv_compute_taken: the launchers' own dispatch, nothing is launched).  direction: "fwd",
    "dgrad", "wgrad"; fold: the upsample-folded entry point of that direction (g.up0).  Says nothing about the Winograd routes,
    which are fp32 kernels and are chosen before the direct ones (winograd_ok, winograd_fused_ok ...)."""
    code = {"fwd": 0, "dgrad": 1, "wgrad": 2}[direction] | (4 if fold else 0)
    d = g.dgrad_desc(B, H, W) if (direction == "dgrad" and not fold) else g.desc(B, H, W)
    return int(_lib.lib().segsde_conv_compute_taken(ctypes.byref(d), code))


def split_bf16(x):
    """(h, m, l): the three bf16 numbers (as float32 tensors of x's shape) the split-bf16 convolution loops make of every fp32
    operand, h + m + l == x exactly (segsde_split_bf16_planes)"""
    x = _f32(x).contiguous()
    out = [torch.empty(x.shape, dtype=torch.int16, device=x.device) for _ in range(3)]
    check(_lib.lib().segsde_split_bf16_planes(_p(x), x.numel(), _p(out[0]), _p(out[1]), _p(out[2]), _stream(x)), "split_bf16_planes")
    return tuple((t.to(torch.int32) << 16).view(torch.float32) for t in out)


# ----------------------------------------------------------------------------------------------
# BatchNorm / activations / pooling / resampling
# ----------------------------------------------------------------------------------------------
def _rows(t):
    """(M, C, ld) of an NHWC (or [M, C]) tensor"""
    if t.dim() == 2:
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError("[M, C] tensor must be channel-contiguous, got strides %s for shape %s" % (t.stride(), tuple(t.shape)))
        return t.shape[0], t.shape[1], int(t.stride(0)) if t.shape[0] > 1 else t.shape[1]
    B, H, W, C = t.shape
    return B * H * W, C, nhwc_ld(t)


def bn_stats(x, running_mean, running_var, momentum, eps, update_running=True, num_batches_tracked=None):
    M, C, ld = _rows(x)
    L = _lib.lib()
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    nb = L.segsde_bn_stats_workspace(M, C)
    ws = _ws(nb, x)
    _timed('hbm_bn_stats', 4.0 * M * C, x, lambda: check(L.segsde_bn_stats(_p(_f32(x)), ld, M, C, _p(mean), _p(invstd), _p(running_mean if update_running else None),
                            _p(running_var if update_running else None), float(momentum), float(eps),
                            _p(num_batches_tracked), _p(ws), nb, _stream(x)), "bn_stats"))
    return mean, invstd


_BN_PARTIALS_WS = {}          # channel count -> workspace bytes (a pure function of C)


def bn_stats_from_partials(part, M, running_mean, running_var, momentum, eps, update_running=True, num_batches_tracked=None):
    """batch statistics from the partial sums a conv_forward(want_stats=True) launch produced (same outputs / running
    update as bn_stats, without reading the activation tensor again)"""
    rows, _, C = part.shape
    L = _lib.lib()
    mi = torch.empty((2, C), dtype=torch.float32, device=part.device)      # one allocation: ~70 calls per step of the small workloads
    mean, invstd = mi[0], mi[1]
    nb = _BN_PARTIALS_WS.get(C)
    if nb is None:
        nb = _BN_PARTIALS_WS[C] = L.segsde_bn_stats_from_partials_workspace(C)
    ws = _ws(nb, part)
    check(L.segsde_bn_stats_from_partials(_p(part), rows, M, C, _p(mean), _p(invstd),
                                          _p(running_mean if update_running else None),
                                          _p(running_var if update_running else None), float(momentum), float(eps),
                                          _p(num_batches_tracked), _p(ws), nb, _stream(part)), "bn_stats_from_partials")
    return mean, invstd


def bn_eval_stats(running_mean, running_var, eps):
    C = running_mean.numel()
    mean = torch.empty(C, dtype=torch.float32, device=running_mean.device)
    invstd = torch.empty_like(mean)
    check(_lib.lib().segsde_bn_eval_stats(_p(running_mean), _p(running_var), C, float(eps), _p(mean), _p(invstd),
                                          _stream(running_mean)), "bn_eval_stats")
    return mean, invstd


def bn_fold(pairs, cb=None, gamma=None, beta=None, running_mean=None, running_var=None, eps=1e-5):
    """A frozen BatchNorm folded into the convolution in front of it (segsde_bn_fold): ``bn_fold(w, cb, gamma, beta, running_mean,
    running_var, eps) -> (w', b')`` with w' = w * s per output channel, b' = beta - running_mean * s (+ cb * s), s = gamma /
    sqrt(running_var + eps); cb / gamma / beta may be None (no conv bias; affine=False).  ``bn_fold([(w, cb, gamma, beta,
    running_mean, running_var, eps), ...]) -> [(w', b'), ...]``: the pairs of a whole model in ONE launch."""
    single = isinstance(pairs, torch.Tensor)
    if single:
        pairs = [(pairs, cb, gamma, beta, running_mean, running_var, eps)]
    assert pairs
    dev = pairs[0][0].device
    jobs = (_lib.BnFoldJob * (len(pairs) + 1))()
    outs, keep, blk = [], [], 0
    for i, (w, b, ga, be, rm, rv, e) in enumerate(pairs):
        w = _f32(w.detach(), "weight").contiguous()
        O, I, KH, KW = w.shape
        vecs = [None if t is None else _f32(t.detach()).contiguous() for t in (b, ga, be, rm, rv)]
        assert vecs[3] is not None and vecs[4] is not None and all(t is None or (t.numel() == O and t.device == dev) for t in vecs)
        assert w.device == dev
        wo, bo = torch.empty_like(w), torch.empty(O, dtype=torch.float32, device=dev)
        jobs[i] = _lib.BnFoldJob(w.data_ptr(), *[0 if t is None else t.data_ptr() for t in vecs], wo.data_ptr(), bo.data_ptr(),
                                 float(e), O, I, KH, KW, blk, 0)
        blk += max(1, min(2048, (w.numel() + 1023) // 1024))
        outs.append((wo, bo))
        keep.append((w, vecs))                       # contiguous copies stay alive until the launch is queued
    jobs[len(pairs)] = _lib.BnFoldJob(0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, blk, 0)
    raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
    check(_lib.lib().segsde_bn_fold(_p(raw), len(pairs), blk, _stream(outs[0][0])), "bn_fold")
    return outs[0] if single else outs


def bn_apply(x, mean, invstd, gamma, beta, residual=None, act="none", drop_p=0.0, seed=0, out=None):
    M, C, ld = _rows(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device) if out is None else out
    ldr = _rows(residual)[2] if residual is not None else 0
    _timed('hbm_bn_apply', (8.0 + (4.0 if residual is not None else 0.0)) * M * C, x, lambda: check(_lib.lib().segsde_bn_apply(_p(x), ld, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(residual), ldr, _p(y),
                                     _rows(y)[2], ACT[act], float(drop_p), int(seed), _stream(x)), "bn_apply"))
    return y


def bn_apply_mask(x, mean, invstd, gamma, beta, residual=None, act="none"):
    """bn_apply that also packs the sign of its output, one bit per element of the [M][C] index space (segsde_bn_apply_mask), for
    bn_backward(mask=...).  Returns (y, mask); mask is None where the kernel has no mask flavour (channel counts that are no
    multiple of 4, unaligned pitches / pointers) -- y then comes from the plain kernel and the backward pass reads it."""
    M, C, ld = _rows(x)
    L = _lib.lib()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ldr = _rows(residual)[2] if residual is not None else 0
    nbytes = (8.0 + (4.0 if residual is not None else 0.0)) * M * C
    if C % 4 == 0:
        mask = torch.empty(L.segsde_bn_mask_words(M, C), dtype=torch.int32, device=x.device)
        if _taken("bn_apply_mask", 'hbm_bn_apply', nbytes + 0.125 * M * C, x, lambda: L.segsde_bn_apply_mask(
                _p(x), ld, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(residual), ldr, _p(y), _rows(y)[2], ACT[act], 0.0, 0,
                _p(mask), _stream(x))):
            return y, mask
    _timed('hbm_bn_apply', nbytes, x, lambda: check(L.segsde_bn_apply(_p(x), ld, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(residual), ldr, _p(y),
                                                                       _rows(y)[2], ACT[act], 0.0, 0, _stream(x)), "bn_apply"))
    return y, None


def bn_backward(dy, y, x, mean, invstd, gamma, act="none", drop_p=0.0, seed=0, batch_stats=True, need_dx=True,
                need_dres=False, beta=None, dgamma_out=None, dbeta_out=None, mask=None, note=None):
    """y=None selects the remask mode of segsde_bn_backward (act none / plain ReLU: mask recomputed from x, beta needed).
    dgamma_out / dbeta_out: dense [C] tensors to write into (gradient-bucket slices, ddp.grad_destination).
    mask: the bits bn_apply_mask packed (ReLU, no dropout): segsde_bn_backward_mask reads them in place of y, with bit-identical
    results; where that entry does not take the call (pitch / alignment of dy or of the destinations) the saved y is read.
    note: a dict that receives "mask_used": did this call read the packed bits."""
    M, C, ldx = _rows(x)
    L = _lib.lib()

    def _dst(t):
        ok = t is not None and tuple(t.shape) == (C,) and t.is_contiguous() and t.dtype == torch.float32
        return t if ok else torch.empty(C, dtype=torch.float32, device=x.device)
    dgamma, dbeta = _dst(dgamma_out), _dst(dbeta_out)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_dx else None
    dres = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_dres else None
    nb = L.segsde_bn_backward_workspace(M, C)
    ws = _ws(nb, x)
    if note is not None:
        note["mask_used"] = False
    if mask is not None:
        # both passes read dy, x and 1 bit per element: reduce 8.125, apply 8.125 + the tensors it writes
        # (without a saved y there is nothing to fall back on: a decline is an error then)
        if _taken("bn_backward_mask", 'hbm_bn_backward', (16.25 + (4.0 if need_dx else 0.0) + (4.0 if need_dres else 0.0)) * M * C, x,
                  lambda: L.segsde_bn_backward_mask(_p(_f32(dy)), _rows(dy)[2], _p(mask), _p(x), ldx, M, C, _p(mean), _p(invstd),
                                                    _p(gamma), ACT[act], float(drop_p), int(batch_stats), _p(dgamma), _p(dbeta),
                                                    _p(dx), C, _p(dres), C, _p(ws), nb, _stream(x)), may_decline=y is not None):
            if note is not None:
                note["mask_used"] = True
            return dx, dres, dgamma, dbeta
    _timed('hbm_bn_backward', (8.0 + (4.0 if y is not None else 0.0) + (4.0 if need_dx else 0.0) + (4.0 if need_dres else 0.0)) * M * C + 8.0 * M * C, x, lambda: check(L.segsde_bn_backward(_p(_f32(dy)), _rows(dy)[2], _p(y), _rows(y)[2] if y is not None else ldx, _p(x), ldx, M, C,
                               _p(mean), _p(invstd), _p(gamma), _p(beta), ACT[act], float(drop_p), int(seed), int(batch_stats), _p(dgamma), _p(dbeta),
                               _p(dx), C, _p(dres), C, _p(ws), nb, _stream(x)), "bn_backward"))
    return dx, dres, dgamma, dbeta


# ---- cross-replica BatchNorm: the four stages of segsde_bn_sync_* (the all-gather between them is the caller's: functional.BNActFn)
_BN_SYNC_ROW = {}             # channel count -> doubles per exchange row (a pure function of C)


def bn_sync_row_len(C):
    """doubles in one exchange row: C sums, C second sums, the row count, padding to 16 bytes (include/segsde_hip.h)"""
    n = _BN_SYNC_ROW.get(C)
    if n is None:
        n = _BN_SYNC_ROW[C] = _lib.lib().segsde_bn_sync_row_bytes(C) // 8
    return n


def bn_sync_stats_local(x, partials=None):
    """this rank's statistics row (float64 [bn_sync_row_len(C)]) from x, or from the partial sums [rows][2][C] a
    conv_forward(want_stats=True) launch left behind (x then only gives the row count)"""
    M, C, ld = _rows(x)
    L = _lib.lib()
    row = torch.empty(bn_sync_row_len(C), dtype=torch.float64, device=x.device)
    if partials is not None:
        nb = _BN_PARTIALS_WS.get(C)
        if nb is None:
            nb = _BN_PARTIALS_WS[C] = L.segsde_bn_stats_from_partials_workspace(C)
        ws = _ws(nb, x)
        check(L.segsde_bn_sync_stats_local_from_partials(_p(partials), partials.shape[0], M, C, _p(row), _p(ws), nb, _stream(x)),
              "bn_sync_stats_local_from_partials")
        return row
    nb = L.segsde_bn_stats_workspace(M, C)
    ws = _ws(nb, x)
    _timed('hbm_bn_stats', 4.0 * M * C, x, lambda: check(L.segsde_bn_sync_stats_local(_p(_f32(x)), ld, M, C, _p(row), _p(ws), nb, _stream(x)),
                                                         "bn_sync_stats_local"))
    return row


def bn_sync_stats_global(rows, C, running_mean, running_var, momentum, eps, update_running=True, num_batches_tracked=None):
    """rows: the gathered table, float64 [W, bn_sync_row_len(C)] in rank order -> (mean, invstd, inv_count); inv_count is the
    device float 1 / (float)M_total that bn_sync_backward_global reads"""
    rows = _dense(rows, "rows")
    W = rows.shape[0]
    if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != bn_sync_row_len(C):
        raise ValueError("rows must be float64 [W, %d], got %s %s" % (bn_sync_row_len(C), rows.dtype, tuple(rows.shape)))
    mi = torch.empty((3, C), dtype=torch.float32, device=rows.device)     # one allocation; inv_count is mi[2, :1]
    mean, invstd, inv_count = mi[0], mi[1], mi[2, :1]
    check(_lib.lib().segsde_bn_sync_stats_global(_p(rows), W, C, _p(mean), _p(invstd), _p(running_mean if update_running else None),
                                                 _p(running_var if update_running else None), float(momentum), float(eps),
                                                 _p(num_batches_tracked), _p(inv_count), _stream(rows)), "bn_sync_stats_global")
    return mean, invstd, inv_count


def bn_sync_backward_local(dy, y, x, mean, invstd, gamma, act="none", drop_p=0.0, seed=0, need_dres=False, beta=None,
                           dgamma_out=None, dbeta_out=None, mask=None):
    """the reductions of bn_backward, stopped after the fold -> (row, dgamma, dbeta, mask_used): this rank's float dgamma / dbeta
    (written into dgamma_out / dbeta_out where given) and the same sums as the float64 exchange row.  y=None: the remask mode;
    mask: the packed ReLU bits, read in place of y where segsde_bn_backward_mask would take the call (else y is)."""
    M, C, ldx = _rows(x)
    L = _lib.lib()

    def _dst(t):
        ok = t is not None and tuple(t.shape) == (C,) and t.is_contiguous() and t.dtype == torch.float32
        return t if ok else torch.empty(C, dtype=torch.float32, device=x.device)
    dgamma, dbeta = _dst(dgamma_out), _dst(dbeta_out)
    row = torch.empty(bn_sync_row_len(C), dtype=torch.float64, device=x.device)
    nb = L.segsde_bn_backward_workspace(M, C)
    ws = _ws(nb, x)
    lddy = _rows(dy)[2]
    if mask is not None:
        if _taken("bn_sync_backward_local_mask", 'hbm_bn_backward', 8.125 * M * C, x,
                  lambda: L.segsde_bn_sync_backward_local(_p(_f32(dy)), lddy, _p(None), 0, _p(mask), _p(x), ldx, M, C, _p(mean), _p(invstd),
                                                          _p(gamma), _p(None), ACT[act], float(drop_p), 0, int(need_dres), _p(dgamma),
                                                          _p(dbeta), _p(row), _p(ws), nb, _stream(x)), may_decline=y is not None):
            return row, dgamma, dbeta, True
    ldy = _rows(y)[2] if y is not None else ldx
    _timed('hbm_bn_backward', (8.0 + (4.0 if y is not None else 0.0)) * M * C, x, lambda: check(L.segsde_bn_sync_backward_local(
        _p(_f32(dy)), lddy, _p(y), ldy, _p(None), _p(x), ldx, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), ACT[act], float(drop_p),
        int(seed), int(need_dres), _p(dgamma), _p(dbeta), _p(row), _p(ws), nb, _stream(x)), "bn_sync_backward_local"))
    return row, dgamma, dbeta, False


def bn_sync_backward_global(rows, inv_count, dy, y, x, mean, invstd, gamma, act="none", drop_p=0.0, seed=0, need_dx=True,
                            need_dres=False, beta=None, mask=None):
    """rows: the gathered backward rows, float64 [W, bn_sync_row_len(C)] -> (dx, dres): the apply pass of bn_backward with the
    sums over all ranks and 1 / M_total (inv_count, from bn_sync_stats_global).  mask: pass it exactly when the local stage read it."""
    M, C, ldx = _rows(x)
    rows = _dense(rows, "rows")
    if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != bn_sync_row_len(C):
        raise ValueError("rows must be float64 [W, %d], got %s %s" % (bn_sync_row_len(C), rows.dtype, tuple(rows.shape)))
    W = rows.shape[0]
    L = _lib.lib()
    tot = torch.empty((2, C + (-C) % 4), dtype=torch.float32, device=x.device)      # both totals 16-byte aligned
    dg, db = tot[0], tot[1]
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_dx else None
    dres = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_dres else None
    lddy = _rows(dy)[2]
    nbytes = ((8.0 if (need_dx or mask is None and y is None) else 4.0) + (4.0 if need_dx else 0.0) + (4.0 if need_dres else 0.0)) * M * C
    if mask is not None:
        if _taken("bn_sync_backward_global_mask", 'hbm_bn_backward', nbytes + 0.125 * M * C, x,
                  lambda: L.segsde_bn_sync_backward_global(_p(_f32(dy)), lddy, _p(None), 0, _p(mask), _p(x), ldx, M, C, _p(mean),
                                                           _p(invstd), _p(gamma), _p(None), ACT[act], float(drop_p), 0, _p(rows), W,
                                                           _p(inv_count), _p(dg), _p(db), _p(dx), C, _p(dres), C, _stream(x)),
                  may_decline=y is not None):
            return dx, dres
    ldy = _rows(y)[2] if y is not None else ldx
    _timed('hbm_bn_backward', nbytes + (4.0 if y is not None else 0.0) * M * C, x, lambda: check(L.segsde_bn_sync_backward_global(
        _p(_f32(dy)), lddy, _p(y), ldy, _p(None), _p(x), ldx, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), ACT[act], float(drop_p),
        int(seed), _p(rows), W, _p(inv_count), _p(dg), _p(db), _p(dx), C, _p(dres), C, _stream(x)), "bn_sync_backward_global"))
    return dx, dres


def act_backward(dy, y, act, need_dbias=False, need_dz=True):
    M, C, ldy = _rows(y)
    L = _lib.lib()
    dz = torch.empty(y.shape, dtype=torch.float32, device=y.device) if need_dz else None
    dbias = torch.empty(C, dtype=torch.float32, device=y.device) if need_dbias else None
    nb = L.segsde_colsum_workspace(M, C)
    ws = _ws(nb, y)
    _timed('hbm_act_backward', (8.0 + (4.0 if need_dz else 0.0)) * M * C, y, lambda: check(L.segsde_act_backward(_p(_f32(dy)), _rows(dy)[2], _p(y), ldy, M, C, ACT[act], _p(dz), C, _p(dbias), _p(ws), nb,
                                _stream(y)), "act_backward"))
    return dz, dbias


def colsum(x):
    M, C, ld = _rows(x)
    if C == 1 and ld == 1 and M >= 4096 and M % 64 == 0:
        # a single column (the bias gradient of a disparity head: 8 M values) gives the column kernel one float per row
        # to chew on -- 0.85 ms for 33 MB; as 64 columns of M / 64 rows it is an ordinary coalesced reduction (+ a 64-value sum)
        return colsum(x.reshape(M // 64, 64)).sum().reshape(1)
    L = _lib.lib()
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    nb = L.segsde_colsum_workspace(M, C)
    ws = _ws(nb, x)
    check(L.segsde_colsum(_p(_f32(x)), ld, M, C, _p(out), _p(ws), nb, _stream(x)), "colsum")
    return out



def feat_dist_forward(a, b):
    """||a - b||_2 of two NHWC tensors of one shape (channel slices allowed) -> 0-dim, on the device (torch.dist, train.py:480-483)"""
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("feature distance of tensors of different shapes: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    M, C, lda = _rows(a)
    ldb = _rows(b)[2]
    L = _lib.lib()
    out = torch.empty((), dtype=torch.float32, device=a.device)
    nb = L.segsde_feat_dist_workspace(M, C)
    ws = _ws(nb, a)
    _timed('hbm_feat_dist', 8.0 * M * C, a, lambda: check(L.segsde_feat_dist_forward(
        _p(_f32(a)), lda, _p(_f32(b)), ldb, M, C, _p(out), _p(ws), nb, _stream(a)), "feat_dist_forward"))
    return out


def feat_dist_backward(a, b, dist, grad):
    """d dist / d a scaled by the upstream gradient ``grad`` (a device scalar) -> dense NHWC like a"""
    M, C, lda = _rows(a)
    ldb = _rows(b)[2]
    L = _lib.lib()
    da = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    _timed('hbm_feat_dist_bwd', 12.0 * M * C, a, lambda: check(L.segsde_feat_dist_backward(
        _p(_f32(a)), lda, _p(_f32(b)), ldb, M, C, _p(_f32(dist)), _p(_f32(grad)), _p(da), C, _stream(a)), "feat_dist_backward"))
    return da

def maxpool_forward(x):
    B, H, W, C = x.shape
    x = x.contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    _timed('hbm_maxpool_fwd', 4.0 * x.numel() * 1.25 + 0.25 * x.numel(), x, lambda: check(_lib.lib().segsde_maxpool3x3s2_forward(_p(_f32(x)), B, H, W, C, _p(y), _p(idx), _stream(x)), "maxpool_fwd"))
    return y, idx


def maxpool_backward(dy, idx, in_shape, accumulate_into=None):
    """accumulate_into: a dense tensor of in_shape that already holds another consumer's gradient of the pooled tensor: the
    result is added to it in the kernel and that tensor is returned"""
    B, H, W, C = in_shape
    out_shape = (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    if idx.dtype != torch.uint8:
        raise TypeError("idx must be uint8 (the window taps maxpool_forward returns), got %s" % idx.dtype)
    if tuple(idx.shape) != out_shape or tuple(dy.shape) != out_shape:
        raise ValueError("dy %s and idx %s must have the pooled shape %s of in_shape %s" % (
            tuple(dy.shape), tuple(idx.shape), out_shape, tuple(in_shape)))
    dy, idx = _cf32(dy, "dy"), idx.contiguous()
    acc = accumulate_into if (accumulate_into is not None and tuple(accumulate_into.shape) == tuple(in_shape)
                              and accumulate_into.dtype == torch.float32 and accumulate_into.is_contiguous()) else None
    dx = acc if acc is not None else torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    check(_lib.lib().segsde_maxpool3x3s2_backward(_p(dy), _p(idx), B, H, W, C, _p(dx), 1 if acc is not None else 0,
                                                  _stream(dy)), "maxpool_bwd")
    return dx


def resize_bilinear(x, out_hw, align_corners=False):
    B, Hi, Wi, C = x.shape
    Ho, Wo = out_hw
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    check(_lib.lib().segsde_resize_bilinear_forward(_p(_f32(x)), nhwc_ld(x), B, Hi, Wi, C, _p(y), C, Ho, Wo,
                                                    int(align_corners), _stream(x)), "resize_fwd")
    return y


def resize_bilinear_backward(dy, in_hw, align_corners=False):
    B, Ho, Wo, C = dy.shape
    Hi, Wi = in_hw
    dx = torch.empty((B, Hi, Wi, C), dtype=torch.float32, device=dy.device)
    check(_lib.lib().segsde_resize_bilinear_backward(_p(_f32(dy)), nhwc_ld(dy), B, Hi, Wi, C, _p(dx), C, Ho, Wo,
                                                     int(align_corners), _stream(dy)), "resize_bwd")
    return dx


def global_avgpool(x):
    B, H, W, C = x.shape
    y = torch.empty((B, 1, 1, C), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    nws = int(L.segsde_global_avgpool_workspace(B, H * W, C))   # > 0: few images x few channels, the pixels are sliced
    ws = _ws(nws, x) if nws else None
    check(L.segsde_global_avgpool_forward(_p(_f32(x)), nhwc_ld(x), B, H * W, C, _p(y), _p(ws) if nws else None, nws,
                                          _stream(x)), "gap_fwd")
    return y


def global_avgpool_backward(dy, in_shape):
    B, H, W, C = in_shape
    dy = dy.contiguous()
    dx = torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    check(_lib.lib().segsde_global_avgpool_backward(_p(_f32(dy)), B, H * W, C, _p(dx), C, _stream(dy)), "gap_bwd")
    return dx


def gate_forward(f, a):
    f, a = f.contiguous(), a.contiguous()
    y = torch.empty_like(f)
    check(_lib.lib().segsde_gate_forward(_p(_f32(f)), _p(_f32(a)), f.numel(), _p(y), _stream(f)), "gate_fwd")
    return y


def gate_backward(dy, f, a):
    dy, f, a = _cf32(dy, "dy"), _cf32(f, "f"), _cf32(a, "a")
    if dy.numel() != f.numel() or a.numel() != f.numel():
        raise ValueError("gate_backward: dy %s, f %s and a %s differ in size" % (tuple(dy.shape), tuple(f.shape), tuple(a.shape)))
    df, da = torch.empty_like(f), torch.empty_like(a)
    check(_lib.lib().segsde_gate_backward(_p(dy), _p(f), _p(a), f.numel(), _p(df), _p(da), _stream(f)), "gate_bwd")
    return df, da


def _axpby_operands(x, y, out, what):
    """x, y: contiguous float32 copies held by the caller; out: written in place through its address"""
    x = _cf32(x, "x")
    if y is not None:
        y = _cf32(y, "y")
        if y.numel() != x.numel():
            raise ValueError("%s: y %s is not of the size of x %s" % (what, tuple(y.shape), tuple(x.shape)))
    if out is None:
        out = torch.empty_like(x)
    else:
        _f32(_dense(out, "out"), "out")
        if out.numel() != x.numel():
            raise ValueError("%s: out %s is not of the size of x %s" % (what, tuple(out.shape), tuple(x.shape)))
    return x, y, out


def axpby(alpha, x, beta=0.0, y=None, out=None):
    x, y, out = _axpby_operands(x, y, out, "axpby")
    check(_lib.lib().segsde_axpby(x.numel(), float(alpha), _p(x), float(beta), _p(y), _p(out), _stream(x)), "axpby")
    return out


def axpby_dev(alpha_t, x, beta_t=None, y=None, out=None):
    """out = alpha_t[0]*x (+ beta_t[0]*y) with 1-element DEVICE tensors as scalars (no host sync)"""
    x, y, out = _axpby_operands(x, y, out, "axpby_dev")
    alpha_t = _f32(alpha_t, "alpha_t")
    if beta_t is not None:
        beta_t = _f32(beta_t, "beta_t")
    check(_lib.lib().segsde_axpby_dev(x.numel(), _p(alpha_t), _p(x), _p(beta_t), _p(y), _p(out), _stream(x)), "axpby_dev")
    return out


def copy_channels(src, dst):
    M, C, lds = _rows(src)
    M2, C2, ldd = _rows(dst)
    assert M == M2 and C == C2
    check(_lib.lib().segsde_copy_channels(_p(_f32(src)), lds, _p(dst), ldd, M, C, _stream(src)), "copy_channels")
    return dst


def scale_channels(x, scale):
    """x: NHWC [B,H,W,C]; scale [B,C] -> x * scale[b, c] (nn.Dropout2d mask application and its adjoint)"""
    B, Hh, W, C = x.shape
    y = torch.empty((B, Hh, W, C), dtype=torch.float32, device=x.device)
    scale = _cf32(scale, "scale")
    check(_lib.lib().segsde_scale_channels(_p(_f32(x)), nhwc_ld(x), B, Hh * W, C, _p(scale), _p(y), C,
                                           _stream(x)), "scale_channels")
    return y


def dropout(x, p, seed):
    """nn.Dropout(p) on an NHWC tensor with the counter-based mask of ``seed`` (its own adjoint with the same seed)"""
    M, C, ld = _rows(x)
    y = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    check(_lib.lib().segsde_dropout(_p(_f32(x)), ld, M, C, float(p), int(seed), _p(y), C, _stream(x)), "dropout")
    return y


def nchw_to_nhwc(x, mean=0.0, std=1.0, pad_to=1):
    """pad_to > 1 rounds the channel count of the result up to a multiple of pad_to; the extra channels are zero
    (the 3 / 6-channel network input becomes 4 / 8 so that the stem convolution takes the float4 gather)."""
    x = _f32(x).contiguous()
    B, C, H, W = x.shape
    Cp = -(-C // pad_to) * pad_to
    y = torch.empty((B, H, W, Cp), dtype=torch.float32, device=x.device)     # the kernel writes the zero channels too
    check(_lib.lib().segsde_nchw_to_nhwc(_p(x), B, C, H, W, float(mean), float(std), _p(y), Cp, _stream(x)), "nchw_to_nhwc")
    return y


# ----------------------------------------------------------------------------------------------
# network stems (7x7, stride 2, padding 3 on the normalised image): see csrc/conv_igemm.hip "Network stems"
# ----------------------------------------------------------------------------------------------
STEM = os.environ.get("SEGSDE_STEM", "1") != "0"
STEM_TAKEN = {"fwd": 0, "wgrad": 0}


def stem_ok(image, conv):
    """conv: the module holding the stem's state (nn.Conv2d attributes).  The dedicated path needs the reference's stem geometry."""
    return (STEM and image.dim() == 4 and conv.kernel_size == (7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3)
            and conv.dilation == (1, 1) and conv.bias is None and conv.groups == 1 and image.shape[1] == conv.in_channels
            and conv.in_channels <= 8 and conv.out_channels % 4 == 0 and image.shape[2] >= 2 and image.shape[3] >= 2
            and image.shape[0] * (image.shape[2] + 6) * (image.shape[3] + 8) * 8 < 2 ** 31)


def stem_input(image, mean, std):
    """(image - mean) / std as 4 / 8-channel pixels inside a zero border of 3 rows above / below, 3 columns left, 5 right."""
    x = _f32(image).contiguous()
    B, C, H, W = x.shape
    cp = 4 if C <= 4 else 8
    y = torch.empty((B, H + 6, W + 8, cp), dtype=torch.float32, device=x.device)   # the kernel writes the border too
    check(_lib.lib().segsde_nchw_to_nhwc_bordered(_p(x), B, C, H, W, float(mean), float(std), _p(y), cp, 3, 3, H + 6, W + 8,
                                                  _stream(x)), "nchw_to_nhwc_bordered")
    return y


def stem_pack(weight):
    Cout, C = weight.shape[0], weight.shape[1]
    cp = 4 if C <= 4 else 8
    w = _f32(weight.detach()).contiguous()
    out = torch.empty((Cout, 7, 8 * cp), dtype=torch.float32, device=w.device)
    check(_lib.lib().segsde_stem_pack(_p(w), Cout, C, cp, _p(out), _stream(w)), "stem_pack")
    return out


def stem_forward(xpad, wstem, C, want_stats=False, bias=None, act="none"):
    """xpad: stem_input(); wstem: stem_pack(); C: real input planes (FLOP accounting) -> y [B, Ho, Wo, Cout] (, partials).
    bias / act: y = act(conv + bias) through segsde_stem7x7_forward_bias_act (the stem behind a folded frozen BatchNorm)"""
    B, Hp, Wp, cp = xpad.shape
    Cout = wstem.shape[0]
    H, W = Hp - 6, Wp - 8
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=xpad.device)
    part = None
    if want_stats:
        rows = int(_lib.lib().segsde_stem7x7_stats_rows(B, Hp, Wp, cp, Cout))
        if rows > 0:
            part = torch.empty((rows, 2, Cout), dtype=torch.float64, device=xpad.device)
    flops = 2.0 * B * Ho * Wo * Cout * C * 49
    if bias is not None or act != "none":
        assert not want_stats
        _timed("conv_fwd", flops, xpad, lambda: check(_lib.lib().segsde_stem7x7_forward_bias_act(
            _p(xpad), B, Hp, Wp, cp, _p(wstem), Cout, _p(bias), ACT[act], _p(y), _stream(xpad)), "stem7x7_forward_bias_act"),
            "stem c%d k7 s2 %dx%d" % (C, H, W), executed=2.0 * B * Ho * Wo * Cout * 56 * cp)
        STEM_TAKEN["fwd"] += 1
        return y
    _timed("conv_fwd", flops, xpad, lambda: check(_lib.lib().segsde_stem7x7_forward(
        _p(xpad), B, Hp, Wp, cp, _p(wstem), Cout, _p(y), _p(part), _stream(xpad)), "stem7x7_forward"),
        "stem c%d k7 s2 %dx%d" % (C, H, W), executed=2.0 * B * Ho * Wo * Cout * 56 * cp)
    STEM_TAKEN["fwd"] += 1
    return (y, part) if want_stats else y


def stem_wgrad(xpad, dy, C):
    B, Hp, Wp, cp = xpad.shape
    _, Ho, Wo, Cout = dy.shape
    dy = _f32(dy)
    dw = torch.empty((Cout, C, 7, 7), dtype=torch.float32, device=dy.device)
    nbytes = int(_lib.lib().segsde_stem7x7_wgrad_workspace(B, Hp, Wp, cp, Cout))
    ws = _ws(nbytes, dy)
    flops = 2.0 * B * Ho * Wo * Cout * C * 49
    _timed("conv_wgrad", flops, dy, lambda: check(_lib.lib().segsde_stem7x7_wgrad(
        _p(xpad), B, Hp, Wp, cp, _p(dy), nhwc_ld(dy), Cout, C, _p(dw), _p(ws), nbytes, _stream(dy)), "stem7x7_wgrad"),
        "stem c%d k7 s2 %dx%d" % (C, Hp - 6, Wp - 8), executed=2.0 * B * Ho * Wo * Cout * 56 * cp)
    STEM_TAKEN["wgrad"] += 1
    return dw


def nhwc_to_nchw(x):
    B, H, W, C = x.shape
    y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    check(_lib.lib().segsde_nhwc_to_nchw(_p(_f32(x)), nhwc_ld(x), B, C, H, W, _p(y), _stream(x)), "nhwc_to_nchw")
    return y


# ----------------------------------------------------------------------------------------------
# pose
# ----------------------------------------------------------------------------------------------
def pose_matrix(axisangle, translation, invert):
    """axisangle / translation: [B, F, 1, 3] network outputs; frame 0 is used (joint_segmentation_depth.py:48-49)."""
    assert axisangle.is_contiguous() and translation.is_contiguous()
    B = axisangle.shape[0]
    stride = axisangle.stride(0) if B > 1 else axisangle[0].numel()
    M = torch.empty((B, 4, 4), dtype=torch.float32, device=axisangle.device)
    check(_lib.lib().segsde_pose_matrix_forward(_p(_f32(axisangle)), _p(_f32(translation)), B, int(stride), int(invert),
                                                _p(M), _stream(axisangle)), "pose_fwd")
    return M


def pose_matrix_backward(axisangle, translation, dM, invert):
    _dense(_f32(axisangle, "axisangle"), "axisangle"), _dense(_f32(translation, "translation"), "translation")
    dM = _cf32(dM, "dM")
    B = axisangle.shape[0]
    stride = axisangle.stride(0) if B > 1 else axisangle[0].numel()
    daa, dtr = torch.zeros_like(axisangle), torch.zeros_like(translation)
    check(_lib.lib().segsde_pose_matrix_backward(_p(axisangle), _p(translation), _p(dM), B, int(stride),
                                                 int(invert), _p(daa), _p(dtr), _stream(axisangle)), "pose_bwd")
    return daa, dtr


# ----------------------------------------------------------------------------------------------
# monodepth loss
# ----------------------------------------------------------------------------------------------
def warp_forward(disp, inv_K, K, T, src, min_depth, max_depth, want_grid=False, want_depth=False):
    B, _, hs, ws = disp.shape
    _, _, H, W = src.shape
    color = torch.empty((B, 3, H, W), dtype=torch.float32, device=src.device)
    grid = torch.empty((B, H, W, 2), dtype=torch.float32, device=src.device) if want_grid else None
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=src.device) if want_depth else None
    disp, inv_K, K, T, src = _cf32(disp, "disp"), _cf32(inv_K, "inv_K"), _cf32(K, "K"), _cf32(T, "T"), _cf32(src, "src")
    _timed('hbm_warp_fwd', 4.0 * B * (hs * ws + (3 + 3 + (2 if want_grid else 0) + (1 if want_depth else 0)) * H * W), src, lambda: check(_lib.lib().segsde_warp_forward(_p(disp), hs, ws, _p(inv_K),
                                         _p(K), _p(T), _p(src),
                                         B, H, W, float(min_depth), float(max_depth), _p(color), _p(grid), _p(depth),
                                         _stream(src)), "warp_fwd"))
    return color, grid, depth


def warp_backward(gcolor, disp, inv_K, K, T, src, min_depth, max_depth, g_disp_up, gT):
    """accumulates into g_disp_up [B,H,W] and gT [B,4,4]"""
    B, _, hs, ws = disp.shape
    _, _, H, W = src.shape
    L = _lib.lib()
    nb = L.segsde_warp_backward_workspace(B, H, W)
    ws_ = _ws(nb, src)
    gcolor, disp, inv_K, K, T, src = _cf32(gcolor, "gcolor"), _c(disp), _c(inv_K), _c(K), _c(T), _c(src)
    _dense(g_disp_up, "g_disp_up"), _dense(gT, "gT")
    check(L.segsde_warp_backward(_p(gcolor), _p(disp), hs, ws, _p(inv_K),
                                 _p(K), _p(T), _p(src), B, H, W, float(min_depth),
                                 float(max_depth), _p(g_disp_up), _p(gT), _p(ws_), nb, _stream(src)), "warp_bwd")


def reprojection_error(pred, target, no_ssim, out_plane):
    """out_plane: a [B,H,W] view (channel of a [B,n,H,W] tensor)"""
    B, _, H, W = pred.shape
    assert out_plane.stride(2) == 1 and out_plane.stride(1) == W
    pred, target = _cf32(pred, "pred"), _cf32(target, "target")
    check(_lib.lib().segsde_reprojection_error_forward(_p(pred), _p(target), B, H, W,
                                                       int(no_ssim), _p(out_plane), int(out_plane.stride(0)) if B > 1 else H * W,
                                                       _stream(pred)), "reproj_err_fwd")


def reprojection_error_backward(pred, target, gerr_plane, no_ssim):
    B, _, H, W = pred.shape
    L = _lib.lib()
    nb = 0 if no_ssim else L.segsde_reprojection_error_backward_workspace(B, H, W)
    ws_ = _ws(nb, pred) if nb else None
    pred, target = _c(pred), _c(target)
    if gerr_plane.stride(2) != 1 or gerr_plane.stride(1) != W:
        raise ValueError("gerr_plane must be a [B,H,W] view with dense rows, got strides %s" % (gerr_plane.stride(),))
    gpred = torch.empty_like(pred)
    check(L.segsde_reprojection_error_backward(_p(pred), _p(target), _p(gerr_plane),
                                               int(gerr_plane.stride(0)) if B > 1 else H * W, B, H, W, int(no_ssim),
                                               _p(gpred), _p(ws_), nb, _stream(pred)), "reproj_err_bwd")
    return gpred


def photometric_identity(src0, src1, target, no_ssim):
    """err(src_f, target), f = 0, 1 -> [B,2,H,W] (the auto-mask's identity terms, the same for every scale)"""
    B, _, Hh, W = target.shape
    ident = torch.empty((B, 2, Hh, W), dtype=torch.float32, device=target.device)
    src0, src1, target = _cf32(src0, "src0"), _cf32(src1, "src1"), _cf32(target, "target")
    _timed('hbm_photometric_identity', 4.0 * B * Hh * W * (9 + 2), target, lambda: check(_lib.lib().segsde_photometric_identity(_p(src0), _p(src1),
                                                 _p(target), B, Hh, W, int(no_ssim), _p(ident),
                                                 _stream(target)), "photometric_identity"))
    return ident


def photometric_forward(pred0, pred1, target, ident, noise, no_ssim, avg, want_selection=True):
    """fused SSIM+L1 errors of both warped frames + auto-mask minimum -> (sum [1], sel uint8 [B,H,W], identity_selection)"""
    B, _, Hh, W = target.shape
    L = _lib.lib()
    sel = torch.empty((B, Hh, W), dtype=torch.uint8, device=target.device)
    isel = torch.empty((B, Hh, W), dtype=torch.float32, device=target.device) if (want_selection and ident is not None) else None
    out = torch.empty(1, dtype=torch.float32, device=target.device)
    nb = L.segsde_photometric_workspace(B, Hh, W)
    ws_ = _ws(nb, target)
    pred0, pred1, target = _cf32(pred0, "pred0"), _cf32(pred1, "pred1"), _cf32(target, "target")
    ident, noise = _c(ident), _c(noise)
    _timed('hbm_photometric_fwd', B * Hh * W * (4.0 * (9 + (2 if ident is not None else 0) + (2 if noise is not None else 0) + (1 if isel is not None else 0)) + 1.0), target, lambda: check(L.segsde_photometric_forward(_p(pred0), _p(pred1), _p(target),
                                       _p(ident), _p(noise), B, Hh, W, int(no_ssim), int(avg), _p(sel), _p(isel), _p(out),
                                       _p(ws_), nb, _stream(target)), "photometric_forward"))
    return out, sel, isel


def photometric_backward(pred0, pred1, target, sel, has_ident, disp, inv_K, K, T0, T1, src0, src1, min_depth, max_depth,
                         no_ssim, avg, scale, weight, gT0, gT1):
    """-> g_disp_up [B,H,W] (d loss / d upsampled disparity, both frames); gT0 / gT1 [B,4,4] are accumulated into with the
    device scalar ``weight`` (upstream gradient of this scale's loss)"""
    B, _, Hh, W = target.shape
    _, _, hs, ws = disp.shape
    L = _lib.lib()
    gup = torch.empty((B, Hh, W), dtype=torch.float32, device=target.device)
    nb = L.segsde_photometric_workspace(B, Hh, W)
    ws_ = _ws(nb, target)
    pred0, pred1, target, disp, src0, src1 = _c(pred0), _c(pred1), _c(target), _c(disp), _c(src0), _c(src1)
    inv_K, K, T0, T1 = _c(inv_K), _c(K), _c(T0), _c(T1)
    sel = _c(sel)
    _dense(gT0, "gT0"), _dense(gT1, "gT1")
    _timed('hbm_photometric_bwd', B * (Hh * W * (4.0 * (9 + 6 + 1) + 1.0) + 4.0 * hs * ws), target, lambda: check(L.segsde_photometric_backward(_p(pred0), _p(pred1), _p(target), _p(sel),
                                        2 if has_ident else 0, _p(disp), hs, ws, _p(inv_K),
                                        _p(K), _p(T0), _p(T1), _p(src0),
                                        _p(src1), B, Hh, W, float(min_depth), float(max_depth), int(no_ssim),
                                        int(avg), float(scale), _p(weight), _p(gup), _p(gT0), _p(gT1), _p(ws_), nb,
                                        _stream(target)), "photometric_backward"))
    return gup


def automask_min(ident, noise, reproj, avg, want_selection=True):
    B, nr, H, W = reproj.shape
    L = _lib.lib()
    sel = torch.empty((B, H, W), dtype=torch.uint8, device=reproj.device)
    isel = torch.empty((B, H, W), dtype=torch.float32, device=reproj.device) if (want_selection and ident is not None) else None
    out = torch.empty(1, dtype=torch.float32, device=reproj.device)
    nb = L.segsde_automask_workspace(B, H, W)
    ws_ = _ws(nb, reproj)
    ident, noise, reproj = _c(ident), _c(noise), _cf32(reproj, "reproj")
    check(L.segsde_automask_min_forward(_p(ident), _p(noise), _p(reproj), nr, int(avg), B, H, W, _p(sel), _p(isel),
                                        _p(out), _p(ws_), nb, _stream(reproj)), "automask_fwd")
    return out, sel, isel


def automask_min_backward(sel, has_ident, n_reproj, avg, scale):
    B, H, W = sel.shape
    g = torch.empty((B, n_reproj, H, W), dtype=torch.float32, device=sel.device)
    sel = _c(sel)
    check(_lib.lib().segsde_automask_min_backward(_p(sel), 2 if has_ident else 0, n_reproj, int(avg), B, H, W, float(scale),
                                                  _p(g), _stream(sel)), "automask_bwd")
    return g


def smoothness_forward(disp, img):
    B, _, h, w = disp.shape
    L = _lib.lib()
    mean = torch.empty(B, dtype=torch.float32, device=disp.device)
    out = torch.empty(1, dtype=torch.float32, device=disp.device)
    nb = L.segsde_smoothness_workspace(B, h, w)
    ws_ = _ws(nb, disp)
    disp, img = _cf32(disp, "disp"), _cf32(img, "img")
    _timed('hbm_smooth_fwd', 16.0 * B * h * w, disp, lambda: check(L.segsde_smoothness_forward(_p(disp), _p(img), B, h, w, _p(mean), _p(out),
                                      _p(ws_), nb, _stream(disp)), "smooth_fwd"))
    return out, mean


def smoothness_backward(disp, img, mean, scale, gdisp):
    """accumulates into gdisp [B,1,h,w]"""
    B, _, h, w = disp.shape
    L = _lib.lib()
    nb = L.segsde_smoothness_workspace(B, h, w)
    ws_ = _ws(nb, disp)
    disp, img, mean = _c(disp), _c(img), _c(mean)
    _dense(gdisp, "gdisp")
    _timed('hbm_smooth_bwd', 24.0 * B * h * w, disp, lambda: check(L.segsde_smoothness_backward(_p(disp), _p(img), _p(mean), B, h, w, float(scale),
                                       _p(gdisp), _p(ws_), nb, _stream(disp)), "smooth_bwd"))


def smooth_loss_forward(disp, img):
    """get_smooth_loss(disp, img) without the mean normalisation (models/monodepth_layers.py:208-221) -> [1]"""
    B, _, h, w = disp.shape
    L = _lib.lib()
    out = torch.empty(1, dtype=torch.float32, device=disp.device)
    nb = L.segsde_smooth_loss_workspace(B, h, w)
    ws_ = _ws(nb, disp)
    disp, img = _cf32(disp, "disp"), _cf32(img, "img")
    check(L.segsde_smooth_loss_forward(_p(disp), _p(img), B, h, w, _p(out), _p(ws_), nb,
                                       _stream(disp)), "smooth_loss_fwd")
    return out


def smooth_loss_backward(disp, img, scale):
    B, _, h, w = disp.shape
    L = _lib.lib()
    g = torch.zeros((B, 1, h, w), dtype=torch.float32, device=disp.device)
    nb = L.segsde_smooth_loss_workspace(B, h, w)
    ws_ = _ws(nb, disp)
    disp, img = _c(disp), _c(img)
    check(L.segsde_smooth_loss_backward(_p(disp), _p(img), B, h, w, float(scale), _p(g), _p(ws_), nb,
                                        _stream(disp)), "smooth_loss_bwd")
    return g


def ssim_map(x, y):
    """SSIM.forward (models/monodepth_layers.py:240-254): per-channel clamp((1 - SSIM) / 2, 0, 1) of two [B,C,H,W] images"""
    B, C, Hh, W = x.shape
    assert tuple(y.shape) == tuple(x.shape)
    out = torch.empty((B, C, Hh, W), dtype=torch.float32, device=x.device)
    x, y = _cf32(x, "x"), _cf32(y, "y")
    check(_lib.lib().segsde_ssim_map_forward(_p(x), _p(y), B, C, Hh, W, _p(out),
                                             _stream(x)), "ssim_map_fwd")
    return out


def ssim_map_backward(x, y, gout, need_x=True, need_y=True):
    B, C, Hh, W = x.shape
    gx = torch.empty((B, C, Hh, W), dtype=torch.float32, device=x.device) if need_x else None
    gy = torch.empty((B, C, Hh, W), dtype=torch.float32, device=x.device) if need_y else None
    x, y, gout = _c(x), _c(y), _cf32(gout, "gout")
    check(_lib.lib().segsde_ssim_map_backward(_p(x), _p(y), _p(gout), B, C, Hh, W,
                                              _p(gx), _p(gy), _stream(x)), "ssim_map_bwd")
    return gx, gy


def backproject_depth(depth, inv_K):
    """BackprojectDepth.forward (models/monodepth_layers.py:169-174): depth [B,1,H,W], inv_K [B,4,4] -> cam_points [B,4,H*W]"""
    B, _, Hh, W = depth.shape
    out = torch.empty((B, 4, Hh * W), dtype=torch.float32, device=depth.device)
    depth, inv_K = _cf32(depth, "depth"), _cf32(inv_K, "inv_K")
    check(_lib.lib().segsde_backproject_depth(_p(depth), _p(inv_K), B, Hh, W, _p(out),
                                              _stream(depth)), "backproject_depth")
    return out


def project3d(points, K, T, Hh, W, eps=1e-7):
    """Project3D.forward (models/monodepth_layers.py:188-199): points [B,4,H*W] -> sampling grid [B,H,W,2]"""
    B = points.shape[0]
    assert tuple(points.shape) == (B, 4, Hh * W)
    out = torch.empty((B, Hh, W, 2), dtype=torch.float32, device=points.device)
    points, K, T = _cf32(points, "points"), _cf32(K, "K"), _cf32(T, "T")
    check(_lib.lib().segsde_project3d(_p(points), _p(K), _p(T), B, Hh, W,
                                      float(eps), _p(out), _stream(points)), "project3d")
    return out


def backproject_depth_backward(g_cam, inv_K, Hh, W):
    """adjoint of backproject_depth w.r.t. the depth: g_cam [B,4,H*W] -> [B,1,H,W]"""
    B = g_cam.shape[0]
    out = torch.empty((B, 1, Hh, W), dtype=torch.float32, device=g_cam.device)
    g_cam, inv_K = _cf32(g_cam, "g_cam"), _cf32(inv_K, "inv_K")
    check(_lib.lib().segsde_backproject_depth_backward(_p(g_cam), _p(inv_K), B, Hh, W, _p(out),
                                                       _stream(g_cam)), "backproject_depth_backward")
    return out


def project3d_backward(points, K, T, g_pix, Hh, W, eps=1e-7, need_points=True, need_T=True):
    """adjoint of project3d: g_pix [B,H,W,2] -> (d points [B,4,H*W] or None, d T [B,4,4] or None)"""
    B = points.shape[0]
    L = _lib.lib()
    gp = torch.empty_like(points, memory_format=torch.contiguous_format) if need_points else None
    gT = torch.empty((B, 4, 4), dtype=torch.float32, device=points.device) if need_T else None
    nbytes = L.segsde_project3d_backward_workspace(B, Hh, W) if need_T else 0
    ws = _ws(nbytes, points) if need_T else None
    points, K, T, g_pix = _cf32(points, "points"), _cf32(K, "K"), _cf32(T, "T"), _cf32(g_pix, "g_pix")
    check(L.segsde_project3d_backward(_p(points), _p(K), _p(T),
                                      _p(g_pix), B, Hh, W, float(eps), _p(gp), _p(gT), _p(ws), nbytes,
                                      _stream(points)), "project3d_backward")
    return gp, gT


# ----------------------------------------------------------------------------------------------
# segmentation loss, mix, masks
# ----------------------------------------------------------------------------------------------
def cross_entropy_forward(logits_nhwc, target, ignore_index, class_weight=None, pixel_weights=None):
    M, C, ld = _rows(logits_nhwc)
    L = _lib.lib()
    out = torch.empty(2, dtype=torch.float32, device=logits_nhwc.device)
    nb = L.segsde_cross_entropy_workspace(M)
    ws_ = _ws(nb, logits_nhwc)
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == M
    _timed('hbm_ce_fwd', M * (4.0 * C + 8.0), logits_nhwc, lambda: check(L.segsde_cross_entropy_forward(_p(_f32(logits_nhwc)), ld, M, C, _p(target), int(ignore_index), _p(class_weight),
                                         _p(pixel_weights), _p(out), _p(ws_), nb, _stream(logits_nhwc)), "ce_fwd"))
    return out


def cross_entropy_backward(logits_nhwc, target, ignore_index, scale, class_weight=None, pixel_weights=None):
    M, C, ld = _rows(logits_nhwc)
    dl = torch.empty(logits_nhwc.shape, dtype=torch.float32, device=logits_nhwc.device)
    _timed('hbm_ce_bwd', M * (8.0 * C + 8.0), logits_nhwc, lambda: check(_lib.lib().segsde_cross_entropy_backward(_p(logits_nhwc), ld, M, C, _p(target), int(ignore_index),
                                                   _p(class_weight), _p(pixel_weights), _p(_f32(scale)), _p(dl), C,
                                                   _stream(logits_nhwc)), "ce_bwd"))
    return dl


def mix(mask, x):
    """x: [B,C,H,W] fp32, NCHW-contiguous or channels-last; mask [Bm,H,W] int64 / float32"""
    B, C, H, W = x.shape
    if not (x.stride(3) == 1 or x.stride(1) == 1):
        x = x.contiguous()
    out = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
    if mask.dtype == torch.int64:
        is64 = 1
    elif mask.dtype == torch.float32:
        is64 = 0
    else:
        raise TypeError("mask must be int64 or float32")
    mask = mask.contiguous()
    sb = x.stride(0) if B > 1 else C * H * W
    _timed('hbm_mix', B * H * W * (12.0 * C + (8.0 if is64 else 4.0)), x, lambda: check(_lib.lib().segsde_mix(_p(mask), is64, mask.shape[0], _p(_f32(x)), B, C, H, W, int(sb), int(x.stride(1)),
                                int(x.stride(2)), int(x.stride(3)), _p(out), _stream(x)), "mix"))
    return out


def mix_labels(mask, target):
    B, H, W = target.shape
    mask, target = _c(mask), _c(target)
    out = torch.empty_like(target)
    check(_lib.lib().segsde_mix_labels(_p(mask), _p(target), B, H, W, _p(out), _stream(target)),
          "mix_labels")
    return out


def depthcomp_mask(depths, margin, fg_threshold):
    """fg_threshold: a float for every image, or a DEVICE tensor [B] (one threshold per image, train.py:592-599)"""
    B = depths.shape[0]
    HW = depths[0].numel()
    mask = torch.empty((B,) + tuple(depths.shape[-2:]), dtype=torch.int64, device=depths.device)
    per = None
    if torch.is_tensor(fg_threshold):
        per = _f32(fg_threshold.reshape(-1)).to(depths.device).contiguous()
        if per.numel() != B:
            raise ValueError("one foreground threshold per image: got %d for a batch of %d" % (per.numel(), B))
    depths = _cf32(depths, "depths")
    check(_lib.lib().segsde_depthcomp_mask(_p(depths), B, HW, float(margin),
                                           0.0 if per is not None else float(fg_threshold), _p(per), _p(mask),
                                           _stream(depths)), "depthcomp_mask")
    return mask


def depth_threshold_mask(depth, t1, t2=0.0, two=False):
    depth = depth.contiguous()
    mask = torch.empty_like(depth)
    check(_lib.lib().segsde_depth_threshold_mask(_p(_f32(depth)), depth.numel(), float(t1), float(t2), int(two), _p(mask),
                                                 _stream(depth)), "depth_threshold_mask")
    return mask


def class_mask(pred, classes):
    pred, classes = pred.contiguous(), classes.contiguous().to(torch.int64)
    mask = torch.empty_like(pred)
    check(_lib.lib().segsde_class_mask(_p(pred), pred.numel(), _p(classes), classes.numel(), _p(mask), _stream(pred)),
          "class_mask")
    return mask


# the whole batch per launch (csrc/mixmask.hip): the "depth", "depthhist" and "class" masks of Trainer.generate_mix_mask
MIX_CLASS_SLOTS = 256         # class ids -1 .. 254 in slots 0 .. 255
MIX_HIST_BINS = 100           # np.histogram(..., bins=100), train.py:619


def upload(host, device):
    """one host -> device copy the host does not wait for (through pinned memory on a ROCm device)"""
    if device.type == "cuda":
        return host.pin_memory().to(device, non_blocking=True)
    return host.to(device)


def _mix_batch(t, dtype, name):
    """-> (dense tensor, B, pixels per image) of a [B, ...] batch"""
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError("%s must be a %s tensor, got %s" % (name, dtype, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() < 2 or t.numel() < 1:
        raise ValueError("%s must be a non-empty batch [B, ...], got %s" % (name, tuple(t.shape)))
    B, HW = int(t.shape[0]), t[0].numel()
    if HW >= 2 ** 31:
        raise ValueError("%s: %d pixels per image, the kernels index fewer than 2^31" % (name, HW))
    return t.contiguous(), B, HW


def _mix_per_image(t, dtype, like, shape, name):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError("%s must be a %s tensor, got %s" % (name, dtype, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.device != like.device:
        raise ValueError("%s is on %s, the batch on %s" % (name, t.device, like.device))
    if tuple(t.shape) != shape:
        raise ValueError("%s must have shape %s (one row per image), got %s" % (name, shape, tuple(t.shape)))
    return t


def depth_hist_thresholds(depths, u, apply_log=True, want_counts=False):
    """The thresholds of the "depthhist" mix mask (train.py:616-631) for a batch: depths float32 [B, ...], u float32 [B] on the same
    device (the reference's ``torch.rand(1)`` per image) -> (table float32 [B,4] = {min_depth, max_depth, threshold, found} per
    image, counts int32 [B,100] or None).  The histogram is np.histogram(log(1 + depth), bins=100, density=True) restated in fp32
    (segsde_depth_hist_thresholds in include/segsde_hip.h); ``apply_log=False`` takes the histogram of the values as they are.
    An image without a bin for max_depth (found = 0) takes max_depth of the image before it, image 0 its top edge.  Three
    launches, nothing returns to the host."""
    d, B, HW = _mix_batch(depths, torch.float32, "depths")
    u = _mix_per_image(u, torch.float32, d, (B,), "u").contiguous()
    table = torch.empty((B, 4), dtype=torch.float32, device=d.device)
    counts = torch.empty((B, MIX_HIST_BINS), dtype=torch.int32, device=d.device) if want_counts else None
    L = _lib.lib()
    nb = L.segsde_depth_hist_workspace(B, HW)
    ws_ = _ws(nb, d)
    check(L.segsde_depth_hist_thresholds(_p(d), B, HW, int(bool(apply_log)), _p(u), _p(table), _p(counts), _p(ws_), nb, _stream(d)),
          "depth_hist_thresholds")
    return table, counts


def depth_threshold_mask_batch(depths, thr):
    """mask[b] = (depths[b] >= thr[b]).float() for a batch in one launch: depths float32 [B, ...], thr float32 [B] on the same
    device, possibly a strided view (column 2 of depth_hist_thresholds' table is read in place) -> float32, depths' shape."""
    d, B, HW = _mix_batch(depths, torch.float32, "depths")
    thr = _mix_per_image(thr, torch.float32, d, (B,), "thr")
    stride = int(thr.stride(0)) if B > 1 else 0
    if stride < 0:
        thr, stride = thr.contiguous(), 1
    mask = torch.empty_like(d)
    check(_lib.lib().segsde_depth_threshold_mask_batch(_p(d), B, HW, _p(thr), stride, _p(mask), _stream(d)),
          "depth_threshold_mask_batch")
    return mask


def class_presence(pred):
    """pred int64 [B, ...] -> int32 [B,256]: pixels of image b with class id k in [b, k + 1], ids -1 .. 254 (others: nowhere)"""
    p, B, HW = _mix_batch(pred, torch.int64, "pred")
    counts = torch.empty((B, MIX_CLASS_SLOTS), dtype=torch.int32, device=p.device)
    check(_lib.lib().segsde_class_presence(_p(p), B, HW, _p(counts), _stream(p)), "class_presence")
    return counts


def class_mask_batch(pred, selected):
    """mask[b] = selected[b, pred[b] + 1] (0 for ids outside -1 .. 254): pred int64 [B, ...], selected uint8 [B,256] on the same
    device -> int64, pred's shape.  transformmasks.generate_class_mask of every image against its own class list, one launch."""
    p, B, HW = _mix_batch(pred, torch.int64, "pred")
    selected = _mix_per_image(selected, torch.uint8, p, (B, MIX_CLASS_SLOTS), "selected").contiguous()
    mask = torch.empty_like(p)
    check(_lib.lib().segsde_class_mask_batch(_p(p), B, HW, _p(selected), _p(mask), _stream(p)), "class_mask_batch")
    return mask


# ----------------------------------------------------------------------------------------------
# trainer-side callers
# ----------------------------------------------------------------------------------------------
MT_CHUNK = 65536


def multi_tensor_table(dsts, srcs):
    """device table of segsde_mt_chunk {dst, src, n} covering every (dst, src) tensor pair in chunks of <= 65536 floats"""
    rows = []
    for d, s in zip(dsts, srcs):
        assert d.dtype == torch.float32 and s.dtype == torch.float32 and d.is_contiguous() and s.is_contiguous()
        assert d.numel() == s.numel() and d.device == s.device
        n, dp, sp = d.numel(), d.data_ptr(), s.data_ptr()
        for o in range(0, n, MT_CHUNK):
            rows.append((dp + 4 * o, sp + 4 * o, min(MT_CHUNK, n - o)))
    if not rows:
        return None
    return torch.tensor(rows, dtype=torch.int64).to(dsts[0].device)


def multi_tensor_lerp(table, alpha, one_minus_alpha, like):
    """dst = alpha*dst + one_minus_alpha*src for every chunk of the table (one launch)"""
    check(_lib.lib().segsde_multi_tensor_lerp(_p(table), int(table.shape[0]), float(alpha), float(one_minus_alpha),
                                              _stream(like)), "multi_tensor_lerp")


def pseudo_label(prob, threshold, ignore_index, want_max=False, want_weight=True):
    """prob: [B,C,H,W] (NCHW, dense) -> (label int64 [B,H,W], count uint64-as-int64 [1], max_prob or None,
    pixel_weight [B,H,W] or None)"""
    prob = _f32(prob).contiguous()
    B, C, H, W = prob.shape
    label = torch.empty((B, H, W), dtype=torch.int64, device=prob.device)
    count = torch.empty(1, dtype=torch.int64, device=prob.device)
    maxp = torch.empty((B, H, W), dtype=torch.float32, device=prob.device) if want_max else None
    pw = torch.empty((B, H, W), dtype=torch.float32, device=prob.device) if want_weight else None
    check(_lib.lib().segsde_pseudo_label(_p(prob), B, C, H * W, float(threshold), int(ignore_index), _p(label), _p(maxp),
                                         _p(count), _p(pw), _stream(prob)), "pseudo_label")
    if pw is not None:
        pw._segsde_finite = True      # count / total: cannot be NaN (cross_entropy2d skips its host-side NaN check)
    return label, count, maxp, pw


def color_jitter(x, params, order):
    """x [B,3,H,W] dense NCHW; params [B,4] device tensor of (brightness, contrast, saturation, hue) factors; order: a
    permutation of (0, 1, 2, 3) -- see segsde_color_jitter"""
    x = _f32(x).contiguous()
    B, C, Hh, W = x.shape
    assert C == 3 and tuple(params.shape) == (B, 4)
    y = torch.empty_like(x)
    arr = (ctypes.c_int * 4)(*[int(o) for o in order])
    params = _cf32(params, "params")
    check(_lib.lib().segsde_color_jitter(_p(x), B, Hh * W, _p(params), arr, _p(y), _stream(x)), "color_jitter")
    return y


def gaussian_blur(x, wy, wx):
    """x [B,C,H,W] dense NCHW; wy / wx: 1-D device tensors of (odd many) normalised taps for the column / row pass"""
    x = _f32(x).contiguous()
    B, C, Hh, W = x.shape
    tmp, y = torch.empty_like(x), torch.empty_like(x)
    wy, wx = _cf32(wy, "wy"), _cf32(wx, "wx")
    _timed('hbm_blur', 16.0 * x.numel(), x, lambda: check(_lib.lib().segsde_gaussian_blur(_p(x), B * C, Hh, W, _p(wy), wy.numel(), _p(wx),
                                          wx.numel(), _p(tmp), _p(y), _stream(x)), "gaussian_blur"))
    return y


def softmax_to_nchw(logits_nhwc):
    """class softmax of NHWC logits [B,H,W,C] -> dense NCHW probabilities [B,C,H,W] (train.py:666)"""
    B, Hh, W, C = logits_nhwc.shape
    out = torch.empty((B, C, Hh, W), dtype=torch.float32, device=logits_nhwc.device)
    _timed('hbm_softmax', 8.0 * B * Hh * W * C, logits_nhwc, lambda: check(_lib.lib().segsde_softmax_nhwc_to_nchw(_p(_f32(logits_nhwc)), nhwc_ld(logits_nhwc), B, Hh * W, C, _p(out),
                                                 _stream(logits_nhwc)), "softmax_nhwc_to_nchw"))
    return out


def onehot_select_(prob_nchw, onehot, is_labeled):
    """mix_use_gt (train.py:667-672), in place: ``prob[i] = onehot[i]`` for every sample with ``is_labeled[i]``.
    prob: [B,C,H,W] fp32 dense; onehot: [B,C,H,W] int64 / float32 / uint8 (the loader's planes); is_labeled: [B]
    bool / integer tensor (moved to the device as uint8, never read back)."""
    B, C, Hh, W = prob_nchw.shape
    if tuple(onehot.shape) != (B, C, Hh, W):
        raise ValueError("onehot_lbl %s does not match the teacher softmax %s" % (tuple(onehot.shape), tuple(prob_nchw.shape)))
    if not prob_nchw.is_contiguous() or prob_nchw.dtype != torch.float32:
        raise ValueError("onehot_select_ works in place on a dense fp32 NCHW tensor")
    code = {torch.float32: 0, torch.int64: 1, torch.uint8: 2, torch.bool: 2}.get(onehot.dtype)
    if code is None:
        onehot, code = onehot.to(torch.int64), 1
    onehot = onehot.to(prob_nchw.device).contiguous()
    flags = torch.as_tensor(is_labeled).reshape(-1).to(device=prob_nchw.device).ne(0).to(torch.uint8).contiguous()
    if flags.numel() != B:
        raise ValueError("is_labeled has %d entries for a batch of %d" % (flags.numel(), B))
    check(_lib.lib().segsde_onehot_select(_p(prob_nchw), _p(onehot), code, _p(flags), B, C, Hh * W, _stream(prob_nchw)),
          "onehot_select")
    return prob_nchw


def minmax_normalize(x, as_uint8=False):
    """x: [B, ...] -> (x - min_b) / (max_b - min_b) per sample b (train.py:690-697); as_uint8: the 8-bit image
    loader/depth_estimator.py:83-91 stores (mul(255).byte() of the normalised map) instead"""
    x = _f32(x).contiguous()
    B = x.shape[0]
    HW = x[0].numel()
    out = torch.empty(x.shape, dtype=torch.uint8 if as_uint8 else torch.float32, device=x.device)
    L = _lib.lib()
    nb = L.segsde_minmax_normalize_workspace(B, HW)
    ws_ = _ws(nb, x)
    check(L.segsde_minmax_normalize(_p(x), B, HW, None if as_uint8 else _p(out), None, _p(out) if as_uint8 else None,
                                    _p(ws_), nb, _stream(x)), "minmax_normalize")
    return out


def disp_to_depth_upsampled(disp, out_hw, min_depth, max_depth):
    """[B,1,hs,ws] disparity -> [B,1,H,W] depth (loss/monodepth_loss.py:54-62)"""
    disp = _f32(disp).contiguous()
    B, _, hs, ws = disp.shape
    Hh, W = out_hw
    depth = torch.empty((B, 1, Hh, W), dtype=torch.float32, device=disp.device)
    check(_lib.lib().segsde_disp_to_depth(_p(disp), hs, ws, B, Hh, W, float(min_depth), float(max_depth), _p(depth),
                                          _stream(disp)), "disp_to_depth")
    return depth


def confusion_update(hist, gt, pred=None, logits=None):
    """hist: int64 [C*C] on the device (accumulated in place); gt: int64 [B,H,W]; pred int64 [B,H,W] or logits [B,C,H,W]
    (NCHW-logical, any of dense NCHW / channels-last memory)."""
    gt = gt.contiguous()
    B = gt.shape[0]
    HW = gt.numel() // B
    C = int(round(hist.numel() ** 0.5))
    if logits is not None:
        lg = _f32(logits)
        assert lg.shape[1] == C and lg.shape[0] == B and lg.shape[2] * lg.shape[3] == HW
        sb, sc, sh, sw = lg.stride()
        if sh != lg.shape[3] * sw:      # rows must follow each other with the pixel stride
            lg = lg.contiguous()
            sb, sc, sh, sw = lg.stride()
        check(_lib.lib().segsde_confusion_update(_p(lg), sb, sc, sw, None, _p(gt), B, HW, C, _p(hist), _stream(gt)),
              "confusion_update")
    else:
        pred = pred.contiguous().to(torch.int64)
        check(_lib.lib().segsde_confusion_update(None, 0, 0, 0, _p(pred), _p(gt), B, HW, C, _p(hist), _stream(gt)),
              "confusion_update")
    return hist


# ----------------------------------------------------------------------------------------------
# device side of the data loader (csrc/batchprep.hip; loader/device_batch.py is the caller)
# ----------------------------------------------------------------------------------------------
def _u8(t, name):
    if t.dtype != torch.uint8:
        raise TypeError("%s must be uint8, got %s" % (name, t.dtype))
    return t.contiguous()


def _crop_args(B, crop_xy, flip):
    if crop_xy is not None and (crop_xy.dtype != torch.int32 or tuple(crop_xy.shape) != (B, 2)):
        raise TypeError("crop_xy must be int32 [B,2]")
    if flip is not None and (flip.dtype != torch.uint8 or tuple(flip.shape) != (B,)):
        raise TypeError("flip must be uint8 [B]")
    return (None if crop_xy is None else crop_xy.contiguous()), (None if flip is None else flip.contiguous())


def _out_like(t, shape, dtype, like, name):
    """a caller's output buffer: exactly the tensor the kernel writes, or a fresh one"""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), like.device))
    return t


def batchprep_crop(frames, crop_xy, flip, ch, cw, u8_out=None, f32_out=None):
    """frames [B,H,W,3] uint8 -> (uint8 [B,3,ch,cw], float32 [B,3,ch,cw] = u8 / 255); flip first, then crop"""
    frames = _u8(frames, "frames")
    B, H, W, C = frames.shape
    if C != 3:
        raise ValueError("frames must be [B,H,W,3]")
    crop_xy, flip = _crop_args(B, crop_xy, flip)
    u8_out = _out_like(u8_out, (B, 3, ch, cw), torch.uint8, frames, "u8_out")
    f32_out = _out_like(f32_out, (B, 3, ch, cw), torch.float32, frames, "f32_out")
    check(_lib.lib().segsde_batchprep_crop(_p(frames), B, H, W, _p(crop_xy), _p(flip), int(ch), int(cw), _p(u8_out), _p(f32_out),
                                           _stream(frames)), "batchprep_crop")
    return u8_out, f32_out


def batchprep_pyramid_level(src, coef, u8_out=None, f32_out=None):
    """src [...,Hs,Ws] uint8 planes -> the level below (exactly half in both directions), uint8 and float32; coef: int32 [2,7,12]
    (loader/device_batch.lanczos_half_table)"""
    src = _u8(src, "src")
    Hs, Ws = src.shape[-2:]
    if Hs % 2 or Ws % 2:
        Hd, Wd = (Hs + 1) // 2, (Ws + 1) // 2          # the library rejects it (SEGSDE_ERR_SHAPE)
    else:
        Hd, Wd = Hs // 2, Ws // 2
    lead = tuple(src.shape[:-2])
    if coef.dtype != torch.int32 or tuple(coef.shape) != (2, 7, 12):
        raise TypeError("coef must be int32 [2,7,12]")
    u8_out = _out_like(u8_out, lead + (Hd, Wd), torch.uint8, src, "u8_out")
    f32_out = _out_like(f32_out, lead + (Hd, Wd), torch.float32, src, "f32_out")
    planes = src.numel() // (Hs * Ws)
    coef = _c(coef)
    check(_lib.lib().segsde_batchprep_pyramid_level(_p(src), planes, Hs, Ws, _p(coef), Hd, Wd,
                                                    _p(u8_out), _p(f32_out), _stream(src)), "batchprep_pyramid_level")
    return u8_out, f32_out


def batchprep_labels(lbl, crop_xy, flip, ch, cw, lut, is_labeled=None, ignore_index=250, n_classes=0, want_onehot=False):
    """lbl [B,H,W] uint8 -> int64 [B,ch,cw] through the 256-entry table `lut` (int64), and optionally the one-hot planes"""
    lbl = _u8(lbl, "lbl")
    B, H, W = lbl.shape
    crop_xy, flip = _crop_args(B, crop_xy, flip)
    if lut.dtype != torch.int64 or lut.numel() != 256:
        raise TypeError("lut must be int64 [256]")
    if is_labeled is not None and (is_labeled.dtype != torch.uint8 or tuple(is_labeled.shape) != (B,)):
        raise TypeError("is_labeled must be uint8 [B]")
    out = torch.empty((B, ch, cw), dtype=torch.int64, device=lbl.device)
    onehot = torch.empty((B, n_classes, ch, cw), dtype=torch.int64, device=lbl.device) if want_onehot else None
    lut = _c(lut)
    check(_lib.lib().segsde_batchprep_labels(_p(lbl), B, H, W, _p(crop_xy), _p(flip), int(ch), int(cw), _p(lut),
                                             _p(is_labeled), int(ignore_index), int(n_classes), _p(out), _p(onehot), _stream(lbl)),
          "batchprep_labels")
    return out, onehot


def batchprep_plane(src, crop_xy, flip, ch, cw):
    """src [B,H,W] uint8 -> float32 [B,1,ch,cw] = u8 / 255"""
    src = _u8(src, "src")
    B, H, W = src.shape
    crop_xy, flip = _crop_args(B, crop_xy, flip)
    out = torch.empty((B, 1, ch, cw), dtype=torch.float32, device=src.device)
    check(_lib.lib().segsde_batchprep_plane(_p(src), B, H, W, _p(crop_xy), _p(flip), int(ch), int(cw), _p(out), _stream(src)),
          "batchprep_plane")
    return out


COLOR_JITTER_MAX_PIXELS = (2 ** 32 - 1) // 255        # SEGSDE_COLOR_JITTER_MAX_PIXELS: 255 * h * w fits the uint32 sum of L


def _host_table(t, B, cols, name):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.shape != ((B,) if cols is None else (B, cols)):
        raise ValueError("%s must have shape %s, got %s" % (name, (B,) if cols is None else (B, cols), a.shape))
    return a


def batchprep_color_jitter(u8, apply, alpha, hue_shift, order, f32_out=None, ops=15):
    """torchvision 0.7.0's PIL ColorJitter + ToTensor on planar uint8 images: u8 [...,B,3,h,w] (batchprep_crop's output; leading
    dimensions are frames, whose images share the sample's parameters) -> float32 of the same shape.  Per-sample HOST tables
    (numpy arrays or tensors; they are validated here and then uploaded): apply [B] bool, alpha [B,3] = the brightness, contrast
    and saturation factors (cast to float32 as C casts a double), hue_shift [B] integers in 0..255 = (uint8)(hue_factor * 255),
    order [B,4] = a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue per sample.  All four operations run in that
    order.  ``ops``: bit i set = operation i runs (15, all four, is ColorJitter; alpha 1.0 is an exact identity of a blend, but a
    hue step with shift 0 still alters pixels through its HSV round trip, so a single operation is run by masking the others)."""
    u8 = _u8(u8, "u8")
    if u8.dim() < 4 or u8.shape[-3] != 3:
        raise ValueError("u8 must be [...,B,3,h,w], got %s" % (tuple(u8.shape),))
    B, _, h, w = u8.shape[-4:]
    if min(B, h, w) < 1:
        raise ValueError("u8 is empty: %s" % (tuple(u8.shape),))
    apply = _host_table(apply, B, None, "apply")
    alpha = _host_table(alpha, B, 3, "alpha")
    hue_shift = _host_table(hue_shift, B, None, "hue_shift")
    order = _host_table(order, B, 4, "order")
    if hue_shift.dtype.kind not in "iu":
        raise ValueError("hue_shift must be integers")
    if ((hue_shift < 0) | (hue_shift > 255)).any():
        raise ValueError("hue_shift outside 0..255")
    if order.dtype.kind not in "iu" or not (np.sort(order.astype(np.int64), axis=1) == np.arange(4)).all():
        raise ValueError("every row of order must be a permutation of 0..3")
    if h * w > COLOR_JITTER_MAX_PIXELS:
        raise ValueError("images of %dx%d pixels: the contrast mean is summed in 32 bits, at most %d pixels" % (h, w, COLOR_JITTER_MAX_PIXELS))
    if int(ops) != ops or not 0 <= ops <= 15:
        raise ValueError("ops is a mask of the four operations (0..15)")
    images = u8.numel() // (3 * h * w)
    if images < 1 or images > 65535:
        raise ValueError("%d images in one call (1..65535)" % images)
    f32_out = _out_like(f32_out, tuple(u8.shape), torch.float32, u8, "f32_out")
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(u8.device, non_blocking=True)
    tables = (dev(apply != 0, np.uint8), dev(alpha, np.float32), dev(hue_shift, np.int32), dev(order, np.uint8))
    sums = torch.empty((images,), dtype=torch.int32, device=u8.device)
    check(_lib.lib().segsde_batchprep_color_jitter(_p(u8), images, B, h, w, _p(tables[0]), _p(tables[1]), _p(tables[2]), _p(tables[3]),
                                                   int(ops), _p(sums), _p(f32_out), _stream(u8)), "batchprep_color_jitter")
    return f32_out


def batchprep_labels_rgb(lbl, crop_xy, flip, ch, cw, colors, ignore_id=-1, is_labeled=None, ignore_index=250, n_classes=0,
                         want_onehot=False):
    """lbl [B,H,W,3] uint8 colour-coded label map -> int64 [B,ch,cw]: the index of the last entry of `colors` (int32 [n], r | g << 8
    | b << 16) equal to the pixel, 0 when none is; id `ignore_id` becomes ignore_index.  Optionally the one-hot planes."""
    lbl = _u8(lbl, "lbl")
    if lbl.dim() != 4 or lbl.shape[-1] != 3:
        raise ValueError("lbl must be [B,H,W,3], got %s" % (tuple(lbl.shape),))
    B, H, W, _ = lbl.shape
    crop_xy, flip = _crop_args(B, crop_xy, flip)
    if colors.dtype != torch.int32 or colors.dim() != 1:
        raise TypeError("colors must be int32 [n]")
    if is_labeled is not None and (is_labeled.dtype != torch.uint8 or tuple(is_labeled.shape) != (B,)):
        raise TypeError("is_labeled must be uint8 [B]")
    out = torch.empty((B, ch, cw), dtype=torch.int64, device=lbl.device)
    onehot = torch.empty((B, n_classes, ch, cw), dtype=torch.int64, device=lbl.device) if want_onehot else None
    colors = _c(colors)
    check(_lib.lib().segsde_batchprep_labels_rgb(_p(lbl), B, H, W, _p(crop_xy), _p(flip), int(ch), int(cw), _p(colors),
                                                 colors.numel(), int(ignore_id), _p(is_labeled), int(ignore_index), int(n_classes),
                                                 _p(out), _p(onehot), _stream(lbl)), "batchprep_labels_rgb")
    return out, onehot


RESAMPLE_MAX_TAPS = 64        # SEGSDE_RESAMPLE_MAX_TAPS: the widest window table the resampling kernels stage


def _resize_desc(desc):
    if desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 8 or desc.shape[0] < 1 or not desc.is_contiguous():
        raise TypeError("desc must be a contiguous int64 [n,8] tensor")
    return desc


def batchprep_resample_rows(desc, max_rows, Wd, max_taps, max_span):
    """the horizontal pass of Pillow's 8-bit Lanczos resampler over the samples `desc` describes (int64 [n,8] on the device: src, dst,
    bounds, weights, in_h, in_w, taps, 0; include/segsde_hip.h) -- loader/device_batch.pil_resize builds it"""
    desc = _resize_desc(desc)
    check(_lib.lib().segsde_batchprep_resample_rows(_p(desc), desc.shape[0], int(max_rows), int(Wd), int(max_taps), int(max_span),
                                                    _stream(desc)), "batchprep_resample_rows")


def batchprep_resample_cols(desc, row_bytes, Hd, max_taps, max_span):
    """the vertical pass: rows of `row_bytes` bytes, Hd output rows per sample"""
    desc = _resize_desc(desc)
    check(_lib.lib().segsde_batchprep_resample_cols(_p(desc), desc.shape[0], int(row_bytes), int(Hd), int(max_taps), int(max_span),
                                                    _stream(desc)), "batchprep_resample_cols")


def batchprep_resize_nearest(desc, Hd, Wd, channels):
    """Image.NEAREST through per-axis index tables (desc rows: src, dst, row table, column table, in_h, in_w, 0, 0)"""
    desc = _resize_desc(desc)
    check(_lib.lib().segsde_batchprep_resize_nearest(_p(desc), desc.shape[0], int(Hd), int(Wd), int(channels), _stream(desc)),
          "batchprep_resize_nearest")


# ----------------------------------------------------------------------------------------------
# label selection (csrc/labelsel.hip; label_selection.py)
# ----------------------------------------------------------------------------------------------
DEPTH_ERROR_TYPES = ("abs", "abs_inv_log", "abs_inv", "sq", "abs_rel", "sq_rel", "abs_log")      # SEGSDE_DEPTH_ERR_*
POOL_TRANSFORMS = ("none", "inv_clamp", "log_inv_clamp")                                          # SEGSDE_POOL_*
LABELSEL_FPS_MAX_N = 32000                                                                        # SEGSDE_LABELSEL_FPS_MAX_N
LABELSEL_PATCH_MAX_P = 128                                                                        # SEGSDE_LABELSEL_PATCH_MAX_P


def _nchw_strides(x):
    """element strides of a [B,C,H,W] view as the kernels read it (any layout: dense NCHW, channels-last, pitched slices)"""
    return [int(s) for s in x.stride()]


def labelsel_score(logits, disp_pred=None, disp_pseudo=None, error_types=(), want_maps=False, table=None):
    """logits [B,C,H,W] (any strides), disp_pred / disp_pseudo [B,H,W]; error_types: names from DEPTH_ERROR_TYPES.
    -> (table float32 [B, 1+T] = (entropy_mean, depth_error[0..T)), entropy_map [B,H,W] or None, error_maps [B,T,H,W] or None).
    ``table``: an optional [B, 1+T] dense destination (rows of a larger score table).  Nothing is copied to the host."""
    logits = _f32(logits, "logits")
    B, C, Hh, W = logits.shape
    T = len(error_types)
    try:
        codes = [DEPTH_ERROR_TYPES.index(t) for t in error_types]
    except ValueError:
        raise NotImplementedError(error_types)
    if T:
        disp_pred, disp_pseudo = _f32(disp_pred, "disp_pred").contiguous(), _f32(disp_pseudo, "disp_pseudo").contiguous()
        if tuple(disp_pred.shape) != (B, Hh, W) or tuple(disp_pseudo.shape) != (B, Hh, W):
            raise ValueError("disparities must be [B,H,W] = %s, got %s / %s" % ((B, Hh, W), tuple(disp_pred.shape),
                                                                                tuple(disp_pseudo.shape)))
    else:
        disp_pred = disp_pseudo = None
    if table is None:
        table = torch.empty((B, 1 + T), dtype=torch.float32, device=logits.device)
    elif tuple(table.shape) != (B, 1 + T) or not table.is_contiguous() or table.dtype != torch.float32:
        raise ValueError("table must be a dense float32 [%d, %d]" % (B, 1 + T))
    ent = torch.empty((B, Hh, W), dtype=torch.float32, device=logits.device) if want_maps else None
    err = torch.empty((B, T, Hh, W), dtype=torch.float32, device=logits.device) if want_maps and T else None
    L = _lib.lib()
    nb = L.segsde_labelsel_score_workspace(B, Hh, W, T)
    ws_ = _ws(nb, logits)
    sb, sc, sh, sw = _nchw_strides(logits)
    arr = (ctypes.c_int * max(T, 1))(*codes)
    check(L.segsde_labelsel_score(_p(logits), sb, sc, sh, sw, B, C, Hh, W, _p(disp_pred), _p(disp_pseudo), arr, T, _p(table),
                                  _p(ent), _p(err), _p(ws_), nb, _stream(logits)), "labelsel_score")
    return table, ent, err


def labelsel_pool(x, h, bank, row0, pool="avg", transform="none"):
    """adaptive_{avg,max}_pool2d(x [B,C,H,W], (h, 2h)) -> rows [row0, row0+B) of the float32 bank [N, >= C*h*2h]"""
    x = _f32(x, "features")
    B, C, Hh, W = x.shape
    if pool not in ("avg", "max"):
        raise NotImplementedError(pool)
    if bank.dtype != torch.float32 or bank.dim() != 2 or bank.stride(1) != 1:
        raise ValueError("the bank is a float32 [N, D] tensor with dense rows")
    sb, sc, sh, sw = _nchw_strides(x)
    check(_lib.lib().segsde_labelsel_pool(_p(x), sb, sc, sh, sw, B, C, Hh, W, int(h), int(pool == "max"),
                                          POOL_TRANSFORMS.index(transform), _p(bank), int(bank.stride(0)), int(bank.shape[0]),
                                          int(row0), _stream(x)), "labelsel_pool")
    return bank


def labelsel_normalize_(bank, C, P):
    """in place: (f - mean_c) / std_c per channel over the rows and the P positions of the bank [N, C*P] (torch.std_mean, unbiased)"""
    if bank.dtype != torch.float32 or bank.dim() != 2 or bank.stride(1) != 1 or bank.shape[1] != C * P:
        raise ValueError("the bank is a float32 [N, C*P] tensor with dense rows")
    L = _lib.lib()
    N = int(bank.shape[0])
    nb = L.segsde_labelsel_normalize_workspace(N, int(C), int(P))
    ws_ = _ws(nb, bank)
    check(L.segsde_labelsel_normalize(_p(bank), int(bank.stride(0)), N, int(C), int(P), _p(ws_), nb, _stream(bank)),
          "labelsel_normalize")
    return bank


def labelsel_distance(bank, p=2, bias=None, out=None):
    """[N, D] bank -> [N, N] distances (p = 1 or 2, direct form), + bias[j] per column when given, zero diagonal.
    ``out``: an optional float32 [N, >= N] destination with dense rows (its columns past N are left alone)."""
    if bank.dtype != torch.float32 or bank.dim() != 2 or (bank.shape[1] > 1 and bank.stride(1) != 1):
        raise ValueError("the bank is a float32 [N, D] tensor with dense rows")
    N, D = int(bank.shape[0]), int(bank.shape[1])
    if p not in (1, 2):
        raise NotImplementedError("labelsel_distance: p = %r (only 1 and 2)" % (p,))
    if out is None:
        out = torch.empty((N, N), dtype=torch.float32, device=bank.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != N or out.shape[1] != N or (N > 1 and out.stride(1) != 1):
        raise ValueError("out must be a float32 [N, N] view with dense rows")
    if bias is not None:
        bias = _f32(bias, "bias").to(bank.device).contiguous()
        if bias.numel() != N:
            raise ValueError("one bias per sample: got %d for %d" % (bias.numel(), N))
    ld = int(bank.stride(0)) if N > 1 else D
    ldo = int(out.stride(0)) if N > 1 else N
    check(_lib.lib().segsde_labelsel_distance(_p(bank), ld, N, D, int(p), _p(bias), _p(out), ldo, _stream(bank)), "labelsel_distance")
    return out


def labelsel_patch_distance(bank, C, P, p=2, bias=None, out=None):
    """[N, C*P] bank (patch a of image n: bank[n, c*P + a]) -> [N, N] directed Chamfer distances
    D[i, j] = mean_a min_b ||f_i[:, a] - f_j[:, b]||_p (p = 1 or 2, direct form), + bias[j] per column when given, zero diagonal.
    Not symmetric (except at P = 1); a NaN feature makes every distance it enters NaN.  P <= LABELSEL_PATCH_MAX_P.
    ``out``: an optional float32 [N, >= N] destination with dense rows (its columns past N are left alone)."""
    C, P = int(C), int(P)
    if bank.dtype != torch.float32 or bank.dim() != 2 or bank.shape[1] != C * P or (bank.shape[1] > 1 and bank.stride(1) != 1):
        raise ValueError("the bank is a float32 [N, C*P] tensor with dense rows")
    N = int(bank.shape[0])
    if p not in (1, 2):
        raise NotImplementedError("labelsel_patch_distance: p = %r (only 1 and 2)" % (p,))
    if P > LABELSEL_PATCH_MAX_P:
        raise NotImplementedError("labelsel_patch_distance: P = %d patches per image (at most %d)" % (P, LABELSEL_PATCH_MAX_P))
    if out is None:
        out = torch.empty((N, N), dtype=torch.float32, device=bank.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != N or out.shape[1] != N or (N > 1 and out.stride(1) != 1):
        raise ValueError("out must be a float32 [N, N] view with dense rows")
    if bias is not None:
        bias = _f32(bias, "bias").to(bank.device).contiguous()
        if bias.numel() != N:
            raise ValueError("one bias per sample: got %d for %d" % (bias.numel(), N))
    ld = int(bank.stride(0)) if N > 1 else C * P
    ldo = int(out.stride(0)) if N > 1 else N
    check(_lib.lib().segsde_labelsel_patch_distance(_p(bank), ld, N, C, P, int(p), _p(bias), _p(out), ldo, _stream(bank)),
          "labelsel_patch_distance")
    return out


def labelsel_farthest_point(dist, current, n_new, preselected=None):
    """dist float32 [N, N] (dense rows); current: indices (list / tensor) of the current samples; preselected: indices or None.
    -> (new indices, their distances) as two host lists of ints / a float32 CPU tensor: ONE device-to-host copy after the launch.
    The selection on a matrix that holds NaN is unspecified."""
    if dist.dtype != torch.float32 or dist.dim() != 2 or dist.shape[0] != dist.shape[1] or (dist.shape[1] > 1 and dist.stride(1) != 1):
        raise ValueError("dist is a square float32 matrix with dense rows")
    N = int(dist.shape[0])
    cur = [int(c) for c in (current.tolist() if torch.is_tensor(current) else current)]
    if not cur or min(cur) < 0 or max(cur) >= N:
        raise ValueError("current samples must be a non-empty list of indices in [0, %d)" % N)
    n_new = int(n_new)
    cur_t = torch.tensor(cur, dtype=torch.int32).to(dist.device)
    pre_t = None
    if preselected is not None:
        pre = [int(c) for c in (preselected.tolist() if torch.is_tensor(preselected) else preselected)]
        if pre and (min(pre) < 0 or max(pre) >= N):
            raise ValueError("preselected samples must be indices in [0, %d)" % N)
        m = np.zeros(N, dtype=np.uint8)
        m[pre] = 1
        pre_t = torch.from_numpy(m).to(dist.device)
    res = torch.zeros(1 + 2 * max(n_new, 1), dtype=torch.int32, device=dist.device)      # [count | indices | distances (fp32 bits)]
    ld = int(dist.stride(0)) if N > 1 else N
    check(_lib.lib().segsde_labelsel_farthest_point(_p(dist), ld, N, _p(cur_t), len(cur), _p(pre_t), n_new, _p(res[1:]),
                                                    _p(res[1 + max(n_new, 1):]), _p(res), _stream(dist)), "labelsel_farthest_point")
    host = res.cpu()
    count = int(host[0])
    idx = host[1:1 + count].tolist()
    d = host[1 + max(n_new, 1):1 + max(n_new, 1) + count].view(torch.float32).clone()
    return idx, d


# ----------------------------------------------------------------------------------------------
# rendering of inference outputs (csrc/render.hip; inference.py is the caller)
# ----------------------------------------------------------------------------------------------
RENDER_UNMAPPED = ("keep", "zero")                # SEGSDE_RENDER_UNMAPPED_*
RENDER_MAX_COLORS = 256                           # SEGSDE_RENDER_MAX_COLORS
COLORIZE_MAX_N = 1024                             # SEGSDE_COLORIZE_MAX_N


def _palette(label_colors, like):
    """[n,3] colours (tensor, array, list of triples or the loaders' {id: colour} dict with ids 0..n-1) -> device uint8 [n,3]"""
    if isinstance(label_colors, dict):
        if sorted(label_colors) != list(range(len(label_colors))):
            raise ValueError("a palette dict must have the keys 0..n-1")
        label_colors = [label_colors[i] for i in range(len(label_colors))]
    pal = label_colors if torch.is_tensor(label_colors) else torch.as_tensor(np.asarray(label_colors))
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
        raise ValueError("the palette is [n,3], got %s" % (tuple(pal.shape),))
    if pal.shape[0] > RENDER_MAX_COLORS:
        raise NotImplementedError("palettes of more than %d colours" % RENDER_MAX_COLORS)
    if pal.dtype != torch.uint8:
        if pal.is_floating_point() or bool((pal < 0).any()) or bool((pal > 255).any()):
            raise ValueError("palette entries are integers in 0..255")
        pal = pal.to(torch.uint8)
    return pal.to(like.device).contiguous()


def render_labels(label_colors, logits=None, ids=None, unmapped="keep", return_ids=False):
    """logits [B,C,H,W] (float32, any strides: dense NCHW, channels-last, slices) or ids [B,H,W] (int64 / uint8) -> uint8
    [B,H,W,3] colours of the first-maximum class (and the uint8 id plane [B,H,W] with return_ids).  An id outside the palette
    keeps its value as a grey (``keep``) or turns black (``zero``).  One launch."""
    if (logits is None) == (ids is None):
        raise ValueError("give either logits or ids")
    if unmapped not in RENDER_UNMAPPED:
        raise NotImplementedError("unmapped = %r (one of %s)" % (unmapped, RENDER_UNMAPPED))
    src = logits if ids is None else ids
    pal = _palette(label_colors, src)
    if ids is None:
        logits = _f32(logits, "logits")
        if logits.dim() != 4:
            raise ValueError("logits are [B,C,H,W], got %s" % (tuple(logits.shape),))
        B, C, Hh, W = logits.shape
        sb, sc, sh, sw = (int(s) for s in logits.stride())
        code = 0
    else:
        if ids.dtype not in (torch.int64, torch.uint8):
            raise TypeError("ids must be int64 or uint8, got %s" % ids.dtype)
        if ids.dim() != 3:
            raise ValueError("ids are [B,H,W], got %s" % (tuple(ids.shape),))
        ids = ids.contiguous()
        B, Hh, W = ids.shape
        C, sb, sc, sh, sw = 0, 0, 0, 0, 0
        code = 1 if ids.dtype == torch.int64 else 2          # SEGSDE_DTYPE_I64 / SEGSDE_DTYPE_U8
    rgb = torch.empty((B, Hh, W, 3), dtype=torch.uint8, device=src.device)
    out_ids = torch.empty((B, Hh, W), dtype=torch.uint8, device=src.device) if return_ids else None
    nbytes = B * Hh * W * ((4 * C + 4) if ids is None else (ids.element_size() + 3))
    _timed("hbm_render_labels", float(nbytes), src, lambda: check(_lib.lib().segsde_render_labels(
        _p(logits), sb, sc, sh, sw, _p(ids), code, B, C, Hh, W, _p(pal), int(pal.shape[0]), RENDER_UNMAPPED.index(unmapped), _p(rgb),
        _p(out_ids), _stream(src)), "render_labels"))
    return (rgb, out_ids) if return_ids else rgb


def render_unit_image(x):
    """float32 image [B,C,H,W] in [0,1] (C = 1 or 3, any strides) -> uint8 [B,H,W,C]: mul(255), add(0.5), clamp(0,255), truncate"""
    x = _f32(x, "image")
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise ValueError("the image is [B,1,H,W] or [B,3,H,W], got %s" % (tuple(x.shape),))
    B, C, Hh, W = x.shape
    sb, sc, sh, sw = (int(s) for s in x.stride())
    out = torch.empty((B, Hh, W, C), dtype=torch.uint8, device=x.device)
    _timed("hbm_render_unit_image", float(5 * B * C * Hh * W), x, lambda: check(_lib.lib().segsde_render_unit_image(
        _p(x), sb, sc, sh, sw, B, C, Hh, W, _p(out), _stream(x)), "render_unit_image"))
    return out


def colorize(img, lut, mask_zero=False):
    """img float32 [B,H,W]; lut float32 [N+3,3] (the map's N rows, then its under / over / bad colours) -> float32 [B,H,W,3]:
    the reference's _colorize with max_percentile = 100, per image"""
    img = _f32(img, "image").contiguous()
    if img.dim() != 3:
        raise ValueError("images are [B,H,W], got %s" % (tuple(img.shape),))
    lut = _f32(lut, "lut")
    if lut.dim() != 2 or lut.shape[1] != 3 or lut.shape[0] < 4:
        raise ValueError("the table is [N+3,3], got %s" % (tuple(lut.shape),))
    N = int(lut.shape[0]) - 3
    if N > COLORIZE_MAX_N:
        raise NotImplementedError("colour maps of more than %d entries" % COLORIZE_MAX_N)
    lut = lut.to(img.device).contiguous()
    B, Hh, W = img.shape
    out = torch.empty((B, Hh, W, 3), dtype=torch.float32, device=img.device)
    L = _lib.lib()
    nb = L.segsde_colorize_workspace(B, Hh, W)
    ws_ = _ws(nb, img)
    _timed("hbm_colorize", float(20 * B * Hh * W), img, lambda: check(L.segsde_colorize(
        _p(img), B, Hh, W, _p(lut), N, int(bool(mask_zero)), _p(out), _p(ws_), nb, _stream(img)), "colorize"))
    return out


# ----------------------------------------------------------------------------------------------
# depth evaluation (csrc/depthmetrics.hip; evaluation/metrics.py::runningDepthScore and MonodepthLoss.compute_depth_metrics call it)
# ----------------------------------------------------------------------------------------------
DEPTH_ERROR_COLUMNS = ("abs_rel", "sq_rel", "rms", "log_rms", "a1", "a2", "a3", "n", "n_a1", "n_a2", "n_a3", "med_gt", "med_pred",
                       "ratio")                                             # SEGSDE_DEPTH_ERRORS_COLUMNS


def _depth_map(t, name):
    t = _f32(t, name)
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError("%s is [B,H,W] or [B,1,H,W], got %s" % (name, tuple(t.shape)))
    return t.contiguous()


def depth_errors(gt, pred, min_depth=1e-3, max_depth=80.0, median_scaling=True, scale=1.0, crop=None):
    """gt, pred float32 [B,H,W] or [B,1,H,W] (any strides) -> float64 [B,14] on the device, columns DEPTH_ERROR_COLUMNS: per image
    the seven monocular-depth errors over the pixels with min_depth < gt < max_depth inside crop = (y0, y1, x0, x1), after scaling
    pred by scale * median(gt) / median(pred) (exact medians, numpy's convention) and clamping it to [min_depth, max_depth]; then n,
    the three threshold counts, the two medians and the ratio.  An image without a valid pixel: n = 0, NaN elsewhere.  No host
    synchronisation."""
    gt, pred = _depth_map(gt, "gt"), _depth_map(pred, "pred")
    if gt.shape != pred.shape:
        raise ValueError("gt %s and pred %s differ in shape" % (tuple(gt.shape), tuple(pred.shape)))
    if gt.device != pred.device:
        raise ValueError("gt is on %s, pred on %s" % (gt.device, pred.device))
    B, Hh, W = (int(s) for s in gt.shape)
    if B < 1 or Hh < 1 or W < 1:
        raise ValueError("empty depth maps %s" % (tuple(gt.shape),))
    y0, y1, x0, x1 = (0, Hh, 0, W) if crop is None else (int(c) for c in crop)
    if not (0 <= y0 < y1 <= Hh and 0 <= x0 < x1 <= W):
        raise ValueError("crop (y0, y1, x0, x1) = %r is empty or leaves the %d x %d image" % (crop, Hh, W))
    if not 0 <= min_depth < max_depth:
        raise ValueError("0 <= min_depth < max_depth expected, got %r, %r" % (min_depth, max_depth))
    table = torch.empty((B, len(DEPTH_ERROR_COLUMNS)), dtype=torch.float64, device=gt.device)
    L = _lib.lib()
    nb = L.segsde_depth_errors_workspace(B, Hh, W)
    ws_ = _ws(nb, gt)
    _timed("hbm_depth_errors", float(8 * B * (y1 - y0) * (x1 - x0)), gt, lambda: check(L.segsde_depth_errors(
        _p(gt), _p(pred), B, Hh, W, float(min_depth), float(max_depth), int(bool(median_scaling)), float(scale), y0, y1, x0, x1,
        _p(table), _p(ws_), nb, _stream(gt)), "depth_errors"))
    return table


# ----------------------------------------------------------------------------------------------
# segmentation validation at label resolution (csrc/segeval.hip; evaluation/metrics.py::runningScore.update_from_logits and
# trainer.validate call it)
# ----------------------------------------------------------------------------------------------
def seg_eval(logits, gt, n_classes=None, hist=None, ignore_index=250, want_loss=True, want_ids=False):
    """logits [B,C,Hi,Wi] (NCHW-logical; dense, channels-last or a slice: read in place through its strides), gt int64 [B,Ht,Wt] of any
    size -> (hist, loss_pair, ids).  Per label pixel: the logits interpolated bilinearly (align_corners=True) to the label grid,
    their argmax (lowest index on a tie), ``hist[C * gt + argmax] += 1`` into the int64 [C*C] ``hist`` (a fresh zero one when None and
    ``n_classes`` is given; None back when neither is), the cross-entropy sum and pixel count over ``gt != ignore_index`` as a
    float64 [2] (``want_loss``), the argmax as a uint8 [B,Ht,Wt] plane (``want_ids``).  The resized logits are never materialised; no
    host synchronisation; two calls on the same input return the same bits."""
    if not (torch.is_tensor(logits) and logits.dim() == 4 and logits.is_floating_point()):
        raise TypeError("logits must be a floating-point [B,C,Hi,Wi] tensor")
    if not (torch.is_tensor(gt) and gt.dim() == 3 and gt.dtype == torch.int64):
        raise TypeError("gt must be an int64 [B,Ht,Wt] tensor")
    if gt.shape[0] != logits.shape[0]:
        raise ValueError("logits hold %d images, gt %d" % (logits.shape[0], gt.shape[0]))
    if gt.device != logits.device:
        raise ValueError("logits are on %s, gt on %s" % (logits.device, gt.device))
    B, C, Hi, Wi = (int(s) for s in logits.shape)
    Ht, Wt = int(gt.shape[1]), int(gt.shape[2])
    if min(B, C, Hi, Wi, Ht, Wt) < 1:
        raise ValueError("empty logits %s or labels %s" % (tuple(logits.shape), tuple(gt.shape)))
    if n_classes is not None and int(n_classes) != C:
        raise ValueError("n_classes = %d, but the logits have %d classes" % (n_classes, C))
    if hist is not None:
        if not (torch.is_tensor(hist) and hist.dtype == torch.int64 and hist.numel() == C * C and hist.is_contiguous()):
            raise ValueError("hist must be a contiguous int64 tensor of %d x %d elements" % (C, C))
        if hist.device != logits.device:
            raise ValueError("hist is on %s, logits on %s" % (hist.device, logits.device))
    elif n_classes is not None:
        hist = torch.zeros(C * C, dtype=torch.int64, device=logits.device)
    if want_ids and C > 256:
        raise ValueError("ids are uint8: at most 256 classes, got %d" % C)
    if hist is None and not want_loss and not want_ids:
        raise ValueError("nothing to compute: no hist (or n_classes), want_loss and want_ids are off")
    lg, gt = logits.detach().float(), gt.detach().contiguous()
    pair = torch.empty(2, dtype=torch.float64, device=lg.device) if want_loss else None
    ids = torch.empty((B, Ht, Wt), dtype=torch.uint8, device=lg.device) if want_ids else None
    L = _lib.lib()
    nb = L.segsde_seg_eval_workspace(B, Ht, Wt) if want_loss else 0
    ws_ = _ws(nb, lg) if want_loss else None
    sb, sc, sh, sw = lg.stride()
    nbytes = 4.0 * B * C * Hi * Wi + B * Ht * Wt * (8.0 + (1.0 if want_ids else 0.0))
    _timed("hbm_seg_eval", nbytes, lg, lambda: check(L.segsde_seg_eval(
        _p(lg), sb, sc, sh, sw, B, C, Hi, Wi, _p(gt), Ht, Wt, int(ignore_index), _p(hist), _p(pair), _p(ids), _p(ws_), nb,
        _stream(lg)), "seg_eval"))
    return hist, pair, ids


# ----------------------------------------------------------------------------------------------
# segmentation evaluation with test-time ensembling (csrc/segens.hip; evaluation/metrics.py::runningScore.update_from_views,
# trainer.validate(tta=...) and inference.predict_batch(tta=...) call it)
# ----------------------------------------------------------------------------------------------
SEG_ENS_MAX_VIEWS = 16          # SEGSDE_SEG_ENS_MAX_VIEWS
SEG_ENS_MAX_CLASSES = 171       # SEGSDE_SEG_ENS_MAX_CLASSES


def _seg_ens_views(views, flips, weights):
    """-> (float32 view tensors, flip flags, weights, B, C); everything that can be refused without the library"""
    if not isinstance(views, (list, tuple)):
        raise TypeError("views must be a list of [B,C,h,w] logit tensors")
    K = len(views)
    if K == 0:
        raise ValueError("views is empty: at least one view is needed")
    if K > SEG_ENS_MAX_VIEWS:
        raise ValueError("%d views: at most %d are ensembled in one call" % (K, SEG_ENS_MAX_VIEWS))
    for k, v in enumerate(views):
        if not (torch.is_tensor(v) and v.dim() == 4 and v.is_floating_point()):
            raise TypeError("views[%d] must be a floating-point [B,C,h,w] tensor" % k)
        if min(int(s) for s in v.shape) < 1:
            raise ValueError("views[%d] is empty: %s" % (k, tuple(v.shape)))
        if v.shape[0] != views[0].shape[0]:
            raise ValueError("views[%d] holds %d images, views[0] %d" % (k, v.shape[0], views[0].shape[0]))
        if v.shape[1] != views[0].shape[1]:
            raise ValueError("views[%d] has %d classes, views[0] %d" % (k, v.shape[1], views[0].shape[1]))
        if v.device != views[0].device:
            raise ValueError("views[%d] is on %s, views[0] on %s" % (k, v.device, views[0].device))
    flips = [False] * K if flips is None else [bool(f) for f in flips]
    if len(flips) != K:
        raise ValueError("%d flips for %d views" % (len(flips), K))
    weights = [1.0] * K if weights is None else [float(w) for w in weights]
    if len(weights) != K:
        raise ValueError("%d weights for %d views" % (len(weights), K))
    for k, w in enumerate(weights):
        if not (w >= 0.0 and w != float("inf")):
            raise ValueError("weights[%d] = %r: weights are finite and >= 0" % (k, w))
        if w > 0.0 and float(np.float32(w)) in (0.0, float("inf")):
            raise ValueError("weights[%d] = %r is not representable as a positive float32" % (k, w))
    if not any(w > 0.0 for w in weights):
        raise ValueError("weights %r are all zero" % (weights,))
    B, C = int(views[0].shape[0]), int(views[0].shape[1])
    if C > SEG_ENS_MAX_CLASSES:
        raise NotImplementedError("%d classes: the ensemble kernel holds at most %d on chip" % (C, SEG_ENS_MAX_CLASSES))
    lgs = [v.detach().float() for v in views]
    return lgs, flips, weights, B, C


def _seg_ens_descs(lgs, flips, weights):
    descs = (_lib.SegEnsView * len(lgs))()
    for k, lg in enumerate(lgs):
        sb, sc, sh, sw = lg.stride()
        descs[k] = _lib.SegEnsView(lg.data_ptr(), sb, sc, sh, sw, int(lg.shape[2]), int(lg.shape[3]), int(flips[k]), weights[k])
    return descs


def seg_eval_ensemble_plan(views, size, flips=None, weights=None):
    """-> (tile rows, [route per view]): the plan ``seg_eval_ensemble`` follows for these views and the label size ``size``; a
    route is "lds" (the tile's source footprint is staged in LDS), "direct" (taps read from memory) or None (weight 0)"""
    lgs, flips, weights, B, C = _seg_ens_views(views, flips, weights)
    descs = _seg_ens_descs(lgs, flips, weights)
    staged = (ctypes.c_int * len(lgs))()
    th = _lib.lib().segsde_seg_ens_plan(descs, len(lgs), C, int(size[0]), int(size[1]), staged)
    check(min(th, 0), "seg_eval_ensemble_plan")
    return th, [{1: "lds", 0: "direct"}.get(s) for s in staged]


def seg_eval_ensemble(views, gt=None, flips=None, weights=None, size=None, n_classes=None, hist=None, ignore_index=250,
                      want_loss=True, want_ids=False):
    """Test-time ensembling scored at label resolution in one launch.  views: a list of 1..16 logit tensors [B,C,h_k,w_k] of the same
    images (NCHW-logical; dense, channels-last or a slice: read in place through their strides; half precision is converted like
    ``seg_eval`` converts it); flips[k]: view k is the network's output for the horizontally mirrored image and is mirrored back;
    weights[k] >= 0 (default all 1).  gt int64 [B,Ht,Wt] of any size -> (hist, loss_pair, ids) like ``seg_eval``: per label pixel
    every view is interpolated bilinearly (align_corners=True) to the label grid, turned into class probabilities by a softmax
    and averaged with weights w_k / sum w; ``hist[C * gt + argmax] += 1`` (lowest index on a tie), the sum of -log(mean
    probability of the label) and the pixel count over ``gt != ignore_index`` as a float64 [2], the argmax as a uint8 plane.
    ``gt=None`` with ``size=(Ht, Wt)`` is the inference form: only the ids are computed and returned as (None, None, ids).

    Exact guarantees: two calls return the same bits; a view of weight 0 is not read and the result has the bits of the call
    without it; the weights enter only as float32(w_k / sum w) with the quotient formed in float64, so a common factor changes
    nothing when the scaled weights and their sum are exact in float64 ([2,2,2] gives the bits of [1,1,1]; an arbitrary factor
    need not).  The resized logits and the probabilities are never materialised; no host synchronisation."""
    lgs, flips, weights, B, C = _seg_ens_views(views, flips, weights)
    dev = lgs[0].device
    if gt is None:
        if size is None or len(size) != 2:
            raise ValueError("without gt the label size is needed: size=(Ht, Wt)")
        if hist is not None or n_classes is not None:
            raise ValueError("hist and n_classes need gt: the inference form (gt=None) returns only the ids")
        Ht, Wt = int(size[0]), int(size[1])
        want_loss, want_ids = False, True
    else:
        if not (torch.is_tensor(gt) and gt.dim() == 3 and gt.dtype == torch.int64):
            raise TypeError("gt must be an int64 [B,Ht,Wt] tensor")
        if size is not None and tuple(int(s) for s in size) != tuple(gt.shape[1:]):
            raise ValueError("size = %r, but gt is %s" % (size, tuple(gt.shape)))
        if gt.shape[0] != B:
            raise ValueError("the views hold %d images, gt %d" % (B, gt.shape[0]))
        if gt.device != dev:
            raise ValueError("the views are on %s, gt on %s" % (dev, gt.device))
        Ht, Wt = int(gt.shape[1]), int(gt.shape[2])
    if min(Ht, Wt) < 1:
        raise ValueError("empty label grid %d x %d" % (Ht, Wt))
    if n_classes is not None and int(n_classes) != C:
        raise ValueError("n_classes = %d, but the views have %d classes" % (n_classes, C))
    if hist is not None:
        if not (torch.is_tensor(hist) and hist.dtype == torch.int64 and hist.numel() == C * C and hist.is_contiguous()):
            raise ValueError("hist must be a contiguous int64 tensor of %d x %d elements" % (C, C))
        if hist.device != dev:
            raise ValueError("hist is on %s, the views on %s" % (hist.device, dev))
    elif n_classes is not None:
        hist = torch.zeros(C * C, dtype=torch.int64, device=dev)
    if hist is None and not want_loss and not want_ids:
        raise ValueError("nothing to compute: no hist (or n_classes), want_loss and want_ids are off")
    gt = None if gt is None else gt.detach().contiguous()
    pair = torch.empty(2, dtype=torch.float64, device=dev) if want_loss else None
    ids = torch.empty((B, Ht, Wt), dtype=torch.uint8, device=dev) if want_ids else None
    L = _lib.lib()
    nb = L.segsde_seg_ens_workspace(B, Ht, Wt) if want_loss else 0
    ws_ = _ws(nb, lgs[0]) if want_loss else None
    descs = _seg_ens_descs(lgs, flips, weights)
    nbytes = sum(4.0 * lg.numel() for lg, w in zip(lgs, weights) if w > 0) + B * Ht * Wt * (8.0 + (1.0 if want_ids else 0.0))
    _timed("hbm_seg_eval_ensemble", nbytes, lgs[0], lambda: check(L.segsde_seg_ens(
        descs, len(lgs), B, C, _p(gt), Ht, Wt, int(ignore_index), _p(hist), _p(pair), _p(ids), _p(ws_), nb, _stream(lgs[0])),
        "seg_eval_ensemble"))
    return hist, pair, ids


# ----------------------------------------------------------------------------------------------
# BerHu pseudo-depth loss (csrc/berhu.hip; loss.loss.berhu / berhu_own_car call it)
# ----------------------------------------------------------------------------------------------
BERHU_THRESHOLD = 0.2         # the reference's constant (loss.py:6)


def _berhu_operands(input, target, mask, keep_rows):
    """-> (x, t, m or None, n, H, W, keep_rows or -1): float32, broadcast to one shape, dense"""
    for name, v in (("input", input), ("target", target), ("mask", mask)):
        if v is not None and not (torch.is_tensor(v) and v.is_floating_point()):
            raise TypeError("%s must be a floating-point tensor" % name)
    ops = [input.detach().float(), target.detach().float()] + ([] if mask is None else [mask.detach().float()])
    if any(o.device != ops[0].device for o in ops):
        raise ValueError("input, target and mask are on different devices: %s" % ", ".join(str(o.device) for o in ops))
    ops = [o.contiguous() for o in torch.broadcast_tensors(*ops)]
    x = ops[0]
    if x.numel() < 1:
        raise ValueError("empty operands %s" % (tuple(x.shape),))
    Hh = W = 0
    if keep_rows is None:
        keep_rows = -1
    else:
        if x.dim() < 2:
            raise ValueError("keep_rows needs operands of at least two dimensions [.., H, W], got %s" % (tuple(x.shape),))
        Hh, W, keep_rows = int(x.shape[-2]), int(x.shape[-1]), int(keep_rows)
        if not 0 <= keep_rows <= Hh:
            raise ValueError("keep_rows = %d outside [0, %d]" % (keep_rows, Hh))
    return x, ops[1], (ops[2] if mask is not None else None), x.numel(), Hh, W, keep_rows


def berhu_forward(input, target, mask=None, keep_rows=None, apply_log=False):
    """BerHu loss of loss.py:5-15 -> (loss float32 [1], state float32 [2] = {max a, C}) on the device, a = |target - input| * mask
    (log(1 + .) of both first with ``apply_log``), C = 0.2 max a, loss = mean over every element of a where a <= C, else
    (a^2 + C^2) / (2 C).  ``keep_rows``: rows >= keep_rows of the last-but-one dimension count as masked (the own-car crop) without
    a mask tensor; it combines with ``mask``.  Operands: float32 (other float dtypes are converted), broadcast against each other
    with ``torch.broadcast_tensors``; an operand that is not dense afterwards (a broadcast mask, a slice with gaps) costs one
    contiguous copy.  No host synchronisation; max a == 0 gives loss 0 (and a zero gradient, where the reference has NaN)."""
    x, t, m, n, Hh, W, kr = _berhu_operands(input, target, mask, keep_rows)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    state = torch.empty(2, dtype=torch.float32, device=x.device)
    L = _lib.lib()
    nb = L.segsde_berhu_workspace(n)
    ws_ = _ws(nb, x)
    nbytes = 2.0 * n * (8.0 + (4.0 if m is not None else 0.0))
    _timed("hbm_berhu", nbytes, x, lambda: check(L.segsde_berhu_forward(
        _p(x), _p(t), _p(m), n, Hh, W, kr, int(bool(apply_log)), BERHU_THRESHOLD, _p(loss), _p(state), _p(ws_), nb, _stream(x)),
        "berhu_forward"), "fwd")
    return loss, state


def berhu_backward(input, target, state, gscale, mask=None, keep_rows=None, apply_log=False):
    """d loss / d input of ``berhu_forward`` (same operands, its ``state``) times the DEVICE scalar ``gscale`` (float32, one element)
    -> float32 tensor of the broadcast shape; exactly 0 at masked, cropped and target == input elements.  One launch."""
    x, t, m, n, Hh, W, kr = _berhu_operands(input, target, mask, keep_rows)
    if not (torch.is_tensor(state) and state.dtype == torch.float32 and state.numel() == 2 and state.is_contiguous()):
        raise ValueError("state must be the float32 [2] tensor berhu_forward returned")
    if not (torch.is_tensor(gscale) and gscale.numel() == 1):
        raise ValueError("gscale must be a one-element tensor")
    if state.device != x.device or gscale.device != x.device:
        raise ValueError("state / gscale are not on the operands' device %s" % x.device)
    g = _f32(gscale, "gscale").reshape(1)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    nbytes = n * (12.0 + (4.0 if m is not None else 0.0))
    _timed("hbm_berhu", nbytes, x, lambda: check(_lib.lib().segsde_berhu_backward(
        _p(x), _p(t), _p(m), n, Hh, W, kr, int(bool(apply_log)), _p(state), _p(g), _p(dx), _stream(x)), "berhu_backward"), "bwd")
    return dx
