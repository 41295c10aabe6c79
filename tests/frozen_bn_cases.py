"""Frozen BatchNorm folded into the convolutions of no-grad forward passes (functional.frozen_bn_fold, models/layers.conv_bn,
segsde_bn_fold / segsde_conv2d_forward_residual / segsde_stem7x7_forward_bias_act): shared case functions, run on the GPU
(test_frozen_bn_gpu.py) and through the CPU interpreter (test_frozen_bn_emu.py).  Every case takes the device."""
import copy
import ctypes

import torch
import torch.nn.functional as F

from kernel_cases import assert_close
from improving_segmentation_with_selfsupervised_depth_amd import _lib
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
from improving_segmentation_with_selfsupervised_depth_amd.models.model_parts import ASPPConv
from improving_segmentation_with_selfsupervised_depth_amd.models.resnet_encoder import BasicBlock, Bottleneck, ResnetEncoder

GATE = 3.0       # re-associated fp32 routes: max and rms error within 3x of the reference route's (README "Round-off")
U = 2.0 ** -24   # unit round-off of fp32


# ---------------------------------------------------------------------------------------------
# 1. the fold kernel
# ---------------------------------------------------------------------------------------------
FOLD_SHAPES = [(20, 12, 1), (64, 64, 3), (64, 4, 7), (7, 3, 3)]      # (Cout, Cin, K)


def fold_inputs(shape, device, seed, with_cb, affine=True):
    O, I, K = shape
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(O, I, K, K, generator=gen) * 0.2
    cb = torch.randn(O, generator=gen) if with_cb else None
    gamma = (torch.rand(O, generator=gen) + 0.5) if affine else None
    beta = torch.randn(O, generator=gen) * 0.3 if affine else None
    if affine:
        gamma[1] = -gamma[1]                       # a negative scale
        gamma[O - 1] = -0.25
    mean = torch.randn(O, generator=gen) * 0.5
    var = torch.rand(O, generator=gen) * 1.5 + 0.5
    var[2] = 0.0                                   # invstd = 1 / sqrt(eps)
    d = lambda t: None if t is None else t.to(device)
    return d(w), d(cb), d(gamma), d(beta), d(mean), d(var), 1e-5


def check_fold(inp, out, what):
    """w' bit-equal to fp32 w * (gamma * invstd) with invstd from bn_eval_stats; b' against float64 on the fp32 s (the bits the
    kernel multiplies with): beta - mean * s + cb * s is two products and two sums, each rounded once to fp32 relative to a value
    no larger than |beta| + |mean s| + |cb s| -- the bound 4 * 2^-24 * (|beta| + |mean s| + |cb s|) per channel"""
    w, cb, gamma, beta, mean, var, eps = inp
    wf, bf = out
    _, invstd = H.bn_eval_stats(mean, var, eps)
    s = invstd if gamma is None else gamma * invstd
    assert torch.equal(wf, w * s[:, None, None, None]), what + ": w' is not w * (gamma * invstd) bit for bit"
    s64, m64 = s.double().cpu(), mean.double().cpu()
    b64 = (0.0 if beta is None else beta.double().cpu()) - m64 * s64
    bound = (0.0 if beta is None else beta.double().cpu().abs()) + (m64 * s64).abs()
    if cb is not None:
        b64 = b64 + cb.double().cpu() * s64
        bound = bound + (cb.double().cpu() * s64).abs()
    err = (bf.double().cpu() - b64).abs()
    assert bool((err <= 4 * U * bound).all()), "%s: b' off by %.3e x the bound" % (what, float((err / (4 * U * bound)).max()))
    if (var == 0).any():
        i = int((var == 0).nonzero()[0])
        assert float(invstd[i]) == float(1.0 / torch.sqrt(torch.tensor(eps, dtype=torch.float32)))


def run_fold_kernel(device):
    allp = []
    for i, shape in enumerate(FOLD_SHAPES):
        for with_cb in (False, True):
            inp = fold_inputs(shape, device, 100 + i, with_cb)
            check_fold(inp, H.bn_fold(*inp), "fold %r cb=%s" % (shape, with_cb))
        inp = fold_inputs(shape, device, 200 + i, True, affine=False)
        check_fold(inp, H.bn_fold(*inp), "fold %r affine=False" % (shape,))
        allp.append(fold_inputs(shape, device, 300 + i, bool(i & 1), affine=i != 2))
    outs = H.bn_fold(allp)                              # the four shapes as one table, one launch
    assert len(outs) == len(allp)
    for shape, inp, out in zip(FOLD_SHAPES, allp, outs):
        check_fold(inp, out, "multi-entry fold %r" % (shape,))


# ---------------------------------------------------------------------------------------------
# 2. the residual operand of the direct epilogue
# ---------------------------------------------------------------------------------------------
def _desc(B, Hh, W, C0, Cout, k, dil, pad, ldy, act, compute=0):
    e = dil * (k - 1) + 1
    return _lib.ConvDesc(B=B, H=Hh, W=W, C0=C0, C1=0, ld0=C0, ld1=0, up0=0, Ho=Hh + 2 * pad - e + 1, Wo=W + 2 * pad - e + 1,
                         Cout=Cout, ldy=ldy, ldy2=0, nsplit=0, KH=k, KW=k, stride=1, dil=dil, pad=pad, pad_mode=0, in_div=1,
                         act=H.ACT[act], sum2x2=0, accumulate=0, compute=compute)


# (name, B, H, W, C0, Cout, k, dil, pad)
RES_FULL = ("full_1x1", 1, 16, 16, 64, 128, 1, 1, 0)          # B * H * W = 256: whole 128-row tiles, the raw-buffer path
RES_RAGGED = ("ragged", 1, 5, 7, 8, 20, 1, 1, 0)               # 35 rows of a 128-row tile, 20 of 32 columns: the general path
RES_DIL2 = ("3x3_dil2", 1, 12, 14, 32, 64, 3, 2, 2)
RES_TAIL = ("1x1_n160", 2, 8, 16, 32, 160, 1, 1, 0)            # Cout = 128 + 32: two launches with their own tile widths


def run_residual_case(device, geom, act="relu", bias=True, ld_extra=0, inplace=False, compute=0, seed=0):
    name, B, Hh, W, C0, Cout, k, dil, pad = geom
    what = "%s act=%s bias=%s ld+%d inplace=%s compute=%d" % (name, act, bias, ld_extra, inplace, compute)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hh, W, C0, generator=gen).to(device)
    w = (torch.randn(Cout, C0, k, k, generator=gen) * 0.2).to(device)
    b = torch.randn(Cout, generator=gen).to(device) if bias else None
    ld = Cout + ld_extra
    d1 = _desc(B, Hh, W, C0, Cout, k, dil, pad, ld, act, compute)
    Ho, Wo = d1.Ho, d1.Wo
    rbuf = torch.randn(B, Ho, Wo, ld, generator=gen).to(device)
    lib, wp, st = _lib.lib(), H.pack_weight(w, False), H._stream(x)
    # conv + bias through the existing entry point, then the add and the activation with torch on the device
    d0 = _desc(B, Hh, W, C0, Cout, k, dil, pad, Cout, "none", compute)
    y0 = torch.empty(B, Ho, Wo, Cout, device=device)
    H.check(lib.segsde_conv2d_forward(ctypes.byref(d0), H._p(x), None, H._p(wp), H._p(b), H._p(y0), None, st), "conv2d_forward")
    pre = y0 + rbuf[..., :Cout]
    if inplace:
        ybuf = rbuf.clone()
        res = ybuf
    else:
        ybuf = torch.full((B, Ho, Wo, ld), -7.0, device=device)
        res = rbuf
    H.check(lib.segsde_conv2d_forward_residual(ctypes.byref(d1), H._p(x), None, H._p(wp), H._p(b), H._p(res), ld, H._p(ybuf), st),
            "conv2d_forward_residual " + what)
    y = ybuf[..., :Cout]
    if ld_extra:                                     # the pad columns belong to somebody else
        assert torch.equal(ybuf[..., Cout:], rbuf[..., Cout:] if inplace else torch.full_like(ybuf[..., Cout:], -7.0)), what
    if act in ("none", "relu"):
        want = torch.relu(pre) if act == "relu" else pre
        assert torch.equal(y, want), "%s: max |diff| %.3e" % (what, float((y - want).abs().max()))
        return
    xr = x.double().cpu().permute(0, 3, 1, 2)
    ref = F.conv2d(xr, w.double().cpu(), None if b is None else b.double().cpu(), 1, pad, dil).permute(0, 2, 3, 1)
    ref = ref + rbuf[..., :Cout].double().cpu()
    ref = F.elu(ref) if act == "elu" else torch.sigmoid(ref)
    assert_close(y, ref, what=what)                  # the tolerance of kernel_cases.run_conv_case's activation cases


def run_residual_epilogue(device):
    for geom in (RES_FULL, RES_RAGGED):
        for act in ("none", "relu"):
            for bias in (False, True):
                run_residual_case(device, geom, act, bias)
        run_residual_case(device, geom, "relu", True, ld_extra=4)
        run_residual_case(device, geom, "relu", True, inplace=True)
        run_residual_case(device, geom, "none", False, ld_extra=4, inplace=True)
        run_residual_case(device, geom, "elu", True)
        run_residual_case(device, geom, "sigmoid", True, inplace=True)
    run_residual_case(device, RES_DIL2, "relu", True)
    run_residual_case(device, RES_DIL2, "none", False, inplace=True)
    run_residual_case(device, RES_TAIL, "relu", True, inplace=True)
    run_residual_case(device, RES_FULL, "relu", True, compute=2)
    run_residual_case(device, RES_DIL2, "relu", False, compute=2, inplace=True)
    # the split-bf16 launches above did take the split loop
    d = _desc(1, 16, 16, 64, 128, 1, 1, 0, 128, "relu", 2)
    assert _lib.lib().segsde_conv_compute_taken(ctypes.byref(d), 0) == 2


def run_residual_validation(cdll):
    """answers given before any launch (fake pointers): safe without a GPU"""
    f = lambda a: ctypes.c_void_p(a)
    x, w, y, r = f(1 << 20), f(2 << 20), f(3 << 20), f(4 << 20)
    base = dict(B=1, H=8, W=8, C0=32, C1=0, ld0=32, Ho=8, Wo=8, Cout=32, ldy=32, KH=1, KW=1, stride=1, dil=1, pad=0, in_div=1)
    call = lambda d, res, ldr, yy: cdll.segsde_conv2d_forward_residual(ctypes.byref(d), x, None, w, None, res, ldr, yy, None)
    assert call(_lib.ConvDesc(), r, 32, y) == -2                                        # empty descriptor
    assert call(_lib.ConvDesc(**base), None, 32, y) == -1                               # no residual
    assert call(_lib.ConvDesc(**base), r, 16, y) == -2                                  # pitch below Cout
    # overlap: one element short of disjoint, the same base with another pitch, a shifted alias
    n = 64 * 32 * 4
    assert call(_lib.ConvDesc(**base), f((3 << 20) + n - 4), 32, y) == -2
    assert call(_lib.ConvDesc(**dict(base, ldy=36)), y, 32, y) == -2
    assert call(_lib.ConvDesc(**base), f((3 << 20) + 16), 32, y) == -2
    for k, v in (("sum2x2", 1), ("in_div", 2), ("accumulate", 1), ("nsplit", 16), ("ldy2", 32), ("pad_mode", 2)):
        dd = dict(base, **{k: v})
        if k == "pad_mode":
            dd.update(KH=3, KW=3, pad=1)
        assert call(_lib.ConvDesc(**dd), r, dd["ldy"], y) == -4, k
    assert call(_lib.ConvDesc(**dict(base, Cout=1, ldy=4)), r, 4, y) == -4               # Cout == 1
    assert call(_lib.ConvDesc(**dict(base, Cout=30, ldy=32)), r, 32, y) == -4            # no 16-byte epilogue: Cout % 4
    assert call(_lib.ConvDesc(**dict(base, ldy=34)), r, 36, y) == -4                     # ... pitch % 4
    assert call(_lib.ConvDesc(**base), r, 34, y) == -4                                   # ... residual pitch % 4
    assert call(_lib.ConvDesc(**base), f((4 << 20) + 4), 32, y) == -4                    # ... residual not 16-byte aligned
    assert call(_lib.ConvDesc(**dict(base, compute=3)), r, 32, y) == -4
    assert cdll.segsde_stem7x7_forward_bias_act(None, 1, 38, 72, 4, w, 64, None, 1, y, None) == -1
    assert cdll.segsde_stem7x7_forward_bias_act(x, 1, 38, 72, 4, w, 64, None, 7, y, None) == -2
    assert cdll.segsde_bn_fold(None, 1, 1, None) == -1 and cdll.segsde_bn_fold(x, 0, 1, None) == -2


# ---------------------------------------------------------------------------------------------
# 3. the stem with bias and activation
# ---------------------------------------------------------------------------------------------
def run_stem_bias_act(device):
    gen = torch.Generator().manual_seed(5)
    img = torch.rand(2, 3, 32, 64, generator=gen).to(device)
    w = (torch.randn(64, 3, 7, 7, generator=gen) * 0.1).to(device)
    b = torch.randn(64, generator=gen).to(device)
    xpad, ws = H.stem_input(img, 0.45, 0.225), H.stem_pack(w)
    y0 = H.stem_forward(xpad, ws, 3)
    assert torch.equal(H.stem_forward(xpad, ws, 3, bias=b, act="relu"), torch.relu(y0 + b))
    assert torch.equal(H.stem_forward(xpad, ws, 3, bias=b), y0 + b)


# ---------------------------------------------------------------------------------------------
# 4. blocks and encoders against float64
# ---------------------------------------------------------------------------------------------
def randomize(module, seed):
    """running statistics away from (0, 1), gamma away from 1 (some negative), beta away from 0"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.running_mean.copy_(torch.randn(C, generator=gen) * 0.5)
                m.running_var.copy_(torch.rand(C, generator=gen) * 1.5 + 0.5)
                m.weight.copy_((torch.rand(C, generator=gen) + 0.5) * torch.where(torch.rand(C, generator=gen) < 0.1, -1.0, 1.0))
                m.bias.copy_(torch.randn(C, generator=gen) * 0.3)
    return module


def _cv(conv, x):
    return F.conv2d(x, conv.weight.detach().double().cpu(), None if conv.bias is None else conv.bias.detach().double().cpu(),
                    conv.stride, conv.padding, conv.dilation)


def _bn(bn, x):
    t = lambda v: v.detach().double().cpu()
    return F.batch_norm(x, t(bn.running_mean), t(bn.running_var), t(bn.weight), t(bn.bias), False, 0.0, bn.eps)


def ref_block(blk, x):
    """float64, NCHW, eval mode, from the module's own parameters"""
    if isinstance(blk, ASPPConv):
        return F.relu(_bn(blk[1], _cv(blk[0], x)))
    idt = x if blk.downsample is None else _bn(blk.downsample[1], _cv(blk.downsample[0], x))
    o = F.relu(_bn(blk.bn1, _cv(blk.conv1, x)))
    if isinstance(blk, Bottleneck):
        o = F.relu(_bn(blk.bn2, _cv(blk.conv2, o)))
        return F.relu(_bn(blk.bn3, _cv(blk.conv3, o)) + idt)
    return F.relu(_bn(blk.bn2, _cv(blk.conv2, o)) + idt)


def ref_encoder(enc, img):
    e = enc.encoder
    x = F.relu(_bn(e.bn1, _cv(e.conv1, (img.double().cpu() - 0.45) / 0.225)))
    feats = [x]
    x = F.max_pool2d(x, 3, 2, 1)
    for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
        for blk in layer:
            x = ref_block(blk, x)
        feats.append(x)
    return feats


def _down(cin, cout, stride):
    return torch.nn.Sequential(L.Conv2d(cin, cout, 1, stride, bias=False), L.BatchNorm2d(cout))


# name -> (constructor, input channels, (B, H, W), Winograd size floor removed)
BLOCKS = {
    "bottleneck": (lambda: Bottleneck(64, 16), 64, (2, 10, 14), False),
    "bottleneck_downsample": (lambda: Bottleneck(32, 16, downsample=_down(32, 64, 1)), 32, (2, 10, 14), False),
    "bottleneck_stride2": (lambda: Bottleneck(32, 16, stride=2, downsample=_down(32, 64, 2)), 32, (2, 11, 14), False),
    "bottleneck_dilation2": (lambda: Bottleneck(64, 16, dilation=2), 64, (2, 10, 14), False),
    "basicblock": (lambda: BasicBlock(32, 32), 32, (2, 10, 14), False),
    "asppconv": (lambda: ASPPConv(32, 16, 3), 32, (2, 10, 14), False),
    # 64-channel 3x3 convolutions on the one-kernel Winograd route (bias + ReLU folded there), as at real sizes
    "bottleneck_winograd": (lambda: Bottleneck(256, 64), 256, (1, 8, 16), True),
    "basicblock_winograd": (lambda: BasicBlock(64, 64), 64, (1, 8, 16), True),
}


def errors(got, ref):
    e = got.detach().double().cpu() - ref
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


def gate(on, off, ref, what, report=None):
    """max and rms error of the folded output within GATE x the unfused output's, both against float64"""
    (m1, r1), (m0, r0) = errors(on, ref), errors(off, ref)
    line = "%-28s max %.3e / %.3e = %.2f   rms %.3e / %.3e = %.2f" % (what, m1, m0, m1 / m0, r1, r0, r1 / r0)
    print(line)
    if report is not None:
        report.append((what, m1, m0, r1, r0))
    assert m0 > 0 and r0 > 0, what
    assert m1 <= GATE * m0 and r1 <= GATE * r0, line


def forward_nograd(module, x, on):
    with torch.no_grad(), Fn.frozen_bn_fold(on):
        return module(x)


def run_block(device, name, report=None):
    make, cin, (B, Hh, W), nofloor = BLOCKS[name]
    torch.manual_seed(17)
    blk = randomize(make(), 31).to(device).eval()
    x = torch.randn(B, Hh, W, cin, generator=torch.Generator().manual_seed(3)).to(device)
    old = H.WINOGRAD_MIN_MACS
    if nofloor:
        H.WINOGRAD_MIN_MACS = 0.0
    try:
        off = forward_nograd(blk, x, False)
        Fn.fusion_report(reset=True)
        n0 = H.WINO_FUSED_TAKEN["fwd"]
        on = forward_nograd(blk, x, True)
        rep = Fn.fusion_report(reset=True)["frozen_bn_folded"]
        wino = H.WINO_FUSED_TAKEN["fwd"] - n0
    finally:
        H.WINOGRAD_MIN_MACS = old
    pairs = sum(isinstance(m, torch.nn.BatchNorm2d) for m in blk.modules())
    unfused = 1 if isinstance(blk, BasicBlock) else 0      # conv2 + bn2 + residual: the Winograd geometry takes no residual
    assert rep == {"taken": pairs - unfused, "missed": unfused}, (name, rep)
    if nofloor:     # the folded 3x3 went through the one-kernel Winograd route (and so did BasicBlock's unfused conv2)
        assert wino == 1 + unfused, (name, wino)
    ref = ref_block(blk, x.double().cpu().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    gate(on, off, ref, name, report)
    return blk, x, on, off, ref


def make_encoder(num_layers, device, seed=7):
    torch.manual_seed(seed)
    kw = {"replace_stride_with_dilation": [False, False, True]} if num_layers == 50 else {}
    return randomize(ResnetEncoder(num_layers, False, **kw), seed + 1).to(device).eval()


ENCODER_PAIRS = {18: (20, 8), 50: (53, 0)}      # (conv -> BatchNorm pairs, of them BasicBlock conv2 / bn2 / residual)


def run_encoder(device, num_layers, size=(2, 3, 64, 128), report=None):
    enc = make_encoder(num_layers, device)
    img = torch.rand(*size, generator=torch.Generator().manual_seed(9)).to(device)
    Fn.fusion_report(reset=True)
    with torch.no_grad():
        off = enc.forward_nhwc(img)
        assert "frozen_bn_folded" not in Fn.fusion_report(reset=True)
        with Fn.frozen_bn_fold():
            on = enc.forward_nhwc(img)
    rep = Fn.fusion_report(reset=True)["frozen_bn_folded"]
    pairs, residual3x3 = ENCODER_PAIRS[num_layers]
    # 7. coverage: every pair folded, the stem included; ResNet-18 keeps conv2 / bn2 / residual of each BasicBlock unfused
    assert rep == {"taken": pairs - residual3x3, "missed": residual3x3}, rep
    refs = ref_encoder(enc, img)
    for i, (a, b, r) in enumerate(zip(on, off, refs)):
        gate(a, b, r.permute(0, 2, 3, 1), "resnet%d feature %d" % (num_layers, i), report)


# ---------------------------------------------------------------------------------------------
# 5. the switch does nothing where it must not
# ---------------------------------------------------------------------------------------------
def run_switch_is_inert(device):
    make, cin, (B, Hh, W), _ = BLOCKS["bottleneck_downsample"]
    torch.manual_seed(17)
    proto = randomize(make(), 41).to(device)
    x = torch.randn(B, Hh, W, cin, generator=torch.Generator().manual_seed(4)).to(device)
    Fn.fusion_report(reset=True)

    # BatchNorm in train mode, no gradients: batch statistics, running statistics updated identically
    outs = []
    for on in (False, True):
        blk = copy.deepcopy(proto).train()
        outs.append((forward_nograd(blk, x, on), {k: v.clone() for k, v in blk.state_dict().items()}))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(outs[0][1][k], outs[1][1][k]) for k in outs[0][1])

    # eval mode with gradients enabled: same outputs, same gradients
    grads = []
    for on in (False, True):
        blk = copy.deepcopy(proto).eval()
        xx = x.clone().requires_grad_(True)
        with Fn.frozen_bn_fold(on):
            y = blk(xx)
            (y * y).sum().backward()
        grads.append((y.detach(), xx.grad) + tuple(p.grad for p in blk.parameters()))
    assert len(grads[0]) == len(grads[1]) and all(torch.equal(a, b) for a, b in zip(*grads))

    # dropout requested behind an eval-mode BatchNorm (ASPP.project): the mask comes from the host generator's seed
    conv, bn = L.Conv2d(cin, 16, 1, bias=False).to(device), randomize(L.BatchNorm2d(16), 43).to(device).eval()
    ys = []
    for on in (False, True):
        torch.manual_seed(123)
        with torch.no_grad(), Fn.frozen_bn_fold(on):
            ys.append(L.conv_bn(conv, bn, x, act="relu", drop_p=0.5))
    assert torch.equal(ys[0], ys[1]) and bool((ys[0] == 0).any())
    rep = Fn.fusion_report(reset=True)
    assert rep["frozen_bn_folded"]["taken"] == 0 and rep["frozen_bn_folded"]["missed"] > 0, rep

    # switch off: nothing is counted, nothing is cached
    blk = copy.deepcopy(proto).eval()
    forward_nograd(blk, x, False)
    assert "frozen_bn_folded" not in Fn.fusion_report()
    assert all(not m._bn_fold for m in blk.modules() if isinstance(m, L.Conv2d))
    assert Fn.FROZEN_BN_FOLD[0] is False, "the switch must be off by default"


# ---------------------------------------------------------------------------------------------
# 6. the cache
# ---------------------------------------------------------------------------------------------
def run_cache(device, monkeypatch):
    make, cin, (B, Hh, W), _ = BLOCKS["bottleneck"]
    torch.manual_seed(17)
    blk = randomize(make(), 51).to(device).eval()
    x = torch.randn(B, Hh, W, cin, generator=torch.Generator().manual_seed(6)).to(device)
    calls = []
    real = H.bn_fold
    monkeypatch.setattr(H, "bn_fold", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    first = forward_nograd(blk, x, True)
    assert len(calls) == 3                                   # conv1 / conv2 / conv3, folded once each
    again = forward_nograd(blk, x, True)
    assert len(calls) == 3 and torch.equal(first, again)     # nothing changed: no launch, the cached tensors
    xr = x.double().cpu().permute(0, 3, 1, 2)

    def edited(what, n_refold):
        off = forward_nograd(blk, x, False)                      # the switch-off pass of the edited module
        n = len(calls)
        on = forward_nograd(blk, x, True)
        assert len(calls) == n + n_refold, (what, len(calls) - n)
        gate(on, off, ref_block(blk, xr).permute(0, 2, 3, 1), "cache: " + what)
        return on

    prev = first
    with torch.no_grad():
        blk.bn1.running_mean.add_(0.3)
    cur = edited("running_mean edited in place", 1)
    assert not torch.equal(cur, prev)
    prev = cur
    with torch.no_grad():
        blk.bn2.weight.mul_(1.5)
    cur = edited("gamma edited in place", 1)
    assert not torch.equal(cur, prev)
    prev = cur
    with torch.no_grad():
        blk.conv3.weight.mul_(0.7)
    cur = edited("weight edited in place", 1)
    assert not torch.equal(cur, prev)
    prev = cur
    sd = {k: (v * 1.25 if k.endswith("running_var") or k.endswith("conv1.weight") else v.clone()) for k, v in blk.state_dict().items()}
    blk.load_state_dict(sd)
    cur = edited("load_state_dict", 3)
    assert not torch.equal(cur, prev)
    assert len(calls) == 9 and torch.equal(forward_nograd(blk, x, True), cur) and len(calls) == 9
