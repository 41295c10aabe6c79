"""The packed 1-bit ReLU mask of the residual BatchNorms (segsde_bn_apply_mask / segsde_bn_backward_mask) against the saved-output
mode of segsde_bn_apply / segsde_bn_backward on the same inputs: shared by tests/test_bn_bitmask_gpu.py (real library) and
tests/test_bn_bitmask_emu.py (interpreter build of the same sources).  Everything is compared bit for bit: the mask mode changes
where the ReLU derivative is read from, not one operation of the arithmetic."""
import ctypes

import numpy as np
import torch

from improving_segmentation_with_selfsupervised_depth_amd import _lib
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

RELU = H.ACT["relu"]
# (M, C, pitch): the smallest shapes at which the word packing can go wrong
SHAPES = [(1, 4, 4),          # one quad, one partial word
          (7, 4, 4),          # 28 bits: a tail word
          (3, 8, 12),         # pitch > C: the bit index follows the logical [M][C] index
          (5, 12, 12),        # 60 bits: a tail word behind a full one, C / 4 no power of two
          (33, 20, 20),       # C / 4 = 5: the division path (cv_shift < 0), 660 bits
          (257, 64, 64),      # several blocks, words across block boundaries, per-thread channel parameters (fixed_c)
          (1030, 256, 256)]   # several reduction blocks
EMU_SHAPES = [(3, 8, 12), (33, 20, 20), (5, 12, 12)]
GUARD = 0x5A5A5A5A


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _bits(t):
    """fp32 tensor as its bit patterns (NaN == NaN, -0 != +0: stricter than torch.equal)"""
    return t.contiguous().view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), "%s differs (%d of %d elements)" % (
        what, int((_bits(a) != _bits(b)).sum()), a.numel())


def _pitched(M, C, pitch, device, fill=None):
    buf = torch.randn(M, pitch, device=device) if fill is None else torch.full((M, pitch), fill, device=device)
    return buf, buf[:, :C]


def make_inputs(M, C, pitch, device, seed=0):
    """x, residual, dy at the given pitch; gamma with negative entries; a few exact y == 0 (residual = -BN(x) as the kernel itself
    computes it), one NaN in dy on such an element (the derivative is 0 there: dy * 0 must stay NaN as in the saved-y mode)"""
    torch.manual_seed(1000 * M + C + seed)
    L = _lib.lib()
    st = H._stream(torch.empty(1, device=device))
    _, x = _pitched(M, C, pitch, device)
    _, res = _pitched(M, C, pitch, device)
    _, dy = _pitched(M, C, pitch, device)
    gamma = torch.randn(C, device=device)
    gamma[::3] = -gamma[::3].abs() - 0.1
    beta = torch.randn(C, device=device)
    mean, invstd = x.mean(0).contiguous(), (1.0 / (x.var(0, unbiased=False) + 1e-2).sqrt()).contiguous()
    z = torch.empty(M, C, device=device)      # BN(x) exactly as bn_apply_kernel forms it
    _lib.check(L.segsde_bn_apply(_p(x), pitch, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), None, 0, _p(z), C, 0, 0.0, 0, st),
               "bn_apply")
    n = M * C
    planted = sorted({0, n // 3, n - 1, (5 * n) // 7})
    for i in planted:
        res[i // C, i % C] = -z[i // C, i % C]
    dy[planted[-1] // C, planted[-1] % C] = float("nan")
    return dict(M=M, C=C, pitch=pitch, x=x, res=res, dy=dy, gamma=gamma, beta=beta, mean=mean, invstd=invstd, planted=planted, st=st)


def host_mask(y):
    """(y > 0) of the logical [M][C] tensor packed in index order: bit i % 32 of word i / 32, zeros past the end"""
    b = (y.detach().cpu().numpy().reshape(-1) > 0).astype(np.uint8)
    b = np.concatenate([b, np.zeros((-len(b)) % 32, np.uint8)])
    return np.packbits(b, bitorder="little").view("<u4")


def forward_pair(d):
    """-> (y of segsde_bn_apply, y of segsde_bn_apply_mask, mask words); checks the mask against the host packing"""
    L = _lib.lib()
    M, C, pitch, dev = d["M"], d["C"], d["pitch"], d["x"].device
    _, y0 = _pitched(M, C, pitch, dev, fill=7.0)
    _, y1 = _pitched(M, C, pitch, dev, fill=7.0)
    nw = L.segsde_bn_mask_words(M, C)
    assert nw == (M * C + 31) // 32
    mask = torch.full((nw + 1,), GUARD, dtype=torch.int32, device=dev)      # garbage in, one guard word behind
    args = (_p(d["x"]), pitch, M, C, _p(d["mean"]), _p(d["invstd"]), _p(d["gamma"]), _p(d["beta"]), _p(d["res"]), pitch)
    _lib.check(L.segsde_bn_apply(*args, _p(y0), pitch, RELU, 0.0, 0, d["st"]), "bn_apply")
    _lib.check(L.segsde_bn_apply_mask(*args, _p(y1), pitch, RELU, 0.0, 0, _p(mask), d["st"]), "bn_apply_mask")
    same_bits(y1, y0, "y")
    for i in d["planted"]:
        assert float(y0[i // C, i % C]) == 0.0, "planted zero %d is %r" % (i, float(y0[i // C, i % C]))
    got = mask.cpu().numpy().view("<u4")
    assert got[nw] == GUARD, "wrote behind segsde_bn_mask_words"
    want = host_mask(y0)
    assert np.array_equal(got[:nw], want), "mask words differ at %s" % (np.nonzero(got[:nw] != want)[0][:8],)
    return y0, mask[:nw]


def backward_pair(d, y, mask, batch_stats, need_dx, need_dres):
    L = _lib.lib()
    M, C, pitch, dev = d["M"], d["C"], d["pitch"], d["x"].device
    nb = L.segsde_bn_backward_workspace(M, C)
    out = []
    for use_mask in (False, True):
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        dg, db = torch.full((C,), 3.0, device=dev), torch.full((C,), 3.0, device=dev)
        dx = _pitched(M, C, pitch, dev, fill=3.0)[1] if need_dx else None
        dr = _pitched(M, C, pitch, dev, fill=3.0)[1] if need_dres else None
        tail = (int(batch_stats), _p(dg), _p(db), _p(dx), pitch, _p(dr), pitch, _p(ws), nb, d["st"])
        if use_mask:
            rc = L.segsde_bn_backward_mask(_p(d["dy"]), pitch, _p(mask), _p(d["x"]), pitch, M, C, _p(d["mean"]), _p(d["invstd"]),
                                           _p(d["gamma"]), RELU, 0.0, *tail)
        else:
            rc = L.segsde_bn_backward(_p(d["dy"]), pitch, _p(y), pitch, _p(d["x"]), pitch, M, C, _p(d["mean"]), _p(d["invstd"]),
                                      _p(d["gamma"]), None, RELU, 0.0, 0, *tail)
        _lib.check(rc, "bn_backward%s" % ("_mask" if use_mask else ""))
        out.append((dx, dr, dg, db))
    for name, a, b in zip(("dx", "dres", "dgamma", "dbeta"), out[0], out[1]):
        assert (a is None) == (b is None)
        if a is not None:
            same_bits(b, a, "%s (batch_stats=%d need_dx=%d need_dres=%d)" % (name, batch_stats, need_dx, need_dres))
    return out[0]


def run_shape(device, M, C, pitch):
    d = make_inputs(M, C, pitch, device)
    y, mask = forward_pair(d)
    for batch_stats in (True, False):
        for need_dx, need_dres in ((True, True), (False, True), (True, False)):
            dx, dres, dg, db = backward_pair(d, y, mask, batch_stats, need_dx, need_dres)
    # the NaN of dy sits on an element whose derivative is 0: the reference mode hands it on (dy * 0), and so did the mask mode
    i = d["planted"][-1]
    assert bool(torch.isnan(db[i % C]))


def run_unsupported(device):
    """no channel quads: the mask entry points refuse, the Python route runs the saved-output path and counts it as missed"""
    L = _lib.lib()
    for C in (3, 6):
        M = 9
        torch.manual_seed(C)
        x, res, dy = (torch.randn(M, C, device=device) for _ in range(3))
        mean, invstd = x.mean(0).contiguous(), (1.0 / (x.var(0, unbiased=False) + 1e-5).sqrt()).contiguous()
        gamma, beta = torch.randn(C, device=device), torch.randn(C, device=device)
        y = torch.empty(M, C, device=device)
        mask = torch.zeros(L.segsde_bn_mask_words(M, C), dtype=torch.int32, device=device)
        st = H._stream(x)
        assert L.segsde_bn_apply_mask(_p(x), C, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(res), C, _p(y), C, RELU, 0.0, 0,
                                      _p(mask), st) == -4
        nb = L.segsde_bn_backward_workspace(M, C)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=device)
        dg, db, dx = torch.empty(C, device=device), torch.empty(C, device=device), torch.empty(M, C, device=device)
        assert L.segsde_bn_backward_mask(_p(dy), C, _p(mask), _p(x), C, M, C, _p(mean), _p(invstd), _p(gamma), RELU, 0.0, 1, _p(dg),
                                         _p(db), _p(dx), C, None, C, _p(ws), nb, st) == -4
        # Python level
        grads = []
        for on in (True, False):
            xs = [t.reshape(1, 3, 3, C).clone().requires_grad_(True) for t in (x, res)]
            g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            Fn.fusion_report(reset=True)
            old, Fn.BN_BITMASK = Fn.BN_BITMASK, on
            try:
                out = Fn.BNActFn.apply(xs[0], g, b, xs[1], None, None, True, 0.1, 1e-5, "relu", 0.0, 0)
                out.backward(dy.reshape(1, 3, 3, C))
            finally:
                Fn.BN_BITMASK = old
            rep = Fn.fusion_report(reset=True).get("bn_backward_bitmask")
            assert rep == ({"taken": 0, "missed": 1} if on else None), rep
            grads.append([out.detach(), xs[0].grad, xs[1].grad, g.grad, b.grad])
        for a, b in zip(*grads):
            same_bits(a, b, "C=%d fallback" % C)
    # a mask entry point without ReLU, or with dropout, refuses as well
    M, C = 8, 8
    x = torch.randn(M, C, device=device)
    v = torch.ones(C, device=device)
    mask = torch.zeros(2, dtype=torch.int32, device=device)
    ws = torch.empty(max(L.segsde_bn_backward_workspace(M, C), 16), dtype=torch.uint8, device=device)
    o = torch.empty(M, C, device=device)
    for act, drop in ((H.ACT["elu"], 0.0), (RELU, 0.5)):
        assert L.segsde_bn_backward_mask(_p(x), C, _p(mask), _p(x), C, M, C, _p(v), _p(v), _p(v), act, drop, 1, _p(v.clone()),
                                         _p(v.clone()), _p(o), C, None, C, _p(ws), ws.numel(), H._stream(x)) == -4
    assert L.segsde_bn_apply_mask(_p(x), C, M, C, _p(v), _p(v), None, None, None, 0, _p(o), C, RELU, 0.5, 1, _p(mask),
                                  H._stream(x)) == -4


def run_bottleneck(device):
    """two bottleneck blocks (identity skip; strided with a downsample branch), forward + backward through BNActFn with the route
    on and forced off: outputs, input and parameter gradients bit-identical, the route counted once per residual BatchNorm"""
    from torch import nn
    from improving_segmentation_with_selfsupervised_depth_amd.models.layers import BatchNorm2d, Conv2d
    from improving_segmentation_with_selfsupervised_depth_amd.models.resnet_encoder import Bottleneck
    torch.manual_seed(3)
    down = nn.Sequential(Conv2d(32, 64, 1, 2, bias=False), BatchNorm2d(64))
    net = nn.Sequential(Bottleneck(32, 8), Bottleneck(32, 16, stride=2, downsample=down)).to(device).train()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn_like(p))          # gammas of both signs
    x0 = torch.randn(2, 6, 10, 32, device=device)
    gy = torch.randn(2, 3, 5, 64, device=device)
    runs = []
    for on in (True, False):
        net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        Fn.fusion_report(reset=True)
        old, Fn.BN_BITMASK = Fn.BN_BITMASK, on
        try:
            y = net(x)
            y.backward(gy)
        finally:
            Fn.BN_BITMASK = old
        rep = Fn.fusion_report(reset=True).get("bn_backward_bitmask")
        assert rep == ({"taken": 2, "missed": 0} if on else None), rep
        runs.append(dict([("y", y.detach()), ("dx", x.grad)] + [(k, p.grad) for k, p in net.named_parameters()]))
    assert all(v is not None for v in runs[0].values())
    for k in runs[0]:
        same_bits(runs[0][k], runs[1][k], k)
