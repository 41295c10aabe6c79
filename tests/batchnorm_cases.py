"""The BatchNorm kernels of csrc/elementwise.hip (segsde_bn_stats / segsde_bn_eval_stats, segsde_bn_apply, segsde_bn_backward in its
saved-output and remask modes, the mask entry points) against plain torch in float64 on the CPU, stage by stage, at the shapes,
pitches and values that dense random tensors of one block do not reach: ragged and capped reductions, every launch shape of
colreduce_kernel, the shift / division / fixed_c index paths, scalar kernels chosen by a pitch or a pointer, a pitch per operand,
dropout, ELU / sigmoid next to a residual, offset and degenerate statistics, a second trip of the grid-stride loops.  Shared by
tests/test_batchnorm_gpu.py (real library) and tests/test_batchnorm_emu.py (interpreter build of the same sources).

The stored fp32 ``mean`` / ``invstd`` and the ``y`` handed to the backward kernels are inputs of those operations: the references
read the very fp32 values (widened), they do not recompute them.  The float32 oracle is the same formulas in float32 torch on the
CPU from the same inputs, sums by ``tensor.sum(0)``.  No tolerance is a constant: every compared quantity gives, per channel,

    ratio = e_kernel / max(e_fp32, 2^-23 * scale)          (both errors against float64)

and a test fails when the worst channel's ratio exceeds K.  ``scale``: [M, C] tensors (y, dx, dres): ``max_m |f64[:, c]|``;
dbeta: ``sum_m |dz|``; dgamma: ``sum_m |dz * xhat|``; mean: ``sum_m |x| / M``; invstd and the running buffers: the value's own
magnitude.  Remask and mask modes are compared bit for bit with the saved-output mode, never with float64.  Nothing is left out of
any comparison.  K and the figures it comes from are in profiles/batchnorm_edges.md.

``M == 1``: torch refuses a single value per channel in training mode; the kernel keeps the biased variance (0) in the running
update (``M > 1 ? var * M / (M - 1) : var``), and so does the reference here."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import bn_bitmask_cases as BM
from oracle import dropout as OD
from improving_segmentation_with_selfsupervised_depth_amd import _lib
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

EPS23 = 2.0 ** -23
# smallest power of two that is at least twice the worst ratio of the MI355X run (profiles/batchnorm_edges.md); 8 at the most
K = 4.0
BN_EPS = float(np.float32(1e-5))          # the fp32 values the kernels receive, widened
MOM = float(np.float32(0.1))
P_DROP = float(np.float32(0.3))
SEED = 0x1234567
GUARD = 77.0
ACTS = ("none", "relu", "elu", "sigmoid")

RECORDS = []            # (group, case, tensor, channel, e_kernel, unit, ratio, ok)


def record(group, case, tensor, e_k, unit):
    """e_k, unit: one figure per channel; the worst channel is recorded"""
    e_k, unit = e_k.double().reshape(-1), unit.double().reshape(-1)
    ratio = torch.where(e_k == 0, torch.zeros_like(e_k), e_k / unit)
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    c = int(ratio.argmax())
    r = float(ratio[c])
    ok = r <= K
    RECORDS.append((group, case, tensor, c, float(e_k[c]), float(unit[c]), r, ok))
    print("BN-EDGE | %s | %s | %s | ch %d | %.3e | %.3e | %.2f | %s" % (group, case, tensor, c, float(e_k[c]), float(unit[c]), r,
                                                                      "ok" if ok else "MISSES THE RULE"))
    return ok


def finish(first):
    rows = RECORDS[first:]
    worst = {}
    for g, _, t, _, _, _, r, _ in rows:
        worst[(g, t)] = max(worst.get((g, t), 0.0), r)
    for (g, t), r in sorted(worst.items()):
        print("BN-EDGE-WORST | %s | %s | %.2f" % (g, t, r))
    bad = [r for r in rows if not r[-1]]
    assert not bad, "error against float64 above K = %g times the fp32 reference's: %s" % (K, bad)


def rec_cols(group, case, tensor, got, r64, r32):
    """an [M, C] tensor, per column"""
    got = got.double()
    record(group, case, tensor, (got - r64).abs().amax(0),
           torch.maximum((r32.double() - r64).abs().amax(0), EPS23 * r64.abs().amax(0)))


def rec_vec(group, case, tensor, got, r64, r32, scale):
    """a per-channel quantity with its scale"""
    record(group, case, tensor, (got.double() - r64).abs(), torch.maximum((r32.double() - r64).abs(), EPS23 * scale.double()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------------------------ operands
def spec(M, C, pitch=None, off=0):
    return (M, C, pitch or C, off)


def spec_name(s):
    M, C, ld, off = s
    return "M%d C%d" % (M, C) + ("" if ld == C else " pitch %d" % ld) + (" off %d" % off if off else "")


class Opd:
    """an [M, C] operand: columns off .. off + C of a guard-filled [M, ld] buffer on ``device``"""

    def __init__(self, M, C, ld, off, device, value=None):
        assert off + C <= ld
        buf = torch.full((M, ld), GUARD, dtype=torch.float32)
        if value is not None:
            buf[:, off:off + C] = value
        self.buf = buf.to(device)
        self.v = self.buf[:, off:off + C]
        self.M, self.C, self.ld, self.off = M, C, ld, off
        self.slack = torch.ones(ld, dtype=torch.bool)
        self.slack[off:off + C] = False
        assert (self.v.data_ptr() % 16 == 0) == (off % 4 == 0)
        self.before = self.buf.clone() if value is not None else None

    def cpu(self):
        return self.v.detach().cpu().contiguous()

    def check(self, what):
        if self.before is not None:
            assert torch.equal(self.buf, self.before), "%s: an input changed" % what
        elif bool(self.slack.any()):
            assert bool((self.buf.cpu()[:, self.slack] == GUARD).all()), "%s: slack columns of an output were written" % what


def k_stats(xo, rm=None, rv=None, nbt=None):
    L = _lib.lib()
    mean = torch.full((xo.C,), GUARD, dtype=torch.float32).to(xo.v.device)
    invstd = mean.clone()
    nb = L.segsde_bn_stats_workspace(xo.M, xo.C)
    ws = H._ws(nb, xo.v)
    _lib.check(L.segsde_bn_stats(_p(xo.v), xo.ld, xo.M, xo.C, _p(mean), _p(invstd), _p(rm), _p(rv), MOM, BN_EPS, _p(nbt), _p(ws), nb,
                                 H._stream(xo.v)), "bn_stats")
    return mean, invstd


def k_apply(xo, mean, invstd, gamma, beta, ro, yo, act, p=0.0, seed=0):
    _lib.check(_lib.lib().segsde_bn_apply(_p(xo.v), xo.ld, xo.M, xo.C, _p(mean), _p(invstd), _p(gamma), _p(beta),
                                          _p(None if ro is None else ro.v), 0 if ro is None else ro.ld, _p(yo.v), yo.ld, H.ACT[act],
                                          p, seed, H._stream(xo.v)), "bn_apply")


def k_backward(dyo, yo, xo, mean, invstd, gamma, beta, act, p, seed, batch_stats, dxo, dro):
    """yo None: the remask mode.  -> (dgamma, dbeta)"""
    L = _lib.lib()
    M, C, dev = xo.M, xo.C, xo.v.device
    dg, db = torch.full((C,), GUARD).to(dev), torch.full((C,), GUARD).to(dev)
    nb = L.segsde_bn_backward_workspace(M, C)
    ws = H._ws(nb, xo.v)
    _lib.check(L.segsde_bn_backward(_p(dyo.v), dyo.ld, _p(None if yo is None else yo.v), xo.ld if yo is None else yo.ld, _p(xo.v),
                                    xo.ld, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), H.ACT[act], p, seed, int(batch_stats),
                                    _p(dg), _p(db), _p(None if dxo is None else dxo.v), C if dxo is None else dxo.ld,
                                    _p(None if dro is None else dro.v), C if dro is None else dro.ld, _p(ws), nb, H._stream(xo.v)),
               "bn_backward")
    return dg, db


# ---------------------------------------------------------------------------------------------------------------- references
def act_fn(t, act):
    if act == "relu":
        return torch.where(t > 0, t, torch.zeros_like(t))
    if act == "elu":
        return F.elu(t)
    if act == "sigmoid":
        return torch.sigmoid(t)
    return t


def act_grad_from_out(y, act):
    if act == "relu":
        return (y > 0).to(y.dtype)
    if act == "elu":
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    if act == "sigmoid":
        return y * (1 - y)
    return torch.ones_like(y)


def ref_stats(dt, x, rm0, rv0):
    xx = x.to(dt)
    M = xx.shape[0]
    mu = xx.sum(0) / M
    var = ((xx - mu) ** 2).sum(0) / M
    unb = var * M / (M - 1) if M > 1 else var          # M == 1: the kernel's convention (see the module docstring)
    return dict(mean=mu, invstd=1 / torch.sqrt(var + BN_EPS), var=var, rm=(1 - MOM) * rm0.to(dt) + MOM * mu,
                rv=(1 - MOM) * rv0.to(dt) + MOM * unb)


def ref_apply(dt, x, mean, invstd, gamma, beta, res, act, keep=None, p=0.0):
    t = (x.to(dt) - mean.to(dt)) * invstd.to(dt)
    if gamma is not None:
        t = t * gamma.to(dt) + beta.to(dt)
    if res is not None:
        t = t + res.to(dt)
    t = act_fn(t, act)
    if keep is not None:
        t = torch.where(keep, t / (1 - p), torch.zeros_like(t))
    return t


def ref_backward(dt, dy, y, x, mean, invstd, gamma, act, keep=None, p=0.0):
    g, yy = dy.to(dt), y.to(dt)
    if keep is not None:
        yy = yy * (1 - p)
        g = torch.where(keep, g / (1 - p), torch.zeros_like(g))
    dz = g * act_grad_from_out(yy, act)
    if keep is not None:
        dz = torch.where(keep, dz, torch.zeros_like(dz))
    M = x.shape[0]
    xh = (x.to(dt) - mean.to(dt)) * invstd.to(dt)
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    s = invstd.to(dt) * (gamma.to(dt) if gamma is not None else 1)
    return dict(dz=dz, dbeta=dbeta, dgamma=dgamma, s_beta=dz.abs().sum(0), s_gamma=(dz * xh).abs().sum(0),
                dx1=s * (dz - dbeta / M - xh * dgamma / M), dx0=s * dz)


# -------------------------------------------------------------------------------------------------------------------- values
REGIMES = ("R0", "R1 1e2", "R1 1e3", "R2", "R3", "R5 last row", "R5 row 256")


def make_values(M, C, regime="R0", seed=0):
    """x, res, dy [M, C]; gamma (every third entry negative), beta [C]"""
    gen = _gen(100003 * seed + 7919 * (M % 9973) + C + 31 * REGIMES.index(regime))
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    mu = sign * (0.5 + 2.5 * torch.rand(C, generator=gen))
    sd = 0.5 + 1.5 * torch.rand(C, generator=gen)
    if regime.startswith("R1"):
        mu, sd = sign * 100.0, torch.full((C,), 1.0 if regime == "R1 1e2" else 0.1)
    if regime == "R2":
        sd = torch.logspace(-3, 3, C) if C > 1 else torch.tensor([1e-3])
    x = torch.randn(M, C, generator=gen) * sd + mu
    if regime == "R3":
        x[:, ::5] = 3.25
        x[:, 1] = 0.0
    gamma = torch.randn(C, generator=gen)
    gamma[::3] = -gamma[::3].abs() - 0.1
    beta = torch.randn(C, generator=gen)
    res, dy = torch.randn(M, C, generator=gen), torch.randn(M, C, generator=gen)
    if regime.startswith("R5"):
        row = M - 1 if regime == "R5 last row" else 256
        keep_row = dy[row].clone()
        dy.zero_()
        dy[row] = keep_row
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta)


# ------------------------------------------------------------------------------------------------------------------ pipeline
ALL_FLAGS = ((1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 1, 0), (0, 0, 1))      # (batch_stats, dx, dres)


def check_stats(group, case, xo, x, seed=0):
    """segsde_bn_stats on the operand, running buffers and counter included -> the kernel's (mean, invstd) on the device"""
    dev = xo.v.device
    x64 = x.double()
    rm0 = (0.7 * x64.mean(0)).float()                   # same sign as the batch mean: the update does not cancel
    rv0 = (1.3 * x64.var(0, unbiased=False) + 0.25).float()
    rm, rv, nbt = rm0.clone().to(dev), rv0.clone().to(dev), torch.tensor([41 + seed], dtype=torch.int64).to(dev)
    mean, invstd = k_stats(xo, rm, rv, nbt)
    xo.check(case)
    assert int(nbt.cpu()[0]) == 42 + seed, (case, "num_batches_tracked")
    r64, r32 = ref_stats(torch.float64, x, rm0, rv0), ref_stats(torch.float32, x, rm0, rv0)
    got = dict(mean=mean.cpu(), invstd=invstd.cpu(), rm=rm.cpu(), rv=rv.cpu())
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (case, k, "not finite")
    rec_vec(group, case, "mean", got["mean"], r64["mean"], r32["mean"], x64.abs().sum(0) / x.shape[0])
    for k, name in (("invstd", "invstd"), ("rm", "running_mean"), ("rv", "running_var")):
        rec_vec(group, case, name, got[k], r64[k], r32[k], r64[k].abs())
    # without buffers and counter the same statistics, bit for bit
    mean2, invstd2 = k_stats(xo)
    BM.same_bits(mean2, mean, case + ": mean without running buffers")
    BM.same_bits(invstd2, invstd, case + ": invstd without running buffers")
    return mean, invstd, r64


def keep_mask(M, C, p, seed, device):
    """the counter-based draw on the logical index m * C + c, from the specification (oracle/dropout.py); the mask dropout_kernel
    makes is a second witness that must equal it"""
    keep = torch.from_numpy(OD.keep(seed, (M, C), p))
    witness = (H.dropout(torch.ones(M, C, dtype=torch.float32).to(device), p, seed) != 0).cpu()
    assert torch.equal(witness, keep), ("dropout_kernel's mask is not the specification's", int((witness != keep).sum()))
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p)) <= 0.02, ("keep fraction", frac)
    return keep


def pipeline(device, group, s, vals, act, use_res, affine, p=0.0, flags=((1, 1, 1),), stats=None, lds=None, remask=False,
             tag=""):
    """statistics (once per operand: ``stats`` hands them on), apply, backward in the saved-output mode for every (batch_stats, dx,
    dres) of ``flags``, each against float64; with ``remask`` the remask mode bit for bit against the saved-output mode.
    lds: {operand: (pitch, offset)} for x, res, y, dy, dx, dres where they differ from the shape's own"""
    M, C, ld, off = s
    lds = lds or {}
    mk = lambda name, value=None: Opd(M, C, *lds.get(name, (ld, off)), device, value)
    case = "%s%s %s%s%s%s" % (spec_name(s), tag, act, "+res" if use_res else "", "" if affine else " no affine",
                              " p%.1f" % p if p else "")
    x, res, dy = vals["x"], (vals["res"] if use_res else None), vals["dy"]
    if stats is None:
        xo = mk("x", x)
        mean, invstd, _ = check_stats(group, spec_name(s) + tag, xo, x)
        stats = (xo, mean, invstd)
    xo, mean, invstd = stats
    mean_c, invstd_c = mean.cpu(), invstd.cpu()
    gamma, beta = (vals["gamma"], vals["beta"]) if affine else (None, None)
    gd, bd = (gamma.to(device), beta.to(device)) if affine else (None, None)
    ro = mk("res", res) if use_res else None
    keep = keep_mask(M, C, p, SEED, device) if p else None
    # ---- apply
    yo = mk("y")
    k_apply(xo, mean, invstd, gd, bd, ro, yo, act, p, SEED)
    y = yo.cpu()
    assert bool(torch.isfinite(y).all()), (case, "y not finite")
    for o in (xo, ro, yo):
        if o is not None:
            o.check(case + " apply")
    rec_cols(group, case, "y", y, ref_apply(torch.float64, x, mean_c, invstd_c, gamma, beta, res, act, keep, p),
             ref_apply(torch.float32, x, mean_c, invstd_c, gamma, beta, res, act, keep, p))
    if p:
        y0o = mk("y")
        k_apply(xo, mean, invstd, gd, bd, ro, y0o, act, 0.0, 0)
        y0 = y0o.cpu()
        live = y0 != 0
        assert torch.equal((y != 0)[live], keep[live]) and bool((y[~live] == 0).all()), (case, "keep mask implied by y")
    # ---- backward from the saved output
    dyo = mk("dy", dy)
    r64 = ref_backward(torch.float64, dy, y, x, mean_c, invstd_c, gamma, act, keep, p)
    r32 = ref_backward(torch.float32, dy, y, x, mean_c, invstd_c, gamma, act, keep, p)
    saved = {}
    for bs, need_dx, need_dres in flags:
        fcase = case + " bs%d dx%d dres%d" % (bs, need_dx, need_dres)
        dxo, dro = (mk("dx") if need_dx else None), (mk("dres") if need_dres else None)
        dg, db = k_backward(dyo, yo, xo, mean, invstd, gd, bd, act, p, SEED, bs, dxo, dro)
        for o in (xo, dyo, yo, dxo, dro):
            if o is not None:
                o.check(fcase)
        rec_vec(group, fcase, "dgamma", dg.cpu(), r64["dgamma"], r32["dgamma"], r64["s_gamma"])
        rec_vec(group, fcase, "dbeta", db.cpu(), r64["dbeta"], r32["dbeta"], r64["s_beta"])
        if need_dx:
            rec_cols(group, fcase, "dx", dxo.cpu(), r64["dx%d" % bs], r32["dx%d" % bs])
        if need_dres:
            rec_cols(group, fcase, "dres", dro.cpu(), r64["dz"], r32["dz"])
        saved[(bs, need_dx)] = (dg, db, dxo)
    # ---- remask mode (no saved output; y is what bn_apply produced from the same x, gamma, beta, no residual)
    if remask:
        assert act in ("none", "relu") and not use_res and not p
        for (bs, need_dx), (dg0, db0, dx0) in saved.items():
            dxo = mk("dx") if need_dx else None
            dg, db = k_backward(dyo, None, xo, mean, invstd, gd, bd, act, 0.0, 0, bs, dxo, None)
            what = case + " remask bs%d dx%d" % (bs, need_dx)
            BM.same_bits(dg, dg0, what + " dgamma")
            BM.same_bits(db, db0, what + " dbeta")
            if need_dx:
                BM.same_bits(dxo.v, dx0.v, what + " dx")
                dxo.check(what)
    return dict(stats=stats, y=y, yo=yo, r64=r64, saved=saved, case=case)


# -------------------------------------------------------------------------------------------------------------------- shapes
RED_SHAPES = [spec(1, 4), spec(7, 3),
              spec(255, 1), spec(257, 2),              # two reduction blocks, the second ragged
              spec(513, 5),
              spec(300, 19, 24, 3),                    # scalar kernels, the pointer 12 bytes off a 16-byte boundary
              spec(300, 20, 24, 4),                    # VW = 4 on a pitch
              spec(300, 20, 24, 3),                    # quads of channels and of pitch: scalar by the pointer alone
              spec(300, 8, 9),                         # scalar by the pitch
              spec(515, 65),                           # scalar, two column blocks
              spec(515, 68),                           # VW = 4, a second column block of one quad
              spec(1030, 64)]
CAPPED_SHAPES = [spec(131073, 4), spec(131073, 3)]     # red_blocks capped at 512: rows_per 257, block 510 has 3 rows, block 511 none
APPLY_SHAPES = RED_SHAPES + [spec(5, 12), spec(33, 20),      # CV = 3 and 5: the division path
                             spec(257, 64),                  # fixed_c
                             spec(33, 2048)]                 # fixed_c at 512 vectors per row (blocks alternate between row halves)
REMASK_CONFIGS = [("none", True), ("none", False), ("relu", True), ("relu", False)]      # (act, affine)


def run_shape(device, s, group="shapes"):
    """one shape at R0: ELU with a residual from the saved output; the four remask configurations"""
    first = len(RECORDS)
    M, C = s[0], s[1]
    vals = make_values(M, C)
    reduce_only = s in CAPPED_SHAPES
    out = pipeline(device, group, s, vals, "elu", True, True, flags=((1, 0, 0),) if reduce_only else ((1, 1, 1), (0, 1, 0)))
    for act, affine in (REMASK_CONFIGS[2:3] if reduce_only else REMASK_CONFIGS):
        pipeline(device, group, s, vals, act, False, affine, flags=((1, 0, 0),) if reduce_only else ((1, 1, 0), (0, 1, 0), (1, 0, 0)),
                 stats=out["stats"], remask=True)
    finish(first)


def run_remask_nonfinite(device):
    """NaN, -Inf and a negative gradient on elements a plain ReLU switched off: the saved-output mode forms dy * 0 (NaN, NaN, -0),
    and the remask mode must hand on the same bits, in dx (batch statistics off: dx = gamma * invstd * dz) and in the sums"""
    M, C = 9, 8
    vals = make_values(M, C, seed=7)
    xo = Opd(M, C, C, 0, device, vals["x"])
    mean, invstd = k_stats(xo)
    gd, bd = vals["gamma"].to(device), vals["beta"].to(device)
    yo = Opd(M, C, C, 0, device)
    k_apply(xo, mean, invstd, gd, bd, None, yo, "relu")
    off = torch.nonzero(yo.cpu().reshape(-1) == 0).reshape(-1)
    assert off.numel() >= 3
    dy = vals["dy"].clone()
    spots = [(int(i) // C, int(i) % C) for i in off[:3]]
    for (m, c), v in zip(spots, (float("nan"), float("-inf"), -1.5)):
        dy[m, c] = v
    dyo = Opd(M, C, C, 0, device, dy)
    out = []
    for y in (yo, None):
        dxo = Opd(M, C, C, 0, device)
        dg, db = k_backward(dyo, y, xo, mean, invstd, gd, bd, "relu", 0.0, 0, 0, dxo, None)
        out.append((dxo.cpu(), dg.cpu(), db.cpu()))
    for name, a, b in zip(("dx", "dgamma", "dbeta"), out[0], out[1]):
        BM.same_bits(b, a, "remask with non-finite dy: " + name)
    dx = out[1][0]
    assert bool(torch.isnan(dx[spots[0]])) and bool(torch.isnan(dx[spots[1]])) and float(dx[spots[2]]) == 0.0
    assert bool(torch.isnan(out[1][2][spots[0][1]]))


def run_own_pitches(device):
    """x, res, y, dy, dx, dres each at a pitch of its own (multiples of 4: the VW = 4 kernels), slack columns guarded"""
    first = len(RECORDS)
    s = spec(300, 20)
    lds = dict(x=(24, 4), res=(28, 0), y=(32, 8), dy=(36, 12), dx=(40, 4), dres=(44, 24))
    assert len(set(v[0] for v in lds.values())) == 6 and all(v[0] % 4 == 0 and v[1] % 4 == 0 for v in lds.values())
    vals = make_values(*s[:2], seed=1)
    out = pipeline(device, "pitches", s, vals, "relu", True, True, flags=ALL_FLAGS, lds=lds, tag=" six pitches")
    pipeline(device, "pitches", s, vals, "relu", False, True, flags=((1, 1, 0), (0, 1, 0)), lds=lds, stats=out["stats"], remask=True,
             tag=" six pitches")
    # and odd ones: the scalar kernels
    lds = dict(x=(21, 1), res=(23, 0), y=(25, 2), dy=(27, 5), dx=(29, 3), dres=(31, 11))
    pipeline(device, "pitches", s, vals, "elu", True, True, flags=ALL_FLAGS, lds=lds, tag=" six odd pitches")
    finish(first)


# --------------------------------------------------------------------------------------------------------------------- flags
FLAG_SHAPES = [spec(1030, 64), spec(300, 20, 24, 4), spec(300, 19, 24, 3)]          # dense VW = 4, pitched, scalar
DROP_SHAPES = [spec(1030, 64), spec(3001, 20, 24, 4), spec(3200, 19, 24, 3)]        # M * C >= 60000


def run_flags(device, s):
    first = len(RECORDS)
    vals = make_values(*s[:2], seed=2)
    stats = None
    for act in ACTS:
        for use_res in (False, True):
            for affine in (True, False):
                out = pipeline(device, "flags", s, vals, act, use_res, affine, flags=ALL_FLAGS, stats=stats)
                stats = out["stats"]
    finish(first)


def run_dropout(device, s):
    first = len(RECORDS)
    assert s[0] * s[1] >= 60000
    vals = make_values(*s[:2], seed=3)
    stats = None
    for act in ("relu", "elu"):
        for use_res in (False, True):
            out = pipeline(device, "dropout", s, vals, act, use_res, True, p=P_DROP, flags=((1, 1, 1), (0, 1, 0)), stats=stats)
            stats = out["stats"]
    finish(first)


# ------------------------------------------------------------------------------------------------------------------- regimes
REGIME_SHAPES = [spec(1030, 64), spec(300, 19, 24, 3)]


def run_regime(device, regime):
    first = len(RECORDS)
    for s in REGIME_SHAPES:
        M, C = s[0], s[1]
        vals = make_values(M, C, regime, seed=4)
        x64 = vals["x"].double()
        if regime.startswith("R1"):
            nominal = 1e2 if regime == "R1 1e2" else 1e3
            rel = x64.mean(0).abs() / x64.std(0, unbiased=False)
            assert bool((rel >= nominal / 2).all()) and bool((rel <= 2 * nominal).all()), (regime, rel)
        if regime == "R2":
            var = x64.var(0, unbiased=False)
            assert float(var.min()) < BN_EPS < 1.0 < float(var.max())
        tag = " " + regime
        out = pipeline(device, regime, s, vals, "elu", True, True, flags=((1, 1, 1),), tag=tag)
        plain = pipeline(device, regime, s, vals, "none", False, True, flags=((1, 1, 0),), stats=out["stats"], remask=True, tag=tag)
        if regime.startswith("R1"):
            rows = [r for r in RECORDS[first:] if r[2] == "invstd" and r[1].startswith(spec_name(s))]
            print("BN-EDGE-R1 | %s | %s | invstd ratio %.3f" % (regime, spec_name(s), rows[-1][6]))
        if regime == "R3":
            _, mean, invstd = out["stats"]
            const = torch.zeros(C, dtype=torch.bool)
            const[::5] = True
            const[1] = True
            mean, invstd = mean.cpu(), invstd.cpu()
            want = torch.tensor(1.0 / np.sqrt(np.float64(BN_EPS)), dtype=torch.float64).float()
            assert bool((invstd[const] == want).all()), "var = 0 must give invstd = 1 / sqrt(eps)"
            assert bool((mean[const] == vals["x"][0, const]).all()), "the mean of a constant channel is its value"
            # xhat = 0 there: act none without residual gives beta, dgamma is exactly 0
            assert bool((plain["y"][:, const] == vals["beta"][const]).all()), "xhat is not 0 on a constant channel"
            for dg, db, dxo in list(out["saved"].values()) + list(plain["saved"].values()):
                assert bool((dg.cpu()[const] == 0).all()), "dgamma of a constant channel is not exactly 0"
                assert bool(torch.isfinite(dg.cpu()).all()) and bool(torch.isfinite(db.cpu()).all())
                assert dxo is None or bool(torch.isfinite(dxo.cpu()).all())
    finish(first)


def run_planted_zeros(device):
    """R4: ReLU after a residual with y == 0 exactly at planted elements (res = -BN(x) as the kernel's own apply forms it)"""
    first = len(RECORDS)
    for s in REGIME_SHAPES:
        M, C, ld, off = s
        vals = make_values(M, C, seed=5)
        xo = Opd(M, C, ld, off, device, vals["x"])
        mean, invstd, _ = check_stats("R4", spec_name(s) + " R4", xo, vals["x"])
        zo = Opd(M, C, ld, off, device)
        k_apply(xo, mean, invstd, vals["gamma"].to(device), vals["beta"].to(device), None, zo, "none")
        z = zo.cpu()
        n = M * C
        planted = sorted({0, n // 3, n - 1, (5 * n) // 7, 255 * C, 256 * C + 1})
        rows, cols = torch.tensor([i // C for i in planted]), torch.tensor([i % C for i in planted])
        vals["res"][rows, cols] = -z[rows, cols]
        out = pipeline(device, "R4", s, vals, "relu", True, True, flags=ALL_FLAGS, stats=(xo, mean, invstd), tag=" R4")
        assert bool((out["y"][rows, cols] == 0).all()), "planted zeros are not zero"
        assert bool((out["r64"]["dz"][rows, cols] == 0).all())
        assert bool((vals["dy"][rows, cols] != 0).all())
        dro = Opd(M, C, ld, off, device)
        k_backward(Opd(M, C, ld, off, device, vals["dy"]), out["yo"], xo, mean, invstd, vals["gamma"].to(device),
                   vals["beta"].to(device), "relu", 0.0, 0, 1, None, dro)
        assert bool((dro.cpu()[rows, cols] == 0).all()), "the derivative at y == 0 is not 0"
    finish(first)


# ---------------------------------------------------------------------------------------------------------------- eval stats
def run_eval_stats(device):
    first = len(RECORDS)
    for C in (1, 19, 300):                                # 300: two blocks
        gen = _gen(70 + C)
        rm, rv = torch.randn(C, generator=gen), torch.rand(C, generator=gen) * 2
        rv[0] = 0.0
        mean, invstd = H.bn_eval_stats(rm.to(device), rv.to(device), BN_EPS)
        BM.same_bits(mean.cpu(), rm, "eval mean")
        r64, r32 = 1 / torch.sqrt(rv.double() + BN_EPS), 1 / torch.sqrt(rv + BN_EPS)
        rec_vec("eval", "C%d" % C, "invstd", invstd.cpu(), r64, r32, r64.abs())
    finish(first)


# --------------------------------------------------------------------------------------------------------------- second trip
TRIP_CASES = [(4194381, 1, 1),        # scalar, three trips
              (2097667, 4, 4),        # VW = 4, fixed_c
              (700000, 12, 4),        # CV = 3: the division path
              (4100, 2048, 4)]        # 512 vectors per row: the block count rounded to a multiple of 2


def run_second_trip(device, M, C, VW):
    # ew_blocks caps the grid at 8192 blocks of 256 threads: more channel vectors than that make every thread loop again
    assert M * C / VW > 8192 * 256
    first = len(RECORDS)
    s = spec(M, C)
    vals = make_values(M, C, seed=6)
    out = pipeline(device, "second trip", s, vals, "elu", True, True, flags=((1, 1, 1),))
    pipeline(device, "second trip", s, vals, "relu", False, True, flags=((1, 1, 0),), stats=out["stats"], remask=True)
    del out, vals
    if C in (4, 2048):              # the mask mode: its wave-uniform trip count and word stores, bit for bit
        d = BM.make_inputs(M, C, C, device)
        y, mask = BM.forward_pair(d)
        d["dy"].nan_to_num_(1.0)                     # (the NaN make_inputs plants would blank a quarter of dx at C = 4)
        BM.backward_pair(d, y, mask, True, True, True)
    finish(first)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _e2e_reference(dt, calls, gamma, beta, act, C):
    rm, rv = torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt)
    outs = []
    for x, res, dy in calls:
        leaf = lambda t, shape: t.detach().clone().reshape(shape).to(dt).requires_grad_(True)
        xx, rr, g, b = leaf(x, (-1, C)), (None if res is None else leaf(res, (-1, C))), leaf(gamma, (C,)), leaf(beta, (C,))
        z = F.batch_norm(xx, rm, rv, g, b, True, MOM, BN_EPS)
        z.retain_grad()
        out = act_fn(z if rr is None else z + rr, act)
        out.backward(dy.reshape(-1, C).to(dt))
        outs.append(dict(y=out.detach(), dx=xx.grad, dres=None if rr is None else rr.grad, dgamma=g.grad, dbeta=b.grad, dz=z.grad,
                         rm=rm.clone(), rv=rv.clone()))
    return outs


def run_end_to_end(device):
    """functional.BNActFn (statistics from x) forward and backward, twice, against F.batch_norm under autograd"""
    first = len(RECORDS)
    for C in (19, 64):
        for act in ("none", "elu"):
            for use_res in (False, True):
                gen = _gen(900 + C + 7 * ACTS.index(act) + use_res)
                shape = (2, 9, 13, C)
                sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
                mu, sd = sign * (0.5 + 2.5 * torch.rand(C, generator=gen)), 0.5 + 1.5 * torch.rand(C, generator=gen)
                calls = [(torch.randn(shape, generator=gen) * sd + mu, torch.randn(shape, generator=gen) if use_res else None,
                          torch.randn(shape, generator=gen)) for _ in range(2)]
                gamma = torch.randn(C, generator=gen)
                gamma[::3] = -gamma[::3].abs() - 0.1
                beta = torch.randn(C, generator=gen)
                r64s, r32s = (_e2e_reference(dt, calls, gamma, beta, act, C) for dt in (torch.float64, torch.float32))
                rm, rv = torch.zeros(C).to(device), torch.ones(C).to(device)
                nbt = torch.zeros(1, dtype=torch.int64).to(device)
                for i, (x, res, dy) in enumerate(calls):
                    case = "C%d %s%s call %d" % (C, act, "+res" if use_res else "", i + 1)
                    leaf = lambda t: t.detach().clone().to(device).requires_grad_(True)
                    xd, rd, g, b = leaf(x), (None if res is None else leaf(res)), leaf(gamma), leaf(beta)
                    out = Fn.BNActFn.apply(xd, g, b, rd, rm, rv, True, MOM, BN_EPS, act, 0.0, 0, None, None, nbt)
                    out.backward(dy.to(device))
                    assert int(nbt.cpu()[0]) == i + 1, (case, "num_batches_tracked")
                    r64, r32 = r64s[i], r32s[i]
                    flat = lambda t: t.detach().cpu().reshape(-1, C)
                    rec_cols("end to end", case, "y", flat(out), r64["y"], r32["y"])
                    rec_cols("end to end", case, "dx", flat(xd.grad), r64["dx"], r32["dx"])
                    if use_res:
                        rec_cols("end to end", case, "dres", flat(rd.grad), r64["dres"], r32["dres"])
                    x64 = x.reshape(-1, C).double()
                    xh = (x64 - x64.mean(0)) / torch.sqrt(x64.var(0, unbiased=False) + BN_EPS)
                    rec_vec("end to end", case, "dgamma", g.grad.cpu(), r64["dgamma"], r32["dgamma"], (r64["dz"] * xh).abs().sum(0))
                    rec_vec("end to end", case, "dbeta", b.grad.cpu(), r64["dbeta"], r32["dbeta"], r64["dz"].abs().sum(0))
                    rec_vec("end to end", case, "running_mean", rm.cpu(), r64["rm"], r32["rm"], r64["rm"].abs())
                    rec_vec("end to end", case, "running_var", rv.cpu(), r64["rv"], r32["rv"], r64["rv"].abs())
    finish(first)
