"""Cross-replica (synchronized) BatchNorm: the four stages of segsde_bn_sync_* (csrc/elementwise.hip), functional.BNActFn with a
process group, models.layers.SyncBatchNorm2d and ddp.convert_sync_batchnorm.  Shared by tests/test_sync_bn_emu.py (interpreter build
of the kernel sources), tests/test_sync_bn_gloo.py (two and three CPU processes over gloo, interpreted kernels) and
tests/test_sync_bn_gpu.py (real library).

The oracle is FULL-BATCH BatchNorm in float64 torch on the CPU over the concatenation of all ranks' rows: forward, running buffers,
and dx / dres / dgamma / dbeta of the loss sum_r loss_r.  The tolerance is the rule of tests/batchnorm_cases.py, with its K, its
error accounting (rec_cols / rec_vec / finish) and its float32 reference (the same full-batch formulas in float32 torch): per
channel, e_kernel / max(e_fp32, 2^-23 * scale) <= K.  Scales as there; weight gradients of the convolutions of the gloo stack:
sum |dy| * |x| over the terms of each entry.  As there, the stored fp32 mean / invstd and the y handed to the backward stages are
inputs of the later stages.  One gathered row (W = 1) is compared bit for bit with the single-process kernels.  Nothing is left out
of any comparison.  The worst ratios of the MI355X run are in profiles/sync_bn.md."""
import datetime
import os
import socket
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

import batchnorm_cases as BC
import bn_bitmask_cases as BM
from oracle import dropout as OD
from improving_segmentation_with_selfsupervised_depth_amd import _lib
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = BC.K
Opd, _p = BC.Opd, BC._p
GUARD = BC.GUARD

# (rows per rank, C, pitch, column offset): the smallest that reach each path
CHUNK_CASES = [((5, 3), 6, None, 0),            # scalar path, unequal counts
               ((1, 7), 3, None, 0),            # a rank with a single row
               ((64, 64), 8, None, 0),          # vector path
               ((33, 31, 2), 64, 72, 4),        # three ranks, pitched and offset operands
               ((300, 212), 4, None, 0),        # more than one reduction block per rank
               ((256,), 8, None, 0)]            # W = 1
# (act, residual, gamma / beta, drop_p)
COMBOS = [("none", False, True, 0.0),           # remask mode (y not read)
          ("relu", False, True, 0.0),           # remask mode
          ("relu", True, True, 0.0),            # bitmask mode where C % 4 == 0, saved output otherwise
          ("elu", True, True, 0.0),             # saved output
          ("elu", True, True, BC.P_DROP),       # dropout inside apply and both backward stages
          ("elu", True, False, 0.0),            # gamma = None
          ("relu", False, False, 0.0)]          # gamma = None in the remask mode
PARTIAL_CASES = [CHUNK_CASES[2], CHUNK_CASES[3], CHUNK_CASES[4]]
PARTIAL_ROWS = (3, 70)
ONE_RANK_SHAPES = [BC.spec(7, 3), BC.spec(300, 19, 24, 3), BC.spec(300, 20, 24, 4), BC.spec(515, 68), BC.spec(1030, 64)]


def case_name(c):
    chunks, C, pitch, off = c
    return "chunks %s C%d" % ("+".join(str(m) for m in chunks), C) + (" pitch %d off %d" % (pitch, off) if pitch else "")


# ------------------------------------------------------------------------------------------------------------- the C ABI, on Opd
def row_len(C):
    return H.bn_sync_row_len(C)


def _new_row(C, dev):
    return torch.full((row_len(C),), GUARD, dtype=torch.float64).to(dev)


def k_local_stats(xo):
    L = _lib.lib()
    row = _new_row(xo.C, xo.v.device)
    nb = L.segsde_bn_stats_workspace(xo.M, xo.C)
    ws = H._ws(nb, xo.v)
    _lib.check(L.segsde_bn_sync_stats_local(_p(xo.v), xo.ld, xo.M, xo.C, _p(row), _p(ws), nb, H._stream(xo.v)), "bn_sync_stats_local")
    return row


def k_local_stats_partials(part, M):
    L = _lib.lib()
    rows, _, C = part.shape
    row = _new_row(C, part.device)
    nb = L.segsde_bn_stats_from_partials_workspace(C)
    ws = H._ws(nb, part)
    _lib.check(L.segsde_bn_sync_stats_local_from_partials(_p(part), rows, M, C, _p(row), _p(ws), nb, H._stream(part)),
               "bn_sync_stats_local_from_partials")
    return row


def k_global_stats(rows, C, rm=None, rv=None, nbt=None):
    dev = rows.device
    mean = torch.full((C,), GUARD, dtype=torch.float32).to(dev)
    invstd, inv_count = mean.clone(), torch.full((1,), GUARD, dtype=torch.float32).to(dev)
    _lib.check(_lib.lib().segsde_bn_sync_stats_global(_p(rows), rows.shape[0], C, _p(mean), _p(invstd), _p(rm), _p(rv), BC.MOM, BC.BN_EPS,
                                                      _p(nbt), _p(inv_count), H._stream(rows)), "bn_sync_stats_global")
    return mean, invstd, inv_count


def k_apply_mask(xo, mean, invstd, gamma, beta, ro, yo, act):
    L = _lib.lib()
    mask = torch.full((L.segsde_bn_mask_words(xo.M, xo.C),), BM.GUARD, dtype=torch.int32).to(xo.v.device)
    _lib.check(L.segsde_bn_apply_mask(_p(xo.v), xo.ld, xo.M, xo.C, _p(mean), _p(invstd), _p(gamma), _p(beta),
                                      _p(None if ro is None else ro.v), 0 if ro is None else ro.ld, _p(yo.v), yo.ld, H.ACT[act], 0.0, 0,
                                      _p(mask), H._stream(xo.v)), "bn_apply_mask")
    return mask


def k_backward_mask(dyo, mask, xo, mean, invstd, gamma, dxo, dro):
    L = _lib.lib()
    M, C, dev = xo.M, xo.C, xo.v.device
    dg, db = torch.full((C,), GUARD).to(dev), torch.full((C,), GUARD).to(dev)
    nb = L.segsde_bn_backward_workspace(M, C)
    ws = H._ws(nb, xo.v)
    _lib.check(L.segsde_bn_backward_mask(_p(dyo.v), dyo.ld, _p(mask), _p(xo.v), xo.ld, M, C, _p(mean), _p(invstd), _p(gamma),
                                         H.ACT["relu"], 0.0, 1, _p(dg), _p(db), _p(None if dxo is None else dxo.v),
                                         C if dxo is None else dxo.ld, _p(None if dro is None else dro.v), C if dro is None else dro.ld,
                                         _p(ws), nb, H._stream(xo.v)), "bn_backward_mask")
    return dg, db


def k_bwd_local(dyo, yo, mask, xo, mean, invstd, gamma, beta, act, p, seed, has_dres):
    """yo None and mask None: the remask mode; mask: the bitmask mode (yo is not passed on) -> (row, dgamma, dbeta)"""
    L = _lib.lib()
    M, C, dev = xo.M, xo.C, xo.v.device
    dg, db = torch.full((C,), GUARD).to(dev), torch.full((C,), GUARD).to(dev)
    row = _new_row(C, dev)
    nb = L.segsde_bn_backward_workspace(M, C)
    ws = H._ws(nb, xo.v)
    y = None if (yo is None or mask is not None) else yo
    _lib.check(L.segsde_bn_sync_backward_local(_p(dyo.v), dyo.ld, _p(None if y is None else y.v), xo.ld if y is None else y.ld, _p(mask),
                                               _p(xo.v), xo.ld, M, C, _p(mean), _p(invstd), _p(gamma), _p(beta), H.ACT[act], p, seed,
                                               int(has_dres), _p(dg), _p(db), _p(row), _p(ws), nb, H._stream(xo.v)),
               "bn_sync_backward_local")
    return row, dg, db


def k_bwd_global(dyo, yo, mask, xo, mean, invstd, gamma, beta, act, p, seed, rows, inv_count, dxo, dro):
    """-> (sum dgamma, sum dbeta) over the gathered rows, as floats"""
    M, C, dev = xo.M, xo.C, xo.v.device
    tot = torch.full((2, C + (-C) % 4), GUARD).to(dev)
    tg, tb = tot[0, :C], tot[1, :C]
    y = None if (yo is None or mask is not None) else yo
    _lib.check(_lib.lib().segsde_bn_sync_backward_global(
        _p(dyo.v), dyo.ld, _p(None if y is None else y.v), xo.ld if y is None else y.ld, _p(mask), _p(xo.v), xo.ld, M, C, _p(mean),
        _p(invstd), _p(gamma), _p(beta), H.ACT[act], p, seed, _p(rows), rows.shape[0], _p(inv_count), _p(tg), _p(tb),
        _p(None if dxo is None else dxo.v), C if dxo is None else dxo.ld, _p(None if dro is None else dro.v),
        C if dro is None else dro.ld, H._stream(xo.v)), "bn_sync_backward_global")
    return tg, tb


def _keep(M, C, p, device):
    """the counter-based draw on the logical index m * C + c of ONE rank's operand (each rank draws on its own rows), from the
    specification (oracle/dropout.py); dropout_kernel's mask is a second witness that must equal it"""
    keep = torch.from_numpy(OD.keep(BC.SEED, (M, C), p))
    witness = (H.dropout(torch.ones(M, C, dtype=torch.float32).to(device), p, BC.SEED) != 0).cpu()
    assert torch.equal(witness, keep), ("dropout_kernel's mask is not the specification's", int((witness != keep).sum()))
    return keep


def _running0(x):
    x64 = x.double()
    var = x64.var(0, unbiased=False) if x.shape[0] > 1 else torch.zeros(x.shape[1], dtype=torch.float64)
    return (0.7 * x64.mean(0)).float(), (1.3 * var + 0.25).float()


# -------------------------------------------------------------------------------------- 1. stage-level chunk emulation, one process
def _forward_stats(device, group, name, chunks, C, x, rows, xos):
    """the global stage on every emulated rank: the same bits everywhere, and the full-batch statistics"""
    Mt = sum(chunks)
    rm0, rv0 = _running0(x)
    first = None
    for r in range(len(chunks)):
        rm, rv, nbt = rm0.clone().to(device), rv0.clone().to(device), torch.tensor([41], dtype=torch.int64).to(device)
        mean, invstd, inv = k_global_stats(rows, C, rm, rv, nbt)
        assert int(nbt.cpu()[0]) == 42, (name, "num_batches_tracked")
        if first is None:
            first = (mean, invstd, inv, rm, rv)
        else:
            for a, b, what in zip((mean, invstd, inv, rm, rv), first, ("mean", "invstd", "1 / M", "running_mean", "running_var")):
                BM.same_bits(a, b, "%s: %s of rank %d against rank 0" % (name, what, r))
    mean, invstd, inv, rm, rv = first
    assert float(inv.cpu()[0]) == float(np.float32(1.0) / np.float32(Mt)), (name, "1 / (float)M_total")
    for xo in xos:
        xo.check(name + " statistics")
    r64, r32 = BC.ref_stats(torch.float64, x, rm0, rv0), BC.ref_stats(torch.float32, x, rm0, rv0)
    got = dict(mean=mean.cpu(), invstd=invstd.cpu(), rm=rm.cpu(), rv=rv.cpu())
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (name, k, "not finite")
    BC.rec_vec(group, name, "mean", got["mean"], r64["mean"], r32["mean"], x.double().abs().sum(0) / Mt)
    for k, what in (("invstd", "invstd"), ("rm", "running_mean"), ("rv", "running_var")):
        BC.rec_vec(group, name, what, got[k], r64[k], r32[k], r64[k].abs())
    # without buffers and counter the same statistics
    mean2, invstd2, _ = k_global_stats(rows, C)
    BM.same_bits(mean2, mean, name + ": mean without running buffers")
    BM.same_bits(invstd2, invstd, name + ": invstd without running buffers")
    return mean, invstd, inv


def _check_rows(name, rows, chunks, C):
    rc = rows.cpu()
    assert tuple(rc.shape) == (len(chunks), 2 * C + 2) and rc.shape[1] * 8 % 16 == 0, (name, "row layout")
    assert torch.equal(rc[:, 2 * C], torch.tensor(chunks, dtype=torch.float64)), (name, "row counts", rc[:, 2 * C])
    assert bool((rc[:, 2 * C + 1] == 0).all()), (name, "row padding")


def _combo(device, group, name, chunks, sl, C, ld, off, vals, xos, mean, invstd, inv, combo):
    act, use_res, affine, p = combo
    case = "%s %s%s%s%s" % (name, act, "+res" if use_res else "", "" if affine else " no affine", " p%.1f" % p if p else "")
    x, dy, res = vals["x"], vals["dy"], (vals["res"] if use_res else None)
    gamma, beta = (vals["gamma"], vals["beta"]) if affine else (None, None)
    gd, bd = (gamma.to(device), beta.to(device)) if affine else (None, None)
    mean_c, invstd_c = mean.cpu(), invstd.cpu()
    remask = act in ("none", "relu") and not use_res and not p
    bitmask = act == "relu" and use_res and not p and C % 4 == 0 and ld % 4 == 0 and off % 4 == 0
    mk = lambda m, value=None: Opd(m, C, ld, off, device, value)
    # ---- apply, per rank
    ros, yos, masks, keeps = [], [], [], []
    for m, s, xo in zip(chunks, sl, xos):
        ro, yo = (mk(m, res[s]) if use_res else None), mk(m)
        if bitmask:
            masks.append(k_apply_mask(xo, mean, invstd, gd, bd, ro, yo, act))
        else:
            BC.k_apply(xo, mean, invstd, gd, bd, ro, yo, act, p, BC.SEED)
            masks.append(None)
        keeps.append(_keep(m, C, p, device) if p else None)
        for o in (xo, ro, yo):
            if o is not None:
                o.check(case + " apply")
        ros.append(ro)
        yos.append(yo)
    y = torch.cat([yo.cpu() for yo in yos])
    keep = torch.cat(keeps) if p else None
    assert bool(torch.isfinite(y).all()), (case, "y not finite")
    BC.rec_cols(group, case, "y", y, BC.ref_apply(torch.float64, x, mean_c, invstd_c, gamma, beta, res, act, keep, p),
                BC.ref_apply(torch.float32, x, mean_c, invstd_c, gamma, beta, res, act, keep, p))
    # ---- backward: local stage per rank, the rows stacked as the all-gather leaves them, global stage per rank
    dyos = [mk(m, dy[s]) for m, s in zip(chunks, sl)]
    rows, locs = [], []
    for m, s, xo, yo, dyo, mask in zip(chunks, sl, xos, yos, dyos, masks):
        row, dg, db = k_bwd_local(dyo, None if remask else yo, mask, xo, mean, invstd, gd, bd, act, p, BC.SEED, use_res)
        rows.append(row)
        locs.append((dg, db))
    rows = torch.stack(rows)
    _check_rows(case + " backward", rows, chunks, C)
    r64 = BC.ref_backward(torch.float64, dy, y, x, mean_c, invstd_c, gamma, act, keep, p)
    r32 = BC.ref_backward(torch.float32, dy, y, x, mean_c, invstd_c, gamma, act, keep, p)
    dxs, drs, tot0 = [], [], None
    for r, (m, s, xo, yo, dyo, mask) in enumerate(zip(chunks, sl, xos, yos, dyos, masks)):
        # this rank's parameter gradients: the sums over its own rows
        kr = None if keep is None else keep[s]
        l64 = BC.ref_backward(torch.float64, dy[s], y[s], x[s], mean_c, invstd_c, gamma, act, kr, p)
        l32 = BC.ref_backward(torch.float32, dy[s], y[s], x[s], mean_c, invstd_c, gamma, act, kr, p)
        rcase = case + " rank %d" % r
        BC.rec_vec(group, rcase, "dgamma", locs[r][0].cpu(), l64["dgamma"], l32["dgamma"], l64["s_gamma"])
        BC.rec_vec(group, rcase, "dbeta", locs[r][1].cpu(), l64["dbeta"], l32["dbeta"], l64["s_beta"])
        rowc = rows[r].cpu()
        assert torch.equal(rowc[:C].float(), locs[r][0].cpu()) and torch.equal(rowc[C:2 * C].float(), locs[r][1].cpu()), \
            (rcase, "the row and the float sums differ")
        dxo, dro = mk(m), (mk(m) if use_res else None)
        tg, tb = k_bwd_global(dyo, None if remask else yo, mask, xo, mean, invstd, gd, bd, act, p, BC.SEED, rows, inv, dxo, dro)
        if tot0 is None:
            tot0 = (tg, tb)
        else:
            BM.same_bits(tg, tot0[0], rcase + ": sum dgamma against rank 0")
            BM.same_bits(tb, tot0[1], rcase + ": sum dbeta against rank 0")
        for o in (xo, yo, dyo, dxo, dro):
            if o is not None:
                o.check(rcase + " backward")
        dxs.append(dxo.cpu())
        if use_res:
            drs.append(dro.cpu())
    BC.rec_vec(group, case, "sum dgamma", tot0[0].cpu(), r64["dgamma"], r32["dgamma"], r64["s_gamma"])
    BC.rec_vec(group, case, "sum dbeta", tot0[1].cpu(), r64["dbeta"], r32["dbeta"], r64["s_beta"])
    BC.rec_cols(group, case, "dx", torch.cat(dxs), r64["dx1"], r32["dx1"])
    if use_res:
        BC.rec_cols(group, case, "dres", torch.cat(drs), r64["dz"], r32["dz"])


def _chunk_setup(device, case, seed):
    chunks, C, pitch, off = case
    ld = pitch or C
    vals = BC.make_values(sum(chunks), C, seed=seed)
    bounds = np.cumsum((0,) + tuple(chunks))
    sl = [slice(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])]
    xos = [Opd(m, C, ld, off, device, vals["x"][s]) for m, s in zip(chunks, sl)]
    return chunks, C, ld, off, vals, sl, xos


def run_chunks(device, case):
    """an [M, C] operand split into row chunks: local stage per chunk, rows stacked, global stage and apply per chunk, every
    activation / operand combination, against the full-batch oracle"""
    first = len(BC.RECORDS)
    chunks, C, ld, off, vals, sl, xos = _chunk_setup(device, case, 11)
    name = case_name(case)
    rows = torch.stack([k_local_stats(xo) for xo in xos])
    _check_rows(name, rows, chunks, C)
    mean, invstd, inv = _forward_stats(device, "sync chunks", name, chunks, C, vals["x"], rows, xos)
    for combo in COMBOS:
        _combo(device, "sync chunks", name, chunks, sl, C, ld, off, vals, xos, mean, invstd, inv, combo)
    BC.finish(first)


def hand_partials(x, nrows):
    """a conv-epilogue partials table [nrows][2][C] of the rows of x: row i of the table sums the rows i, i + nrows, ... (tables
    with more rows than x has leave the rest zero, as tiles without pixels would)"""
    part = torch.zeros(nrows, 2, x.shape[1], dtype=torch.float64)
    x64 = x.double()
    for i in range(min(nrows, x.shape[0])):
        part[i, 0], part[i, 1] = x64[i::nrows].sum(0), (x64[i::nrows] ** 2).sum(0)
    return part


def run_partials_source(device, case, nrows):
    """rank 0 takes its row from a hand-made partials table, the others from x: the statistics against the oracle"""
    first = len(BC.RECORDS)
    chunks, C, ld, off, vals, sl, xos = _chunk_setup(device, case, 13)
    name = "%s rank 0 from %d partial rows" % (case_name(case), nrows)
    part = hand_partials(vals["x"][sl[0]], nrows).to(device)
    before = part.clone()
    rows = torch.stack([k_local_stats_partials(part, chunks[0])] + [k_local_stats(xo) for xo in xos[1:]])
    assert torch.equal(part, before), (name, "the partials changed")
    _check_rows(name, rows, chunks, C)
    _forward_stats(device, "sync partials", name, chunks, C, vals["x"], rows, xos)
    BC.finish(first)


# ------------------------------------------------------------------------------------------------- 2. one rank changes nothing
def run_one_rank(device, s):
    """one gathered row, statistics from x: bit-identical to segsde_bn_stats / segsde_bn_apply / segsde_bn_backward (saved output,
    remask) / segsde_bn_backward_mask on the same operands"""
    M, C, ld, off = s
    name = BC.spec_name(s) + " one rank"
    vals = BC.make_values(M, C, seed=12)
    x, dy = vals["x"], vals["dy"]
    mk = lambda value=None: Opd(M, C, ld, off, device, value)
    xo = mk(x)
    rm0, rv0 = _running0(x)
    bufs = [(rm0.clone().to(device), rv0.clone().to(device), torch.tensor([7], dtype=torch.int64).to(device)) for _ in range(2)]
    mean_a, invstd_a = BC.k_stats(xo, *bufs[0])
    rows = k_local_stats(xo).reshape(1, -1)
    _check_rows(name, rows, (M,), C)
    mean, invstd, inv = k_global_stats(rows, C, *bufs[1])
    xo.check(name)
    for a, b, what in ((mean, mean_a, "mean"), (invstd, invstd_a, "invstd"), (bufs[1][0], bufs[0][0], "running_mean"),
                       (bufs[1][1], bufs[0][1], "running_var")):
        BM.same_bits(a, b, name + ": " + what)
    assert int(bufs[1][2].cpu()[0]) == int(bufs[0][2].cpu()[0]) == 8, (name, "num_batches_tracked")
    quads = C % 4 == 0 and ld % 4 == 0 and off % 4 == 0
    gd, bd = vals["gamma"].to(device), vals["beta"].to(device)
    dyo = mk(dy)
    # (mode, act, residual, affine, p)
    modes = [("saved", "elu", True, True, 0.0), ("saved", "relu", True, True, 0.0), ("saved", "elu", True, False, BC.P_DROP),
             ("remask", "relu", False, True, 0.0), ("remask", "none", False, False, 0.0)]
    if quads:
        modes.append(("mask", "relu", True, True, 0.0))
    for mode, act, use_res, affine, p in modes:
        what = "%s: %s %s%s%s%s" % (name, mode, act, "+res" if use_res else "", "" if affine else " no affine", " p%.1f" % p if p else "")
        g, b = (gd, bd) if affine else (None, None)
        ro = mk(vals["res"]) if use_res else None
        yo, mask = mk(), None
        if mode == "mask":
            mask = k_apply_mask(xo, mean, invstd, g, b, ro, yo, act)
        else:
            BC.k_apply(xo, mean, invstd, g, b, ro, yo, act, p, BC.SEED)
        ysaved = None if mode == "remask" else yo
        dx_a, dr_a = mk(), (mk() if use_res else None)
        if mode == "mask":
            dg_a, db_a = k_backward_mask(dyo, mask, xo, mean, invstd, g, dx_a, dr_a)
        else:
            dg_a, db_a = BC.k_backward(dyo, ysaved, xo, mean, invstd, g, b, act, p, BC.SEED, 1, dx_a, dr_a)
        row, dg, db = k_bwd_local(dyo, ysaved, mask, xo, mean, invstd, g, b, act, p, BC.SEED, use_res)
        dx, dr = mk(), (mk() if use_res else None)
        tg, tb = k_bwd_global(dyo, ysaved, mask, xo, mean, invstd, g, b, act, p, BC.SEED, row.reshape(1, -1), inv, dx, dr)
        for o in (xo, dyo, yo, ro, dx, dr):
            if o is not None:
                o.check(what)
        BM.same_bits(dg, dg_a, what + " dgamma")
        BM.same_bits(db, db_a, what + " dbeta")
        BM.same_bits(tg, dg_a, what + " sum dgamma")
        BM.same_bits(tb, db_a, what + " sum dbeta")
        BM.same_bits(dx.v, dx_a.v, what + " dx")
        if use_res:
            BM.same_bits(dr.v, dr_a.v, what + " dres")


def run_one_rank_partials(device):
    """one gathered row from a partials table: the bits of segsde_bn_stats_from_partials, at each of its three folds"""
    for nrows, C in ((3, 6), (64, 8), (70, 64), (1100, 20)):
        gen = torch.Generator().manual_seed(31 * nrows + C)
        M = 16 * nrows
        s = torch.randn(nrows, C, generator=gen, dtype=torch.float64) * 4 + 16
        part = torch.stack([s, s * s / 16 + torch.rand(nrows, C, generator=gen, dtype=torch.float64) * 8], 1).contiguous().to(device)
        outs = []
        for sync in (False, True):
            rm, rv = torch.zeros(C).to(device), torch.ones(C).to(device)
            nbt = torch.tensor([3], dtype=torch.int64).to(device)
            if sync:
                mean, invstd, _ = k_global_stats(k_local_stats_partials(part, M).reshape(1, -1), C, rm, rv, nbt)
            else:
                mean, invstd = H.bn_stats_from_partials(part, M, rm, rv, BC.MOM, BC.BN_EPS, num_batches_tracked=nbt)
            assert int(nbt.cpu()[0]) == 4
            outs.append((mean, invstd, rm, rv))
        for a, b, what in zip(outs[1], outs[0], ("mean", "invstd", "running_mean", "running_var")):
            BM.same_bits(a, b, "%d partial rows C%d: %s" % (nrows, C, what))


class count_gathers:
    """counts the calls of torch.distributed.all_gather_into_tensor inside the block"""

    def __enter__(self):
        import torch.distributed as dist
        self.n, self._orig = 0, dist.all_gather_into_tensor

        def counted(*a, **k):
            self.n += 1
            return self._orig(*a, **k)
        dist.all_gather_into_tensor = counted
        return self

    def __exit__(self, *exc):
        import torch.distributed as dist
        dist.all_gather_into_tensor = self._orig
        return False


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_module_one_rank(device, backend):
    """models.layers.SyncBatchNorm2d in a one-rank process group given explicitly (so the collectives run) against BatchNorm2d on the
    same tensors: every output, gradient and buffer bit for bit, in the three backward modes and with dropout; two collectives per
    training call, none in eval mode, none with the default group of one rank"""
    import torch.distributed as dist
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
    dist.init_process_group(backend, init_method="tcp://127.0.0.1:%d" % free_port(), rank=0, world_size=1,
                            timeout=datetime.timedelta(seconds=120))
    try:
        C, shape = 8, (2, 5, 7, 8)
        gen = torch.Generator().manual_seed(77)
        x0, res0, dy0 = (torch.randn(shape, generator=gen) for _ in range(3))
        gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        for act, use_res, p in (("relu", True, 0.0), ("relu", False, 0.0), ("elu", True, 0.0), ("elu", True, 0.3)):
            outs = []
            for kind in ("plain", "sync", "default group"):
                bn = L.BatchNorm2d(C) if kind == "plain" else L.SyncBatchNorm2d(C, process_group=dist.group.WORLD if kind == "sync" else None)
                with torch.no_grad():
                    bn.weight.copy_(gamma)
                    bn.bias.copy_(beta)
                bn.to(device).train()
                leaf = lambda t: t.clone().to(device).requires_grad_(True)
                x, res = leaf(x0), (leaf(res0) if use_res else None)
                torch.manual_seed(5)                  # the dropout seed is drawn from the CPU generator
                with count_gathers() as cnt:
                    y = bn(x, residual=res, act=act, drop_p=p)
                    y.backward(dy0.to(device))
                assert cnt.n == (2 if kind == "sync" else 0), (kind, act, cnt.n)
                bn.eval()
                with count_gathers() as cnt:
                    xe = leaf(x0)
                    ye = bn(xe, residual=res.detach() if use_res else None, act=act)
                    ye.backward(dy0.to(device))
                assert cnt.n == 0, (kind, "eval mode issued a collective")
                outs.append(dict(y=y.detach(), dx=x.grad, dres=None if res is None else res.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                                 rm=bn.running_mean, rv=bn.running_var, ye=ye.detach(), dxe=xe.grad))
                assert int(bn.num_batches_tracked) == 1
            for kind, o in zip(("sync", "default group"), outs[1:]):
                for k, v in o.items():
                    if v is not None:
                        BM.same_bits(v, outs[0][k], "%s %s%s p%.1f: %s" % (kind, act, "+res" if use_res else "", p, k))
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------ 4. conversion
def run_conversion():
    """ddp.convert_sync_batchnorm on the R18 joint model; launches no kernel"""
    import model_cases as MC
    from improving_segmentation_with_selfsupervised_depth_amd import ddp
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
    cfg = MC.contract_cfgs()["cfgs"]["r18_jsd"]
    torch.manual_seed(3)
    m = get_model(cfg, 19)
    checkpoint = {k: v.clone() for k, v in get_model(cfg, 19).state_dict().items()}      # saved before any conversion
    keys = list(m.state_dict().keys())
    named = list(m.named_parameters())
    buffers = list(m.named_buffers())
    opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)
    is_sync = lambda mod: {n for n, b in mod.named_modules() if isinstance(b, L.SyncBatchNorm2d)}
    all_bn = {n for n, b in m.named_modules() if isinstance(b, L.BatchNorm2d)}
    enc_bn = {n for n in all_bn if n.startswith("models.encoder.")}
    pose_bn = {n for n in all_bn if n.startswith("models.pose")}
    assert enc_bn and pose_bn and len(all_bn) > len(enc_bn) + len(pose_bn)
    assert not is_sync(m)
    assert ddp.convert_sync_batchnorm(m, only=["encoder"]) is m
    assert is_sync(m) == enc_bn
    ddp.convert_sync_batchnorm(m)
    assert is_sync(m) == all_bn - pose_bn, "the pose networks are converted only when asked"
    marker = object()
    for b in m.modules():
        if isinstance(b, L.SyncBatchNorm2d):
            assert b.process_group is None
            b.process_group = marker
    ddp.convert_sync_batchnorm(m, only=["pose_encoder", "pose"])
    assert is_sync(m) == all_bn
    ddp.convert_sync_batchnorm(m)                     # twice: a no-op
    assert is_sync(m) == all_bn
    assert all(b.process_group is marker for n, b in m.named_modules() if n in all_bn - pose_bn)
    try:
        ddp.convert_sync_batchnorm(m, only=["no such sub-model"])
        raise AssertionError("an unknown sub-model name was accepted")
    except KeyError:
        pass
    assert list(m.state_dict().keys()) == keys
    now = list(m.named_parameters())
    assert [k for k, _ in now] == [k for k, _ in named] and all(a is b for (_, a), (_, b) in zip(now, named))
    assert all(a is b for (_, a), (_, b) in zip(m.named_buffers(), buffers)) and len(buffers) == len(list(m.named_buffers()))
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], m.parameters()))
    for b in m.modules():
        if isinstance(b, L.SyncBatchNorm2d):
            b.process_group = None
    res = m.load_state_dict(checkpoint, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, checkpoint[k]) for k, v in m.state_dict().items())
    # outside an initialised process group the converted module is BatchNorm2d
    assert all(b._group() is None for b in m.modules() if isinstance(b, L.SyncBatchNorm2d))


# ------------------------------------------------------------------------------------------------------------- 5. GPU integration
def run_integration(device, backend):
    """A one-rank process group around the real ResNet-18 joint model at the smallest size tests/model_cases.py uses: the model
    converted with the group given explicitly (so every BatchNorm outside the pose networks runs the four stages and both
    collectives), GradAllReducer around it, one forward and the two backward() calls of trainer.train_step.  Losses, every parameter
    gradient and every buffer equal those of the unconverted model bit for bit: with one gathered row both statistics sources
    reproduce the single-process folds, so the conv-epilogue hand-off stays (the fusion counters are compared too) and no layer
    falls back to a tolerance."""
    import torch.distributed as dist
    import bench
    import model_cases as MC
    from oracle import nets as N
    from improving_segmentation_with_selfsupervised_depth_amd import ddp
    from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss
    from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import cross_entropy2d
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
    cfg = MC.contract_cfgs()["cfgs"]["r18_jsd"]
    sd = N.build_state_dict(cfg, 19, seed=3, randomize_bn=True)
    B, Hh, W = 2, 64, 128
    _, inp = MC._bench_inputs(B, Hh, W, 17, device)
    gen = torch.Generator().manual_seed(4)
    noise = {s: torch.randn(B, 2, Hh, W, generator=gen) for s in range(4)}
    dist.init_process_group(backend, init_method="tcp://127.0.0.1:%d" % free_port(), rank=0, world_size=1,
                            timeout=datetime.timedelta(seconds=120))
    try:
        outs = []
        for convert in (False, True):
            m = get_model(cfg, 19)
            m.load_state_dict(sd, strict=True)
            m.to(device).train()
            MC.dropout_eval(m)
            if convert:
                ddp.convert_sync_batchnorm(m, process_group=dist.group.WORLD)
            n_sync = sum(isinstance(b, L.SyncBatchNorm2d) for b in m.modules())
            assert (n_sync > 20) == convert
            lo = get_monodepth_loss(bench.loss_cfg(B, Hh, W), True)
            lo.tiebreak_noise = noise
            red = ddp.GradAllReducer(m, bucket_mb=4.0, always=True)
            torch.manual_seed(23)
            Fn.fusion_report(reset=True)
            with count_gathers() as cnt:
                out = m(inp)
                lo.generate_images_pred(inp, out)
                mono = lo.compute_losses(inp, out)["loss"]
                seg = cross_entropy2d(out["semantics"], inp["lbl"])
                with red.no_sync():
                    mono.backward(retain_graph=True)
                seg.backward()
            red.finish()
            outs.append(dict(mono=mono.detach().clone(), seg=seg.detach().clone(), gathers=cnt.n, fusion=Fn.fusion_report(reset=True),
                             grads={k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()},
                             bufs={k: b.detach().clone() for k, b in m.named_buffers()}))
            red.close()
        base, got = outs
        assert base["gathers"] == 0 and got["gathers"] >= 2 * 20 and got["gathers"] % 2 == 0, (base["gathers"], got["gathers"])
        assert got["fusion"] == base["fusion"], (got["fusion"], base["fusion"])
        BM.same_bits(got["mono"], base["mono"], "monodepth loss")
        BM.same_bits(got["seg"], base["seg"], "segmentation loss")
        for k, a in base["grads"].items():
            b = got["grads"][k]
            assert (a is None) == (b is None), k
            if a is not None:
                BM.same_bits(b, a, "gradient of " + k)
        for k, a in base["bufs"].items():
            assert torch.equal(got["bufs"][k], a), "buffer " + k
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------ 3. two and three ranks over gloo, CPU
GLOO_STEPS = 3                    # two plain training steps, then one with two backward() calls on the shared trunk
# The stack is compared END TO END (four layers forward, four backward, the statistics recomputed by each reference from its own
# activations), not stage by stage from shared fp32 inputs as above.  Its worst ratio under the interpreter is 3.72 (dres, three
# ranks, first step; 1.51 with two ranks), above K / 2 = 2: by the rule of tests/batchnorm_cases.py (the smallest power of two that
# is at least twice the worst ratio, 8 at the most) the stack is held to 8.  The stage-level cases keep K = 4 (worst on the MI355X:
# 1.45).  profiles/sync_bn.md has the figures.
K_STACK = 8.0
GLOO_LR = 0.05
PARAMS = ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias")
BUFFERS = ("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")


def make_stack():
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L

    class Stack(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = L.Conv2d(4, 6, 3, padding=1, bias=False)
            self.bn1 = L.BatchNorm2d(6)
            self.conv2 = L.Conv2d(6, 8, 1, bias=False)
            self.bn2 = L.BatchNorm2d(8)

        def forward(self, x, res):
            h = self.bn1(self.conv1(x), residual=res, act="relu")
            return self.bn2(self.conv2(h), act="elu")
    torch.manual_seed(5)
    net = Stack()
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for bn in (net.bn1, net.bn2):
            bn.weight.copy_(torch.randn(bn.num_features, generator=gen))
            bn.weight[::3] = -bn.weight[::3].abs() - 0.1
            bn.bias.copy_(torch.randn(bn.num_features, generator=gen))
    return net


def gloo_data(total):
    """per step: x [B, 8, 8, 4], res [B, 8, 8, 6], loss weights w [B, 8, 8, 8] (loss_r = sum(out_r * w_r)) and the 0 / 1 pattern that
    splits w between the two backward() calls of the last step; B = the global batch"""
    gen = torch.Generator().manual_seed(8)
    return [dict(x=torch.randn(total, 8, 8, 4, generator=gen) * 1.5 + 0.5, res=torch.randn(total, 8, 8, 6, generator=gen),
                 w=torch.randn(total, 8, 8, 8, generator=gen), split=(torch.rand(total, 8, 8, 8, generator=gen) < 0.5).float())
            for _ in range(GLOO_STEPS)]


def _gloo_body(rank, world, batches, convert):
    import torch.distributed as dist
    from improving_segmentation_with_selfsupervised_depth_amd import ddp
    net = make_stack()
    if convert:
        ddp.convert_sync_batchnorm(net)
    red = ddp.GradAllReducer(net, bucket_mb=0.001)
    data = gloo_data(sum(batches))
    lo = sum(batches[:rank])
    hi = lo + batches[rank]
    saved = []
    orig_global = H.bn_sync_stats_global

    def recording(*a, **k):
        out = orig_global(*a, **k)
        saved.append((out[0].clone(), out[1].clone()))
        return out
    H.bn_sync_stats_global = recording
    steps = []
    net.train()
    for step, d in enumerate(data):
        rec = dict(params0={k: p.detach().clone() for k, p in net.named_parameters()},
                   bufs0={k: b.detach().clone() for k, b in net.named_buffers()})
        net.zero_grad(set_to_none=True)
        x, res = d["x"][lo:hi].clone().requires_grad_(True), d["res"][lo:hi].clone().requires_grad_(True)
        w = d["w"][lo:hi]
        del saved[:]
        with count_gathers() as cnt:
            out = net(x, res)
            if step == GLOO_STEPS - 1:           # as train_step: the first backward() keeps the graph and the reducer back
                wa = w * d["split"][lo:hi]
                with red.no_sync():
                    (out * wa).sum().backward(retain_graph=True)
                (out * (w - wa)).sum().backward()
            else:
                (out * w).sum().backward()
        red.finish()
        rec.update(out=out.detach().clone(), dx=x.grad.clone(), dres=res.grad.clone(), gathers=cnt.n,
                   grads={k: p.grad.detach().clone() for k, p in net.named_parameters()},
                   bufs={k: b.detach().clone() for k, b in net.named_buffers()}, saved=[(a.clone(), b.clone()) for a, b in saved])
        steps.append(rec)
        with torch.no_grad():
            for p in net.parameters():
                p -= GLOO_LR * p.grad
    # eval mode: no collective, forward or backward
    net.eval()
    d = data[0]
    x, res = d["x"][lo:hi].clone().requires_grad_(True), d["res"][lo:hi].clone().requires_grad_(True)
    net.zero_grad(set_to_none=True)
    with count_gathers() as cnt:
        (net(x, res) * d["w"][lo:hi]).sum().backward()
    red.finish()
    dist.barrier()
    return dict(steps=steps, eval_gathers=cnt.n)


def _gloo_worker(rank, world, port, outdir, batches, convert):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    import emu
    emu.install()
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=90))
    try:
        torch.save(_gloo_body(rank, world, batches, convert), os.path.join(outdir, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


_GLOO_RUNS = {}


def gloo_run(batches, convert=True, limit=300.0):
    """the workers' records, [rank]; every worker under a time limit, and a failed rank ends all of them"""
    key = (tuple(batches), bool(convert))
    if key in _GLOO_RUNS:
        return _GLOO_RUNS[key]
    import torch.multiprocessing as mp
    world = len(batches)
    with tempfile.TemporaryDirectory() as outdir:
        ctx = mp.spawn(_gloo_worker, args=(world, free_port(), outdir, tuple(batches), bool(convert)), nprocs=world, join=False)
        deadline = time.time() + limit
        try:
            while not ctx.join(timeout=2.0):          # raises when a worker failed, after ending the others
                if time.time() > deadline:
                    raise TimeoutError("the gloo workers did not finish within %.0f s" % limit)
        finally:
            for p in ctx.processes:
                if p.is_alive():
                    p.terminate()
            for p in ctx.processes:
                p.join(10)
        out = [torch.load(os.path.join(outdir, "rank%d.pt" % r), weights_only=False) for r in range(world)]
    _GLOO_RUNS[key] = out
    return out


class _RefBN(torch.autograd.Function):
    """training-mode BatchNorm of an [M, C] tensor by the formulas of batchnorm_cases.ref_stats / ref_apply / ref_backward, in the
    dtype of its input: the float32 reference is then float32 throughout (F.batch_norm on the CPU keeps its float32 statistics in
    double accumulators, which the rule's "same formulas in float32" does not mean).  -> gamma * xhat + beta; xhat is kept on
    ctx.owner for the gradient scales; the running buffers are updated in place"""

    @staticmethod
    def forward(ctx, z, gamma, beta, rm, rv, owner):
        M = z.shape[0]
        mu = z.sum(0) / M
        var = ((z - mu) ** 2).sum(0) / M
        invstd = 1 / torch.sqrt(var + BC.BN_EPS)
        rm.copy_((1 - BC.MOM) * rm + BC.MOM * mu)
        rv.copy_((1 - BC.MOM) * rv + BC.MOM * (var * M / (M - 1)))
        xh = (z - mu) * invstd
        ctx.save_for_backward(xh, invstd, gamma)
        owner["xh"] = xh
        return xh * gamma + beta

    @staticmethod
    def backward(ctx, dz):
        xh, invstd, gamma = ctx.saved_tensors
        M = xh.shape[0]
        dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
        return invstd * gamma * (dz - dbeta / M - xh * dgamma / M), dgamma, dbeta, None, None, None


def stack_oracle(dt, P, Bf, x, res, w):
    """the stack on the whole global batch in plain torch (convolutions in NCHW, BatchNorm on [M, C]), loss = sum(out * w) = the
    sum of the ranks' losses"""
    leaf = lambda t: t.detach().clone().to(dt).requires_grad_(True)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])           # NCHW -> [M, C]
    xx, rr = leaf(x), leaf(res)                                              # NHWC leaves: their gradients come out [B, H, W, C]
    p = {k: leaf(P[k]) for k in PARAMS}
    b = {k: Bf[k].detach().clone().to(dt) for k in BUFFERS}
    o1, o2 = {}, {}
    z1 = F.conv2d(nchw(xx), p["conv1.weight"], padding=1)
    t1 = _RefBN.apply(rows(z1), p["bn1.weight"], p["bn1.bias"], b["bn1.running_mean"], b["bn1.running_var"], o1)
    h = BC.act_fn(t1 + rr.reshape(-1, rr.shape[-1]), "relu")                 # [M, 6]
    hh = h.reshape(x.shape[0], x.shape[1], x.shape[2], -1)
    z2 = F.conv2d(nchw(hh), p["conv2.weight"])
    t2 = _RefBN.apply(rows(z2), p["bn2.weight"], p["bn2.bias"], b["bn2.running_mean"], b["bn2.running_var"], o2)
    out = F.elu(t2)
    for t in (z1, t1, z2, t2):
        t.retain_grad()
    (out * w.reshape(-1, w.shape[-1]).to(dt)).sum().backward()
    flat = lambda t: t.detach().reshape(-1, t.shape[-1])
    r = dict(out=out.detach(), dx=flat(xx.grad), dres=flat(rr.grad), grads={k: p[k].grad.detach() for k in PARAMS}, bufs=b)
    sums = lambda t: t.detach().abs().sum(0)
    r["scale"] = {"bn1.weight": sums(t1.grad * o1["xh"]), "bn1.bias": sums(t1.grad), "bn2.weight": sums(t2.grad * o2["xh"]),
                  "bn2.bias": sums(t2.grad),
                  "conv1.weight": torch.nn.grad.conv2d_weight(nchw(xx).detach().abs(), p["conv1.weight"].shape, z1.grad.abs(), padding=1),
                  "conv2.weight": torch.nn.grad.conv2d_weight(nchw(hh).detach().abs(), p["conv2.weight"].shape, z2.grad.abs())}
    return r


def gloo_compare(batches, convert=True):
    """every rank's outputs, input gradients and averaged parameter gradients and the running buffers of every step against the
    full-batch oracle (from the parameters and buffers the step started with, the ranks' own fp32 values); -> the records
    (group, case, tensor, channel, e_kernel, unit, ratio, _), taken off batchnorm_cases.RECORDS: the caller holds them to K_STACK"""
    runs = gloo_run(batches, convert)
    world, data = len(batches), gloo_data(sum(batches))
    group = "gloo %s%s" % ("+".join(str(b) for b in batches), "" if convert else " unconverted")
    first = len(BC.RECORDS)
    for step, d in enumerate(data):
        recs = [r["steps"][step] for r in runs]
        for r in range(1, world):
            for k in PARAMS:
                BM.same_bits(recs[r]["params0"][k], recs[0]["params0"][k], "step %d rank %d: parameter %s" % (step, r, k))
        r64, r32 = (stack_oracle(dt, recs[0]["params0"], recs[0]["bufs0"], d["x"], d["res"], d["w"]) for dt in (torch.float64, torch.float32))
        case = "step %d" % step
        flat = lambda t: t.reshape(-1, t.shape[-1])
        for name in ("out", "dx", "dres"):
            BC.rec_cols(group, case, name, torch.cat([flat(rec[name]) for rec in recs]), r64[name], r32[name])
        for r, rec in enumerate(recs):
            for k in PARAMS:
                # the reducer's average over the ranks, times the number of ranks: the gradient of the sum of the ranks' losses
                BC.rec_vec(group, case + " rank %d" % r, "grad " + k, rec["grads"][k].double().reshape(-1) * world, r64["grads"][k].reshape(-1),
                           r32["grads"][k].reshape(-1), r64["scale"][k].reshape(-1))
            for k in BUFFERS:
                BC.rec_vec(group, case + " rank %d" % r, k, rec["bufs"][k], r64["bufs"][k], r32["bufs"][k], r64["bufs"][k].abs())
    rows = BC.RECORDS[first:]
    del BC.RECORDS[first:]
    return rows


def stack_worst(rows):
    worst = {}
    for g, _, t, _, _, _, r, _ in rows:
        worst[(g, t)] = max(worst.get((g, t), 0.0), r)
    for (g, t), r in sorted(worst.items()):
        print("BN-EDGE-WORST | %s | %s | %.2f" % (g, t, r))
    return worst
