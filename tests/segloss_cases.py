"""The segmentation loss kernels (csrc/segmix.hip: cross-entropy forward / backward in their dense and strided forms, pseudo_label,
confusion_update; csrc/depthmix.hip: the teacher softmax and the min-max normalisation) against plain torch in float64, at the shapes
and values that random 19-class logits of one small tile do not reach: ragged multi-tile launches, class counts on either side of
the dense limit, pitched and misaligned views, class and pixel weights, offset and saturated logits, threshold / tie / signed-zero
pixels.  Shared by tests/test_segloss_gpu.py (real library) and tests/test_segloss_emu.py (interpreter build of the same sources).

References: ``F.cross_entropy(reduction="none")``, ``torch.softmax``, ``torch.max`` and oracle/segmix.py / oracle/metrics.py, in
float64 (the truth) and in float32 on the CPU (what the reference's own arithmetic achieves, ``e_ref``).  No tolerance is a constant:

* per-pixel loss: ``r = max_m |nll - nll64| / (1 + nll64)``; ``r_kernel <= K * max(r_fp32, 2^-23)``
* sums of per-pixel terms (the kernels add fp32 terms in double): ``|num - num64| <= K * max(r_fp32, 2^-23) * sum_m w_m (1 + nll64_m)``.
  The double sum is rounded to fp32 once (2^-24 relative, within the floor's share of the bound)
* gradients and softmax: ``max |g - g64| <= K * max(max |g_fp32 - g64|, 2^-23 * max |scale * w|)``

K (below) and the figures it comes from are in profiles/segloss_edges.md.  Integer and selection outputs are compared exactly.  The
only pixels left out of a comparison are those with an ignored target, known from the inputs."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import metrics as OM, segmix as OS
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

IGN = 250
EPS = 2.0 ** -23
# smallest power of two that is at least twice the worst ratio of the MI355X run (profiles/segloss_edges.md); 8 at the most
K = 8.0

RECORDS = []            # (group, case, tensor, e_kernel, unit, ratio, ok); ``unit`` is the figure that K multiplies


def record(group, case, tensor, e_k, unit):
    ratio = 0.0 if e_k == 0 else (e_k / unit if unit > 0 else float("inf"))
    ok = bool(np.isfinite(e_k)) and ratio <= K
    RECORDS.append((group, case, tensor, e_k, unit, ratio, ok))
    print("SEGLOSS | %s | %s | %s | %.3e | %.3e | %.2f | %s" % (group, case, tensor, e_k, unit, ratio, "ok" if ok else "MISSES THE RULE"))
    return ok


def finish(first):
    rows = RECORDS[first:]
    worst = {}
    for g, _, t, _, _, r, _ in rows:
        worst[(g, t)] = max(worst.get((g, t), 0.0), r)
    for (g, t), r in sorted(worst.items()):
        print("SEGLOSS-WORST | %s | %s | %.2f" % (g, t, r))
    bad = [r for r in rows if not r[-1]]
    assert not bad, "error against float64 above K = %g times the fp32 reference's: %s" % (K, bad)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------------- cross-entropy reference
def ce_reference(dtype, x, t, cw, pw, scale):
    """per-pixel nll (unweighted), weights w_m = cw[t_m] * pw_m (0 on ignored pixels), num = sum w nll, den = sum cw[t] over the
    kept pixels, and d (scale * num) / d x by autograd, all in ``dtype`` on the CPU"""
    xx = x.detach().to(dtype).requires_grad_(True)
    nll = F.cross_entropy(xx, t, reduction="none", ignore_index=IGN)
    keep = t != IGN
    w = torch.ones(t.numel(), dtype=dtype)
    if cw is not None:
        w = cw.to(dtype)[torch.where(keep, t, torch.zeros_like(t))]
    den = torch.where(keep, w, torch.zeros_like(w)).sum()
    if pw is not None:
        w = w * pw.to(dtype)
    w = torch.where(keep, w, torch.zeros_like(w))
    num = (w * nll).sum()
    (num * float(scale)).backward()
    return dict(nll=nll.detach(), w=w, num=num.detach(), den=den, grad=xx.grad, keep=keep)


def pixel_ratio_unit(r32, r64):
    """max(r_fp32, 2^-23) over the kept pixels (2^-23 where none is kept)"""
    keep = r64["keep"]
    if not bool(keep.any()):
        return EPS
    r = ((r32["nll"].double() - r64["nll"]).abs() / (1 + r64["nll"]))[keep].max()
    return max(float(r), EPS)


def check_ce(group, case, out, dl, r32, r64, scale):
    """out = (num, den) and dl of the kernels against the two references; exact: den, rows of ignored pixels"""
    keep = r64["keep"]
    out, dl = out.detach().cpu(), dl.detach().cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all()), (group, case, "not finite")
    assert float(out[1]) == float(r64["den"].float()), (group, case, "denominator", float(out[1]), float(r64["den"]))
    assert bool((dl[~keep] == 0).all()), (group, case, "rows of ignored pixels carry gradient")
    unit = pixel_ratio_unit(r32, r64)
    ok = record(group, case, "num", abs(float(out[0].double() - r64["num"])), unit * float((r64["w"] * (1 + r64["nll"])).sum()))
    e_ref = float((r32["grad"].double() - r64["grad"]).abs().max())
    wmax = float(r64["w"].abs().max()) * abs(float(scale))
    ok &= record(group, case, "grad", float((dl.double() - r64["grad"]).abs().max()), max(e_ref, EPS * wmax))
    return ok


# --------------------------------------------------------------------------------------------------------------- A: the sweep
CS = (1, 3, 19, 20, 64, 65)             # 20: CE_PIX * C even; 64: the last dense size; 65: the first that falls back
MS = (1, 255, 256, 257, 700)
VIEWS = ("dense", "pitched", "offset")
TMODES = ("none", "some", "tail", "all")
OPTS = [(cw, pw, tm) for cw in (False, True) for pw in (False, True) for tm in TMODES]


def path_of(view, C):
    return "dense" if view == "dense" and C <= 64 else "strided"


def sweep_plan():
    """every (view, C, M) with two of the sixteen (class_weight, pixel_weights, targets) settings, chosen by position so that
    every value of every axis meets both kernel paths (``assert_coverage``)"""
    plan = []
    for i, (view, C, M) in enumerate(itertools.product(VIEWS, CS, MS)):
        for rep in range(2):
            plan.append((view, C, M) + OPTS[(2 * i + rep) % len(OPTS)])
    return plan


def assert_coverage(plan):
    for path in ("dense", "strided"):
        rows = [p for p in plan if path_of(p[0], p[1]) == path]
        want = dict(C=set(c for c in CS if c <= 64 or path == "strided"), M=set(MS), cw={False, True}, pw={False, True}, tm=set(TMODES),
                    view={"dense"} if path == "dense" else set(VIEWS))
        got = dict(view=set(p[0] for p in rows), C=set(p[1] for p in rows), M=set(p[2] for p in rows), cw=set(p[3] for p in rows),
                   pw=set(p[4] for p in rows), tm=set(p[5] for p in rows))
        assert got == want, (path, got)
        assert set((p[2], p[5]) for p in rows) == set(itertools.product(MS, TMODES)), (path, "M x targets")
        for col in (3, 4):                     # every C with class_weight / pixel_weights off and on
            assert set((p[1], p[col]) for p in rows) == set(itertools.product(want["C"], (False, True))), (path, col)


def make_targets(gen, M, C, mode):
    t = torch.randint(0, C, (M,), generator=gen)
    if mode == "some":
        t[torch.rand(M, generator=gen) < 0.2] = IGN
    elif mode == "tail":                       # every pixel of the last (ragged) 256-pixel tile
        t[256 * ((M - 1) // 256):] = IGN
    elif mode == "all":
        t[:] = IGN
    return t


def make_view(x, view, device, gen):
    """-> (the [M,C] view handed to the kernels, the buffer it lives in)"""
    M, C = x.shape
    if view == "dense":
        buf = x.to(device).contiguous()
        v = buf
        assert v.data_ptr() % 16 == 0
    elif view == "pitched":                    # columns 2 .. 2+C of a buffer of pitch C + 5
        wide = torch.randn(M, C + 5, generator=gen)
        wide[:, 2:2 + C] = x
        buf = wide.to(device)
        v = buf[:, 2:2 + C]
        assert v.stride(0) == C + 5 or M == 1
    else:                                      # dense rows, one float into the buffer: the base is not 16-byte aligned
        flat = torch.randn(M * C + 4, generator=gen)
        flat[1:1 + M * C] = x.reshape(-1)
        buf = flat.to(device)
        v = buf[1:1 + M * C].view(M, C)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    assert torch.equal(v.cpu(), x)
    return v, buf


def run_ce(device, x, t, cw, pw, scale, view, gen):
    """the two kernels on ``x`` seen through ``view``; the buffer (padding and logits) must come back unchanged"""
    v, buf = make_view(x, view, device, gen)
    before = buf.clone()
    d = lambda a: None if a is None else a.to(device)
    tt, cwd, pwd = d(t), d(cw), d(pw)
    out = H.cross_entropy_forward(v, tt, IGN, cwd, pwd)
    dl = H.cross_entropy_backward(v, tt, IGN, torch.tensor([scale], dtype=torch.float32).to(device), cwd, pwd)
    assert tuple(dl.shape) == tuple(x.shape) and dl.is_contiguous()
    assert torch.equal(buf, before), "the source buffer changed"
    return out, dl


def run_sweep(device):
    first = len(RECORDS)
    plan = sweep_plan()
    assert_coverage(plan)
    for i, (view, C, M, use_cw, use_pw, tm) in enumerate(plan):
        gen = _gen(1000 + i)
        x = torch.randn(M, C, generator=gen) * 10 + 30
        t = make_targets(gen, M, C, tm)
        cw = torch.rand(C, generator=gen) + 0.5 if use_cw else None
        pw = torch.rand(M, generator=gen) + 0.25 if use_pw else None
        scale = float(torch.tensor(1.0 / M, dtype=torch.float32))
        r64, r32 = ce_reference(torch.float64, x, t, cw, pw, scale), ce_reference(torch.float32, x, t, cw, pw, scale)
        out, dl = run_ce(device, x, t, cw, pw, scale, view, gen)
        name = "%s C%d M%d %s%s %s" % (view, C, M, "c" if use_cw else "-", "p" if use_pw else "-", tm)
        check_ce("A " + path_of(view, C), name, out, dl, r32, r64, scale)
        if not use_cw:
            assert float(out[1]) == float(int((t != IGN).sum())), (name, "count")
        if tm == "all":
            assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and bool((dl == 0).all()), (name, "all pixels ignored")
    finish(first)


# ------------------------------------------------------------------------------------- B: per-pixel loss at offset logits
SHIFTS = (0.0, 40.0, 300.0, -60.0)
SPREADS = (1.0, 8.0, 30.0)
B_C, B_M = 19, 257                      # two tiles, the second ragged (one pixel)


def b_inputs(shift, spread):
    gen = _gen(int(7 + 13 * SHIFTS.index(shift) + SPREADS.index(spread)))
    x = torch.randn(B_M, B_C, generator=gen) * spread + shift
    t = torch.randint(0, B_C, (B_M,), generator=gen)
    confident = torch.rand(B_M, generator=gen) < 0.5          # the arg-max as target: the near-zero-loss regime
    t = torch.where(confident, x.argmax(1), t)
    t[torch.rand(B_M, generator=gen) < 0.2] = IGN
    t[B_M - 1] = int(x[B_M - 1].argmax())                      # the pixel of the ragged tile is kept
    return x, t


def probe_pixels(device, v, t, kept):
    """one launch per kept pixel with a one-hot pixel_weights vector: out[0] is that pixel's loss, read at its real place"""
    tt = t.to(device)
    pw = torch.zeros(t.numel(), dtype=torch.float32).to(device)
    res = torch.zeros(len(kept), dtype=torch.float32).to(device)
    for j, m in enumerate(kept):
        pw[m] = 1.0
        res[j] = H.cross_entropy_forward(v, tt, IGN, None, pw)[0]
        pw[m] = 0.0
    return res.cpu()


def run_pixel_case(device, shift, spread, views=("dense", "pitched")):
    first = len(RECORDS)
    x, t = b_inputs(shift, spread)
    keep = t != IGN
    kept = [int(m) for m in torch.nonzero(keep).reshape(-1)]
    assert 180 <= len(kept) <= 230 and B_M - 1 in kept
    nll64 = F.cross_entropy(x.double(), t, reduction="none", ignore_index=IGN)[keep]
    nll32 = F.cross_entropy(x, t, reduction="none", ignore_index=IGN)[keep]
    rel = lambda a: float(((a.double() - nll64).abs() / (1 + nll64)).max())
    unit = max(rel(nll32), EPS)
    for view in views:
        v, _ = make_view(x, view, device, _gen(3))
        got = probe_pixels(device, v, t, kept)
        assert bool(torch.isfinite(got).all())
        record("B " + path_of(view, B_C), "shift %g spread %g" % (shift, spread), "nll", rel(got), unit)
    finish(first)


def run_saturated_rows(device):
    """[1e4, -1e4, 0, ...] with the high and the low class as target: exp underflows to 0 in float64 as well, so the loss
    (0 and 2e4) and the gradient are exact, and the gradient is 0 wherever the softmax is"""
    x = torch.zeros(2, B_C)
    x[:, 0], x[:, 1] = 1e4, -1e4
    t = torch.tensor([0, 1])
    r64 = ce_reference(torch.float64, x, t, None, None, 1.0)
    assert r64["nll"].tolist() == [0.0, 2e4] and bool((r64["grad"][:, 2:] == 0).all()) and float(r64["grad"][0].abs().max()) == 0.0
    for view in VIEWS:
        out, dl = run_ce(device, x, t, None, None, 1.0, view, _gen(4))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all()), view
        assert float(out[0]) == 2e4 and float(out[1]) == 2.0, (view, out)
        assert torch.equal(dl.cpu().double(), r64["grad"]), (view, dl)
        v, _ = make_view(x, view, device, _gen(4))
        assert probe_pixels(device, v, t, [0, 1]).tolist() == [0.0, 2e4], view


# ----------------------------------------------------------------------------------------------- C: grid-stride (GPU only)
def run_grid_stride_ce(device):
    """M = 1024 * 256 + 300: every block of the capped grid takes a second tile, the last tile is ragged"""
    first = len(RECORDS)
    M, C = 1024 * 256 + 300, 19
    gen = _gen(21)
    x = torch.randn(M, C, generator=gen) * 10 + 30
    t = make_targets(gen, M, C, "some")
    cw, pw = torch.rand(C, generator=gen) + 0.5, torch.rand(M, generator=gen) + 0.25
    scale = float(torch.tensor(1.0 / M, dtype=torch.float32))
    r64, r32 = ce_reference(torch.float64, x, t, cw, pw, scale), ce_reference(torch.float32, x, t, cw, pw, scale)
    for view in ("dense", "pitched"):
        out, dl = run_ce(device, x, t, cw, pw, scale, view, gen)
        check_ce("C " + path_of(view, C), "M %d" % M, out, dl, r32, r64, scale)
    out, _ = run_ce(device, x, t, None, None, scale, "dense", gen)
    assert float(out[1]) == float(int((t != IGN).sum()))
    finish(first)


def run_grid_stride_pseudo_label(device):
    B, C, HW = 3, 3, (4096 * 256 + 77) // 3
    assert B * HW == 4096 * 256 + 77
    prob = torch.softmax(torch.randn(B, C, 1, HW, generator=_gen(22)) * 4, dim=1)
    check_pseudo_label(device, prob)


# ---------------------------------------------------------------------------------------- D: cross_entropy2d through autograd
def d_reference(dtype, logits, target, cw, pw):
    """oracle.segmix.cross_entropy2d with autograd, and the per-pixel terms of the same chain (resize included)"""
    x = logits.detach().to(dtype).requires_grad_(True)
    c = lambda a: None if a is None else a.to(dtype)
    loss = OS.cross_entropy2d(x, target, c(cw), c(pw))
    loss.backward()
    with torch.no_grad():
        y = x.detach()
        if y.shape[2] != target.shape[1] and y.shape[3] != target.shape[2]:
            y = F.interpolate(y, size=tuple(target.shape[1:]), mode="bilinear", align_corners=True)
        t = target.reshape(-1)
        nll = F.cross_entropy(y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]), t, reduction="none", ignore_index=IGN)
        keep = t != IGN
        w = torch.ones(t.numel(), dtype=dtype) if cw is None else c(cw)[torch.where(keep, t, torch.zeros_like(t))]
        den = torch.where(keep, w, torch.zeros_like(w)).sum()
        if pw is not None:
            den = torch.tensor(float(t.numel()), dtype=dtype)
            if not bool(torch.isnan(pw).any()):
                w = w * c(pw).reshape(-1)
        w = torch.where(keep, w, torch.zeros_like(w))
    return dict(loss=loss.detach(), grad=x.grad, nll=nll, w=w, den=den, keep=keep)


def run_ce2d_case(device, name, logits, target, cw=None, pw=None, channels_last=False):
    from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import cross_entropy2d
    r64, r32 = d_reference(torch.float64, logits, target, cw, pw), d_reference(torch.float32, logits, target, cw, pw)
    lg = logits.to(device)
    if channels_last:
        lg = lg.contiguous(memory_format=torch.channels_last)
    lg = lg.clone(memory_format=torch.preserve_format).requires_grad_(True)
    d = lambda a: None if a is None else a.to(device)
    loss = cross_entropy2d(lg, d(target), d(cw), d(pw))
    loss.backward()
    got, grad = loss.detach().cpu().double(), lg.grad.detach().cpu().double()
    if not bool(r64["keep"].any()):            # whatever the oracle gives (0 / 0)
        assert (bool(torch.isnan(got)) and bool(torch.isnan(r64["loss"]))) or float(got) == float(r64["loss"]), (name, got, r64["loss"])
        assert torch.equal(torch.isnan(grad), torch.isnan(r64["grad"])) and torch.equal(grad.nan_to_num(), r64["grad"].nan_to_num()), name
        print("SEGLOSS | D | %s | loss %s, gradient all %s as the oracle's" % (name, float(got), float(grad.reshape(-1)[0])))
        return
    # the mean is a sum of per-pixel terms over den: the float64 loss of the oracle is that sum
    unit = pixel_ratio_unit(r32, r64)
    total = float((r64["w"] * r64["nll"]).sum() / r64["den"])
    assert abs(total - float(r64["loss"])) <= 1e-12 * max(1.0, abs(total)), (name, total, float(r64["loss"]))
    record("D", name, "loss", abs(float(got - r64["loss"])), unit * float((r64["w"] * (1 + r64["nll"])).sum() / r64["den"]))
    e_ref = float((r32["grad"].double() - r64["grad"]).abs().max())
    record("D", name, "grad", float((grad - r64["grad"]).abs().max()), max(e_ref, EPS * float(r64["w"].abs().max() / r64["den"])))


def run_ce2d(device):
    first = len(RECORDS)
    gen = _gen(31)
    B, C, Hh, W = 2, 19, 9, 13
    logits = torch.randn(B, C, Hh, W, generator=gen) * 10 + 30
    target = torch.randint(0, C, (B, Hh, W), generator=gen)
    target[torch.rand(B, Hh, W, generator=gen) < 0.2] = IGN
    cw, pw = torch.rand(C, generator=gen) + 0.5, torch.rand(B, Hh, W, generator=gen) + 0.25
    big = torch.randint(0, C, (B, 2 * Hh, 2 * W), generator=gen)
    big[torch.rand(B, 2 * Hh, 2 * W, generator=gen) < 0.2] = IGN
    pw_nan = pw.clone()
    pw_nan[1, 4, 5] = float("nan")
    for cl in (False, True):
        tag = " channels-last" if cl else " NCHW"
        run_ce2d_case(device, "plain" + tag, logits, target, channels_last=cl)
        run_ce2d_case(device, "target x2" + tag, logits, big, channels_last=cl)
        run_ce2d_case(device, "class + pixel weights" + tag, logits, target, cw, pw, channels_last=cl)
    run_ce2d_case(device, "target x2, class + pixel weights", logits, big, cw, torch.rand(B, 2 * Hh, 2 * W, generator=gen) + 0.25, channels_last=True)
    run_ce2d_case(device, "NaN pixel weight", logits, target, None, pw_nan, channels_last=True)
    run_ce2d_case(device, "NaN pixel weight, class weights", logits, target, cw, pw_nan)
    run_ce2d_case(device, "all ignored", logits, torch.full_like(target, IGN), channels_last=True)
    run_ce2d_case(device, "all ignored, pixel weights", logits, torch.full_like(target, IGN), None, pw)
    finish(first)


# --------------------------------------------------------------------------------------------------------- E: pseudo_label
THR = 0.968


def _bits(a):
    return a.contiguous().view(torch.int32)


def check_pseudo_label(device, prob, expect_count=None):
    """label, max (bitwise), count and pixel weight of the kernel against torch.max and oracle.segmix.pseudo_label"""
    lab, weight = OS.pseudo_label(prob, IGN, THR)
    mx = torch.max(prob, dim=1)[0]
    count = int((mx >= torch.tensor(THR, dtype=torch.float32)).sum())
    assert weight == count / float(lab.numel())
    if expect_count is not None:
        assert count == expect_count, (count, expect_count)
    got_lab, got_count, got_max, got_w = H.pseudo_label(prob.to(device), THR, IGN, want_max=True, want_weight=True)
    assert torch.equal(got_lab.cpu(), lab), "labels differ at %d pixels" % int((got_lab.cpu() != lab).sum())
    assert torch.equal(_bits(got_max.cpu()), _bits(mx)), "max_prob is not bit-exact"
    assert int(got_count.cpu()[0]) == count, (int(got_count.cpu()[0]), count)
    assert torch.equal(got_w.cpu(), torch.full(tuple(lab.shape), weight, dtype=torch.float32)), "pixel_weight"
    return lab, mx


def run_pseudo_label_edges(device):
    t968 = torch.tensor(THR, dtype=torch.float32)
    below = torch.nextafter(t968, torch.tensor(0.0))
    assert float(below) < float(t968) and _bits(t968.reshape(1))[0] - _bits(below.reshape(1))[0] == 1
    B, C, Hh, W = 2, 19, 5, 53                                  # HW = 265: three blocks, the image boundary inside the second
    gen = _gen(41)
    prob = torch.softmax(torch.randn(B, C, Hh, W, generator=gen), dim=1)      # random pixels: max well below the threshold
    assert float(prob.max()) < 0.9
    flat = prob.reshape(B, C, Hh * W)

    def put(b, p, col):
        flat[b, :, p] = col

    rest = (1 - t968) / (C - 1)
    at = torch.full((C,), float(rest)); at[7] = t968
    under = torch.full((C,), float(rest)); under[7] = below
    tie = torch.zeros(C); tie[4] = 0.5; tie[11] = 0.5
    last = torch.full((C,), 0.001); last[C - 1] = 0.982
    spots = {}
    for b, p0 in ((0, 0), (0, 253), (1, 3), (1, Hh * W - 6)):   # first tile, across the 256 boundary, second image, its last pixels
        for k, (name, col) in enumerate((("at", at), ("under", under), ("zero", torch.zeros(C)), ("negzero", -torch.zeros(C)),
                                         ("tie", tie), ("last", last))):
            put(b, p0 + k, col)
            spots.setdefault(name, []).append((b, p0 + k))
    prob = flat.reshape(B, C, Hh, W).contiguous()
    n_spots = 4
    lab, mx = check_pseudo_label(device, prob, expect_count=2 * n_spots)     # "at" and "last" count, "under" does not
    labf, mxf = lab.reshape(B, -1), mx.reshape(B, -1)
    want = dict(at=7, under=7, zero=IGN, negzero=IGN, tie=4, last=C - 1)
    for name, where in spots.items():
        for b, p in where:
            assert int(labf[b, p]) == want[name], (name, b, p, int(labf[b, p]))
    for b, p in spots["negzero"]:
        assert int(_bits(mxf[b, p].reshape(1))[0]) == -2 ** 31               # -0.0 comes back as -0.0
    # C = 1: the label is 0, or ignore_index where the only plane is (either) zero
    one = torch.rand(2, 1, Hh, W, generator=gen) * 0.9
    of = one.reshape(2, -1)
    of[0, 0], of[0, 1], of[0, 2], of[1, 264], of[1, 263], of[1, 0] = 0.0, -0.0, t968, below, 1.0, t968
    lab1, _ = check_pseudo_label(device, one.contiguous(), expect_count=3)
    assert lab1.reshape(2, -1)[0, :3].tolist() == [IGN, IGN, 0]


# ------------------------------------------------------------------------------------------------------ F: confusion_update
def first_argmax(logits):
    """index of the first maximum over dim 1, from comparisons alone"""
    C = logits.shape[1]
    idx = torch.arange(C).reshape(1, C, 1, 1).expand_as(logits)
    return torch.where(logits == logits.max(1, keepdim=True)[0], idx, torch.full_like(idx, C)).min(1)[0]


def run_confusion(device):
    B, Hh, W = 1, 129, 129                                      # B * HW = 16641: odd, and more than the 256 * 64 pixels of one block
    assert (B * Hh * W) % 2 == 1 and B * Hh * W > 256 * 64
    for C in (1, 19, 64):
        gen = _gen(50 + C)
        gt = torch.randint(0, C, (B, Hh, W), generator=gen)
        skip = torch.rand(B, Hh, W, generator=gen)
        for lo, v in ((0.00, -1), (0.05, C), (0.10, 250), (0.15, 255)):      # 5 % each: skipped by 0 <= gt < C
            gt[(skip >= lo) & (skip < lo + 0.05)] = v
        assert all(int((gt == v).sum()) > 0 for v in (-1, C, 250, 255))
        # predictions, some out of range: the kernel skips those pairs (np.bincount would misplace or raise)
        pred = torch.randint(0, C, (B, Hh, W), generator=gen)
        bad = torch.rand(B, Hh, W, generator=gen)
        pred[bad < 0.03] = -1
        pred[(bad >= 0.03) & (bad < 0.06)] = C
        pred[(bad >= 0.06) & (bad < 0.09)] = 250
        ok = (pred >= 0) & (pred < C)
        assert int((~ok & (gt >= 0) & (gt < C)).sum()) > 0
        want = OM.confusion_matrix([gt[ok].numpy()], [pred[ok].numpy()], C)
        hist = torch.zeros(C * C, dtype=torch.int64).to(device)
        H.confusion_update(hist, gt.to(device), pred=pred.to(device))
        assert np.array_equal(hist.cpu().numpy().reshape(C, C), want), ("pred", C)
        H.confusion_update(hist, gt.to(device), pred=pred.to(device))              # a second call accumulates
        assert np.array_equal(hist.cpu().numpy().reshape(C, C), 2 * want), ("pred twice", C)
        # logits on four levels: ties in nearly every pixel, the first index wins
        logits = torch.randint(0, 4, (B, C, Hh, W), generator=gen).float()
        arg = first_argmax(logits)
        if C > 1:
            assert int((logits == logits.max(1, keepdim=True)[0]).sum(1).max()) > 1
        want = OM.confusion_matrix([gt.numpy()], [arg.numpy()], C)
        total = np.zeros((C, C))
        hist = torch.zeros(C * C, dtype=torch.int64).to(device)
        for lg in (logits.to(device), logits.to(device).contiguous(memory_format=torch.channels_last)):
            H.confusion_update(hist, gt.to(device), logits=lg)
            total += want
            assert np.array_equal(hist.cpu().numpy().reshape(C, C), total), ("logits", C, lg.stride())
    hist = torch.zeros(65 * 65, dtype=torch.int64).to(device)
    small = torch.zeros(1, 4, 4, dtype=torch.int64).to(device)
    try:
        H.confusion_update(hist, small, pred=small)
    except RuntimeError as e:
        assert "bad shape" in str(e), e
    else:
        raise AssertionError("C = 65 must be refused")
    assert int(hist.cpu().sum()) == 0


# ---------------------------------------------------------------------------------------- G: teacher softmax and min-max
SOFTMAX_REGIMES = ((4.0, 0.0), (40.0, 0.0), (4.0, 80.0), (60.0, -90.0))      # (spread, shift)


def check_softmax(name, got, x):
    """x: [B,H,W,C] float32 on the CPU; got: the kernel's [B,C,H,W]"""
    p64 = torch.softmax(x.double().permute(0, 3, 1, 2), dim=1)
    p32 = torch.softmax(x.permute(0, 3, 1, 2), dim=1)
    g = got.detach().cpu()
    assert g.is_contiguous() and tuple(g.shape) == tuple(p64.shape) and bool(torch.isfinite(g).all()), name
    record("G", name, "softmax", float((g.double() - p64).abs().max()), max(float((p32.double() - p64).abs().max()), EPS))
    record("G", name, "row sum", float((g.double().sum(1) - 1).abs().max()), max(float((p32.double().sum(1) - 1).abs().max()), EPS))


def run_softmax(device):
    first = len(RECORDS)
    gen = _gen(61)
    B, Hh, W = 2, 7, 37                                         # HW * 19 odd: the second image's base is not 16-byte aligned
    for C in (1, 19, 160):
        for spread, shift in SOFTMAX_REGIMES:
            x = torch.randn(B, Hh, W, C, generator=gen) * spread + shift
            name = "C%d spread %g shift %g" % (C, spread, shift)
            xd = x.to(device)
            if C == 19:
                assert (Hh * W * C) % 2 == 1 and xd[1].data_ptr() % 16 != 0
            check_softmax(name, H.softmax_to_nchw(xd), x)
            wide = torch.randn(B, Hh, W, C + 13, generator=gen)
            wide[..., 3:3 + C] = x
            wd = wide.to(device)
            check_softmax(name + " pitched", H.softmax_to_nchw(wd[..., 3:3 + C]), x)
            assert torch.equal(wd.cpu(), wide)
    big = torch.randn(1, 40, 40, 19, generator=gen) * 4         # 1600 pixels: seven tiles, the last ragged
    check_softmax("C19 1x40x40", H.softmax_to_nchw(big.to(device)), big)
    try:
        H.softmax_to_nchw(torch.zeros(1, 2, 2, 161).to(device))
    except RuntimeError as e:
        assert "bad shape" in str(e), e
    else:
        raise AssertionError("C = 161 must be refused")
    finish(first)


def run_minmax(device):
    gen = _gen(62)
    for shape in ((3, 1, 3, 5), (3, 1, 17, 31), (2, 1, 40, 50)):              # below one block, two blocks, eight blocks
        x = torch.rand(shape, generator=gen) * 3 - 1
        x[1] = 0.625                                             # a constant image: 0 / 0 in the reference
        want = OS.normalize_disparity(x)
        assert bool(torch.isnan(want[1]).all()) and not bool(torch.isnan(want[0]).any())
        got = H.minmax_normalize(x.to(device)).cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (shape, "NaN positions")
        assert torch.equal(got.nan_to_num(), want.nan_to_num()), (shape, "values")
