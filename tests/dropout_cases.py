"""The in-kernel dropout draw against a specification that stands outside the package (oracle/dropout.py, plain numpy), and the
models with dropout ON against the float64 oracle with the very mask the kernels drew.  Shared by tests/test_dropout_gpu.py (real
library) and tests/test_dropout_emu.py (interpreter build of the same sources).

Kernel cases (A .. C): every mask comparison is exact, and so is every value comparison of A and B.  The expected mask is the
specification's, never ``y != 0`` of the code under test: a ReLU zero is not a dropped element.
  A  hipops.dropout: y == where(keep, x * keep_scale(p), +0.0) bit for bit, dense, on channel slices of a wider buffer (both
     operands; the buffer around the slice untouched) and past the grid cap of ew_blocks
  B  the draw fused into segsde_bn_apply, at its three index paths: the call with drop_p = 0 gives t, the dropped call gives
     t * keep_scale where kept and +0.0 elsewhere, bit for bit (one fp32 product; the build sets -ffp-contract=off)
  C  the backward kernels regenerate the same mask: dres (and dx without batch statistics) is zero exactly where the specification
     drops or the activation's derivative is zero, and nowhere else
  E  statistics of the specification itself (no kernel involved; A and B bind the kernels to it) and the separation of the seeds'
     windows

Model cases (M1 .. M3): a recorder logs, by module path, every seed the forward pass hands to a kernel (and the [B, C] scale of
every Dropout2d site); the oracle gets the masks back through ``Ctx.drop_masks``, built from those seeds by the specification.
Sites are matched by name.  Criteria, none of them derived from what the kernels give:
  outputs and input gradients: the project's rule for re-associated routes (photometric_cases.py),
      max|got - f64| <= 3 * max|oracle32 - f64| + 1e-6 * max|f64|
  with "oracle32" the same oracle graph in float32 with the same masks; parameter gradients: model_cases.gradients_vs_truth with
  its floors, unchanged.  The figures of the MI355X run are in profiles/dropout_draw.md."""
import functools
import json
import math

import numpy as np
import torch
from torch import nn

import batchnorm_cases as BC
import bn_bitmask_cases as BM
import model_cases as MC
import pitched_cases as PC
import sync_bn_cases as SB
from oracle import dropout as OD
from oracle import nets as N
from improving_segmentation_with_selfsupervised_depth_amd import _lib
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
from improving_segmentation_with_selfsupervised_depth_amd.models.joint_segmentation_depth_decoder import JointSegDepthDecoder
from improving_segmentation_with_selfsupervised_depth_amd.models.model_parts import ASPP
from improving_segmentation_with_selfsupervised_depth_amd.models.monodepth_layers import ConvBlock

Opd, _p = BC.Opd, BC._p
EW_CAP = 8192 * 256                     # threads of the largest grid ew_blocks / ew_blocks_cv hand out (csrc/elementwise.hip)
RECORDS = []                            # (case, quantity, kernel error, yardstick, ratio): what profiles/dropout_draw.md tabulates


# ---------------------------------------------------------------------------------------------------------- the specification
@functools.lru_cache(maxsize=64)
def _spec_keep(seed, M, C, p32):
    return torch.from_numpy(OD.keep(seed, (M, C), p32))


def spec_keep(seed, M, C, p):
    """the specification's keep mask [M, C] for the fp32 value of p the C entry points receive (shared, never written)"""
    return _spec_keep(int(seed), int(M), int(C), float(np.float32(p)))


def spec_scale(p):
    return torch.tensor(float(OD.keep_scale(p)), dtype=torch.float32)


def expected_drop(t, keep, p):
    """where(keep, t * keep_scale, +0.0): one fp32 product per kept element"""
    return torch.where(keep, t * spec_scale(p), torch.zeros_like(t))


def _same_mask(got, want, what):
    bad = got != want
    assert not bool(bad.any()), "%s: the mask differs from the specification's at %d of %d elements, first at logical index %d" % (
        what, int(bad.sum()), bad.numel(), int(torch.nonzero(bad.reshape(-1))[0]))


# --------------------------------------------------------------------------------------------------------- A. dropout_kernel
SPEC_CASES = [(1030, 64, 0.5, 1234), (300, 19, 0.1, 0), (777, 24, 0.3, 2 ** 31 - 2), (257, 7, 2.0 ** -24, 5),
              (64, 64, 0.999, 2 ** 40 + 3), (64, 8, 0.5, 2 ** 63 + 5)]
CAP_CASE = (8193, 257, 0.5, 1234)       # M * C just above the grid cap: the second trip of the grid-stride loop
SLICE_PLACEMENTS = ("P1", "P2", "P3")   # aligned to 16 bytes with a pitch of quads; 8 and 12 bytes off with odd pitches


def case_id(c):
    M, C, p, seed = c
    return "M%d-C%d-p%.3g-seed%#x" % (M, C, p, seed)


def _values(M, C, seed=0):
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(1000 + 7 * M + C + seed)) * 2.0
    assert bool((x != 0).all())
    return x


def run_spec_dense(device, case):
    M, C, p, seed = case
    x = _values(M, C)
    keep = spec_keep(seed, M, C, p)
    y = H.dropout(x.to(device), p, seed).cpu()
    _same_mask(y != 0, keep, "dropout " + case_id(case))
    BM.same_bits(y, expected_drop(x, keep, p), "dropout %s: y against where(keep, x * keep_scale, 0)" % case_id(case))
    # the extremes of p draw as the specification says, not "nearly all" / "nearly none"
    if p == 2.0 ** -24:
        assert int((~keep).sum()) == int((torch.from_numpy(OD.u24(seed, np.arange(M * C))) == 0).sum())


def k_dropout(xs, p, seed, ys):
    """segsde_dropout on channel slices of NHWC buffers, both pitches taken from the operands"""
    M, C, ldx = H._rows(xs)
    _lib.check(_lib.lib().segsde_dropout(_p(xs), ldx, M, C, float(p), int(seed), _p(ys), H._rows(ys)[2], H._stream(xs)), "dropout")


def run_spec_slices(device, case):
    """x and y as channel slices (pitch above C, base at a channel offset): the mask follows the logical index m * C + c, and
    nothing around either slice changes"""
    M, C, p, seed = case
    x = _values(M, C, seed=1)
    keep = spec_keep(seed, M, C, p)
    want = expected_drop(x, keep, p)
    x4 = x.reshape(1, 1, M, C).to(device)
    for pname in SLICE_PLACEMENTS:
        off, extra = PC.placement(pname, C)
        what = "dropout %s %s" % (case_id(case), pname)
        xs = PC.slab(x4, off, extra, seed=1)
        assert (xs.data_ptr() % 16 == 0) == (pname == "P1")
        y = H.dropout(xs, p, seed).cpu().reshape(M, C)                      # pitched input, dense output
        _same_mask(y != 0, keep, what + " (input slice)")
        BM.same_bits(y, want, what + " (input slice)")
        assert PC.intact(xs), what + ": the buffer around the input slice was written"
        offy, extray = {"P1": (8, 4), "P2": (3, 5), "P3": (1, 4)}[pname]                    # a pitch and an offset of its own
        ys = PC.slab(torch.zeros_like(x4), offy, extray, seed=2)
        k_dropout(xs, p, seed, ys)
        got = ys.cpu().reshape(M, C).contiguous()
        _same_mask(got != 0, keep, what + " (both slices)")
        BM.same_bits(got, want, what + " (both slices)")
        buf, snap = ys._slab
        snap[..., offy:offy + C] = want.reshape(1, 1, M, C).to(device)
        assert PC.intact(ys), what + ": the output slice's buffer was written outside the slice"
        assert PC.intact(xs), what + ": the buffer around the input slice was written"


def run_identity_and_refusal(device):
    """p = 0 returns x; p = 1 (and beyond) stays refused by the C entry point"""
    x = _values(37, 19).to(device)
    BM.same_bits(H.dropout(x, 0.0, 1234).cpu(), x.cpu(), "dropout p = 0")
    y = torch.empty_like(x)
    for p in (1.0, 1.5, -0.1):
        rc = _lib.lib().segsde_dropout(_p(x), 19, 37, 19, p, 1, _p(y), 19, H._stream(x))
        assert rc != 0, ("segsde_dropout accepted p", p)


# ------------------------------------------------------------------------------------------- B. the draw fused into bn_apply
# (M, C, pitch, offset): M * C >= 60000 as batchnorm_cases.run_dropout asks.  Index paths of bn_apply_kernel:
#   "shift"   C a power of two: m = e >> cv_shift; ew_blocks_cv makes the grid stride a multiple of the channel vectors per row for
#             every power of two, so these launches also keep their channels per thread (fixed_c), vector (VW = 4) and scalar
#   "div4"    C = 24: vectors of 4, m = e / 6
#   "scalar"  C = 19: VW = 1, m = e / 19
FUSED_PATHS = {"shift": [BC.spec(1030, 64), BC.spec(1030, 64, 72, 4), BC.spec(1030, 64, 67, 1)],
               "div4": [BC.spec(2501, 24), BC.spec(2501, 24, 32, 4)],
               "scalar": [BC.spec(3200, 19), BC.spec(3200, 19, 24, 3)]}
# one shape per path past the kernel's own grid cap: bn_apply_impl launches ew_blocks_cv(M * C / VW, C / VW) blocks of 256 threads
# over M * C / VW channel vectors, at most 8192 blocks: the second trip begins above 8192 * 256 vectors
FUSED_CAP = {"shift": BC.spec(131073, 64), "div4": BC.spec(349526, 24), "scalar": BC.spec(110377, 19)}
FUSED_P, FUSED_SEED = 0.3, (0x1234567 << 20) + 99             # a seed above 2^32: its upper bits reach the hash
FUSED_OUTCOME = {}                                              # (path, shape name) -> "bitwise" | max ulp distance


def _vw(s):
    M, C, ld, off = s
    return 4 if (C % 4 == 0 and ld % 4 == 0 and off % 4 == 0) else 1


def _bn_inputs(s, seed):
    M, C = s[0], s[1]
    vals = BC.make_values(M, C, seed=seed)
    x64 = vals["x"].double()
    vals["mean"] = x64.mean(0).float()
    vals["invstd"] = (1 / torch.sqrt(x64.var(0, unbiased=False) + BC.BN_EPS)).float()
    return vals


def run_fused_apply(device, path, s, configs=None):
    M, C, ld, off = s
    if s in FUSED_CAP.values():
        assert M * C // _vw(s) > EW_CAP
    vals = _bn_inputs(s, 21)
    keep = spec_keep(FUSED_SEED, M, C, FUSED_P)
    xo = Opd(M, C, ld, off, device, vals["x"])
    ro_full = Opd(M, C, ld, off, device, vals["res"])
    mean, invstd = vals["mean"].to(device), vals["invstd"].to(device)
    gd, bd = vals["gamma"].to(device), vals["beta"].to(device)
    for act, use_res in (configs or [(a, r) for a in ("relu", "elu") for r in (False, True)]):
        what = "bn_apply %s %s %s%s" % (path, BC.spec_name(s), act, "+res" if use_res else "")
        ro = ro_full if use_res else None
        t_o, y_o = Opd(M, C, ld, off, device), Opd(M, C, ld, off, device)
        BC.k_apply(xo, mean, invstd, gd, bd, ro, t_o, act, 0.0, 0)
        BC.k_apply(xo, mean, invstd, gd, bd, ro, y_o, act, FUSED_P, FUSED_SEED)
        for o in (xo, ro, t_o, y_o):
            if o is not None:
                o.check(what)
        t, y = t_o.cpu(), y_o.cpu()
        live = t != 0                                        # (a ReLU zero stays zero, kept or not)
        _same_mask((y != 0)[live], keep[live], what)
        assert bool((y[~keep] == 0).all()) and not bool(torch.signbit(y[~keep]).any()), what + ": a dropped element is not +0.0"
        BM.same_bits(y, expected_drop(t, keep, FUSED_P), what + ": y against where(keep, t * keep_scale, 0)")
        FUSED_OUTCOME[(path, BC.spec_name(s), act, use_res)] = "bitwise"
        print("DROPOUT-FUSED | %s | %s | %s%s | VW %d | bitwise" % (path, BC.spec_name(s), act, "+res" if use_res else "", _vw(s)))


# --------------------------------------------------------------------------------------- C. backward regenerates the same mask
BACKWARD_SHAPES = [BC.spec(1030, 64), BC.spec(2501, 24, 32, 4), BC.spec(3200, 19, 24, 3)]


def _expected_live(act, keep, t):
    """where dz = dy * mask * act'(y) is not zero, for dy != 0: kept, and (ReLU) the undropped output positive"""
    return keep & (t > 0) if act == "relu" else keep


def run_backward_mask(device, s):
    """segsde_bn_backward from the saved output, with and without batch statistics, and the two stages of the cross-replica
    backward on a single-rank group: dres = dz is non-zero exactly where the specification keeps (and the ReLU is on); without batch
    statistics so is dx = gamma * invstd * dz"""
    M, C, ld, off = s
    vals = _bn_inputs(s, 22)
    assert bool((vals["dy"] != 0).all()) and bool((vals["gamma"] != 0).all())
    keep = spec_keep(FUSED_SEED, M, C, FUSED_P)
    xo, dyo = Opd(M, C, ld, off, device, vals["x"]), Opd(M, C, ld, off, device, vals["dy"])
    ro = Opd(M, C, ld, off, device, vals["res"])
    mean, invstd = vals["mean"].to(device), vals["invstd"].to(device)
    gd, bd = vals["gamma"].to(device), vals["beta"].to(device)
    for act in ("relu", "elu"):
        what = "bn_backward %s %s" % (BC.spec_name(s), act)
        t_o, y_o = Opd(M, C, ld, off, device), Opd(M, C, ld, off, device)
        BC.k_apply(xo, mean, invstd, gd, bd, ro, t_o, act, 0.0, 0)
        BC.k_apply(xo, mean, invstd, gd, bd, ro, y_o, act, FUSED_P, FUSED_SEED)
        t = t_o.cpu()
        if act == "elu":
            assert bool((t > -1).all()) and bool((t != 0).all())             # the derivative y + 1 is not zero anywhere
        live = _expected_live(act, keep, t)
        for bs in (1, 0):
            dxo, dro = Opd(M, C, ld, off, device), Opd(M, C, ld, off, device)
            BC.k_backward(dyo, y_o, xo, mean, invstd, gd, bd, act, FUSED_P, FUSED_SEED, bs, dxo, dro)
            for o in (xo, dyo, y_o, dxo, dro):
                o.check(what)
            dres, dx = dro.cpu(), dxo.cpu()
            _same_mask(dres != 0, live, "%s bs%d dres" % (what, bs))
            if not bs:
                _same_mask(dx != 0, live, what + " bs0 dx")
        # the cross-replica stages, one rank: local sums, the row as the all-gather leaves it, global apply
        inv = torch.tensor([np.float32(1.0) / np.float32(M)], dtype=torch.float32).to(device)
        row, dg, db = SB.k_bwd_local(dyo, y_o, None, xo, mean, invstd, gd, bd, act, FUSED_P, FUSED_SEED, True)
        dxo, dro = Opd(M, C, ld, off, device), Opd(M, C, ld, off, device)
        SB.k_bwd_global(dyo, y_o, None, xo, mean, invstd, gd, bd, act, FUSED_P, FUSED_SEED, row.reshape(1, -1), inv, dxo, dro)
        _same_mask(dro.cpu() != 0, live, what + " sync dres")
        # the sums of the local stage see the same mask: they are the column sums of the dres just checked
        dz = dro.cpu().double()
        unit = torch.maximum(BC.EPS23 * dz.abs().sum(0), torch.tensor(1e-30, dtype=torch.float64))
        assert bool(((db.cpu().double() - dz.sum(0)).abs() <= 4 * unit).all()), what + " sync dbeta is not the column sum of dz"


def run_dropoutfn_backward(device):
    """functional.DropoutFn: the adjoint draws the forward's mask -- where(keep, w * keep_scale, 0) bit for bit"""
    p, seed, shape = 0.2, 2 ** 31 - 2, (2, 9, 13, 24)
    M, C = 2 * 9 * 13, 24
    gen = torch.Generator().manual_seed(17)
    x = (torch.randn(shape, generator=gen) + 0.5)
    w = torch.randn(shape, generator=gen)
    assert bool((w != 0).all()) and bool((x != 0).all())
    keep = spec_keep(seed, M, C, p).reshape(shape)
    xi = x.clone().to(device).requires_grad_(True)
    y = Fn.DropoutFn.apply(xi, p, seed)
    (y * w.to(device)).sum().backward()
    BM.same_bits(y.detach().cpu(), expected_drop(x, keep, p), "DropoutFn forward")
    BM.same_bits(xi.grad.cpu(), expected_drop(w, keep, p), "DropoutFn backward")


# -------------------------------------------------------------------------------------- E. statistics of the specification
STAT_P, STAT_SEEDS, STAT_N = (0.1, 0.5), (0, 1, 1234, 2 ** 31 - 2), 1 << 22
STAT_LAGS, STAT_CHANNELS, Z_MAX = (1, 2, 3, 4, 19, 64, 256, 8192), (64, 256), 5.0


def stat_zscores(p, seed):
    """name -> z (an array for the per-channel fractions): each statistic minus its expectation under an ideal Bernoulli(1 - p)
    sequence, over its standard deviation there"""
    N_ = STAT_N
    q = 1.0 - float(np.float32(p))
    pq = q * (1 - q)
    b = OD.keep(seed, N_, p).astype(np.float64) - q
    out = {"fraction": b.sum() / math.sqrt(N_ * pq)}
    for lag in STAT_LAGS:
        out["lag %d" % lag] = float(np.dot(b[:-lag], b[lag:])) / (pq * math.sqrt(N_ - lag))
    b1 = OD.keep(seed + 1, N_, p).astype(np.float64) - q
    out["seed + 1"] = float(np.dot(b, b1)) / (pq * math.sqrt(N_))
    for C in STAT_CHANNELS:
        out["channels %d" % C] = b.reshape(-1, C).sum(0) / math.sqrt(N_ // C * pq)
    return out


def run_statistics():
    rows, count, worst = [], 0, (0.0, None)
    for p in STAT_P:
        for seed in STAT_SEEDS:
            zs = stat_zscores(p, seed)
            for name, z in zs.items():
                z = np.atleast_1d(np.asarray(z, dtype=np.float64))
                count += z.size
                zmax = float(np.abs(z).max())
                rows.append((p, seed, name, zmax))
                print("DROPOUT-Z | p %.1f | seed %d | %s | %.2f" % (p, seed, name, zmax))
                if zmax > worst[0]:
                    worst = (zmax, (p, seed, name))
    print("DROPOUT-Z-WORST | %.2f | %s | %d statistics" % (worst[0], worst[1], count))
    assert count == len(STAT_P) * len(STAT_SEEDS) * (2 + len(STAT_LAGS) + sum(STAT_CHANNELS))
    bad = [r for r in rows if not r[3] <= Z_MAX]
    assert not bad, "|z| above %g: %s" % (Z_MAX, bad)
    return rows


def seed_stream(n, manual_seed=0):
    """the first n seeds layers._seed() hands out after torch.manual_seed(manual_seed), restated (the caller's generator state is
    left as it was)"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(manual_seed)
        return [int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) for _ in range(n)]


MIN_GAP = 1 << 33            # more elements than a 32-bit count allows, with margin: windows further apart than this never meet


def run_window_separation():
    seeds = seed_stream(4096)
    assert len(set(seeds)) == len(seeds)
    gap = OD.window_gap(seeds)
    print("DROPOUT-WINDOW | 4096 seeds after manual_seed(0) | gap 2^%.1f" % math.log2(gap))
    assert gap >= MIN_GAP, gap
    d = OD.shift_distance(np.arange(1, 1 << 22, dtype=np.uint64))
    k = int(d.argmin()) + 1
    print("DROPOUT-WINDOW | seed differences below 2^22 | smallest |k G mod 2^64| 2^%.1f at k = %d" % (math.log2(float(d.min())), k))
    assert int(d.min()) >= MIN_GAP, (k, int(d.min()))
    # window_gap itself: two seeds whose windows meet are told apart from two that do not
    assert OD.window_gap([7, 7]) == 0 and OD.window_gap([0, 1]) == min(OD.G, (1 << 64) - OD.G)
    return gap, int(d.min()), k


# ---------------------------------------------------------------------------------------------------------------- the recorder
class Recorder:
    """For the duration of a forward pass: every seed models.layers._seed hands out, and per dropout site -- named by the path of
    its nn.Dropout / nn.Dropout2d module in ``model.named_modules()``, the reference's state-dict layout -- what the kernels were
    given: (p, NHWC shape, seed) of the draws fused into BatchNorm2d.forward and of functional.DropoutFn, the [B, C] scale of
    hipops.scale_channels for Dropout2d."""

    def __init__(self, model):
        self.modules = dict(model.named_modules())
        self.names = {id(m): n for n, m in self.modules.items()}
        self.seeds, self.sites, self._stack, self._undo = [], {}, [], []

    def _log(self, site, **kw):
        assert site in self.modules and isinstance(self.modules[site], (nn.Dropout, nn.Dropout2d)), (site, "is no dropout module")
        assert site not in self.sites, (site, "ran twice in one forward")
        assert abs(self.modules[site].p - kw["p"]) < 1e-12, (site, self.modules[site].p, kw["p"])
        self.sites[site] = kw

    def _fused_site(self, bn):
        """ASPP.project and the class head: Sequential(..., BatchNorm2d, ReLU, Dropout, ...)"""
        parent, _, idx = self.names[id(bn)].rpartition(".")
        return (parent + "." if parent else "") + str(int(idx) + 2)

    def __enter__(self):
        rec = self
        seed0, bn0, scale0 = L._seed, L.BatchNorm2d.forward, H.scale_channels
        drop0 = Fn.DropoutFn.apply

        def seed():
            s = seed0()
            rec.seeds.append(s)
            return s

        def bn_forward(bn, x, residual=None, act="none", drop_p=0.0, grad_box=None):
            n0 = len(rec.seeds)
            y = bn0(bn, x, residual, act, drop_p, grad_box)
            if drop_p > 0 and not L.GRAPH_SAFE_DROPOUT[0]:
                assert len(rec.seeds) == n0 + 1, "a fused dropout draws exactly one seed"
                rec._log(rec._fused_site(bn), kind="fused", p=float(drop_p), shape=tuple(x.shape), seed=rec.seeds[-1])
            return y

        def drop_apply(x, p, seed_):
            assert rec._stack and rec.seeds and rec.seeds[-1] == seed_, "DropoutFn's seed did not come from layers._seed"
            rec._log(rec._stack[-1] + "head.0", kind="elementwise", p=float(p), shape=tuple(x.shape), seed=seed_)
            return drop0(x, p, seed_)

        def scale_channels(x, scale):
            assert rec._stack, "scale_channels outside a ConvBlock"
            rec._log(rec._stack[-1] + "block.3", kind="channel", p=float(rec.modules[rec._stack[-1] + "block.3"].p),
                     shape=tuple(x.shape), scale=scale.detach().cpu().clone())
            return scale0(x, scale)

        L._seed, L.BatchNorm2d.forward, H.scale_channels = seed, bn_forward, scale_channels
        Fn.DropoutFn.apply = staticmethod(drop_apply)

        def undo():
            L._seed, L.BatchNorm2d.forward, H.scale_channels = seed0, bn0, scale0
            del Fn.DropoutFn.apply
        self._undo.append(undo)
        for name, m in self.modules.items():
            if isinstance(m, (ConvBlock, JointSegDepthDecoder)):
                prefix = name + "." if name else ""
                h1 = m.register_forward_pre_hook(functools.partial(self._enter_module, prefix))
                h2 = m.register_forward_hook(self._leave_module)
                self._undo += [h1.remove, h2.remove]
        return self

    def _enter_module(self, prefix, module, args):
        self._stack.append(prefix)

    def _leave_module(self, module, args, out):
        self._stack.pop()

    def __exit__(self, *exc):
        for u in self._undo:
            u()
        self._undo = []
        return False

    def provider(self):
        """-> (drop_masks callable for oracle.nets.Ctx, the list of sites it has been asked for)"""
        used = []

        def drop_masks(site, shape_nchw, p, two_d):
            assert site in self.sites, "the oracle drops at %r, the model did not (its sites: %s)" % (site, sorted(self.sites))
            s = self.sites[site]
            used.append(site)
            B, C, Hh, W = shape_nchw
            assert abs(s["p"] - p) < 1e-12 and s["shape"] == (B, Hh, W, C) and two_d == (s["kind"] == "channel"), (site, s, shape_nchw, p)
            if two_d:
                assert tuple(s["scale"].shape) == (B, C) and bool(((s["scale"] == 0) | (s["scale"] > 1)).all())
                return (s["scale"] != 0).reshape(B, C, 1, 1)
            return torch.from_numpy(OD.keep(s["seed"], (B, Hh, W, C), s["p"])).permute(0, 3, 1, 2)
        return drop_masks, used


def check_sites(rec, used, what):
    assert sorted(used) == sorted(rec.sites), (what, "sites of the oracle", sorted(used), "sites of the model", sorted(rec.sites))


# ----------------------------------------------------------------------------------------------------------------- model cases
def rule(case, quantity, got, t64, t32):
    """max|got - f64| <= 3 * max|oracle32 - f64| + 1e-6 * max|f64|"""
    got = got.detach().double().cpu()
    e, yard, sc = float((got - t64).abs().max()), float((t32.double() - t64).abs().max()), float(t64.abs().max())
    ok = e <= 3.0 * yard + 1e-6 * sc
    RECORDS.append((case, quantity, e, yard, e / max(yard, 1e-300)))
    print("DROPOUT-MODEL | %s | %s | kernel %.3e | oracle32 %.3e | ratio %.2f | scale %.3e | %s"
          % (case, quantity, e, yard, e / max(yard, 1e-300), sc, "ok" if ok else "MISSES THE RULE"))
    return ok


def grads_vs_truth(case, named_params, g32, g64):
    e_prod, e_ref = [], []
    for k, p in named_params:
        t = g64.get(k)
        if t is None or p.grad is None or float(t.abs().max()) == 0:
            continue
        den = float(t.norm()) + 1e-30
        e_prod.append(float((p.grad.detach().double().cpu() - t).norm()) / den)
        e_ref.append(float((g32[k].double() - t).norm()) / den)
    for q, f in (("parameter gradients, median", np.median), ("parameter gradients, worst", np.max)):
        RECORDS.append((case, q, float(f(e_prod)), float(f(e_ref)), float(f(e_prod)) / max(float(f(e_ref)), 1e-300)))
        print("DROPOUT-MODEL | %s | %s | kernel %.3e | oracle32 %.3e | ratio %.2f" % ((case, q) + RECORDS[-1][2:]))
    MC.gradients_vs_truth(named_params, g32, g64, case)


def _leaves(sd, dt):
    """an oracle state dict in dtype dt: parameters as leaves, buffers as copies"""
    out = {}
    for k, v in sd.items():
        v = v.detach().cpu().clone()
        if v.is_floating_point():
            v = v.to(dt)
            if "running" not in k:
                v.requires_grad_(True)
        out[k] = v
    return out


def _grads(sdo):
    return {k: v.grad for k, v in sdo.items() if v.is_floating_point() and v.requires_grad}


def run_aspp(device):
    """M1: ASPP alone in train mode, the p = 0.5 draw fused behind project's BatchNorm"""
    torch.manual_seed(11)
    m = ASPP(32, [1, 2], True, 16).to(device).train()
    gen = torch.Generator().manual_seed(12)
    x, w = torch.randn(2, 32, 12, 20, generator=gen), torch.randn(2, 16, 12, 20, generator=gen)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    xd = MC.cl(x.to(device))
    with Recorder(m) as rec:
        y = Fn.to_nchw(m(Fn.to_nhwc(xd)))
    (y * w.to(device)).sum().backward()
    assert sorted(rec.sites) == ["project.3"] and rec.sites["project.3"]["shape"] == (2, 12, 20, 16), rec.sites
    e = dict(rates=[1, 2], pooling=True)
    res = {}
    for dt in (torch.float64, torch.float32):
        masks, used = rec.provider()
        sdo, xo = _leaves(sd, dt), x.clone().to(dt).requires_grad_(True)
        yo = N._aspp(N.Ctx(sdo, True, True, masks), "", e, xo)
        (yo * w.to(dt)).sum().backward()
        check_sites(rec, used, "ASPP")
        res[dt] = (yo.detach(), xo.grad, _grads(sdo))
    (y64, gx64, g64), (y32, gx32, g32) = res[torch.float64], res[torch.float32]
    dropped = float((y64 == 0).double().mean())
    assert 0.5 < dropped < 0.95, dropped                   # half dropped, and the ReLU zeros among the kept
    ok = rule("M1 ASPP", "output", y, y64, y32)
    ok &= rule("M1 ASPP", "input gradient", xd.grad, gx64, gx32)
    grads_vs_truth("M1 ASPP", list(m.named_parameters()), g32, g64)
    assert ok, "M1: output or input gradient misses the rule (figures above)"


def _jsd(device, golden):
    g = golden("decoders")
    a1 = json.loads(str(g["dd1_args_json"]))
    depth_args = dict(num_ch_dec=a1["num_ch_dec"], max_scale_size=a1["max_scale_size"])       # plain ConvBlocks: two dropout sites
    sa = dict(layers=[9], head_inter=True, output_stride=1, layer_out_channels=8, head_inter_channels=8, layer_dropout=0.2,
              head_dropout=0.1)
    torch.manual_seed(21)
    m = JointSegDepthDecoder(MC.ENC, a1["num_ch_dec"], 5, weights="none", depth_args=dict(depth_args), **sa).to(device).train()
    feats = [g["jsd1_f%d" % i] for i in range(5)]
    plan = N.decoder_plan(MC.ENC, range(4), num_ch_dec=a1["num_ch_dec"])
    return m, feats, plan, sa


def run_joint_decoder(device, golden):
    """M2: JointSegDepthDecoder with layer_dropout (functional.DropoutFn) and head_dropout (fused behind the head's BatchNorm)"""
    m, feats, plan, sa = _jsd(device, golden)
    w = torch.randn(2, 5, 32, 48, generator=torch.Generator().manual_seed(22))
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    fs = [MC.cl(f.to(device)) for f in feats]
    with Recorder(m) as rec:
        y = m(fs)
    (y * w.to(device)).sum().backward()
    assert sorted(rec.sites) == ["head.0", "head.4"], sorted(rec.sites)
    assert rec.sites["head.0"]["seed"] != rec.sites["head.4"]["seed"], "two sites drew from one seed"
    assert sorted(rec.seeds) == sorted(s["seed"] for s in rec.sites.values())
    res = {}
    for dt in (torch.float64, torch.float32):
        masks, used = rec.provider()
        # (copies: the fixture's tensors are shared with other tests and stay as they are)
        sdo, fo = _leaves(sd, dt), [f.detach().clone().to(dt).requires_grad_(True) for f in feats]
        yo = N.jsd_forward(N.Ctx(sdo, True, True, masks), "", plan, fo, sa)
        (yo * w.to(dt)).sum().backward()
        check_sites(rec, used, "JointSegDepthDecoder")
        res[dt] = (yo.detach(), [f.grad for f in fo], _grads(sdo))
    (y64, gf64, g64), (y32, gf32, g32) = res[torch.float64], res[torch.float32]
    ok = rule("M2 JointSegDepthDecoder", "semantics", y, y64, y32)
    for i, f in enumerate(fs):
        if gf64[i] is None:
            assert f.grad is None or float(f.grad.abs().max()) == 0, ("feature", i)
            continue
        ok &= rule("M2 JointSegDepthDecoder", "gradient of feature %d" % i, f.grad, gf64[i], gf32[i])
    grads_vs_truth("M2 JointSegDepthDecoder", list(m.named_parameters()), g32, g64)
    assert ok, "M2: output or input gradients miss the rule (figures above)"


def run_seed_plumbing(device, golden):
    """seeds are fresh per forward, absent in eval mode, a function of the CPU generator's state, and far enough apart"""
    m, feats, _, _ = _jsd(device, golden)
    fs = [f.to(device) for f in feats]

    def forward():
        with Recorder(m) as rec, torch.no_grad():
            m(fs)
        return rec
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        a, b = forward(), forward()
        assert len(a.seeds) == len(b.seeds) == 2 and not set(a.seeds) & set(b.seeds), (a.seeds, b.seeds)
        assert OD.window_gap(a.seeds) >= MIN_GAP and OD.window_gap(a.seeds + b.seeds) >= MIN_GAP
        torch.manual_seed(5)
        a2, b2 = forward(), forward()
        assert (a2.seeds, b2.seeds) == (a.seeds, b.seeds), "torch.manual_seed does not determine the seeds"
        assert [a2.sites[k]["seed"] for k in sorted(a.sites)] == [a.sites[k]["seed"] for k in sorted(a.sites)]
        torch.manual_seed(6)
        assert forward().seeds != a.seeds
        m.eval()
        e = forward()
        assert e.seeds == [] and e.sites == {}, (e.seeds, e.sites)
        m.train()
    assert a.seeds == seed_stream(2, 5), "the seeds are not the generator's first draws"


def jsd_dropout_cfg():
    cfg = json.loads(json.dumps(MC.contract_cfgs()["cfgs"]["r18_jsd"]))
    cfg["segmentation_args"].update(head_inter=True, layer_dropout=0.2)
    cfg["depth_args"]["dropout"] = 0.1
    return cfg


def run_full_model(device, golden):
    """M3: the r18_jsd contract model with every kind of dropout site on (both ASPPs, layer and head dropout, Dropout2d in every
    ConvBlock of both decoders): forward, monodepth loss plus cross-entropy, backward, against the oracle in float64 on the host"""
    from oracle import photometric as P, segmix as S
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss
    from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import cross_entropy2d
    name, case = "r18_jsd", "M3 r18_jsd"
    g = golden("nets")
    cfg = jsd_dropout_cfg()
    sd = N.build_state_dict(cfg, 19, seed=1234, randomize_bn=True)
    model = get_model(cfg, 19)
    model.load_state_dict(sd, strict=True)
    model.to(device).train()
    inputs = {}
    for k, v in g.items():
        if k.startswith(name + "_in_color"):
            parts = k[len(name) + 4:].rsplit("_", 2)
            inputs[("color", int(parts[1]), int(parts[2]))] = v.to(device)
    inputs[("K", 0)], inputs[("inv_K", 0)] = g[name + "_in_K_0"].to(device), g[name + "_in_inv_K_0"].to(device)
    for f in (0, -1, 1):
        inputs[("color_aug", f, 0)] = inputs[("color", f, 0)]
    B, _, Hh, W = inputs[("color", 0, 0)].shape
    mono = dict(num_scales=4, frame_ids=[0, -1, 1], height=Hh, width=W, min_depth=0.1, max_depth=100, test_min_depth=1e-3,
                test_max_depth=80, disparity_smoothness=1e-3, no_ssim=False, avg_reprojection=False, disable_automasking=False)
    # (torch.manual_seed also seeds the device generator the Dropout2d draws come from: both states are put back)
    with torch.random.fork_rng(devices=[] if str(device) == "cpu" else [torch.cuda.current_device()]):
        torch.manual_seed(31)
        with Recorder(model) as rec:
            out = model(inputs)
    loss_obj = get_monodepth_loss({"training": {"batch_size": B, "monodepth_loss": mono}}, is_train=True)
    loss_obj.tiebreak_noise = {s: g[name + "_noise_%d" % s] for s in range(4)}
    loss_obj.generate_images_pred(inputs, out)
    total = loss_obj.compute_losses(inputs, out)["loss"] + cross_entropy2d(out["semantics"], g[name + "_lbl"].to(device))
    total.backward()
    # ---- the sites: two ASPPs, the two head sites, nine Dropout2d per decoder (the tenth ConvBlock is the ASPP), by name
    kinds = {}
    for site, s in rec.sites.items():
        kinds.setdefault(s["kind"], []).append(site)
    assert sorted(kinds["fused"]) == ["models.depth.decoder.0.project.3", "models.segmentation.head.4",
                                      "models.segmentation.unet_dec.decoder.0.project.3"], kinds["fused"]
    assert kinds["elementwise"] == ["models.segmentation.head.0"]
    assert len(kinds["channel"]) == 18 and all(k.endswith(".block.3") for k in kinds["channel"]), sorted(kinds["channel"])
    a, b = (rec.sites["models.%s.decoder.0.project.3" % d] for d in ("depth", "segmentation.unet_dec"))
    assert a["shape"] == b["shape"] and a["p"] == b["p"] and a["seed"] != b["seed"]
    assert len(rec.seeds) == 4 and len(set(rec.seeds)) == 4 and OD.window_gap(rec.seeds) >= MIN_GAP, rec.seeds
    # ---- truth and yardstick
    res = {}
    for dt in (torch.float64, torch.float32):
        cast = lambda v: v.to(dt) if v.is_floating_point() else v
        masks, used = rec.provider()
        sdo = _leaves(sd, dt)
        inp = {k: cast(v.cpu()) for k, v in inputs.items()}
        o = N.model_forward(sdo, cfg, inp, train=True, dropout=True, drop_masks=masks)
        check_sites(rec, used, "r18_jsd")
        lo = P.MonodepthLossOracle(**mono, batch_size=B)
        lo.generate_images_pred(inp, o)
        tot = lo.compute_losses(inp, o, tiebreak_noise={s: cast(g[name + "_noise_%d" % s]) for s in range(4)})["loss"]
        tot = tot + S.cross_entropy2d(o["semantics"], g[name + "_lbl"])
        tot.backward()
        res[dt] = ({k: o[k].detach() for k in [("disp", s) for s in range(4)] + ["semantics"]}, _grads(sdo), float(tot))
    (o64, g64, l64), (o32, g32, l32) = res[torch.float64], res[torch.float32]
    print("DROPOUT-MODEL | %s | loss | kernel %.9g | oracle32 %.9g | float64 %.9g" % (case, float(total), l32, l64))
    ok = True
    for k in o64:
        ok &= rule(case, "semantics" if k == "semantics" else "disp %d" % k[1], out[k], o64[k], o32[k])
    grads_vs_truth(case, list(model.named_parameters()), g32, g64)
    assert ok, "M3: an output misses the rule (figures above)"


# ------------------------------------------------------------------------------------------------------------ the capture path
def run_capture_path(device):
    """GRAPH_SAFE_DROPOUT: BatchNorm2d.forward(drop_p = 0.5) is the drop_p = 0 output times a mask of {0, fp32(1 / (1 - p))} from
    torch's generator, and the input gradient is the undropped layer's gradient of dy * mask.  p = 0.5: the scale is 2, so both
    statements hold bit for bit whatever the order of torch's two products"""
    p, C = 0.5, 24
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(2, 7, 9, C, generator=gen) * 1.5 + 0.3
    dy = torch.randn(2, 7, 9, C, generator=gen)
    torch.manual_seed(42)
    bn, bn0 = L.BatchNorm2d(C).to(device).train(), L.BatchNorm2d(C).to(device).train()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=gen))
        bn.bias.copy_(torch.randn(C, generator=gen))
    bn0.load_state_dict(bn.state_dict())
    xa, xb = x.clone().to(device).requires_grad_(True), x.clone().to(device).requires_grad_(True)
    old = L.GRAPH_SAFE_DROPOUT[0]
    L.GRAPH_SAFE_DROPOUT[0] = True
    try:
        with Recorder(bn) as rec:
            y = bn(xa, act="elu", drop_p=p)
        assert rec.seeds == [], "the capture path took a host seed"
    finally:
        L.GRAPH_SAFE_DROPOUT[0] = old
    y0 = bn0(xb, act="elu", drop_p=0.0)
    assert bool((y0 != 0).all())
    mask = (y / y0).detach()
    scale = float(np.float32(1) / (np.float32(1) - np.float32(p)))
    assert bool(((mask == 0) | (mask == scale)).all()), "mask values outside {0, 1 / (1 - p)}"
    frac = float((mask != 0).float().mean())
    n = mask.numel()
    assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), frac
    BM.same_bits(y.detach().cpu(), (y0 * mask).detach().cpu(), "capture path: y against y0 * mask")
    y.backward(dy.to(device))
    y0.backward(dy.to(device) * mask)
    BM.same_bits(xa.grad.cpu(), xb.grad.cpu(), "capture path: input gradient")
    BM.same_bits(bn.weight.grad.cpu(), bn0.weight.grad.cpu(), "capture path: dgamma")
    BM.same_bits(bn.running_var.cpu(), bn0.running_var.cpu(), "capture path: running_var (one update per forward)")
