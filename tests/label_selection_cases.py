"""Label selection (label_selection.py, csrc/labelsel.hip): the cases shared by the interpreter run (test_label_selection_emu.py),
the GPU run (test_label_selection_gpu.py), the fixture generator (tests/golden/make_label_selection.py, which feeds the SAME
seeded inputs to the reference and records what it returns) and the measurement tool (tools/label_selection.py).

Inputs come from numpy's PCG64 generator by seed, so only results travel in tests/golden/label_selection.npz:
  * discrete results (farthest-point indices and distances, chosen lists, dilation masks, NaN patterns): compared bit for bit;
  * e_ref: the error of the reference's own fp32 evaluation against a float64 evaluation of the same expressions (the functions
    ``*_f64`` below), as (max, rms) per case.  The package's error e_pkg against the same float64 must satisfy the package's 3x
    rule, ``gate`` below: e_pkg <= 3 e_ref for the maximum and the rms, and never tighter than 4 units in the last place of the
    float64 value rounded to fp32 (a sum, a square root and a division each round once)."""
import numpy as np
import torch

from conftest import load_golden
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
from improving_segmentation_with_selfsupervised_depth_amd import label_selection as LS
from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import pixel_wise_entropy

_G = {}


def golden():
    if "g" not in _G:
        _G["g"] = load_golden("label_selection")
    return _G["g"]


def rng(*key):
    return np.random.default_rng([20240607] + [int(k) for k in key])


# ------------------------------------------------------------------------------------------------------------------ the 3x rule
def ulp32(v64):
    """spacing of fp32 at the float64 values rounded to fp32"""
    a = np.abs(np.asarray(v64, dtype=np.float64)).astype(np.float32)
    return np.spacing(np.maximum(a, np.float32(1.1754944e-38))).astype(np.float64)


def errors(x, t64):
    e = np.abs(np.asarray(x, dtype=np.float64) - t64)
    return (float(e.max()), float(np.sqrt(np.mean(e * e)))) if e.size else (0.0, 0.0)


def gate(x, t64, e_ref, what):
    """x: the package's fp32 result; t64: float64 truth; e_ref: (max, rms) of the reference's fp32 result against t64.
    Prints both figures, then asserts.  Returns (e_pkg_max, e_pkg_rms)."""
    x, t64 = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(t64, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(x), np.isnan(t64)), what + ": NaN pattern"
    ok = ~np.isnan(t64)
    x, t64 = x[ok], t64[ok]
    e = np.abs(x - t64)
    floor = 4.0 * ulp32(t64)
    e_max, e_rms = errors(x, t64)
    print("%-44s e_ref max %.3e rms %.3e | e_pkg max %.3e rms %.3e" % (what, e_ref[0], e_ref[1], e_max, e_rms))
    if e.size:
        assert np.all(e <= np.maximum(3.0 * e_ref[0], floor)), "%s: max error %.3e > 3 x %.3e" % (what, e_max, e_ref[0])
        assert e_rms <= max(3.0 * e_ref[1], float(np.sqrt(np.mean(floor * floor)))), "%s: rms %.3e > 3 x %.3e" % (what, e_rms, e_ref[1])
    return e_max, e_rms


def layout(t, kind):
    if kind == "nchw":
        return t.contiguous()
    if kind == "cl":
        return t.contiguous(memory_format=torch.channels_last)
    assert kind == "pitched"
    big = torch.zeros(t.shape[:-1] + (t.shape[-1] + 5,), dtype=t.dtype, device=t.device)
    big[..., :t.shape[-1]] = t
    return big[..., :t.shape[-1]]


# ------------------------------------------------------------------------------------------------------------------ farthest point
FP_THREADS = 512                # csrc/labelsel.hip: a thread owns columns t, t + 512, ...: at N = 1025 every thread has a second one


def fps_matrix(kind, N, seed):
    r = rng(1, seed, N)
    if kind == "random":                                   # not a metric, not symmetric; zero diagonal (otherwise a current sample
        m = r.random((N, N), dtype=np.float32)              # wins at once: its own distance is the largest minimum)
        np.fill_diagonal(m, 0)
        return m
    if kind == "ints":                                     # 1..4: ties in the minimum and in the maximum
        m = r.integers(1, 5, (N, N)).astype(np.float32)
        np.fill_diagonal(m, 0)
        return m
    if kind == "zeros":
        return np.zeros((N, N), dtype=np.float32)
    assert kind == "biased"                                # a distance matrix + column bias, zero diagonal
    a = r.random((N, 6), dtype=np.float32)
    m = np.sqrt(((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)).astype(np.float32) + r.random(N, dtype=np.float32)[None, :]
    np.fill_diagonal(m, 0)
    return m


# name: (kind, N, seed, current, n_new, preselected)
FPS_CASES = {
    "n1": ("random", 1, 0, [0], 3, None),
    "n2": ("random", 2, 0, [1], 2, None),
    "n64": ("random", 64, 0, [3], 8, None),
    "n65": ("random", 65, 0, [64], 8, None),
    "n1025": ("random", 2 * FP_THREADS + 1, 0, [5, 700], 6, None),
    "ints65": ("ints", 65, 1, [0], 10, None),
    "ints1025": ("ints", 2 * FP_THREADS + 1, 1, [1], 5, None),
    "pre65": ("random", 65, 2, [12], 8, list(range(10, 41, 2))),
    "pre_complement_low": ("random", 65, 3, [20], 12, list(range(20, 31))),      # 10 additions, then the zero-distance sample 0, then it wins again: stop
    "zeros_stop_at_once": ("zeros", 64, 0, [0], 5, None),
    "zeros_one_then_stop": ("zeros", 64, 0, [5], 5, None),
    "more_than_possible": ("random", 8, 4, [2], 12, None),
    "current_n_minus_1": ("random", 64, 5, [i for i in range(64) if i != 17], 3, None),
    "biased": ("biased", 65, 6, [7, 30], 10, None),
    "biased513": ("biased", FP_THREADS + 1, 6, [0], 9, None),
}


def run_fps(device, names=None):
    g = golden()
    for name, (kind, N, seed, current, n_new, pre) in FPS_CASES.items():
        if names is not None and name not in names:
            continue
        m = torch.from_numpy(fps_matrix(kind, N, seed)).to(device)
        ident = {i: i for i in range(N)}
        new, d = LS.iterative_farthest_point(list(current), {"distances": m, "dist_i_to_img_idx": ident, "img_idx_to_dist_i": ident},
                                             n_new, pre)
        want_i, want_d = g["fps_%s_idx" % name].tolist(), g["fps_%s_dist" % name]
        assert new == want_i, (name, new, want_i)
        got_d = torch.stack([x.reshape(()) for x in d]) if d else torch.zeros(0)
        assert got_d.dtype == torch.float32 and torch.equal(got_d.view(torch.int32), want_d.view(torch.int32)), (name, got_d, want_d)
        assert torch.equal(m.cpu(), torch.from_numpy(fps_matrix(kind, N, seed))), name + ": the matrix was modified"
    # image indices that are not matrix rows go through the two maps
    kind, N, seed, current, n_new, pre = FPS_CASES["pre65"]
    m = torch.from_numpy(fps_matrix(kind, N, seed)).to(device)
    to_img = {i: 1000 + 3 * i for i in range(N)}
    to_row = {v: k for k, v in to_img.items()}
    new, _ = LS.iterative_farthest_point([to_img[c] for c in current], {"distances": m, "dist_i_to_img_idx": to_img,
                                                                         "img_idx_to_dist_i": to_row}, n_new, [to_img[c] for c in pre])
    assert new == [to_img[i] for i in g["fps_pre65_idx"].tolist()]


def run_fps_large(device, N, n_new=6):
    """the LDS layout above 64 KB of dynamic LDS (N > 16 368) up to the stated cap: the matrix |i - j|, made on the device, whose
    selection from sample 0 a few lines of numpy give (ties to the lowest index: np.argmax returns the first maximum)"""
    a = torch.arange(N, device=device, dtype=torch.float32)
    m = (a[:, None] - a[None, :]).abs_()
    ident = {i: i for i in range(N)}
    new, d = LS.iterative_farthest_point([0], {"distances": m, "dist_i_to_img_idx": ident, "img_idx_to_dist_i": ident}, n_new)
    line = np.arange(N, dtype=np.float32)
    mind, want_i, want_d = line.copy(), [], []
    for _ in range(n_new):
        j = int(np.argmax(mind))
        want_i.append(j)
        want_d.append(float(mind[j]))
        mind = np.minimum(mind, np.abs(line - np.float32(j)))
    assert new == want_i and [float(x) for x in d] == want_d, (N, new, want_i)
    assert want_i[:2] == [N - 1, (N - 1) // 2]


# ------------------------------------------------------------------------------------------------------------------ distances
DIST_N, DIST_D, DIST_P = (1, 2, 63, 64, 65, 130), (1, 7, 192, 513), (1, 2)
DIST_CASES = [(N, D, p) for N in DIST_N for D in DIST_D for p in DIST_P]


def dist_bank(N, D):
    return rng(2, N, D).standard_normal((N, D)).astype(np.float32)


def dist_f64(bank, p):
    a = bank.astype(np.float64)
    out = np.empty((a.shape[0], a.shape[0]))
    for i in range(a.shape[0]):
        d = np.abs(a - a[i])
        out[i] = np.sqrt((d * d).sum(1)) if p == 2 else d.sum(1)
    return out


def offdiag(m):
    m = np.asarray(m)
    return m[~np.eye(m.shape[0], dtype=bool)]


def run_distance_case(device, N, D, p):
    g = golden()
    k = DIST_CASES.index((N, D, p))
    bank = dist_bank(N, D)
    out = H.labelsel_distance(torch.from_numpy(bank).to(device), p).cpu().numpy()
    assert out.shape == (N, N) and np.array_equal(out.view(np.int32), out.T.copy().view(np.int32)), "bitwise symmetry"
    assert np.all(np.diag(out) == 0)
    return gate(offdiag(out), offdiag(dist_f64(bank, p)), g["dist_eref"][k].tolist(), "distance N=%d D=%d p=%d" % (N, D, p))


def run_distance_properties(device):
    """identical rows, column bias + zero diagonal, pitched bank and pitched output, refusals"""
    for p in (1, 2):
        bank = dist_bank(65, 192)
        bank[9] = bank[5]
        bank[64] = bank[0]
        bt = torch.from_numpy(bank).to(device)
        plain = H.labelsel_distance(bt, p)
        assert plain[5, 9] == 0 and plain[9, 5] == 0 and plain[0, 64] == 0 and plain[64, 0] == 0
        bias = torch.from_numpy(rng(3, p).random(65, dtype=np.float32)).to(device)
        biased = H.labelsel_distance(bt, p, bias)
        want = plain + bias[None, :]                     # one fp32 addition per entry: exact comparison
        want.fill_diagonal_(0)
        assert torch.equal(biased, want)
        assert not torch.equal(biased, biased.t())
        wide = torch.zeros((65, 200), device=device)
        wide[:, :192] = bt
        assert torch.equal(H.labelsel_distance(wide[:, :192], p), plain)
        buf = torch.full((65, 70), -7.0, device=device)
        H.labelsel_distance(bt, p, out=buf[:, :65])
        assert torch.equal(buf[:, :65], plain) and bool((buf[:, 65:] == -7.0).all())
    try:
        H.labelsel_distance(bt, 3)
        raise AssertionError("p = 3 accepted")
    except NotImplementedError:
        pass
    L = H._lib.lib()
    assert L.segsde_labelsel_distance(H._p(bt), 192, 65, 192, 3, None, H._p(plain), 65, H._stream(bt)) == -4


CFD_N, CFD_C, CFD_H = 65, 24, 2          # _calc_feature_distance cases: D = 24 * 2 * 4 = 192


def cfd_features(const_channel=False):
    f = rng(4).standard_normal((CFD_N, CFD_C, CFD_H, 2 * CFD_H)).astype(np.float32)
    f *= np.linspace(0.5, 20.0, CFD_C, dtype=np.float32)[None, :, None, None]       # channels of very different scale
    f += np.linspace(-30.0, 30.0, CFD_C, dtype=np.float32)[None, :, None, None]
    if const_channel:
        f[:, 3] = 1.25
    return f


def cfd_bias():
    return rng(5).random(CFD_N).astype(np.float32).tolist()


def cfd_f64(f, bias, bias_weight, p, norm):
    f = f.astype(np.float64)
    if norm:
        mean = f.mean(axis=(0, 2, 3), keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            f = (f - mean) / f.std(axis=(0, 2, 3), keepdims=True, ddof=1)
    out = dist_f64(f.reshape(f.shape[0], -1), p)
    if bias_weight > 0:
        out = out + np.asarray(bias, dtype=np.float32).astype(np.float64)[None, :]
    np.fill_diagonal(out, 0)
    return out


CFD_CASES = [(norm, bw, p) for norm in (False, True) for bw in (0, 1) for p in (1, 2)]


def run_calc_feature_distance(device):
    g = golden()
    f = cfd_features()
    feats = [torch.from_numpy(f[i:i + 1]).to(device) for i in range(CFD_N)]
    for k, (norm, bw, p) in enumerate(CFD_CASES):
        out = LS._calc_feature_distance(feats, cfd_bias(), bw, p, norm, False).cpu().numpy()
        assert np.all(np.diag(out) == 0)
        gate(offdiag(out), offdiag(cfd_f64(f, cfd_bias(), bw, p, norm)), g["cfd_eref"][k].tolist(),
             "_calc_feature_distance norm=%d bias=%d p=%d" % (norm, bw, p))
        if bw == 0:
            assert np.array_equal(out.view(np.int32), out.T.copy().view(np.int32))
    assert torch.equal(feats[0].cpu(), torch.from_numpy(f[0:1])), "the caller's features were modified"
    # a FeatureBank argument gives the same matrix as the list
    bank = LS.FeatureBank(CFD_N, CFD_C, CFD_H, "avg", "u3", device)
    bank.add(torch.from_numpy(f).to(device), list(range(CFD_N)))
    assert torch.equal(bank.features().cpu(), torch.from_numpy(f.reshape(CFD_N, -1)))      # bins of one pixel: the identity
    assert torch.equal(LS._calc_feature_distance(bank, [], 0, 2, True, False), LS._calc_feature_distance(feats, [], 0, 2, True, False))
    assert torch.equal(bank.features().cpu(), torch.from_numpy(f.reshape(CFD_N, -1))), "the bank was normalised in place"
    # a constant channel: 0/0 = NaN in every distance, as the reference gives
    fc = cfd_features(const_channel=True)
    out = LS._calc_feature_distance([torch.from_numpy(fc[i:i + 1]).to(device) for i in range(CFD_N)], [], 0, 2, True, False).cpu()
    assert torch.equal(torch.isnan(out), g["cfd_const_isnan"].bool())
    assert bool(torch.isnan(out).any()) and bool((torch.diagonal(out) == 0).all())
    try:
        LS._calc_feature_distance(feats, [], 0, 2, False, True)
        raise AssertionError("patch_wise accepted")
    except NotImplementedError:
        pass


def run_normalize_blocks(device):
    """more elements per channel than one block pass takes (64 blocks x 4096): N*P = 70000 x 4, C = 2, against float64"""
    N, C, P = 70000, 2, 4
    f = rng(6).standard_normal((N, C * P)).astype(np.float32) * 3 + 5
    bank = torch.from_numpy(f).to(device)
    H.labelsel_normalize_(bank, C, P)
    a = f.astype(np.float64).reshape(N, C, P)
    t64 = ((a - a.mean(axis=(0, 2), keepdims=True)) / a.std(axis=(0, 2), keepdims=True, ddof=1)).reshape(N, C * P)
    ft = torch.from_numpy(f).reshape(N, C, P, 1)
    sd, mean = torch.std_mean(ft, dim=[0, 2, 3], keepdim=True)
    gate(bank.cpu().numpy(), t64, errors(((ft - mean) / sd).numpy().reshape(-1), t64.reshape(-1)), "normalize 70000x2x4")


# ------------------------------------------------------------------------------------------------------------------ scores
ERR_TYPES = list(H.DEPTH_ERROR_TYPES)
THR = np.float32(0.07)
# name: (B, C, H, W, layout, logit regime, error types, maps wanted)
SCORE_CASES = {
    "s23x40_c19": (1, 19, 23, 40, "nchw", "spread1", ERR_TYPES, True),
    "s23x40_c2_cl": (2, 2, 23, 40, "cl", "spread30", ERR_TYPES, True),
    "s64x128_c20_pitched": (2, 20, 64, 128, "pitched", "shift300", ERR_TYPES, True),
    "s64x128_c160_cl": (1, 160, 64, 128, "cl", "onehot", ["abs"], False),
    "s64x128_c19_t0": (1, 19, 64, 128, "nchw", "spread1", [], True),
    "s136x2000_c2": (1, 2, 136, 2000, "nchw", "spread1", ["abs", "sq_rel"], True),      # 288 tiles: above one grid pass of 256
}


def score_inputs(name):
    B, C, Hh, W, _, regime, _, _ = SCORE_CASES[name]
    r = rng(7, sorted(SCORE_CASES).index(name))
    x = r.standard_normal((B, C, Hh, W)).astype(np.float32)
    if regime == "spread30":
        x *= 30
    elif regime == "shift300":
        x += 300
    elif regime == "onehot":                                # saturated: exp(x - max) underflows to 0 for every other class
        x[:, 0, ::2] += 500
        x[:, C - 1, 1::2] += 200
    ds = (r.integers(18, 256, (B, Hh, W)) / 255.0).astype(np.float32)       # uint8 / 255, all >= 0.07 ...
    low = [(0, 0), (0, W - 1), (Hh - 1, 0), (Hh - 1, W - 1), (0, W // 2), (Hh // 2, 0), (Hh // 2, W - 1), (Hh - 1, W // 3),
           (min(15, Hh - 1), min(63, W - 1)), (min(16, Hh - 1), min(64, W - 1)), (Hh // 3, min(60, W - 1)), (Hh // 3, min(67, W - 1))]
    for b in range(B):                                      # ... except at the corners, on every edge and across the tile seam (15|16, 63|64)
        for k, (y, xx) in enumerate(low[b::1 + b]):
            ds[b, y, xx] = np.float32(k % 18) / np.float32(255)             # exact zeros included
        ds[b, Hh // 4, W // 4] = THR                                        # exactly 0.07: not masked
    dp = (r.random((B, Hh, W), dtype=np.float32) * 0.9 + 0.003).astype(np.float32)
    dp[ds == dp] += np.float32(0.01)                        # |dp - ds| > 0 everywhere: a zero of the "abs" map is a masked pixel
    return x, dp, ds


def dilate_np(mask, k=7):
    p = k // 2
    m = np.pad(mask, ((0, 0), (p, p), (p, p)))
    out = np.zeros_like(mask)
    for dy in range(k):
        for dx in range(k):
            out |= m[:, dy:dy + mask.shape[1], dx:dx + mask.shape[2]]
    return out


def score_f64(x, dp, ds, types):
    """-> (entropy [B,H,W], error maps [B,T,H,W], masked [B,H,W] bool incl. the own-car rows) in float64"""
    B, C, Hh, W = x.shape
    z = x.astype(np.float64)
    z = z - z.max(1, keepdims=True)
    e = np.exp(z)
    p = e / e.sum(1, keepdims=True)
    ent = -(p * np.log2(p + 1e-30)).sum(1) / np.log2(C)
    a, b = dp.astype(np.float64), ds.astype(np.float64)
    with np.errstate(divide="ignore"):
        ia, ib = np.clip(1 / a, np.float64(np.float32(0.1)), 80), np.clip(1 / b, np.float64(np.float32(0.1)), 80)
    maps = []
    for t in types:
        maps.append({"abs": np.abs(a - b), "abs_inv_log": np.abs(np.log(ib) - np.log(ia)), "abs_inv": np.abs(ib - ia), "sq": (a - b) ** 2,
                     "abs_rel": np.abs(a - b) / (b + 0.1), "sq_rel": (a - b) ** 2 / (b + 0.1),
                     "abs_log": np.abs(np.log(1 + a) - np.log(1 + b))}[t])
    masked = dilate_np(ds < THR)
    masked[:, int(0.87 * Hh):] = True
    maps = np.stack(maps, 1) if maps else np.zeros((B, 0, Hh, W))
    maps = np.where(masked[:, None], 0.0, maps)
    return ent, maps, masked


def run_score_case(device, name):
    g = golden()
    B, C, Hh, W, lay, _, types, want_maps = SCORE_CASES[name]
    x, dp, ds = score_inputs(name)
    ent64, maps64, masked = score_f64(x, dp, ds, types)
    T = len(types)
    logits = layout(torch.from_numpy(x).to(device), lay)
    table, ent, err = H.labelsel_score(logits, torch.from_numpy(dp).to(device) if T else None,
                                       torch.from_numpy(ds).to(device) if T else None, types, want_maps=want_maps)
    assert tuple(table.shape) == (B, 1 + T)
    assert (ent is not None) == want_maps and (err is not None) == (want_maps and T > 0)
    eref = g["score_%s_eref" % name]                       # [1 + T maps | 1 + T scalars][max, rms]
    figs = []
    table = table.cpu().numpy()
    assert np.isfinite(table).all()
    if want_maps:
        ent = ent.cpu().numpy()
        assert np.isfinite(ent).all()
        figs.append(gate(ent, ent64, eref[0].tolist(), name + " entropy map"))
        for t in range(T):
            m = err[:, t].cpu().numpy()
            assert np.array_equal(m == 0, masked) or types[t] != "abs", name + ": dilation mask / own-car cut"
            assert np.all(m[masked] == 0)
            figs.append(gate(m, maps64[:, t], eref[1 + t].tolist(), name + " map " + types[t]))
        if "abs" in types and "mask_" + name in g:                          # the reference's own dilate() on sample 0's mask
            assert np.array_equal(err[0, types.index("abs")].cpu().numpy() == 0, masked[0])
            ref_mask = g["mask_" + name].numpy().astype(bool)
            ref_mask[int(0.87 * Hh):] = True
            assert np.array_equal(masked[0], ref_mask)
    figs.append(gate(table[:, 0], ent64.mean(axis=(1, 2)), eref[1 + T].tolist(), name + " entropy_mean"))
    for t in range(T):
        figs.append(gate(table[:, 1 + t], maps64[:, t].mean(axis=(1, 2)), eref[2 + T + t].tolist(), name + " depth_error " + types[t]))
    return figs


def run_score_rejections(device):
    x = torch.zeros((1, 1, 8, 8), device=device)
    d = torch.zeros((1, 8, 8), device=device)
    for C in (1, 161):
        try:
            H.labelsel_score(torch.zeros((1, C, 8, 8), device=device), d, d, ["abs"])
            raise AssertionError("C = %d accepted" % C)
        except RuntimeError as e:
            assert "unsupported" in str(e)
    try:
        H.labelsel_score(x.expand(1, 19, 8, 8), d, d, ["nope"])
        raise AssertionError("unknown error type accepted")
    except NotImplementedError:
        pass


def run_pixel_wise_entropy(device):
    g = golden()
    x, _, _ = score_inputs("s23x40_c19")
    t = torch.from_numpy(x).to(device)
    ent64, _, _ = score_f64(x, x[:, 0], x[:, 0], [])
    e = pixel_wise_entropy(t)
    assert tuple(e.shape) == (1, 23, 40)
    gate(e.cpu().numpy(), ent64, g["score_s23x40_c19_eref"][0].tolist(), "pixel_wise_entropy")
    n = pixel_wise_entropy(t, normalize=True).cpu().numpy()
    n64 = (ent64 - ent64.min()) / (ent64.max() - ent64.min())
    gate(n, n64, g["pwe_norm_eref"].tolist(), "pixel_wise_entropy normalize=True")
    assert n.min() == 0 and n.max() == 1


# ------------------------------------------------------------------------------------------------------------------ pooling
POOL_SIZES, POOL_H = ((64, 128), (33, 65), (3, 5)), 4
POOL_CASES = [(hw, tr) for hw in POOL_SIZES for tr in H.POOL_TRANSFORMS]


def pool_input(hw):
    x = (rng(8, hw[0]).random((2, 3) + hw, dtype=np.float32) * 0.99 + 0.004).astype(np.float32)
    x[0, 0, 0, 0] = 0                                     # 1 / 0 = inf clamps to 80
    return x


def pool_transform_t(x, tr):
    if tr == "none":
        return x
    x = torch.clamp(1 / x, 0.1, 80)
    return torch.log(x) if tr == "log_inv_clamp" else x


def run_pool(device):
    g = golden()
    figs = []
    for k, (hw, tr) in enumerate(POOL_CASES):
        x = pool_input(hw)
        t32 = pool_transform_t(torch.from_numpy(x), tr)
        with np.errstate(divide="ignore"):
            t64 = pool_transform_t(torch.from_numpy(x).double(), tr)
        for lay in ("nchw", "cl"):
            for pool in ("avg", "max"):
                bank = torch.full((5, 3 * POOL_H * 2 * POOL_H + 2), -7.0, device=device)
                xl = layout(torch.from_numpy(x).to(device), lay)
                H.labelsel_pool(xl, POOL_H, bank, 2, pool, tr)
                got = bank.cpu()
                assert bool((got[:2] == -7).all()) and bool((got[4:] == -7).all()) and bool((got[:, -2:] == -7).all()), "rows / pitch"
                got = got[2:4, :-2]
                fn = torch.nn.functional.adaptive_avg_pool2d if pool == "avg" else torch.nn.functional.adaptive_max_pool2d
                want64 = fn(t64, (POOL_H, 2 * POOL_H)).flatten(1).numpy()
                what = "pool %s %dx%d %s %s" % (pool, hw[0], hw[1], tr, lay)
                if pool == "max" and tr != "log_inv_clamp":     # comparisons, one division and two clamps: exact
                    assert torch.equal(got, fn(t32, (POOL_H, 2 * POOL_H)).flatten(1)), what
                else:                                           # logf is not correctly rounded on either side: the 3x rule
                    figs.append(gate(got.numpy(), want64, g["pool_eref"][k][0 if pool == "avg" else 1].tolist(), what))
    return figs


# ------------------------------------------------------------------------------------------------------------------ host mirrors
def toy_scores(n, n_criteria, seed, with_maps=False):
    r = rng(9, seed)
    out = []
    for i in range(n):
        s = {"idx": torch.tensor(100 + i), "label_criterion": [torch.tensor(float(v)) for v in r.random(n_criteria).astype(np.float32)],
             "depth_error": [torch.tensor(float(v)) for v in r.random(n_criteria).astype(np.float32)],
             "entropy_mean": torch.tensor(float(r.random()))}
        if with_maps:
            s["depth_error_map"] = ["m%d_%d" % (i, c) for c in range(n_criteria)]
        out.append(s)
    return out


def run_choose_from_scores():
    g = golden()
    chosen, sc = LS.choose_samples_from_scores(toy_scores(20, 2, 0, True), 6)
    assert chosen == g["choose_scores_list2"].tolist()
    assert [s["used_label_criterion"] for s in sc] == [str(x) for x in g["choose_scores_list2_used"]]
    flat = toy_scores(20, 1, 1)
    for s in flat:
        s["label_criterion"] = s["label_criterion"][0]
    chosen, sc = LS.choose_samples_from_scores(flat, 5)
    assert chosen == g["choose_scores_flat"].tolist()
    assert [s["used_label_criterion"] for s in sc] == [str(x) for x in g["choose_scores_flat_used"]]


def run_initial_and_totals():
    g = golden()
    for k, ds in enumerate(("cityscapes", "camvid", "mapillary")):
        cfg = {"seed": 7 + k, "data": {"dataset": ds}}
        assert LS.get_n_total(cfg) == int(g["n_total"][k])
        state = np.random.get_state()[1].copy()
        assert LS.choose_initial_samples(cfg, 9, "random") == g["initial_random_%s" % ds].tolist()
        assert np.array_equal(np.random.get_state()[1], state), "the global numpy generator was left reseeded"
    try:
        LS.get_n_total({"data": {"dataset": "kitti"}})
        raise AssertionError
    except NotImplementedError:
        pass


# ------------------------------------------------------------------------------------------------------------------ end to end
IFP_N, IFP_C, IFP_H, IFP_CURRENT, IFP_ADD = 97, 24, 2, 2, 30


def ifp_scores(g):
    return [{"idx": torch.tensor(1000 + i), "label_criterion": [g["ifp_criterion"][i].clone()], "depth_error": [torch.tensor(0.5)],
             "entropy_mean": torch.tensor(0.25)} for i in range(IFP_N)]


IFP_ADD_SMALL = 12              # the interpreter run: one workgroup through two barriers per step


def run_ifp_selection(device, n_add=IFP_ADD):
    """the fixture bank (low intrinsic dimension: the reference's choice is stable, the generator asserts a 1e-4 relative lead of the
    winner at every step in float64) -> _calc_feature_distance -> choose_samples_from_ifp = the reference's chosen list"""
    g = golden()
    bank = g["ifp_bank"]
    feats = [bank[i].reshape(1, IFP_C, IFP_H, 2 * IFP_H).to(device) for i in range(IFP_N)]
    to_img = {i: 1000 + i for i in range(IFP_N)}
    to_row = {v: k for k, v in to_img.items()}
    initial = [1000 + int(i) for i in g["ifp_initial"].tolist()]
    for tag, bw, mult in (("plain", 0, None), ("bias", 1.0, None), ("preselect", 0, 2)):
        bias = [float(v) for v in g["ifp_bias"]]
        d = LS._calc_feature_distance(feats, bias, bw, 2, True, False)
        chosen, sc = LS.choose_samples_from_ifp(list(initial), ifp_scores(g), {"distances": 1.0 * d, "dist_i_to_img_idx": to_img,
                                                                                "img_idx_to_dist_i": to_row}, n_add, mult)
        want = g["ifp_chosen%d_%s" % (n_add, tag)].tolist()
        assert chosen == want, (tag, chosen, want)
        assert len(sc) == n_add and all("iterative_farthest_distance" in s for s in sc)


class _Once(torch.nn.Module):
    """forwards to the wrapped model and keeps the outputs per batch (keyed by its image indices): every part of the end-to-end
    case sees the same batches.  Checks what acquire_scores owes the model: no_grad, eval(), inputs on the model's device."""

    def __init__(self, model):
        super().__init__()
        self.model, self.seen, self.calls = model, {}, 0

    def forward(self, inputs):
        self.calls += 1
        key = tuple(inputs["idx"].tolist())
        dev = next(self.model.parameters()).device
        assert all(v.device == dev for k, v in inputs.items() if torch.is_tensor(v) and k != "idx"), "inputs on the model's device"
        if key not in self.seen:
            assert not torch.is_grad_enabled() and not self.model.training, "acquire_scores runs under no_grad in eval()"
            self.seen[key] = self.model(inputs)
        return self.seen[key]


def _tiny_models(device):
    from oracle import nets as N
    from model_cases import contract_cfgs
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    out = []
    for name, seed in (("r18_jsd", 1234), ("r18_mono", 4321)):
        cfg = contract_cfgs()["cfgs"][name]
        m = get_model(cfg, 19)
        m.load_state_dict(N.build_state_dict(cfg, 19, seed=seed, randomize_bn=True), strict=True)
        out.append(_Once(m.to(device)).train())
    return out


class _StandIn(torch.nn.Module):
    """the output dict of the joint model from three fixed random 3x3 convolutions in plain torch: the interpreter run drives
    acquire_scores and every kernel behind it without interpreting a ResNet (minutes per forward pass); the GPU run uses the
    real tiny models above"""

    def __init__(self, seed):
        super().__init__()
        r = rng(12, seed)
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(r.standard_normal((c, 3, 3, 3)).astype(np.float32)),
                                                            requires_grad=False) for c in (19, 1, 16)])

    def forward(self, inputs):
        x = inputs[("color_aug", 0, 0)] - 0.5
        conv = torch.nn.functional.conv2d
        feats = torch.nn.functional.avg_pool2d(conv(x, self.w[2], padding=1), 4)
        return {"semantics": conv(x, self.w[0], padding=1), ("disp", 0): torch.sigmoid(conv(x, self.w[1], padding=1)),
                ("upconv", 3): feats, ("upconv", 4): feats, "bottleneck": feats}


def _tiny_batches(device, n=8, bs=4, hw=(64, 128)):
    r = rng(10)
    batches = []
    for s in range(0, n, bs):
        img = torch.from_numpy(r.random((bs, 3) + hw, dtype=np.float32)).to(device)
        inp = {("color_aug", f, 0): img for f in (0, -1, 1)}
        inp.update({("color", f, 0): img for f in (0, -1, 1)})
        K = torch.eye(4)[None].repeat(bs, 1, 1)
        inp[("K", 0)], inp[("inv_K", 0)] = K.to(device), K.to(device)
        ds = (r.integers(10, 256, (bs, 1) + hw) / 255.0).astype(np.float32)
        inp["pseudo_depth"] = torch.from_numpy(ds).to(device)
        inp["idx"] = torch.tensor([500 + 7 * (s + k) for k in range(bs)])
        batches.append(inp)
    return batches


def score_ref32(x, dp, ds, types):
    """the reference's scoring expressions (loss/loss.py:40-47, label_selection.py:449-488) in fp32 torch on the CPU, batched:
    the e_ref of the end-to-end case, whose inputs -- the model's own outputs -- exist only at run time
    -> (entropy [B,H,W], maps [B,T,H,W]) as numpy"""
    x, dp, ds = torch.from_numpy(x), torch.from_numpy(dp), torch.from_numpy(ds)
    p = torch.softmax(x, dim=1)
    ent = -torch.sum(p * torch.log2(p + 1e-30), dim=1) / np.log2(x.shape[1])
    inv = lambda d: torch.clamp(1 / d, 0.1, 80)      # noqa: E731
    keep = 1 - torch.clamp(torch.nn.functional.conv2d((ds < 0.07).float()[:, None], torch.ones((1, 1, 7, 7)), padding=3), 0, 1)[:, 0]
    maps = []
    for t in types:
        m = {"abs": lambda: torch.abs(dp - ds), "abs_inv_log": lambda: torch.abs(torch.log(inv(ds)) - torch.log(inv(dp))),
             "abs_inv": lambda: torch.abs(inv(ds) - inv(dp)), "sq": lambda: (dp - ds) ** 2,
             "abs_rel": lambda: torch.abs(dp - ds) / (ds + 1e-1), "sq_rel": lambda: ((dp - ds) ** 2) / (ds + 1e-1),
             "abs_log": lambda: torch.abs(torch.log(1 + dp) - torch.log(1 + ds))}[t]() * keep
        m[:, int(0.87 * m.shape[1]):, :] = 0
        maps.append(m)
    return ent.numpy(), (torch.stack(maps, 1) if maps else torch.zeros((x.shape[0], 0) + tuple(ds.shape[1:]))).numpy()


def _to(b, device):
    return {k: (v.to(device) if torch.is_tensor(v) and k != "idx" else v) for k, v in b.items()}


def run_acquire_scores(device, stand_in=False):
    """8 samples at 64 x 128 in batches of 4 through the tiny ResNet-18 joint model and a ResNet-18 depth teacher
    (stand_in: through _StandIn modules, the interpreter run).  The batches live on the HOST, as a DataLoader yields them;
    every figure is held to the 3x rule, e_ref formed here by score_ref32 / torch.cdist on the same model outputs."""
    n, bs = 8, 4
    model, teacher = (_Once(_StandIn(0).to(device)).train(), _Once(_StandIn(1).to(device)).train()) if stand_in else _tiny_models(device)
    batches = _tiny_batches("cpu", n, bs)
    all_idx = [int(i) for b in batches for i in b["idx"]]
    to_score = all_idx[:1] + all_idx[2:]                  # one (current) sample is only a bias-less member of the bank
    types = ["abs", "abs_inv_log", "sq_rel"]
    cfg = {"depth_lambda": 1.0, "entropy_lambda": 0.5, "bias_weight": 0, "depth_error_types": types,
           "ifp_args": {"m": "u3", "pool": "avg", "h": 2, "p": 2, "norm": False}}      # norm: a dead channel of a random model is 0/0
    # (a) score mode, three error types, verbose maps
    scores, fd = LS.acquire_scores(model, batches, to_score, cfg, verbose=True)
    assert [int(s["idx"]) for s in scores] == to_score and fd["dist_i_to_img_idx"] == {}
    assert model.training and model.calls == len(batches), "the model's mode is restored; one forward pass per batch"
    assert all(not v.is_cuda for b in batches for v in b.values() if torch.is_tensor(v)), "the caller's batches were moved"
    with torch.no_grad():
        outs = [model(_to(b, device)) for b in batches]
    x = torch.cat([o["semantics"] for o in outs]).float().cpu().numpy()
    dp = torch.cat([o[("disp", 0)][:, 0] for o in outs]).float().cpu().numpy()
    ds = torch.cat([b["pseudo_depth"][:, 0] for b in batches]).cpu().numpy()
    ent64, maps64, _ = score_f64(x, dp, ds, types)
    ent32, maps32 = score_ref32(x, dp, ds, types)
    ks = [all_idx.index(int(s["idx"])) for s in scores]
    assert all(s["entropy_mean"].dim() == 0 and not s["entropy_mean"].is_cuda for s in scores)
    gate(np.stack([s["segmentation_entropy"].cpu().numpy() for s in scores]), ent64[ks], errors(ent32[ks], ent64[ks]), "e2e entropy maps")
    gate([float(s["entropy_mean"]) for s in scores], ent64[ks].mean(axis=(1, 2)),
         errors(torch.from_numpy(ent32[ks]).mean(dim=(1, 2)).numpy(), ent64[ks].mean(axis=(1, 2))), "e2e entropy_mean")
    for t in range(3):
        gate(np.stack([s["depth_error_map"][t].cpu().numpy() for s in scores]), maps64[ks, t], errors(maps32[ks, t], maps64[ks, t]),
             "e2e map " + types[t])
        gate([float(s["depth_error"][t]) for s in scores], maps64[ks, t].mean(axis=(1, 2)),
             errors(torch.from_numpy(maps32[ks, t]).mean(dim=(1, 2)).numpy(), maps64[ks, t].mean(axis=(1, 2))), "e2e depth_error " + types[t])
        for s in scores:
            want = 1.0 * s["depth_error"][t] + 0.5 * s["entropy_mean"]              # the reference's fp32 expression
            assert torch.equal(s["label_criterion"][t], want)
    chosen, _ = LS.choose_samples_from_scores(scores, 3)          # three criteria: one sample each
    assert len(set(chosen)) == 3
    # (b) ifp mode with a distance bias: the bank, the bias column, the maps, then a selection
    cfg2 = dict(cfg, depth_error_types="abs", bias_weight=0.25)
    scores, fd = LS.acquire_scores(model, batches, to_score, cfg2, depth_teacher=teacher, depth_ifp_w=2.0)
    assert fd["dist_i_to_img_idx"] == dict(enumerate(all_idx)) and fd["img_idx_to_dist_i"] == {v: k for k, v in enumerate(all_idx)}
    with torch.no_grad():
        feats = torch.cat([teacher(_to(b, device))[("upconv", 3)] for b in batches]).float().cpu()
    pooled = torch.nn.functional.adaptive_avg_pool2d(feats.double(), (2, 4)).numpy()
    bias = np.zeros(n)
    for s in scores:
        bias[all_idx.index(int(s["idx"]))] = float(np.float32(0.25) * s["label_criterion"][0].numpy())
    d64 = 2.0 * cfd_f64(pooled, bias, 1, 2, False)
    d = fd["distances"].cpu().numpy()
    assert np.all(np.diag(d) == 0)
    flat32 = torch.nn.functional.adaptive_avg_pool2d(feats, (2, 4)).flatten(1)
    d32 = torch.cdist(flat32, flat32, p=2) + torch.tensor(bias, dtype=torch.float32)
    gate(offdiag(d), offdiag(d64), errors(offdiag((2.0 * d32).numpy()), offdiag(d64)), "e2e distances")
    same, fd_dev = LS.acquire_scores(model, [_to(b, device) for b in batches], to_score, cfg2, depth_teacher=teacher, depth_ifp_w=2.0)
    assert torch.equal(fd_dev["distances"], fd["distances"]), "device-resident batches give another result than host batches"
    assert all(torch.equal(a["label_criterion"][0], b["label_criterion"][0]) for a, b in zip(same, scores))
    chosen, sc = LS.choose_samples_from_ifp(all_idx[:2], scores, fd, 2, None)
    assert len(chosen) == 2 and not set(chosen) & set(all_idx[:2])
    # (c) ifp without bias: no model run, zero scores for every sample (the reference's shortcut)
    scores, fd = LS.acquire_scores(None, batches, all_idx, dict(cfg, bias_weight=0), depth_teacher=teacher, depth_ifp_w=1.0)
    assert len(scores) == n and all(s["label_criterion"] == [0] for s in scores)
    # (d) the depth modes fill the bank from the pseudo-disparity
    for mode in ("depth", "logdepth"):
        c3 = dict(cfg, bias_weight=0, ifp_args={"m": mode, "pool": "max", "h": 2, "p": 1, "norm": False})
        _, fd = LS.acquire_scores(None, batches, all_idx, c3, depth_ifp_w=1.0, device=device)
        assert fd["distances"].device.type == torch.device(device).type
        assert tuple(fd["distances"].shape) == (n, n) and bool(torch.isfinite(fd["distances"]).all())
    # (e) list-valued lambdas: one criterion per pair, the depth error repeated behind the first entry
    c4 = dict(cfg, depth_error_types="abs", depth_lambda=[1.0, 0.0], entropy_lambda=[0.0, 1.0])
    scores, _ = LS.acquire_scores(model, batches, to_score, c4)
    s = scores[0]
    assert len(s["label_criterion"]) == 2 and len(s["depth_error"]) == 3
    assert torch.equal(s["label_criterion"][0], 1.0 * s["depth_error"][0] + 0.0 * s["entropy_mean"])
    chosen, _ = LS.choose_samples_from_scores(scores, 2)
    assert len(set(chosen)) == 2


def run_torch_ops(device):
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    assert "segsde::labelsel_distance" in TO.names() and "segsde::labelsel_farthest_point" in TO.names()
    bank = torch.from_numpy(dist_bank(65, 7)).to(device)
    d = torch.ops.segsde.labelsel_distance(bank, 2, None)
    assert torch.equal(d, H.labelsel_distance(bank, 2))
    idx, dist = torch.ops.segsde.labelsel_farthest_point(d, torch.tensor([3]), 4, None)
    want_i, want_d = H.labelsel_farthest_point(d, [3], 4)
    assert idx.tolist() == want_i and torch.equal(dist, want_d)
    g = bank.clone().requires_grad_(True)
    for call in (lambda: torch.ops.segsde.labelsel_distance(g, 2, None),
                 lambda: torch.ops.segsde.labelsel_farthest_point(d.clone().requires_grad_(True), torch.tensor([3]), 4, None)):
        try:
            call()
            raise AssertionError("a forward-only operator took an input that requires grad")
        except RuntimeError as e:
            assert "forward only" in str(e)
    with torch.no_grad():
        assert torch.equal(torch.ops.segsde.labelsel_distance(g, 2, None), d)
