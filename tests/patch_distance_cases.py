"""Patch-wise (directed Chamfer) feature distances (label_selection.patch_feature_distance, section 4b of csrc/labelsel.hip):
the cases shared by the interpreter run (test_patch_distance_emu.py), the GPU run (test_patch_distance_gpu.py), the fixture
generator (tests/golden/make_patch_distance.py, which feeds the SAME seeded inputs to the reference's
``_calc_feature_distance(..., patch_wise=True)`` and records what it returns) and the measurement tool (tools/patch_distance.py).

Inputs come by seed; tests/golden/patch_distance.npz holds results only: e_ref = (max, rms) error of the reference's fp32
evaluation against the float64 evaluation ``patch_f64`` below per case, the NaN pattern of a constant-channel case under
normalisation, and the reference's chosen lists of the selection case.  The package's error against the same float64 goes
through the 3x rule of label_selection_cases.gate (never tighter than 4 ulp of fp32); discrete properties are compared exactly."""
import numpy as np
import torch

import label_selection_cases as LC
from conftest import load_golden
from label_selection_cases import gate, errors, ulp32, rng, offdiag, _StandIn, _Once, _tiny_batches, golden      # noqa: F401
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
from improving_segmentation_with_selfsupervised_depth_amd import label_selection as LS

_G = {}


def fixture():
    if "g" not in _G:
        _G["g"] = load_golden("patch_distance")
    return _G["g"]


# (N, C, (H, W)): P = H * W patches per image; a block of the kernel takes 64 // P images (one when P > 64)
CASES = [
    (1, 3, (1, 2)),          # smallest N
    (2, 1, (1, 1)),          # P = 1, C = 1
    (3, 7, (2, 4)),          # small
    (33, 33, (3, 6)),        # P = 18 does not divide the tile (3 images, 54 of 64 rows); C is one past a chunk of 32
    (65, 24, (2, 4)),        # N is one past 64
    (17, 70, (4, 8)),        # the real P = 32
    (9, 130, (4, 8)),        # five chunks
    (12, 40, (5, 10)),       # P = 50: one image per tile
    (5, 16, (8, 16)),        # P = 128, the cap: 2 x 2 sub-tiles, running minima (640 patch rows, the largest case)
]
GRID = [(k, p, norm) for k in range(len(CASES)) for p in (1, 2) for norm in (False, True)
        if not (norm and CASES[k][0] * CASES[k][2][0] * CASES[k][2][1] < 2)]      # a std over one element is 0/0


def features(N, C, hw, const_channel=None):
    """channels of very different scale and offset, as label_selection_cases.cfd_features"""
    f = rng(20, N, C, hw[0], hw[1]).standard_normal((N, C) + tuple(hw)).astype(np.float32)
    f *= np.linspace(0.5, 20.0, C, dtype=np.float32)[None, :, None, None]
    f += np.linspace(-30.0, 30.0, C, dtype=np.float32)[None, :, None, None]
    if const_channel is not None:
        f[:, const_channel] = 1.25
    return f


def normalize_f64(f):
    f = f.astype(np.float64)
    mean = f.mean(axis=(0, 2, 3), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (f - mean) / f.std(axis=(0, 2, 3), keepdims=True, ddof=1)


def patch_f64(f, bias, bias_weight, p, norm):
    """f [N,C,H,W] -> D[i,j] = mean_a min_b ||f[i,:,a] - f[j,:,b]||_p in float64 (+ bias[j], zero diagonal); NaN propagates
    through np.min as through torch.min"""
    f = normalize_f64(f) if norm else f.astype(np.float64)
    N, C = f.shape[:2]
    v = f.reshape(N, C, -1).transpose(0, 2, 1)                # [N, P, C]
    out = np.empty((N, N))
    with np.errstate(invalid="ignore"):
        for i in range(N):
            d = np.abs(v[i][:, None, None, :] - v[None])      # [P(a), N(j), P(b), C]
            d = np.sqrt((d * d).sum(-1)) if p == 2 else d.sum(-1)
            out[i] = d.min(-1).mean(0)
    if bias_weight > 0:
        out = out + np.asarray(bias, dtype=np.float32).astype(np.float64)[None, :]
    np.fill_diagonal(out, 0)
    return out


def patch_ref32(f, p):
    """the reference's formulation (chunks of 200 images of torch.cdist over the [N*P, C] patch vectors, min over the patches of
    the other image, mean over the own) in fp32 torch on the CPU: the e_ref of the end-to-end case, whose inputs exist only
    at run time.  f: float32 tensor [N,C,H,W] -> [N,N] tensor"""
    N, C = f.shape[:2]
    P = f.shape[2] * f.shape[3]
    v = f.reshape(N, C, P).permute(0, 2, 1).reshape(N * P, C)
    rows = []
    for s in range(0, N, 200):
        n = min(200, N - s)
        d = torch.cdist(v[s * P:(s + n) * P], v, p=p).reshape(n, P, N, P).permute(0, 2, 1, 3)
        rows.append(d.min(dim=-1).values.mean(dim=-1))
    return torch.cat(rows)


def as_list(f, device):
    return [torch.from_numpy(f[i:i + 1]).to(device) for i in range(f.shape[0])]


def run_case(device, k, p, norm):
    """check 1: the error gate of one (case, p, normalisation) and the exact zero diagonal"""
    N, C, hw = CASES[k]
    f = features(N, C, hw)
    out = LS.patch_feature_distance(as_list(f, device), [], 0, p, norm).cpu().numpy()
    assert out.shape == (N, N) and out.dtype == np.float32
    assert np.all(np.diag(out) == 0)
    e_ref = fixture()["eref"][GRID.index((k, p, norm))].tolist()
    return gate(offdiag(out), offdiag(patch_f64(f, [], 0, p, norm)), e_ref,
                "patch distance N=%d C=%d P=%dx%d p=%d norm=%d" % (N, C, hw[0], hw[1], p, norm))


def _bits(t):
    return t.contiguous().view(torch.int32)


PERM_CASES = [(19, 5, (2, 4)), (5, 9, (3, 6)), (5, 6, (8, 16))]      # 8 images per block and 3 blocks; P = 18; P = 128 (sub-tiles)
CONST_CASE = (5, 7, (2, 4), 3)                                      # N, C, (H, W), the constant channel


def run_properties(device):
    """check 2: the discrete properties, exact"""
    for N, C, hw in PERM_CASES:
        P = hw[0] * hw[1]
        f = features(N, C, hw).reshape(N, C, P)
        r = rng(21, N, P)
        src, dst, sub = 1, N - 2, 2
        f[dst] = f[src][:, r.permutation(P)]                  # the same set of patches in another order
        f[sub] = f[0][:, np.r_[np.arange(P - 1), 0]]          # the patches of 2 are a subset of those of 0 (one repeated)
        assert len({0, src, sub, dst}) == 4 and not np.array_equal(f[dst], f[src])
        bank = torch.from_numpy(f.reshape(N, C * P)).to(device)
        for p in (1, 2):
            d = H.labelsel_patch_distance(bank, C, P, p)
            assert d[src, dst] == 0 and d[dst, src] == 0, (N, P, p)
            assert d[sub, 0] == 0 and d[0, sub] > 0, (N, P, p)
            assert torch.equal(_bits(d), _bits(H.labelsel_patch_distance(bank, C, P, p))), "two runs give other bits"
            # the order of the patches of image j does not change a bit of column j
            for j in (0, dst, N - 1):
                g = f.copy()
                g[j] = g[j][:, r.permutation(P)]
                d2 = H.labelsel_patch_distance(torch.from_numpy(g.reshape(N, C * P)).to(device), C, P, p)
                assert torch.equal(_bits(d2[:, j]), _bits(d[:, j])), (N, P, p, j)
                keep = [i for i in range(N) if i != j]
                assert torch.equal(_bits(d2[keep][:, keep]), _bits(d[keep][:, keep])), (N, P, p, j)
            # column bias: one fp32 addition per entry, zero diagonal
            bias = torch.from_numpy(rng(22, N, p).random(N, dtype=np.float32)).to(device)
            want = d + bias[None, :]
            want.fill_diagonal_(0)
            assert torch.equal(H.labelsel_patch_distance(bank, C, P, p, bias), want)
            # pitched bank, pitched out: the same bits, the columns past N untouched
            wide = torch.zeros((N, C * P + 5), device=device)
            wide[:, :C * P] = bank
            assert torch.equal(_bits(H.labelsel_patch_distance(wide[:, :C * P], C, P, p)), _bits(d))
            buf = torch.full((N, N + 6), -7.0, device=device)
            H.labelsel_patch_distance(bank, C, P, p, out=buf[:, :N])
            assert torch.equal(_bits(buf[:, :N]), _bits(d)) and bool((buf[:, N:] == -7.0).all())
            assert not torch.equal(d, d.t()), "the directed distance is not symmetric"
    # P = 1: the pair distance itself, bitwise symmetric
    f = features(70, 33, (1, 1))
    for p in (1, 2):
        d = H.labelsel_patch_distance(torch.from_numpy(f.reshape(70, 33)).to(device), 33, 1, p)
        assert torch.equal(_bits(d), _bits(d.t().contiguous())) and bool((d.diagonal() == 0).all())
    # a constant channel under normalisation: 0/0 = NaN in every distance, as the reference gives; the bank stays as it was
    N, C, hw, ch = CONST_CASE
    fc = features(N, C, hw, const_channel=ch)
    feats = as_list(fc, device)
    out = LS.patch_feature_distance(feats, [], 0, 2, True).cpu()
    assert torch.equal(torch.isnan(out), fixture()["const_isnan"].bool())
    assert bool(torch.isnan(out).any()) and bool((torch.diagonal(out) == 0).all())
    assert all(torch.equal(t.cpu(), torch.from_numpy(fc[i:i + 1])) for i, t in enumerate(feats)), "the caller's features were modified"
    # a single NaN feature: exactly the row and the column of its image
    fn = features(6, 4, (2, 4))
    fn[2, 1, 0, 3] = np.nan
    out = LS.patch_feature_distance(as_list(fn, device), [], 0, 1, False).cpu()
    want = torch.zeros((6, 6), dtype=torch.bool)
    want[2, :] = want[:, 2] = True
    want[2, 2] = False
    assert torch.equal(torch.isnan(out), want)
    # a FeatureBank argument gives the list's matrix and is not normalised in place
    N, C, hw = 9, 6, (2, 4)
    f = features(N, C, hw)
    fb = LS.FeatureBank(N, C, 2, "avg", "u3", device)
    fb.add(torch.from_numpy(f).to(device), list(range(N)))    # bins of one pixel: the identity
    assert torch.equal(_bits(LS.patch_feature_distance(fb, [], 0, 2, True)), _bits(LS.patch_feature_distance(as_list(f, device), [], 0, 2, True)))
    assert torch.equal(fb.features().cpu(), torch.from_numpy(f.reshape(N, -1))), "the bank was normalised in place"


def run_refusals(device):
    """check 3: P = 162 and p = 3 raise NotImplementedError from hipops; the library's own codes"""
    for call in (lambda: LS.patch_feature_distance([torch.zeros((1, 2, 9, 18), device=device)] * 2, [], 0, 2, False),
                 lambda: LS.patch_feature_distance([torch.zeros((1, 2, 2, 4), device=device)] * 2, [], 0, 3, False),
                 lambda: H.labelsel_patch_distance(torch.zeros((2, 2 * 162), device=device), 2, 162),
                 lambda: H.labelsel_patch_distance(torch.zeros((2, 16), device=device), 2, 8, 3)):
        try:
            call()
            raise AssertionError("accepted")
        except NotImplementedError:
            pass
    try:
        H.labelsel_patch_distance(torch.zeros((2, 17), device=device), 2, 8)
        raise AssertionError("a bank that is not [N, C*P] accepted")
    except ValueError:
        pass
    bank, out = torch.zeros((2, 2 * 162), device=device), torch.zeros((2, 2), device=device)
    L = H._lib.lib()
    assert L.segsde_labelsel_patch_distance(H._p(bank), 324, 2, 2, 162, 2, None, H._p(out), 2, H._stream(bank)) == -4
    assert L.segsde_labelsel_patch_distance(H._p(bank), 324, 2, 2, 8, 3, None, H._p(out), 2, H._stream(bank)) == -4
    assert L.segsde_labelsel_patch_distance(H._p(bank), 15, 2, 2, 8, 2, None, H._p(out), 2, H._stream(bank)) == -2


# ------------------------------------------------------------------------------------------------------------------ selection
SEL_N, SEL_C, SEL_HW = LC.IFP_N, LC.IFP_C, (LC.IFP_H, 2 * LC.IFP_H)
SEL_ADDS = (LC.IFP_ADD_SMALL, LC.IFP_ADD)
SEL_VARIANTS = (("plain", 0, None), ("bias", 1.0, None), ("preselect", 0, 2))


def sel_inputs(seed):
    """-> (features [N,C,H,W], criterion [N], bias [N]) float32.  seed 0: the bank of the label-selection fixture (low
    intrinsic dimension); any other seed: a bank of the same recipe from the generator here"""
    if seed == 0:
        g = golden()
        return (g["ifp_bank"].numpy().reshape((SEL_N, SEL_C) + SEL_HW), g["ifp_criterion"].numpy(), g["ifp_bias"].numpy())
    r = rng(23, seed)
    D = SEL_C * SEL_HW[0] * SEL_HW[1]
    latent, proj = r.random((SEL_N, 2)), r.standard_normal((2, D))
    bank = (latent[:, :1] * proj[0] + latent[:, 1:] * proj[1] + 0.01 * r.standard_normal((SEL_N, D))).astype(np.float32)
    crit = r.random(SEL_N).astype(np.float32)
    return bank.reshape((SEL_N, SEL_C) + SEL_HW), crit, (np.float32(0.5) * crit).astype(np.float32)


def sel_scores(crit):
    return [{"idx": torch.tensor(1000 + i), "label_criterion": [torch.tensor(crit[i])], "depth_error": [torch.tensor(0.5)],
             "entropy_mean": torch.tensor(0.25)} for i in range(SEL_N)]


def run_selection(device, n_add):
    """check 4: patch_feature_distance -> choose_samples_from_ifp = the reference's chosen list (the generator asserts a 1e-4
    relative lead of every winner in float64)"""
    g = fixture()
    f, crit, bias = sel_inputs(int(g["sel_seed"]))
    feats = as_list(f, device)
    to_img = {i: 1000 + i for i in range(SEL_N)}
    to_row = {v: k for k, v in to_img.items()}
    initial = [1000 + int(i) for i in g["sel_initial"].tolist()]
    for tag, bw, mult in SEL_VARIANTS:
        d = LS.patch_feature_distance(feats, [float(v) for v in bias], bw, 2, True)
        chosen, sc = LS.choose_samples_from_ifp(list(initial), sel_scores(crit), {"distances": 1.0 * d, "dist_i_to_img_idx": to_img,
                                                                                    "img_idx_to_dist_i": to_row}, n_add, mult)
        want = g["sel_chosen%d_%s" % (n_add, tag)].tolist()
        assert chosen == want, (tag, chosen, want)
        assert len(sc) == n_add and all("iterative_farthest_distance" in s for s in sc)


# ------------------------------------------------------------------------------------------------------------------ end to end
def run_acquire_scores(device, stand_in=False):
    """check 5: acquire_scores with pw: True -- 8 samples at 64 x 128 in batches of 4 through the tiny ResNet-18 pair (stand_in:
    the _StandIn modules, the interpreter run); the distances against float64 with e_ref formed here by patch_ref32 on the same
    model outputs; then a selection on the result.  Fails on the parent commit with NotImplementedError."""
    n, bs = 8, 4
    model, teacher = (_Once(_StandIn(0).to(device)).train(), _Once(_StandIn(1).to(device)).train()) if stand_in else LC._tiny_models(device)
    batches = _tiny_batches("cpu", n, bs)
    all_idx = [int(i) for b in batches for i in b["idx"]]
    to_score = all_idx[:1] + all_idx[2:]
    cfg = {"depth_lambda": 1.0, "entropy_lambda": 0.5, "bias_weight": 0.25, "depth_error_types": "abs",
           "ifp_args": {"m": "u3", "pool": "avg", "h": 2, "p": 2, "norm": False, "pw": True}}
    scores, fd = LS.acquire_scores(model, batches, to_score, cfg, depth_teacher=teacher, depth_ifp_w=2.0)
    assert fd["dist_i_to_img_idx"] == dict(enumerate(all_idx))
    with torch.no_grad():
        feats = torch.cat([teacher(LC._to(b, device))[("upconv", 3)] for b in batches]).float().cpu()
    pooled = torch.nn.functional.adaptive_avg_pool2d(feats.double(), (2, 4)).numpy()
    bias = np.zeros(n)
    for s in scores:
        bias[all_idx.index(int(s["idx"]))] = float(np.float32(0.25) * s["label_criterion"][0].numpy())
    d64 = 2.0 * patch_f64(pooled, bias, 1, 2, False)
    d = fd["distances"].cpu().numpy()
    assert d.shape == (n, n) and np.all(np.diag(d) == 0)
    d32 = patch_ref32(torch.nn.functional.adaptive_avg_pool2d(feats, (2, 4)), 2) + torch.tensor(bias, dtype=torch.float32)
    gate(offdiag(d), offdiag(d64), errors(offdiag((2.0 * d32).numpy()), offdiag(d64)), "e2e patch distances")
    # the plain matrix of the same run differs: the option is not ignored
    _, fd_plain = LS.acquire_scores(model, batches, to_score, dict(cfg, ifp_args=dict(cfg["ifp_args"], pw=False)), depth_teacher=teacher,
                                    depth_ifp_w=2.0)
    assert not torch.equal(fd_plain["distances"], fd["distances"])
    chosen, sc = LS.choose_samples_from_ifp(all_idx[:2], scores, fd, 2, None)
    assert len(chosen) == 2 and not set(chosen) & set(all_idx[:2])


def run_torch_ops(device):
    """check 6"""
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    assert "segsde::labelsel_patch_distance" in TO.names()
    f = features(9, 5, (3, 6))
    bank = torch.from_numpy(f.reshape(9, -1)).to(device)
    bias = torch.from_numpy(rng(24).random(9, dtype=np.float32)).to(device)
    d = torch.ops.segsde.labelsel_patch_distance(bank, 5, 18, 1, bias)
    assert torch.equal(_bits(d), _bits(H.labelsel_patch_distance(bank, 5, 18, 1, bias)))
    assert torch.equal(_bits(torch.ops.segsde.labelsel_patch_distance(bank, 5, 18)), _bits(H.labelsel_patch_distance(bank, 5, 18, 2)))
    g = bank.clone().requires_grad_(True)
    try:
        torch.ops.segsde.labelsel_patch_distance(g, 5, 18, 2, None)
        raise AssertionError("a forward-only operator took an input that requires grad")
    except RuntimeError as e:
        assert "forward only" in str(e)
    with torch.no_grad():
        assert torch.equal(_bits(torch.ops.segsde.labelsel_patch_distance(g, 5, 18, 1, bias)), _bits(d))
