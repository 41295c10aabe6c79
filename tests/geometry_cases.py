"""The parts of the self-supervised depth path that only a golden vector at one tiny shape pinned: edge-aware smoothness
(csrc/loss.hip: smooth_* / plane_* kernels, mean-normalised and plain), the pose matrix (csrc/pose.hip), the stand-alone geometry
layers (csrc/geometry.hip: SSIM map, BackprojectDepth, Project3D and their adjoints) and disp_to_depth_upsampled -- against a float64
evaluation of the same operation, at the shapes where these kernels take another path (several blocks per image with B > 1, the
512-block cap, a second block of 64 poses, mirrored pixels that enter a 3x3 window twice).  And the lifetime of the operands the
Python wrappers hand to the kernels (``run_operand_lifetime``).  Shared by tests/test_geometry_gpu.py (real library) and
tests/test_geometry_emu.py (interpreter build of the same sources).

Reference: oracle.geometry / oracle.photometric and plain torch under autograd, run twice, in float64 (the truth) and in float32
(what plain fp32 arithmetic achieves); it calls nothing of the package under test.  Every compared tensor obeys the project's rule
for re-associated routes (tests/photometric_cases.py)

    max|kernel - f64| <= 3 * max|fp32 oracle - f64| + 1e-6 * max|f64|

and no other tolerance exists here.  The operations are piecewise smooth (|.| in the smoothness, the clamp in SSIM); the conditions
that keep a case off the kinks are computed from float64 alone and asserted, at seeds found once on the CPU (SEEDS)."""
import functools

import torch
import torch.nn.functional as F

from oracle import geometry as G, photometric as P
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn, hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.loader import device_batch as DB
from improving_segmentation_with_selfsupervised_depth_amd.models import monodepth_layers as ML

MIN_DEPTH, MAX_DEPTH = 0.1, 100.0
RECORDS = []            # (case, tensor, e_kernel, e_oracle, scale, ok)
NOTES = []              # (kind, text): the figures that are not records (tie share, seeds in use, lifetime outcome)

# ---------------------------------------------------------------------------------------------------------------- the cases
# smoothness (B, h, w, kind).  "ranges": per-image disparity ranges 0.05 / 1 / 7 (a wrong batch index in the mean or the partials
# shows); "lattice": multiples of 1/8, many exact ties between neighbours; 2 x 65600 = 131 200 pixels = 513 blocks of 256, above the
# 512-block cap: the grid-stride loop runs and smooth_finalize_kernel folds 512 partials
SMOOTH = {"2x2x2": (2, 2, 2, "random"), "3x17x37": (3, 17, 37, "ranges"), "1x2x700": (1, 2, 700, "random"),
          "3x40x2": (3, 40, 2, "random"), "2x24x40-lattice": (2, 24, 40, "lattice"), "1x2x65600": (1, 2, 65600, "random")}
SMOOTH_SCALES = (0.37, 1e-3 / 4)        # the upstream weight of the backward: arbitrary, and disparity_smoothness / 2**2
TIE_GAP = 1e-5                          # random cases: |d_p - d_q| is 0 or at least this share of the image's mean
TIE_SHARE = 0.10                        # lattice case: at least this share of the neighbour pairs are exact ties
POSE_MAGS = (3.1, 0.3, 1e-2, 1e-3, 1e-4, 1e-5, 0.0)
POSE_B = (5, 70)                        # 70: a second block of 64 threads
SSIM_SHAPES = {"1x1x2x2": (1, 1, 2, 2), "2x3x2x5": (2, 3, 2, 5), "1x3x3x2": (1, 3, 3, 2), "2x3x9x13": (2, 3, 9, 13),
               "1x2x17x37": (1, 2, 17, 37)}
SSIM_GAP = 1e-6                         # no window's unclamped value this close to the clamp limits 0 and 1
PROJ_SHAPES = {"1x2x2": (1, 2, 2), "3x6x10": (3, 6, 10), "3x17x37": (3, 17, 37), "2x2x300": (2, 2, 300)}
MIN_Z = 0.1                             # third camera coordinate of every projected point
D2D_SHAPES = [(1, 1, 4, 6), (2, 3, 9, 13), (14, 38, 27, 75), (5, 7, 5, 7)]      # (hs, ws, H, W), B = 2
# found by find_seeds() on the CPU from float64 alone: the first seed at which every condition the case asserts holds
SEEDS = {"smooth 2x2x2": 0, "smooth 3x17x37": 0, "smooth 1x2x700": 0, "smooth 3x40x2": 0, "smooth 2x24x40-lattice": 0,
         "smooth 1x2x65600": 0, "ssim 1x1x2x2": 0, "ssim 2x3x2x5": 0, "ssim 1x3x3x2": 0, "ssim 2x3x9x13": 0, "ssim 1x2x17x37": 0,
         "ssim near-equal": 0, "proj 1x2x2": 0, "proj 3x6x10": 0, "proj 3x17x37": 0, "proj 2x2x300": 0}


# ----------------------------------------------------------------------------------------------------------------- comparison
def check(case, name, got, r32, r64):
    g, a, b = got.detach().double().cpu().reshape(r64.shape), r32.detach().double().cpu(), r64.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), (case, name, "not finite")
    e_k, e_o, sc = float((g - b).abs().max()), float((a - b).abs().max()), float(b.abs().max())
    ok = e_k <= 3 * e_o + 1e-6 * sc
    RECORDS.append((case, name, e_k, e_o, sc, ok))
    print("GEOM-EDGE | %s | %s | %.3e | %.3e | %.3e | %s" % (case, name, e_k, e_o, sc, "ok" if ok else "MISSES THE RULE"))
    return ok


def finish(first):
    bad = [r for r in RECORDS[first:] if not r[-1]]
    assert not bad, "max|kernel - f64| > 3 * max|fp32 oracle - f64| + 1e-6 * max|f64|: %s" % (bad,)


def note(kind, text):
    NOTES.append((kind, text))
    print("GEOM-EDGE-SET | %s | %s" % (kind, text))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------- smoothness
def smooth_inputs(name, seed):
    B, h, w, kind = SMOOTH[name]
    gen = _gen(seed)
    if kind == "lattice":
        disp = torch.randint(1, 6, (B, 1, h, w), generator=gen).float() / 8
    else:
        rng = torch.tensor([0.05, 1.0, 7.0])[:B].reshape(B, 1, 1, 1) if kind == "ranges" else 1.0
        disp = 0.05 + rng * torch.rand(B, 1, h, w, generator=gen)
    return dict(disp=disp, img=torch.rand(B, 3, h, w, generator=gen), base=torch.randn(B, 1, h, w, generator=gen), kind=kind, seed=seed)


def neighbour_gaps(disp):
    """float64: |d_p - d_q| of every horizontal and vertical neighbour pair, as a share of the image's mean disparity"""
    d = disp.double()
    m = d.mean((1, 2, 3), keepdim=True)
    return torch.cat([((d[..., :, :-1] - d[..., :, 1:]).abs() / m).reshape(-1), ((d[..., :-1, :] - d[..., 1:, :]).abs() / m).reshape(-1)])


def smooth_condition(c):
    """random cases: no pair of neighbours is closer than TIE_GAP of the mean without being an exact tie (no pixel is excluded);
    lattice case: the exact ties are at least TIE_SHARE of the pairs.  -> (holds, tie share)"""
    gaps = neighbour_gaps(c["disp"])
    ties = float((gaps == 0).double().mean())
    if c["kind"] == "lattice":
        return ties >= TIE_SHARE, ties
    return bool(((gaps == 0) | (gaps >= TIE_GAP)).all()), ties


def smooth_reference(dtype, disp, img, normalised):
    """-> (loss, per-image mean [B], d loss / d disp) under autograd"""
    d = disp.detach().cpu().to(dtype).requires_grad_(True)
    im = img.detach().cpu().to(dtype)
    mean = d.mean(2, True).mean(3, True)
    loss = P.edge_aware_smoothness(d / (mean + 1e-7), im) if normalised else P.edge_aware_smoothness(d, im)
    loss.backward()
    return loss.detach(), mean.detach().reshape(-1), d.grad


@functools.lru_cache(maxsize=None)
def _smooth_case(name):
    c = smooth_inputs(name, SEEDS["smooth " + name])
    c["ref"] = {(dt, nrm): smooth_reference(dt, c["disp"], c["img"], nrm) for dt in (torch.float32, torch.float64) for nrm in (True, False)}
    return c


def run_smoothness(device, name):
    first = len(RECORDS)
    c = _smooth_case(name)
    holds, ties = smooth_condition(c)
    note("smooth " + name, "seed %d | exact ties %.1f %% of the neighbour pairs" % (c["seed"], 100 * ties))
    assert holds, ("smooth " + name, "neighbour-gap condition does not hold at the recorded seed")
    disp, img = c["disp"].to(device), c["img"].to(device)
    for nrm, tag in ((True, "smooth %s normalised" % name), (False, "smooth %s plain" % name)):
        (l32, m32, g32), (l64, m64, g64) = c["ref"][(torch.float32, nrm)], c["ref"][(torch.float64, nrm)]
        if nrm:
            loss, mean = H.smoothness_forward(disp, img)
            check(tag, "mean", mean, m32, m64)
        else:
            loss = H.smooth_loss_forward(disp, img)
        check(tag, "loss", loss, l32.reshape(1), l64.reshape(1))
        for scale in SMOOTH_SCALES:
            # the training-path adjoint accumulates: a base of the gradient's magnitude, the fp32 oracle does the same addition
            base = c["base"] * float((scale * g64).abs().max())
            if nrm:
                got = base.to(device).clone()
                H.smoothness_backward(disp, img, mean, scale, got)
                check(tag, "base + %.3g * d disp" % scale, got, base + scale * g32, base.double() + scale * g64)
            else:
                check(tag, "%.3g * d disp" % scale, H.smooth_loss_backward(disp, img, scale), scale * g32, scale * g64)
    finish(first)


def run_get_smooth_loss(device):
    """the public layer: B = 1 and B = 64 within the rule, B = 65 raises (the unit-mean table of the plain entry points holds 64)"""
    first = len(RECORDS)
    for B in (1, 64):
        gen = _gen(B)
        disp, img = 0.05 + torch.rand(B, 1, 5, 7, generator=gen), torch.rand(B, 3, 5, 7, generator=gen)
        (l32, _, g32), (l64, _, g64) = (smooth_reference(dt, disp, img, False) for dt in (torch.float32, torch.float64))
        d = disp.to(device).requires_grad_(True)
        loss = ML.get_smooth_loss(d, img.to(device))
        loss.backward()
        check("get_smooth_loss B=%d" % B, "loss", loss, l32, l64)
        check("get_smooth_loss B=%d" % B, "d disp", d.grad, g32, g64)
    gen = _gen(65)
    disp, img = (0.05 + torch.rand(65, 1, 5, 7, generator=gen)).to(device), torch.rand(65, 3, 5, 7, generator=gen).to(device)
    for call in (lambda: ML.get_smooth_loss(disp, img), lambda: H.smooth_loss_backward(disp, img, 1.0)):
        try:
            out = call()
        except RuntimeError as e:
            assert "bad shape" in str(e), e
        else:
            raise AssertionError("B = 65 returned %r instead of raising" % (out,))
    finish(first)


# ----------------------------------------------------------------------------------------------------------------------- pose
def pose_inputs(B, mag, seed=0):
    """[B,2,1,3] operands: frame 0 carries the pose (|axisangle| = mag in a random direction; element 0 is axis-aligned, two exact
    zero components), frame 1 is filled with 7.0 / -3.0 and must not matter"""
    gen = _gen(seed)
    dirs = torch.randn(B, 3, generator=gen, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    dirs[0] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    aa = torch.full((B, 2, 1, 3), 7.0)
    tr = torch.full((B, 2, 1, 3), -3.0)
    aa[:, 0, 0] = (mag * dirs).float()
    tr[:, 0, 0] = 0.3 * torch.randn(B, 3, generator=gen)
    return aa, tr, torch.randn(B, 4, 4, generator=gen)


def pose_reference(dtype, aa, tr, dM, invert):
    a, t = aa[:, 0].detach().cpu().to(dtype).requires_grad_(True), tr[:, 0].detach().cpu().to(dtype).requires_grad_(True)
    M = G.pose_matrix(a, t, invert)
    (M * dM.detach().cpu().to(dtype)).sum().backward()
    return M.detach(), a.grad, t.grad


def run_pose(device, B, invert):
    first = len(RECORDS)
    for mag in POSE_MAGS:
        aa, tr, dM = pose_inputs(B, mag)
        tag = "pose B=%d %s angle=%g" % (B, "inverted" if invert else "forward", mag)
        (M32, a32, t32), (M64, a64, t64) = (pose_reference(dt, aa, tr, dM, invert) for dt in (torch.float32, torch.float64))
        ad, td = aa.to(device), tr.to(device)
        M = H.pose_matrix(ad, td, invert)
        daa, dtr = H.pose_matrix_backward(ad, td, dM.to(device), invert)
        # frame 1: no influence on M, exactly no gradient
        other_a, other_t = ad.clone(), td.clone()
        other_a[:, 1], other_t[:, 1] = -0.25, 11.0
        assert torch.equal(H.pose_matrix(other_a, other_t, invert), M), (tag, "frame 1 changes M")
        assert float(daa[:, 1].abs().max()) == 0.0 and float(dtr[:, 1].abs().max()) == 0.0, (tag, "frame 1 carries gradient")
        check(tag, "M", M, M32, M64)
        check(tag, "d axisangle", daa[:, 0], a32, a64)
        check(tag, "d translation", dtr[:, 0], t32, t64)
        if mag == 0.0:
            # both oracles give a zero angle-gradient at exactly zero angle (torch.norm's sub-gradient); M is [I | t] there
            assert float(a64.abs().max()) == 0.0 and float(a32.abs().max()) == 0.0
            assert float(daa.abs().max()) == 0.0, (tag, "angle gradient at zero angle", daa[:, 0])
            want = torch.eye(4).repeat(B, 1, 1)
            want[:, :3, 3] = -tr[:, 0, 0] if invert else tr[:, 0, 0]
            assert torch.equal(M.cpu(), want), (tag, "M is not [I | t] bit for bit")
    finish(first)


def run_pose_function(device):
    """once through the autograd function the models use"""
    first = len(RECORDS)
    aa, tr, dM = pose_inputs(70, 1e-3, seed=1)
    (M32, a32, t32), (M64, a64, t64) = (pose_reference(dt, aa, tr, dM, True) for dt in (torch.float32, torch.float64))
    a, t = aa.to(device).requires_grad_(True), tr.to(device).requires_grad_(True)
    M = Fn.PoseMatrixFn.apply(a, t, True)
    (M * dM.to(device)).sum().backward()
    check("PoseMatrixFn B=70 inverted angle=0.001", "M", M, M32, M64)
    check("PoseMatrixFn B=70 inverted angle=0.001", "d axisangle", a.grad[:, 0], a32, a64)
    check("PoseMatrixFn B=70 inverted angle=0.001", "d translation", t.grad[:, 0], t32, t64)
    assert float(a.grad[:, 1].abs().max()) == 0.0 and float(t.grad[:, 1].abs().max()) == 0.0
    finish(first)


# ----------------------------------------------------------------------------------------------------------------------- SSIM
def ssim_unclamped(x, y):
    """oracle.photometric.ssim_dissimilarity before its clamp (the condition below needs the distance to the limits)"""
    xp, yp = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    box = lambda t: F.avg_pool2d(t, 3, 1)
    mx, my = box(xp), box(yp)
    sx, sy, sxy = box(xp * xp) - mx * mx, box(yp * yp) - my * my, box(xp * yp) - mx * my
    return (1 - (2 * mx * my + P.SSIM_C1) * (2 * sxy + P.SSIM_C2) / ((mx * mx + my * my + P.SSIM_C1) * (sx + sy + P.SSIM_C2))) / 2


def ssim_inputs(name, seed):
    gen = _gen(seed)
    if name == "near-equal":
        x = torch.rand(2, 3, 9, 13, generator=gen)
        return dict(x=x, y=x + 1e-4 * torch.randn(2, 3, 9, 13, generator=gen), w=torch.randn(2, 3, 9, 13, generator=gen), seed=seed)
    s = SSIM_SHAPES[name]
    return dict(x=torch.rand(*s, generator=gen), y=torch.rand(*s, generator=gen), w=torch.randn(*s, generator=gen), seed=seed)


def ssim_condition(c):
    v = ssim_unclamped(c["x"].double(), c["y"].double())
    return float(torch.minimum(v.abs(), (v - 1).abs()).min()) >= SSIM_GAP


def ssim_reference(dtype, c):
    x, y = c["x"].detach().to(dtype).requires_grad_(True), c["y"].detach().to(dtype).requires_grad_(True)
    out = P.ssim_dissimilarity(x, y)
    (out * c["w"].to(dtype)).sum().backward()
    return out.detach(), x.grad, y.grad


def run_ssim(device, name):
    first = len(RECORDS)
    c = ssim_inputs(name, SEEDS["ssim " + name])
    tag = "ssim " + name
    if name != "near-equal":
        assert ssim_condition(c), (tag, "a window value within %g of the clamp limits at the recorded seed" % SSIM_GAP)
    (o32, x32, y32), (o64, x64, y64) = ssim_reference(torch.float32, c), ssim_reference(torch.float64, c)
    x, y = c["x"].to(device).requires_grad_(True), c["y"].to(device).requires_grad_(True)
    out = ML.SSIM()(x, y)
    (out * c["w"].to(device)).sum().backward()
    check(tag, "map", out, o32, o64)
    check(tag, "d x", x.grad, x32, x64)
    check(tag, "d y", y.grad, y32, y64)
    # one adjoint at a time
    gx, none = H.ssim_map_backward(x.detach(), y.detach(), c["w"].to(device), need_y=False)
    assert none is None and torch.equal(gx, x.grad), (tag, "need_y=False")
    none, gy = H.ssim_map_backward(x.detach(), y.detach(), c["w"].to(device), need_x=False)
    assert none is None and torch.equal(gy, y.grad), (tag, "need_x=False")
    if name == "near-equal":
        # the clamp-at-0 branch: a pixel all of whose windows the float64 value puts on the clamp carries exactly no gradient
        v = ssim_unclamped(c["x"].double(), c["y"].double())
        live = F.max_pool2d(F.pad(((v >= 0) & (v <= 1)).double(), (1, 1, 1, 1), mode="reflect"), 3, 1) > 0
        live = F.max_pool2d(live.double(), 3, 1, 1) > 0         # a mirrored pixel reaches one window further
        dead = ~live
        note(tag, "seed %d | windows on the clamp in float64: %d of %d | min unclamped value %.3e | pixels with no live window %d" % (
            c["seed"], int(((v < 0) | (v > 1)).sum()), v.numel(), float(v.min()), int(dead.sum())))
        assert bool((x64[dead] == 0).all()) and bool((y64[dead] == 0).all())
        assert float(x.grad.cpu()[dead].abs().sum()) == 0.0 and float(y.grad.cpu()[dead].abs().sum()) == 0.0, (tag, "clamped pixel carries gradient")
        # and the windows float64 clamps are exactly 0 in the map
        assert float(out.detach().cpu()[v < 0].abs().sum()) == 0.0
    finish(first)


# ----------------------------------------------------------------------------------------------------- backproject / project
def proj_inputs(name, seed):
    B, h, w = PROJ_SHAPES[name]
    gen = _gen(seed)
    K64 = torch.tensor([[0.58 * w, 0, 0.5 * w, 0], [0, 1.92 * h, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]], dtype=torch.float64)
    K, iK = K64.float().repeat(B, 1, 1), torch.linalg.pinv(K64).float().repeat(B, 1, 1)
    unit = lambda v: v / v.norm(dim=2, keepdim=True)
    aa = 0.05 * unit(torch.randn(B, 1, 3, generator=gen, dtype=torch.float64))
    t = 0.3 * unit(torch.randn(B, 1, 3, generator=gen, dtype=torch.float64))
    return dict(B=B, h=h, w=w, K=K, iK=iK, T=G.pose_matrix(aa, t).float(), depth=0.5 + 20 * torch.rand(B, 1, h, w, generator=gen),
                gw=torch.randn(B, h, w, 2, generator=gen), seed=seed)


def proj_reference(dtype, c):
    depth, T = c["depth"].detach().to(dtype).requires_grad_(True), c["T"].detach().to(dtype).requires_grad_(True)
    K, iK = c["K"].to(dtype), c["iK"].to(dtype)
    pts = G.backproject(depth, iK)
    pts.retain_grad()
    grid = G.project(pts, K, T, c["h"], c["w"])
    (grid * c["gw"].to(dtype)).sum().backward()
    z = ((K @ T)[:, :3, :] @ pts)[:, 2].detach()
    return dict(pts=pts.detach(), grid=grid.detach(), gdepth=depth.grad, gT=T.grad[:, :3], gpts=pts.grad, z=z)


def proj_condition(c):
    return float(proj_reference(torch.float64, c)["z"].min()) >= MIN_Z


def run_projection(device, name):
    first = len(RECORDS)
    c = proj_inputs(name, SEEDS["proj " + name])
    tag = "proj " + name
    r32, r64 = proj_reference(torch.float32, c), proj_reference(torch.float64, c)
    note(tag, "seed %d | smallest third camera coordinate %.3f" % (c["seed"], float(r64["z"].min())))
    assert float(r64["z"].min()) >= MIN_Z, (tag, "a point closer than %g to the camera plane at the recorded seed" % MIN_Z)
    B, h, w = c["B"], c["h"], c["w"]
    back, proj = ML.BackprojectDepth(B, h, w).to(device), ML.Project3D(B, h, w).to(device)
    depth, T = c["depth"].to(device).requires_grad_(True), c["T"].to(device).requires_grad_(True)
    K, iK, gw = c["K"].to(device), c["iK"].to(device), c["gw"].to(device)
    pts = back(depth, iK)
    grid = proj(pts, K, T)
    (grid * gw).sum().backward()
    check(tag, "points", pts, r32["pts"], r64["pts"])
    check(tag, "grid", grid, r32["grid"], r64["grid"])
    check(tag, "d depth", depth.grad, r32["gdepth"], r64["gdepth"])
    check(tag, "d T[:, :3]", T.grad[:, :3], r32["gT"], r64["gT"])
    # each adjoint of Project3D by itself (the other output is not computed)
    p = pts.detach()
    gp, none = H.project3d_backward(p, K, T.detach(), gw, h, w, need_T=False)
    assert none is None
    check(tag, "d points (need_T=False)", gp, r32["gpts"], r64["gpts"])
    none, gT = H.project3d_backward(p, K, T.detach(), gw, h, w, need_points=False)
    assert none is None
    check(tag, "d T[:, :3] (need_points=False)", gT[:, :3], r32["gT"], r64["gT"])
    finish(first)


def run_disp_to_depth(device):
    first = len(RECORDS)
    for hs, ws, Hh, W in D2D_SHAPES:
        disp = torch.rand(2, 1, hs, ws, generator=_gen(hs * 100 + ws))
        want = [G.disp_to_depth(F.interpolate(disp.to(dt), [Hh, W], mode="bilinear", align_corners=False), MIN_DEPTH, MAX_DEPTH)[1]
                for dt in (torch.float32, torch.float64)]
        check("disp_to_depth %dx%d -> %dx%d" % (hs, ws, Hh, W), "depth",
              H.disp_to_depth_upsampled(disp.to(device), (Hh, W), MIN_DEPTH, MAX_DEPTH), want[0], want[1])
    finish(first)


# ----------------------------------------------------------------------------------------------------------- operand lifetime
LIFETIME_SHAPES = [(9, 13), (17, 37)]       # B = 2 (a [1,1,h,w] slice counts as contiguous); every operand below 64 KB
LIFETIME_FAILED = []                        # (wrapper, shape, what) of the last run_operand_lifetime


class _Ops:
    """non-contiguous operands in the forms callers produce: channel slices of wider tensors, expanded and transposed-storage
    matrices, expanded scalars as upstream gradients, W-slices of integer maps"""

    def __init__(self, device, h, w, seed):
        self.dev, self.B, self.h, self.w, self.gen = device, 2, h, w, _gen(seed)

    def rand(self, *s):
        return torch.rand(*s, generator=self.gen).to(self.dev)

    def image(self):
        return self.rand(self.B, 5, self.h, self.w)[:, 1:4]

    def plane(self, lo=0.05, n=1):
        return (lo + self.rand(self.B, n + 2, self.h, self.w))[:, 1:1 + n]

    def shared_matrix(self, m):
        return m.to(self.dev).reshape(1, 4, 4).expand(self.B, 4, 4)

    def transposed_matrix(self, m):
        return m.to(self.dev).transpose(1, 2).contiguous().transpose(1, 2)

    def gradient(self, value, *shape):
        return torch.tensor(value).to(self.dev).expand(*shape)

    def int_map(self, hi, dtype=torch.int64, extra=()):
        return torch.randint(0, hi, (self.B, self.h, self.w + 5) + extra, generator=self.gen).to(dtype).to(self.dev)[:, :, 2:2 + self.w]

    def vector(self, t):
        wide = torch.zeros(2 * t.numel(), dtype=t.dtype)
        wide[::2] = t.reshape(-1)
        return wide.to(self.dev)[::2]

    def columns(self, t):
        wide = torch.zeros((t.shape[0], t.shape[1] + 2), dtype=t.dtype)
        wide[:, 1:-1] = t
        return wide.to(self.dev)[:, 1:-1]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _lifetime(name, shape, call, strided, held_only=None):
    """``call(**operands) -> tuple of tensors`` (outputs and accumulated-into buffers, created inside from fixed values), once on the
    strided operands and once on clones of them held in locals: bit-identical results, inputs untouched"""
    for k, t in strided.items():
        assert not t.is_contiguous(), (name, k, "the test's operand is contiguous")
    snapshot = {k: t.clone() for k, t in strided.items()}
    held = {k: t.clone(memory_format=torch.contiguous_format) for k, t in strided.items()}
    fixed = held_only or {}
    try:
        got = call(**strided, **fixed)
        want = call(**held, **fixed)
    except Exception as e:                     # a wrapper that rejects the form it is documented to take
        LIFETIME_FAILED.append((name, shape, "raised %s: %s" % (type(e).__name__, e)))
        return None
    assert all(t.is_contiguous() for t in held.values())
    for i, (g, w) in enumerate(zip(got, want)):
        if not _same(g, w):
            diff = "" if g is None or w is None or not g.is_floating_point() else " (max diff %.3g)" % float((g.double() - w.double()).abs().max())
            LIFETIME_FAILED.append((name, shape, "output %d differs from the call on held copies%s" % (i, diff)))
    for k, t in strided.items():
        if not _same(t, snapshot[k]):
            LIFETIME_FAILED.append((name, shape, "input %s was modified" % k))
    return want


def _lifetime_wrappers(device, h, w, seed):
    o = _Ops(device, h, w, seed)
    B, shape = o.B, "%dx%d" % (h, w)
    run = lambda name, call, strided, fixed=None: _lifetime(name, shape, call, strided, fixed)
    zeros = lambda *s: torch.zeros(*s, device=device)
    K64 = torch.tensor([[0.58 * w, 0, 0.5 * w, 0], [0, 1.92 * h, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]], dtype=torch.float64)
    K, iK = o.shared_matrix(K64.float()), o.shared_matrix(torch.linalg.pinv(K64).float())        # equal size, both strided
    Ts = [G.pose_matrix(0.02 * torch.randn(B, 1, 3, generator=o.gen), 0.05 * torch.randn(B, 1, 3, generator=o.gen)) for _ in range(2)]
    T0, T1 = o.transposed_matrix(Ts[0]), o.transposed_matrix(Ts[1])
    mats = dict(inv_K=iK, K=K)

    # scale_channels: NHWC channel slice and a strided [B,C] table
    xw = o.rand(B, h, w, 10)
    run("scale_channels", lambda x, scale: (H.scale_channels(x, scale),), dict(x=xw[..., 1:9], scale=o.columns(torch.rand(B, 8, generator=o.gen))))
    # pose_matrix_backward: the operands are read in place (asserted contiguous), the upstream gradient is an expanded scalar
    aa, tr, _ = pose_inputs(B, 0.3, seed)
    run("pose_matrix_backward", lambda dM: H.pose_matrix_backward(aa.to(device), tr.to(device), dM, False), dict(dM=o.gradient(0.7, B, 4, 4)))
    # warp
    disp, src = o.plane(0.2), o.image()
    run("warp_forward", lambda disp, inv_K, K, T, src: H.warp_forward(disp, inv_K, K, T, src, MIN_DEPTH, MAX_DEPTH, True, True),
        dict(disp=disp, T=T0, src=src, **mats))

    def warp_bwd(gcolor, disp, inv_K, K, T, src):
        gup, gT = zeros(B, h, w) + 0.5, zeros(B, 4, 4) - 0.25
        H.warp_backward(gcolor, disp, inv_K, K, T, src, MIN_DEPTH, MAX_DEPTH, gup, gT)
        return gup, gT
    run("warp_backward", warp_bwd, dict(gcolor=o.gradient(0.3, B, 3, h, w), disp=disp, T=T0, src=src, **mats))
    # reprojection error
    pred0, pred1, target = o.image(), o.image(), o.image()

    def reproj_fwd(pred, target):
        out = zeros(B, 2, h, w)
        H.reprojection_error(pred, target, False, out[:, 1])
        return (out,)
    run("reprojection_error", reproj_fwd, dict(pred=pred0, target=target))
    gerr = o.rand(B, 2, h, w)
    run("reprojection_error_backward", lambda pred, target: (H.reprojection_error_backward(pred, target, gerr[:, 1], False),),
        dict(pred=pred0, target=target))
    # fused photometric
    run("photometric_identity", lambda src0, src1, target: (H.photometric_identity(src0, src1, target, False),),
        dict(src0=pred0, src1=pred1, target=target))
    ident, noise = o.plane(0.0, 2), o.plane(-0.5, 2)
    fwd = run("photometric_forward", lambda pred0, pred1, target, ident, noise: H.photometric_forward(pred0, pred1, target, ident, noise, False, False),
              dict(pred0=pred0, pred1=pred1, target=target, ident=ident, noise=noise))
    if fwd is not None:
        selw = torch.zeros(B, h, w + 3, dtype=torch.uint8, device=device)
        selw[:, :, 1:1 + w] = fwd[1]

        def photo_bwd(pred0, pred1, target, sel, disp, inv_K, K, T0, T1, src0, src1):
            gT0, gT1 = zeros(B, 4, 4) + 0.125, zeros(B, 4, 4) - 0.5
            gup = H.photometric_backward(pred0, pred1, target, sel, True, disp, inv_K, K, T0, T1, src0, src1, MIN_DEPTH, MAX_DEPTH, False,
                                         False, 1.0 / (B * h * w), None, gT0, gT1)
            return gup, gT0, gT1
        run("photometric_backward", photo_bwd, dict(pred0=pred0, pred1=pred1, target=target, sel=selw[:, :, 1:1 + w], disp=disp, T0=T0, T1=T1,
                                                    src0=src, src1=o.image(), **mats))
    run("automask_min", lambda ident, noise, reproj: H.automask_min(ident, noise, reproj, False), dict(ident=ident, noise=noise, reproj=o.plane(0.0, 2)))
    # smoothness
    img = o.image()
    sm = run("smoothness_forward", lambda disp, img: H.smoothness_forward(disp, img), dict(disp=disp, img=img))
    if sm is not None:
        def smooth_bwd(disp, img, mean):
            g = zeros(B, 1, h, w) + 0.01
            H.smoothness_backward(disp, img, mean, 0.37, g)
            return (g,)
        run("smoothness_backward", smooth_bwd, dict(disp=disp, img=img, mean=o.columns(sm[1].cpu().reshape(B, 1).repeat(1, 2))[:, 0]))
    run("smooth_loss_forward", lambda disp, img: (H.smooth_loss_forward(disp, img),), dict(disp=disp, img=img))
    run("smooth_loss_backward", lambda disp, img: (H.smooth_loss_backward(disp, img, 0.37),), dict(disp=disp, img=img))
    # SSIM map: the adjoint takes the expanded gradient .sum().backward() hands it
    run("ssim_map", lambda x, y: (H.ssim_map(x, y),), dict(x=pred0, y=target))
    run("ssim_map_backward", lambda x, y, gout: H.ssim_map_backward(x, y, gout), dict(x=pred0, y=target, gout=o.gradient(1.0, B, 3, h, w)))
    # geometry layers
    depth = o.plane(0.5)
    run("backproject_depth", lambda depth, inv_K: (H.backproject_depth(depth, inv_K),), dict(depth=depth, inv_K=iK))
    run("backproject_depth_backward", lambda g_cam, inv_K: (H.backproject_depth_backward(g_cam, inv_K, h, w),),
        dict(g_cam=o.gradient(1.0, B, 4, h * w), inv_K=iK))
    pw = torch.zeros(B, 6, h * w, device=device)
    pw[:, 1:5] = H.backproject_depth(depth.contiguous(), iK.contiguous())
    points = pw[:, 1:5]
    run("project3d", lambda points, K, T: (H.project3d(points, K, T, h, w),), dict(points=points, K=K, T=T0))
    run("project3d_backward", lambda points, K, T, g_pix: H.project3d_backward(points, K, T, g_pix, h, w),
        dict(points=points, K=K, T=T0, g_pix=o.gradient(1.0, B, h, w, 2)))
    # integer maps
    run("mix_labels", lambda mask, target: (H.mix_labels(mask, target),), dict(mask=o.int_map(2), target=o.int_map(19)))
    run("depthcomp_mask", lambda depths: (H.depthcomp_mask(depths, 0.03, 0.25),), dict(depths=o.plane(0.0)))
    # augmentation: strided parameter tables and taps (two of equal size)
    params = o.columns(torch.tensor([[0.9, 1.1, 1.2, 0.05], [1.1, 0.8, 0.7, -0.03]]))
    run("color_jitter", lambda x, params: (H.color_jitter(x, params, (2, 0, 3, 1)),), dict(x=o.image(), params=params))
    taps = [torch.tensor(t) / sum(t) for t in ([1.0, 4.0, 6.0, 4.0, 1.0], [2.0, 3.0, 7.0, 3.0, 2.0])]
    run("gaussian_blur", lambda x, wy, wx: (H.gaussian_blur(x, wy, wx),), dict(x=o.image(), wy=o.vector(taps[0]), wx=o.vector(taps[1])))
    # device batch builder: strided coefficient / lookup tables
    u8 = torch.randint(0, 256, (B, 5, 2 * h, 2 * w), generator=o.gen).to(torch.uint8).to(device)[:, 1:4]
    coefw = torch.zeros(2, 7, 14, dtype=torch.int32)
    coefw[:, :, 1:13] = torch.from_numpy(DB.lanczos_half_table(h, w))
    run("batchprep_pyramid_level", lambda src, coef: H.batchprep_pyramid_level(src, coef), dict(src=u8, coef=coefw.to(device)[:, :, 1:13]))
    crop = o.columns(torch.tensor([[1, 2], [3, 0]], dtype=torch.int32))
    flip = o.vector(torch.tensor([1, 0], dtype=torch.uint8))
    lut = o.vector((torch.arange(256) % 19).to(torch.int64))
    lbl = torch.randint(0, 256, (B, h + 3, w + 9), generator=o.gen).to(torch.uint8).to(device)[:, :, 2:6 + w]
    run("batchprep_labels", lambda lbl, crop_xy, flip, lut: H.batchprep_labels(lbl, crop_xy, flip, h, w, lut, n_classes=19, want_onehot=True),
        dict(lbl=lbl, crop_xy=crop, flip=flip, lut=lut))
    colors = torch.tensor([0x000000, 0x804080, 0xE823F4, 0x464646, 0x9C6666], dtype=torch.int32)
    rgb = colors[torch.randint(0, 5, (B, h + 3, w + 9), generator=o.gen)]
    rgb = torch.stack([rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255], -1).to(torch.uint8).to(device)[:, :, 2:6 + w]
    run("batchprep_labels_rgb", lambda lbl, crop_xy, flip, colors: H.batchprep_labels_rgb(lbl, crop_xy, flip, h, w, colors, n_classes=5, want_onehot=True),
        dict(lbl=rgb, crop_xy=crop, flip=flip, colors=o.vector(colors)))


def _lifetime_layers(device, h, w, seed):
    """the public layers on the operand forms autograd and callers produce, each against the float64 oracle"""
    o = _Ops(device, h, w, seed)
    B, tag = o.B, "layers %dx%d" % (h, w)
    # SSIM()(x, y).mean().backward(): autograd hands the adjoint an expanded gradient
    xw, yw = o.rand(B, 5, h, w).requires_grad_(True), o.rand(B, 5, h, w).requires_grad_(True)
    ML.SSIM()(xw[:, 1:4], yw[:, 1:4]).mean().backward()
    want = []
    for dt in (torch.float32, torch.float64):
        x, y = xw.detach().cpu().to(dt).requires_grad_(True), yw.detach().cpu().to(dt).requires_grad_(True)
        P.ssim_dissimilarity(x[:, 1:4], y[:, 1:4]).mean().backward()
        want.append((x.grad, y.grad))
    check(tag, "SSIM().mean() d x", xw.grad, want[0][0], want[1][0])
    check(tag, "SSIM().mean() d y", yw.grad, want[0][1], want[1][1])
    # BackprojectDepth / Project3D with expanded K / inv_K, .sum().backward()
    c = proj_inputs("3x6x10", seed)
    K64 = torch.tensor([[0.58 * w, 0, 0.5 * w, 0], [0, 1.92 * h, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]], dtype=torch.float64)
    c.update(B=B, h=h, w=w, K=K64.float().repeat(B, 1, 1), iK=torch.linalg.pinv(K64).float().repeat(B, 1, 1), T=c["T"][:B],
             depth=0.5 + 20 * torch.rand(B, 1, h, w, generator=o.gen), gw=torch.ones(B, h, w, 2))
    r32, r64 = proj_reference(torch.float32, c), proj_reference(torch.float64, c)
    assert float(r64["z"].min()) >= MIN_Z
    K, iK = o.shared_matrix(c["K"][0]), o.shared_matrix(c["iK"][0])
    Tw = o.transposed_matrix(c["T"]).requires_grad_(True)
    dw = torch.zeros(B, 3, h, w)
    dw[:, 1:2] = c["depth"]
    dw = dw.to(device).requires_grad_(True)
    assert not K.is_contiguous() and not iK.is_contiguous() and not Tw.is_contiguous() and not dw[:, 1:2].is_contiguous()
    grid = ML.Project3D(B, h, w).to(device)(ML.BackprojectDepth(B, h, w).to(device)(dw[:, 1:2], iK), K, Tw)
    grid.sum().backward()
    check(tag, "Project3D(Backproject).sum() grid", grid, r32["grid"], r64["grid"])
    check(tag, "Project3D(Backproject).sum() d depth", dw.grad[:, 1:2], r32["gdepth"], r64["gdepth"])
    check(tag, "Project3D(Backproject).sum() d T[:, :3]", Tw.grad[:, :3], r32["gT"], r64["gT"])
    # get_smooth_loss on slices
    dispw, imgw = (0.05 + o.rand(B, 3, h, w)).requires_grad_(True), o.rand(B, 5, h, w)
    loss = ML.get_smooth_loss(dispw[:, 1:2], imgw[:, 1:4])
    loss.backward()
    (l32, _, g32), (l64, _, g64) = (smooth_reference(dt, dispw.detach()[:, 1:2], imgw[:, 1:4], False) for dt in (torch.float32, torch.float64))
    check(tag, "get_smooth_loss(slices) loss", loss, l32, l64)
    check(tag, "get_smooth_loss(slices) d disp", dispw.grad[:, 1:2], g32, g64)


def run_raw_pointer_contract(device):
    """buffers a kernel writes or accumulates into through a bare address are never read with the wrong strides: ValueError"""
    B, h, w = 2, 9, 13
    o = _Ops(device, h, w, 7)
    eye = torch.eye(4).repeat(B, 1, 1).to(device)
    disp, img = o.plane(0.2).contiguous(), o.image().contiguous()
    strided_T = torch.zeros(B, 4, 6, device=device)[:, :, 1:5]
    strided_plane = torch.zeros(B, 1, h, w + 2, device=device)[..., 1:1 + w]
    out, mean = H.smoothness_forward(disp, img)
    sel = torch.zeros(B, h, w, dtype=torch.uint8, device=device)
    aa, tr, dM = pose_inputs(B, 0.3)
    calls = {
        "smoothness_backward gdisp": lambda: H.smoothness_backward(disp, img, mean, 1.0, strided_plane),
        "warp_backward g_disp_up": lambda: H.warp_backward(img, disp, eye, eye, eye, img, MIN_DEPTH, MAX_DEPTH, strided_plane[:, 0], eye.clone()),
        "warp_backward gT": lambda: H.warp_backward(img, disp, eye, eye, eye, img, MIN_DEPTH, MAX_DEPTH, torch.zeros(B, h, w, device=device), strided_T),
        "photometric_backward gT0": lambda: H.photometric_backward(img, img, img, sel, False, disp, eye, eye, eye, eye, img, img, MIN_DEPTH, MAX_DEPTH,
                                                                   False, False, 1.0, None, strided_T, eye.clone()),
        "pose_matrix_backward axisangle": lambda: H.pose_matrix_backward(aa.to(device)[:, :1], tr.to(device)[:, :1], dM.to(device), False),
        "reprojection_error_backward gerr_plane": lambda: H.reprojection_error_backward(img, img, strided_plane[:, 0], False),
    }
    for name, call in calls.items():
        try:
            call()
        except ValueError:
            continue
        raise AssertionError("%s: a strided buffer was accepted" % name)
    assert float(strided_plane.abs().max()) == 0.0 and float(strided_T.abs().max()) == 0.0


def run_operand_lifetime(device):
    """every wrapper that copies a strided operand, with all of its pitchable operands strided at once (equal-size ones together: a
    released copy's block is the next copy's), against the same call on held clones; then the layer-level forms against float64"""
    first = len(RECORDS)
    del LIFETIME_FAILED[:]
    for i, (h, w) in enumerate(LIFETIME_SHAPES):
        _lifetime_wrappers(device, h, w, 100 + i)
    failed = sorted(set((n, s) for n, s, _ in LIFETIME_FAILED))
    note("operand lifetime", "%d wrapper calls differ from the call on held copies%s" % (
        len(failed), "".join("; %s %s" % f for f in failed)))
    for f in LIFETIME_FAILED:
        print("GEOM-EDGE-LIFETIME | %s | %s | %s" % f)
    for i, (h, w) in enumerate(LIFETIME_SHAPES):
        _lifetime_layers(device, h, w, 200 + i)
    assert not LIFETIME_FAILED, LIFETIME_FAILED
    finish(first)


# ------------------------------------------------------------------------------------------------------------- seed search
def seed_fits(key, seed):
    kind, name = key.split(" ", 1)
    if kind == "smooth":
        return smooth_condition(smooth_inputs(name, seed))[0]
    if kind == "ssim":
        return name == "near-equal" or ssim_condition(ssim_inputs(name, seed))
    return proj_condition(proj_inputs(name, seed))


def find_seeds(tries=1000):
    out = {}
    for key in SEEDS:
        out[key] = next(s for s in range(tries) if seed_fits(key, s))
    return out


def render_table(log_lines):
    """markdown for profiles/geometry_edges.md from the ``GEOM-EDGE`` lines a ``pytest -s`` run printed"""
    rows = [[f.strip() for f in l[l.index("GEOM-EDGE"):].split("|")] for l in log_lines if "GEOM-EDGE" in l]     # after pytest's dots
    out = ["| case | tensor | e_kernel | e_oracle | scale | ok |", "|---|---|---|---|---|---|"]
    out += ["| %s |" % " | ".join(r[1:7]) for r in rows if r[0] == "GEOM-EDGE" and len(r) == 7]
    out += ["", "Conditions and seeds:", ""] + ["* %s: %s" % (r[1], " | ".join(r[2:])) for r in rows if r[0] == "GEOM-EDGE-SET"]
    return "\n".join(out)


if __name__ == "__main__":      # no argument: the seed search; python tests/geometry_cases.py run.log: the tables of the figures page
    import sys
    print(render_table(open(sys.argv[1]).read().splitlines()) if len(sys.argv) > 1 else find_seeds())
