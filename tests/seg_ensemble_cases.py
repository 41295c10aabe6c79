"""Segmentation evaluation with test-time ensembling (hipops.seg_eval_ensemble, csrc/segens.hip, runningScore.update_from_views,
evaluation/tta.py, trainer.validate(tta=...), inference.predict_batch(tta=...)): the cases shared by the interpreter run
(test_seg_ensemble_emu.py) and the GPU run (test_seg_ensemble_gpu.py).

The oracle is plain torch on the CPU in float64, never the code under test: per view x.double(), .flip(-1) if flagged,
F.interpolate(size, mode="bilinear", align_corners=True), softmax(1); then the weighted mean, its argmax, a bincount, and -log of
the label's mean probability summed and counted.

Near ties: the fp32 probabilities differ from the float64 ones by a few 1e-6, so an argmax comparison means something only away
from ties.  Every generated case sets to 250 the label of each pixel whose float64 top-two gap of the MEAN PROBABILITY is below
1e-4 (asserting that this masks at most 1 % of the pixels); after that the confusion matrix, the count and the ids at the unmasked
pixels are EXACT, and the loss sum is held to the project's 3 x rule: its error against float64 is at most 3 x the error of the
same formulation in fp32 torch on the CPU on the same inputs, with a floor of 1e-6 relative."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from improving_segmentation_with_selfsupervised_depth_amd import _lib
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.evaluation import AverageMeter, runningScore

IGNORE = 250
GAP = 1e-4
C_LIMIT = 171                     # the largest class count the kernel accepts (SEGSDE_SEG_ENS_MAX_CLASSES)

# (seed, (B, C), view sizes, flips, label size, kind).  kind: "ind" = independent 3 * randn views, "cor" = a common 3 * randn base
# resized to every view plus 0.5 * randn
TWELVE = tuple((4 + i, 6 + 2 * i) for i in range(12))
GENERATED = [
    (1, (2, 19), ((12, 20), (24, 40), (18, 30)), (0, 1, 0), (24, 40), "ind"),      # upscale, equal size, odd ratio
    (2, (2, 66), ((16, 32), (33, 65)), (0, 1), (33, 65), "cor"),                   # Mapillary's class count, several tiles
    (3, (1, 19), ((40, 72), (5, 7)), (1, 0), (9, 13), "ind"),                      # downscale: one view per route
    (4, (2, 19), ((9, 17),), (0,), (23, 50), "ind"),                               # K = 1
    (5, (1, 5), TWELVE, tuple(i % 2 for i in range(12)), (28, 44), "cor"),         # the typical K
    (6, (1, 3), ((1, 1), (2, 3)), (0, 1), (4, 6), "ind"),                          # a source of one pixel
    (61, (1, 3), ((1, 1), (2, 3)), (0, 1), (1, 1), "ind"),                         # ... and a label grid of one pixel
    (7, (3, 19), ((6, 10), (6, 10)), (0, 1), (6, 10), "ind"),                      # equal size
    (8, (2, C_LIMIT), ((8, 16), (12, 24)), (0, 1), (16, 32), "ind"),               # the largest class count
]
# routes asserted per view where the case is about them (segsde_seg_ens_plan); test_both_routes_covered looks at all cases
ROUTES = {3: ["direct", "lds"]}
# GPU run only: several blocks per image, a partly filled last tile in both directions
RAGGED = (9, (1, 19), ((37, 70), (75, 141)), (1, 0), (75, 141), "cor")


def case_id(v):
    if isinstance(v, tuple) and v and isinstance(v[0], tuple):
        return "%dviews" % len(v)
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------------------------ oracle
def mean_probability(views, flips, weights, size, dtype):
    """the formulation of the module docstring in ``dtype`` -> [B,C,Ht,Wt]"""
    w = torch.tensor([float(x) for x in weights], dtype=torch.float64)
    w = (w / w.sum()).to(dtype)
    acc = None
    for x, f, wk in zip(views, flips, w):
        x = x.to(dtype)
        if f:
            x = x.flip(-1)
        p = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True).softmax(1)
        acc = wk * p if acc is None else acc + wk * p
    return acc


def score(prob, pred, labels):
    """hist (int64 [C,C]), loss_sum (in prob's dtype, as a float), count -- for the labels as given"""
    C = prob.shape[1]
    in_range = (labels >= 0) & (labels < C)
    hist = torch.bincount(C * labels[in_range] + pred[in_range], minlength=C * C).reshape(C, C)
    counted = in_range & (labels != IGNORE)
    at = prob.gather(1, torch.where(counted, labels, torch.zeros_like(labels))[:, None])[:, 0]
    loss_sum = float((-torch.log(at[counted])).sum())
    return dict(hist=hist, loss_sum=loss_sum, count=int(counted.sum()))


def oracle(views, flips, weights, labels):
    prob = mean_probability(views, flips, weights, labels.shape[-2:], torch.float64)
    pred = prob.argmax(1)
    C = prob.shape[1]
    top = prob.topk(2, dim=1).values if C > 1 else None
    gap = (top[:, 0] - top[:, 1]) if C > 1 else torch.full(pred.shape, float("inf"), dtype=torch.float64)
    return dict(prob=prob, pred=pred, gap=gap, **score(prob, pred, labels))


def mask_near_ties(labels, gap):
    """labels with 250 where the float64 top-two gap of the mean probability is below GAP; at most 1 % of the pixels"""
    near = gap < GAP
    share = float(near.double().mean())
    print("near-tie pixels masked: %d of %d (%.3f %%)" % (int(near.sum()), near.numel(), 100 * share))
    assert share <= 0.01, share
    return torch.where(near, torch.full_like(labels, IGNORE), labels), near


def fp32_error(views, flips, weights, labels, truth):
    """|loss sum of the same formulation in fp32 torch on the CPU - float64 loss sum|"""
    prob = mean_probability(views, flips, weights, labels.shape[-2:], torch.float32)
    return abs(score(prob, prob.argmax(1), labels)["loss_sum"] - truth)


def make_inputs(seed, bc, sizes, label_size, kind):
    B, C = bc
    g = torch.Generator().manual_seed(seed)
    if kind == "cor":
        hb, wb = max(s[0] for s in sizes), max(s[1] for s in sizes)
        base = 3.0 * torch.randn(B, C, hb, wb, generator=g)
        views = [F.interpolate(base, size=s, mode="bilinear", align_corners=True) + 0.5 * torch.randn(B, C, *s, generator=g)
                 for s in sizes]
    else:
        views = [3.0 * torch.randn(B, C, *s, generator=g) for s in sizes]
    Ht, Wt = label_size
    labels = torch.randint(0, C, (B, Ht, Wt), generator=g)
    u = torch.rand(B, Ht, Wt, generator=g)
    labels[u < 0.05] = IGNORE
    labels[(u >= 0.05) & (u < 0.07)] = 255
    labels[(u >= 0.07) & (u < 0.09)] = -1
    return views, labels


@functools.lru_cache(maxsize=None)
def generated(seed, bc, sizes, flips, label_size, kind):
    """views, labels with about 5 % 250 and a few 255 and -1 and the near ties masked, the mask, the float64 oracle of those
    labels and the error of the fp32 formulation.  Computed once per case and shared (read only)."""
    views, labels = make_inputs(seed, bc, sizes, label_size, kind)
    weights = [1.0] * len(views)
    first = oracle(views, flips, weights, labels)
    labels, near = mask_near_ties(labels, first["gap"])
    o = dict(first, **score(first["prob"], first["pred"], labels))
    return views, labels, near, o, fp32_error(views, flips, weights, labels, o["loss_sum"])


def check_loss(pair, o, e_ref, what):
    got_sum, got_count = float(pair[0]), float(pair[1])
    assert got_count == o["count"], (what, got_count, o["count"])
    e = abs(got_sum - o["loss_sum"])
    bound = max(3.0 * e_ref, 1e-6 * abs(o["loss_sum"]))
    print("%-40s loss sum %.9g  truth %.9g  e_pkg %.3e  e_fp32_torch %.3e  bound %.3e" % (what, got_sum, o["loss_sum"], e, e_ref, bound))
    assert e <= bound, "%s: loss-sum error %.3e > %.3e" % (what, e, bound)


def layout(t, kind):
    return t.contiguous() if kind == "nchw" else t.contiguous(memory_format=torch.channels_last)


def bits(pair):
    return pair.cpu().view(torch.int64)


def same(a, b):
    """(hist, pair, ids) triples equal bit for bit"""
    return torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1])) and torch.equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------------------------ 1. generated
def run_generated(device, seed, bc, sizes, flips, label_size, kind):
    B, C = bc
    views, labels, near, o, e_ref = generated(seed, bc, sizes, flips, label_size, kind)
    th, routes = H.seg_eval_ensemble_plan(views, label_size, flips=flips)
    print("plan: %d rows per tile, routes %s" % (th, routes))
    assert th in (1, 2, 4, 8, 16) and all(r in ("lds", "direct") for r in routes)
    if seed in ROUTES:
        assert routes == ROUTES[seed], routes
    lab = labels.to(device)
    for lay in ("nchw", "cl"):
        vs = [layout(v.to(device), lay) for v in views]
        hist, pair, ids = H.seg_eval_ensemble(vs, lab, flips=flips, n_classes=C, want_loss=True, want_ids=True)
        assert hist.dtype == torch.int64 and pair.dtype == torch.float64 and ids.dtype == torch.uint8
        assert tuple(ids.shape) == (B,) + tuple(label_size)
        assert torch.equal(hist.cpu().reshape(C, C), o["hist"]), (lay, "histogram")
        assert torch.equal(ids.cpu().long()[~near], o["pred"][~near]), (lay, "ids")
        check_loss(pair.cpu(), o, e_ref, "case %d %s" % (seed, lay))


def run_both_routes_covered():
    """over the generated cases and the GPU-only one the plan takes both routes (no kernel is launched)"""
    seen = set()
    for seed, bc, sizes, flips, label_size, kind in GENERATED + [RAGGED]:
        views = [torch.zeros(bc + s) for s in sizes]
        seen.update(H.seg_eval_ensemble_plan(views, label_size, flips=flips)[1])
    assert seen == {"lds", "direct"}, seen


def run_class_limit(device):
    import pytest
    assert H.SEG_ENS_MAX_CLASSES == C_LIMIT and H.SEG_ENS_MAX_VIEWS == 16
    v = torch.zeros(1, C_LIMIT + 1, 2, 2, device=device)
    with pytest.raises(NotImplementedError, match=str(C_LIMIT)):
        H.seg_eval_ensemble([v], torch.zeros(1, 2, 2, dtype=torch.int64, device=device))
    # the library says the same of a descriptor that gets past the binding
    d = (_lib.SegEnsView * 1)(_lib.SegEnsView(None, 0, 0, 0, 0, 2, 2, 0, 1.0))
    L = _lib.lib()
    assert L.segsde_seg_ens_plan(d, 1, C_LIMIT + 1, 2, 2, None) == -4 and L.segsde_seg_ens_plan(d, 1, C_LIMIT, 2, 2, None) >= 1


# ------------------------------------------------------------------------------------------------------------------ 2. exact properties
def _case(device, index=0):
    seed, bc, sizes, flips, label_size, kind = GENERATED[index]
    views, labels, near, o, _ = generated(seed, bc, sizes, flips, label_size, kind)
    return [v.to(device) for v in views], list(flips), labels.to(device), near, o, bc[1]


def run_determinism(device):
    """bitwise-equal triples from two calls; 2 x 19 x {32 x 64, 48 x 96 flipped} -> 64 x 128 is several blocks per image"""
    g = torch.Generator().manual_seed(13)
    views = [(3.0 * torch.randn(2, 19, h, w, generator=g)).to(device) for h, w in ((32, 64), (48, 96))]
    labels = torch.randint(0, 19, (2, 64, 128), generator=g).to(device)
    for lay in ("nchw", "cl"):
        vs = [layout(v, lay) for v in views]
        a = H.seg_eval_ensemble(vs, labels, flips=[0, 1], n_classes=19, want_ids=True)
        b = H.seg_eval_ensemble(vs, labels, flips=[0, 1], n_classes=19, want_ids=True)
        assert same(a, b), lay
        assert int(a[0].sum()) == labels.numel() and float(a[1][1]) == labels.numel()


def run_zero_weight(device):
    """a view of weight 0 is not read: the bits of the call without it, wherever it stands in the list"""
    views, flips, lab, _, _, C = _case(device)
    ref = H.seg_eval_ensemble(views[:2], lab, flips=flips[:2], weights=[1.0, 3.0], n_classes=C, want_ids=True)
    poison = torch.full_like(views[2], float("nan"))
    for pos in (0, 1, 2):
        vs, fs, ws = list(views[:2]), list(flips[:2]), [1.0, 3.0]
        vs.insert(pos, poison)
        fs.insert(pos, 1)
        ws.insert(pos, 0.0)
        assert same(H.seg_eval_ensemble(vs, lab, flips=fs, weights=ws, n_classes=C, want_ids=True), ref), pos
    th, routes = H.seg_eval_ensemble_plan(views, tuple(lab.shape[-2:]), flips=flips, weights=[1.0, 0.0, 2.0])
    assert routes[1] is None and None not in (routes[0], routes[2])


def run_weight_scaling(device):
    """the weights enter as float32(w_k / sum w), the quotient formed in float64: [2,2,2] gives the bits of [1,1,1] (both are
    the correctly rounded third), and so does the default; unequal weights change the result"""
    views, flips, lab, _, _, C = _case(device)
    ones = H.seg_eval_ensemble(views, lab, flips=flips, weights=[1, 1, 1], n_classes=C, want_ids=True)
    assert same(H.seg_eval_ensemble(views, lab, flips=flips, weights=[2.0, 2.0, 2.0], n_classes=C, want_ids=True), ones)
    assert same(H.seg_eval_ensemble(views, lab, flips=flips, n_classes=C, want_ids=True), ones)
    other = H.seg_eval_ensemble(views, lab, flips=flips, weights=[1, 5, 1], n_classes=C, want_ids=True)
    assert not torch.equal(bits(other[1]), bits(ones[1]))
    # and the weighted result is the oracle's
    cpu = [v.cpu() for v in views]
    o = oracle(cpu, flips, [1, 5, 1], lab.cpu())
    keep = o["gap"] >= GAP
    assert torch.equal(other[2].cpu().long()[keep], o["pred"][keep])
    assert float(other[1][1]) == o["count"] and abs(float(other[1][0]) - o["loss_sum"]) <= 1e-5 * abs(o["loss_sum"])


def run_flip_pair(device):
    """equal size, views [x, x.flip(-1)] with flips [False, True]: both terms are the same number and their half-sum is exact, so
    ids, loss sum and count are those of the one-view call [x] bit for bit -- and a flipped view is read mirrored"""
    g = torch.Generator().manual_seed(29)
    x = (3.0 * torch.randn(2, 19, 24, 70, generator=g)).to(device)
    labels = torch.randint(0, 19, (2, 24, 70), generator=g).to(device)
    one = H.seg_eval_ensemble([x], labels, n_classes=19, want_ids=True)
    two = H.seg_eval_ensemble([x, x.flip(-1)], labels, flips=[False, True], n_classes=19, want_ids=True)
    assert same(one, two)
    # a mirrored view without its flag is another input
    wrong = H.seg_eval_ensemble([x, x.flip(-1)], labels, flips=[False, False], n_classes=19, want_ids=True)
    assert not torch.equal(wrong[2], one[2]) and not torch.equal(bits(wrong[1]), bits(one[1]))
    # at another label size the two views still interpolate the same numbers
    big = torch.randint(0, 19, (2, 37, 131), generator=g).to(device)
    one = H.seg_eval_ensemble([x], big, n_classes=19, want_ids=True)
    two = H.seg_eval_ensemble([x, x.flip(-1)], big, flips=[False, True], n_classes=19, want_ids=True)
    assert same(one, two)


def run_layouts(device):
    """dense NCHW, channels-last and a channel slice of a wider tensor (in both layouts) give the same bits"""
    views, flips, lab, _, _, C = _case(device)
    ref = H.seg_eval_ensemble([v.contiguous() for v in views], lab, flips=flips, n_classes=C, want_ids=True)
    assert same(H.seg_eval_ensemble([layout(v, "cl") for v in views], lab, flips=flips, n_classes=C, want_ids=True), ref)
    for lay in ("nchw", "cl"):
        wide = []
        for v in views:
            buf = layout(torch.randn(v.shape[0], C + 5, v.shape[2], v.shape[3], device=device), lay)
            buf[:, 2:2 + C] = v
            wide.append(buf[:, 2:2 + C])
            assert not wide[-1].is_contiguous()
        assert same(H.seg_eval_ensemble(wide, lab, flips=flips, n_classes=C, want_ids=True), ref), lay
    # the same under the direct route
    views, flips, lab, _, _, C = _case(device, 2)
    ref = H.seg_eval_ensemble(views, lab, flips=flips, n_classes=C, want_ids=True)
    assert same(H.seg_eval_ensemble([layout(v, "cl") for v in views], lab, flips=flips, n_classes=C, want_ids=True), ref)


def run_half(device):
    """fp16 views equal the call on their .float()"""
    views, flips, lab, _, _, C = _case(device)
    half = [v.half() for v in views]
    assert same(H.seg_eval_ensemble(half, lab, flips=flips, n_classes=C, want_ids=True),
                H.seg_eval_ensemble([h.float() for h in half], lab, flips=flips, n_classes=C, want_ids=True))


def run_accumulation(device):
    import pytest
    views, flips, lab, near, o, C = _case(device)
    hist = torch.zeros(C * C, dtype=torch.int64, device=device)
    back, pair1, none = H.seg_eval_ensemble(views, lab, flips=flips, hist=hist)
    assert back is hist and none is None
    _, pair2, _ = H.seg_eval_ensemble(views, lab, flips=flips, hist=hist)
    assert torch.equal(hist.cpu().reshape(C, C), 2 * o["hist"]), "the second call accumulates into hist"
    assert torch.equal(bits(pair1), bits(pair2)) and float(pair2[1]) == o["count"], "the loss pair is overwritten, not accumulated"
    with pytest.raises(ValueError):
        H.seg_eval_ensemble(views, lab, flips=flips, hist=torch.zeros(C * C - 1, dtype=torch.int64, device=device))
    with pytest.raises(ValueError):
        H.seg_eval_ensemble(views, lab, flips=flips, hist=torch.zeros(C * C, dtype=torch.int32, device=device))
    with pytest.raises(ValueError):
        H.seg_eval_ensemble(views, lab, flips=flips, hist=torch.zeros(C * C, dtype=torch.int64, device="meta"))
    # every label ignored: count 0, the histogram untouched, NaN from update_from_views
    before = hist.clone()
    _, pair, _ = H.seg_eval_ensemble(views, torch.full_like(lab, IGNORE), flips=flips, hist=hist)
    assert float(pair[0]) == 0.0 and float(pair[1]) == 0.0 and torch.equal(hist, before)


def run_inference_form(device):
    """gt=None with size=: the ids of the labelled call, nothing else; hist and the loss are refused"""
    import pytest
    views, flips, lab, _, _, C = _case(device)
    _, _, ids = H.seg_eval_ensemble(views, lab, flips=flips, n_classes=C, want_ids=True)
    h, p, got = H.seg_eval_ensemble(views, flips=flips, size=tuple(lab.shape[-2:]))
    assert h is None and p is None and got.dtype == torch.uint8 and torch.equal(got, ids)
    with pytest.raises(ValueError):
        H.seg_eval_ensemble(views, flips=flips)
    with pytest.raises(ValueError):
        H.seg_eval_ensemble(views, flips=flips, size=(24, 40), hist=torch.zeros(C * C, dtype=torch.int64, device=device))
    with pytest.raises(ValueError):
        H.seg_eval_ensemble(views, flips=flips, size=(24, 40), n_classes=C)


# ------------------------------------------------------------------------------------------------------------------ 3. arguments
def run_python_argument_checks(device):
    """refused in Python, before the library is looked up, naming the offender"""
    import pytest
    v = torch.zeros(2, 5, 4, 6, device=device)
    gt = torch.zeros(2, 8, 12, dtype=torch.int64, device=device)
    saved = _lib._LIB, _lib.LIB_PATH
    _lib._LIB, _lib.LIB_PATH = None, "/nonexistent/libsegsde_hip.so"      # a lookup would raise RuntimeError("... not found")
    try:
        with pytest.raises(ValueError, match="empty"):
            H.seg_eval_ensemble([], gt)
        with pytest.raises(ValueError, match="17 views"):
            H.seg_eval_ensemble([v] * 17, gt)
        with pytest.raises(ValueError, match=r"views\[1\] holds 1 images"):
            H.seg_eval_ensemble([v, v[:1]], gt)
        with pytest.raises(ValueError, match=r"views\[2\] has 4 classes"):
            H.seg_eval_ensemble([v, v, v[:, :4]], gt)
        with pytest.raises(ValueError, match=r"views\[1\] is on meta"):
            H.seg_eval_ensemble([v, torch.zeros(2, 5, 4, 6, device="meta")], gt)
        with pytest.raises(ValueError, match=r"weights\[1\] = -1"):
            H.seg_eval_ensemble([v, v], gt, weights=[1.0, -1.0])
        with pytest.raises(ValueError, match=r"weights\[0\] = nan"):
            H.seg_eval_ensemble([v, v], gt, weights=[float("nan"), 1.0])
        with pytest.raises(ValueError, match=r"weights\[1\] = inf"):
            H.seg_eval_ensemble([v, v], gt, weights=[1.0, float("inf")])
        with pytest.raises(ValueError, match="all zero"):
            H.seg_eval_ensemble([v, v], gt, weights=[0.0, 0.0])
        with pytest.raises(ValueError, match="3 flips"):
            H.seg_eval_ensemble([v, v], gt, flips=[0, 1, 0])
        with pytest.raises(ValueError, match="1 weights"):
            H.seg_eval_ensemble([v, v], gt, weights=[1.0])
        with pytest.raises(ValueError, match="gt 1"):
            H.seg_eval_ensemble([v], gt[:1])
        with pytest.raises(ValueError, match="n_classes = 6"):
            H.seg_eval_ensemble([v], gt, n_classes=6)
        with pytest.raises(ValueError, match="nothing to compute"):
            H.seg_eval_ensemble([v], gt, want_loss=False)
        with pytest.raises(TypeError):
            H.seg_eval_ensemble(v, gt)
        with pytest.raises(TypeError):
            H.seg_eval_ensemble([v, v[0]], gt)
        with pytest.raises(TypeError):
            H.seg_eval_ensemble([v.long()], gt)
        with pytest.raises(TypeError):
            H.seg_eval_ensemble([v], gt.int())
        with pytest.raises(NotImplementedError, match=str(C_LIMIT)):
            H.seg_eval_ensemble([torch.zeros(1, 300, 2, 2, device=device)], gt[:1])
    finally:
        _lib._LIB, _lib.LIB_PATH = saved


# ------------------------------------------------------------------------------------------------------------------ 4. runningScore
def run_running_score(device):
    """update_from_views sums into the matrix of the other update methods and follows update_from_logits' return convention"""
    views, flips, lab, near, o, C = _case(device)
    rs = runningScore(C)
    loss = rs.update_from_views(lab, views, flips=flips, return_loss=True)
    assert rs.update_from_views(lab, views, flips=flips) is None
    assert np.array_equal(rs.confusion_matrix, 2 * o["hist"].numpy().astype(np.float64))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == torch.device(device).type
    mean = o["loss_sum"] / o["count"]
    assert abs(float(loss) - mean) <= 1e-6 * abs(mean), (float(loss), mean)
    ids = runningScore(C).update_from_views(lab, views, flips=flips, return_ids=True)
    both = runningScore(C).update_from_views(lab, views, flips=flips, return_loss=True, return_ids=True)
    assert ids.dtype == torch.uint8 and torch.equal(ids, both[1]) and torch.equal(both[0], loss)
    assert torch.equal(ids.cpu().long()[~near], o["pred"][~near])
    # weights reach the kernel; one view of an equal-size pair scores like update_from_logits
    single = runningScore(C)
    single.update_from_views(lab, views, flips=flips, weights=[0, 1, 0])
    direct = runningScore(C)
    direct.update_from_logits(lab, views[1].flip(-1).contiguous())
    assert np.array_equal(single.confusion_matrix, direct.confusion_matrix)
    nan = runningScore(C).update_from_views(torch.full_like(lab, IGNORE), views, flips=flips, return_loss=True)
    assert bool(torch.isnan(nan))


# ------------------------------------------------------------------------------------------------------------------ 5. tta, validate, predict_batch
TTA = {"scales": [0.5, 1.0, 1.5], "flip": True}


def run_view_sizes():
    from improving_segmentation_with_selfsupervised_depth_amd.evaluation import tta as TT
    assert TT.view_sizes((64, 128), [0.5, 1.0, 1.5]) == [(32, 64), (64, 128), (96, 192)]
    assert TT.view_sizes((512, 1024), [0.75, 1.25, 1.75]) == [(384, 768), (640, 1280), (896, 1792)]
    assert TT.view_sizes((100, 210), [1.0]) == [(96, 224)]                       # 3.125 -> 3, 6.5625 -> 7
    assert TT.view_sizes((48, 80), [1.0]) == [(64, 96)]                          # halves round up: 1.5 -> 2, 2.5 -> 3
    assert TT.view_sizes((64, 128), [0.1]) == [(32, 32)]                         # one multiple at least
    assert TT.view_sizes((60, 90), [0.5, 2.0], multiple_of=1) == [(30, 45), (120, 180)]
    import pytest
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            TT.view_sizes((64, 128), [bad])


def run_make_views(device):
    """sizes, order and flags; scale 1.0 without flip is the input itself; a resized view is resize_bilinear(align_corners=False)
    (the ATen formula in float64 within fp32 rounding), its mirror an exact mirror"""
    from improving_segmentation_with_selfsupervised_depth_amd.evaluation import tta as TT
    g = torch.Generator().manual_seed(31)
    img = torch.rand(2, 3, 64, 128, generator=g).to(device)
    plain = TT.make_views(img, [1.0], False)
    assert len(plain) == 1 and plain[0][0] is img and plain[0][1] is False
    views = TT.make_views(img, TTA["scales"], True)
    assert [tuple(v.shape[-2:]) for v, _ in views] == [(32, 64)] * 2 + [(64, 128)] * 2 + [(96, 192)] * 2
    assert [f for _, f in views] == [False, True] * 3 and views[2][0] is img
    for k in (0, 2, 4):
        assert torch.equal(views[k + 1][0], views[k][0].flip(-1))
        want = F.interpolate(img.cpu().double(), size=tuple(views[k][0].shape[-2:]), mode="bilinear", align_corners=False)
        # the fp32 source coordinate (< 128: ulp 2^-17) carries up to three roundings into the weights; the values are in [0,1]
        assert float((views[k][0].cpu().double() - want).abs().max()) <= 3 * 2.0 ** -17 + 1e-6


class TinyHead(torch.nn.Module):
    """stand-in for the interpreter run, where ResNet-18 passes take minutes: the part of the model's interface the ensemble uses
    (a dict in, a dict with "semantics" out at the input's size, parameters, the training flag, ``use_pose_net``); a fixed 1x1
    convolution in plain torch"""

    def __init__(self):
        super().__init__()
        self.head = torch.nn.Conv2d(3, 19, 1)
        self.use_pose_net = True
        self.pose_flags = []
        with torch.no_grad():
            g = torch.Generator().manual_seed(37)
            self.head.weight.copy_(6.0 * torch.randn(19, 3, 1, 1, generator=g))
            self.head.bias.copy_(torch.randn(19, generator=g))

    def forward(self, inputs):
        self.pose_flags.append(self.use_pose_net)
        return {"semantics": self.head(inputs[("color_aug", 0, 0)])}


def _model(device, kind):
    """(model, monodepth loss or None, batches on the device, cfg): the setup of the seg_eval validate cases -- ResNet-18 joint
    model of model_cases at 64 x 128 with labels at 128 x 256, or the stand-in head"""
    import seg_eval_cases as SE
    if kind == "tiny":
        _, _, batches, cfg = SE._validate_setup()
        cfg = dict(cfg, model=dict(cfg["model"], disable_monodepth=True, disable_pose=True))
        return TinyHead().to(device), None, [{k: v.to(device) for k, v in b.items()} for b in batches], cfg
    return SE._validate_model(device, "r18")


def run_validate(device, kind="r18"):
    """validate(tta=...) against ensemble_forward + hipops.seg_eval_ensemble called by hand: exact, this checks plumbing"""
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    from improving_segmentation_with_selfsupervised_depth_amd.evaluation import tta as TT
    model, mono, batches, cfg = _model(device, kind)
    had_pose = model.use_pose_net
    model.eval()
    total = torch.zeros(19 * 19, dtype=torch.int64, device=device)
    meter, plain_meter, plain = AverageMeter(), AverageMeter(), runningScore(19)
    all_ids = []
    with torch.no_grad():
        for b in batches:
            sems, flags = TT.ensemble_forward(model, dict(b), TTA["scales"], TTA["flip"])
            assert [tuple(s.shape[-2:]) for s in sems] == [(32, 64)] * 2 + [(64, 128)] * 2 + [(96, 192)] * 2
            assert flags == [False, True] * 3
            _, pair, ids = H.seg_eval_ensemble(sems, b["lbl"], flips=flags, hist=total, want_ids=True)
            meter.update((pair[0] / pair[1]).float())
            all_ids.append(ids)
            plain_meter.update(plain.update_from_logits(b["lbl"], model(dict(b))["semantics"], return_loss=True))
    assert model.use_pose_net == had_pose, "ensemble_forward restores use_pose_net"
    if kind == "tiny":
        assert model.pose_flags[:6] == [False] * 6 and model.pose_flags[6] is True
    model.train()
    out = T.validate(model, [dict(b) for b in batches], cfg, 19, monodepth_loss_calculator_val=mono, tta=TTA)
    assert model.training and model.use_pose_net == had_pose, "the training flag and use_pose_net are restored"
    ref = runningScore(19)
    ref._host = total.cpu().numpy().reshape(19, 19).astype(np.float64)
    s_want, iu_want = ref.get_scores()
    assert out["score"] == s_want, (out["score"], s_want)
    for k in iu_want:
        assert out["class_iou"][k] == iu_want[k] or (np.isnan(out["class_iou"][k]) and np.isnan(iu_want[k])), k
    assert out["losses"]["segmentation_loss"] == float(meter.avg), (out["losses"]["segmentation_loss"], float(meter.avg))
    saved = out["imgs_to_save"]
    assert len(saved) == 2
    for j, (img, label, ids, disp) in enumerate(saved):
        assert torch.equal(ids, all_ids[j][0]) and tuple(ids.shape) == tuple(label.shape) == (128, 256)
    assert np.isfinite(out["losses"]["monodepth_loss"]) and (out["losses"]["monodepth_loss"] != 0.0) == (kind == "r18")
    # the same through cfg["training"]["tta"]
    cfg_tta = dict(cfg, training=dict(cfg["training"], tta=TTA, n_tensorboard_imgs=0))
    out_cfg = T.validate(model, [dict(b) for b in batches], cfg_tta, 19, monodepth_loss_calculator_val=mono)
    assert out_cfg["score"] == s_want and out_cfg["losses"]["segmentation_loss"] == out["losses"]["segmentation_loss"]
    # without tta: what update_from_logits gives, as before
    out_plain = T.validate(model, [dict(b) for b in batches], cfg, 19, monodepth_loss_calculator_val=mono)
    assert out_plain["score"] == plain.get_scores()[0]
    assert out_plain["losses"]["segmentation_loss"] == float(plain_meter.avg)
    assert out_plain["score"] != s_want, "the ensemble changes the prediction somewhere"
    import pytest
    with pytest.raises(ValueError, match="loss_fn"):
        T.validate(model, [dict(b) for b in batches], cfg, 19, monodepth_loss_calculator_val=mono, tta=TTA,
                   loss_fn=lambda input, target: input.sum())


def run_predict_batch(device, kind="r18"):
    from improving_segmentation_with_selfsupervised_depth_amd import inference as I
    from improving_segmentation_with_selfsupervised_depth_amd.evaluation import tta as TT
    model, mono, batches, cfg = _model(device, kind)
    model.eval()
    b = batches[0]
    palette = torch.randint(0, 256, (19, 3), generator=torch.Generator().manual_seed(43)).to(torch.uint8)
    with torch.no_grad():
        sems, flags = TT.ensemble_forward(model, dict(b), TTA["scales"], TTA["flip"])
    ids = H.seg_eval_ensemble(sems, flips=flags, size=(64, 128))[2]
    res = I.predict_batch(model, mono, dict(b), palette, segmentation=True, monodepth=False, tta=TTA)
    assert res["pred_ids"].dtype == torch.uint8 and tuple(res["pred_ids"].shape) == (1, 64, 128)
    assert torch.equal(res["pred_ids"], ids)
    assert torch.equal(res["label"], H.render_labels(palette, ids=ids))
    assert torch.equal(res["label"].cpu().long(), palette.long()[ids.cpu().long()])
    plain = I.predict_batch(model, mono, dict(b), palette, segmentation=True, monodepth=False)
    assert torch.equal(plain["pred_ids"].long(), plain["outputs"]["semantics"].argmax(1))
    assert not torch.equal(plain["pred_ids"], ids), "the ensemble changes the prediction somewhere"
