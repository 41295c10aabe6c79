"""Segmentation validation at label resolution (hipops.seg_eval, csrc/segeval.hip, runningScore.update_from_logits, AverageMeter /
AverageMeterDict, trainer.validate): the cases shared by the interpreter run (test_seg_eval_emu.py) and the GPU run
(test_seg_eval_gpu.py).

The oracle is plain torch on the CPU in float64: F.interpolate(x.double(), size, mode="bilinear", align_corners=True), argmax(1),
F.cross_entropy(..., ignore_index=250, reduction="sum") and the count of the pixels it sums.  Nothing is compared against the code
under test.

Near ties: the fp32 interpolant differs from the float64 one by about 1e-5 at |logit| ~ 10, so an argmax comparison means
something only away from ties.  Every generated case sets to 250 the label of each pixel whose float64 top-two gap is below 1e-3
(asserting that this masks at most 1 % of the pixels); after that the confusion matrix, the ids at the unmasked pixels and the
count are EXACT, and the loss sum is held to the project's 3 x rule: its error against float64 is at most 3 x the error of the
unfused package path (Fn.resize_bilinear + cross_entropy_forward) on the same input, with a floor of 1e-6 relative (the unfused
path can land on the float64 value)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from improving_segmentation_with_selfsupervised_depth_amd import _lib
from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H
from improving_segmentation_with_selfsupervised_depth_amd.evaluation import AverageMeter, AverageMeterDict, runningScore

IGNORE = 250
GAP = 1e-3

# (seed, (B, C, Hi, Wi, Ht, Wt), route): "lds" = the tile's source footprint is staged in LDS, "direct" = taps read from memory
# (segsde_seg_eval_plan; asserted, so that both routes stay covered)
GENERATED = [
    (1, (2, 19, 12, 20, 24, 40), "lds"),         # 2 x
    (2, (2, 19, 9, 17, 23, 50), "lds"),          # odd ratios
    (3, (1, 5, 7, 11, 28, 44), "lds"),           # 4 x
    (4, (2, 66, 16, 32, 33, 65), "lds"),         # Mapillary's class count; two tiles along x, three along y
    (5, (2, 11, 8, 8, 8, 24), "lds"),            # one axis equal
    (6, (1, 19, 40, 72, 9, 13), "direct"),       # downscale: the footprint of a tile does not fit
    (7, (3, 19, 6, 10, 6, 10), "lds"),           # equal size: must also equal confusion_update bit for bit
    (8, (1, 19, 5, 9, 1, 1), "lds"),             # out == 1
    (9, (1, 3, 1, 1, 4, 6), "lds"),              # in == 1
]


def case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------------------------ oracle
def oracle(logits, labels):
    """float32 logits [B,C,Hi,Wi], int64 labels [B,Ht,Wt] (CPU) -> dict: up (float64 interpolant), pred, gap (top-two), hist
    (int64 [C,C]), loss_sum, count -- for the labels as given"""
    C = logits.shape[1]
    up = F.interpolate(logits.double(), size=tuple(labels.shape[-2:]), mode="bilinear", align_corners=True)
    pred = up.argmax(1)
    top = up.topk(2, dim=1).values if C > 1 else None
    gap = (top[:, 0] - top[:, 1]) if C > 1 else torch.full(pred.shape, float("inf"), dtype=torch.float64)
    return dict(up=up, pred=pred, gap=gap, **score(up, pred, labels))


def score(up, pred, labels):
    C = up.shape[1]
    in_range = (labels >= 0) & (labels < C)
    hist = torch.bincount(C * labels[in_range] + pred[in_range], minlength=C * C).reshape(C, C)
    counted = in_range & (labels != IGNORE)
    lab = torch.where(counted, labels, torch.full_like(labels, IGNORE))          # F.cross_entropy raises on 255 / -1
    loss_sum = float(F.cross_entropy(up, lab, ignore_index=IGNORE, reduction="sum"))
    return dict(hist=hist, loss_sum=loss_sum, count=int(counted.sum()))


def mask_near_ties(labels, gap):
    """labels with 250 where the float64 top-two gap is below GAP; at most 1 % of the pixels"""
    near = gap < GAP
    share = float(near.double().mean())
    print("near-tie pixels masked: %d of %d (%.3f %%)" % (int(near.sum()), near.numel(), 100 * share))
    assert share <= 0.01, share
    return torch.where(near, torch.full_like(labels, IGNORE), labels), near


@functools.lru_cache(maxsize=None)
def generated(seed, shape):
    """3 * randn logits; labels uniform in [0,C) with about 5 % 250 and a few 255 and -1, near ties masked; the oracle of those
    labels.  Computed once per case and shared (read only)."""
    B, C, Hi, Wi, Ht, Wt = shape
    g = torch.Generator().manual_seed(seed)
    logits = 3.0 * torch.randn(B, C, Hi, Wi, generator=g)
    labels = torch.randint(0, C, (B, Ht, Wt), generator=g)
    u = torch.rand(B, Ht, Wt, generator=g)
    labels[u < 0.05] = IGNORE
    labels[(u >= 0.05) & (u < 0.07)] = 255
    labels[(u >= 0.07) & (u < 0.09)] = -1
    first = oracle(logits, labels)
    labels, near = mask_near_ties(labels, first["gap"])
    o = dict(first, **score(first["up"], first["pred"], labels))
    return logits, labels, near, o


def unfused_loss_sum(logits_dev, labels_dev):
    """the package's unfused path: the resized tensor, then the cross-entropy kernel (its float32 sum)"""
    C = logits_dev.shape[1]
    x = Fn.resize_bilinear(Fn.to_nhwc(logits_dev.contiguous()), tuple(labels_dev.shape[-2:]), align_corners=True).contiguous()
    lab = torch.where((labels_dev >= 0) & (labels_dev < C), labels_dev, torch.full_like(labels_dev, IGNORE))
    return float(H.cross_entropy_forward(x, lab.reshape(-1).contiguous(), IGNORE)[0])


def check_loss(pair, o, e_ref, what):
    got_sum, got_count = float(pair[0]), float(pair[1])
    assert got_count == o["count"], (what, got_count, o["count"])
    e = abs(got_sum - o["loss_sum"])
    bound = max(3.0 * e_ref, 1e-6 * abs(o["loss_sum"]))
    print("%-40s loss sum %.9g  truth %.9g  e_pkg %.3e  e_unfused %.3e  bound %.3e" % (what, got_sum, o["loss_sum"], e, e_ref, bound))
    assert e <= bound, "%s: loss-sum error %.3e > %.3e" % (what, e, bound)


def layout(t, kind):
    return t.contiguous() if kind == "nchw" else t.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------ 1. generated
def run_generated(device, seed, shape, route):
    B, C, Hi, Wi, Ht, Wt = shape
    logits, labels, near, o = generated(seed, shape)
    plan = _lib.lib().segsde_seg_eval_plan(C, Hi, Wi, Ht, Wt)
    assert (plan in (4, 8, 16)) if route == "lds" else plan == 0, (plan, route)
    lab = labels.to(device)
    e_ref = abs(unfused_loss_sum(logits.to(device), lab) - o["loss_sum"])
    for kind in ("nchw", "cl"):
        lg = layout(logits.to(device), kind)
        hist, pair, ids = H.seg_eval(lg, lab, n_classes=C, want_loss=True, want_ids=True)
        assert hist.dtype == torch.int64 and pair.dtype == torch.float64 and ids.dtype == torch.uint8
        assert tuple(ids.shape) == (B, Ht, Wt)
        assert torch.equal(hist.cpu().reshape(C, C), o["hist"]), (kind, "histogram")
        assert torch.equal(ids.cpu().long()[~near], o["pred"][~near]), (kind, "ids")
        check_loss(pair.cpu(), o, e_ref, "%s %s" % (case_id(shape), kind))
    if (Hi, Wi) == (Ht, Wt):
        same = torch.zeros(C * C, dtype=torch.int64, device=device)
        H.confusion_update(same, lab, logits=logits.to(device))
        assert torch.equal(same, hist), "equal sizes: seg_eval and confusion_update differ"


# ------------------------------------------------------------------------------------------------------------------ 2. ties, accumulation
def run_ties(device):
    """classes 1 and 3 hold the same plane, everywhere the maximum: identical inputs go through identical arithmetic, so the
    lower index wins at every ratio"""
    g = torch.Generator().manual_seed(11)
    for Hi, Wi, Ht, Wt in ((6, 10, 12, 20), (5, 7, 13, 30), (6, 10, 6, 10), (20, 30, 3, 4), (4, 4, 16, 4), (1, 1, 3, 3), (3, 5, 1, 1)):
        logits = torch.randn(2, 5, Hi, Wi, generator=g)
        logits[:, 1] = logits[:, 1].abs() + 6.0
        logits[:, 3] = logits[:, 1]
        labels = torch.randint(0, 5, (2, Ht, Wt), generator=g)
        for kind in ("nchw", "cl"):
            hist, _, ids = H.seg_eval(layout(logits.to(device), kind), labels.to(device), n_classes=5, want_loss=False, want_ids=True)
            assert bool((ids == 1).all()), (Hi, Wi, Ht, Wt, kind)
            assert int(hist.reshape(5, 5)[:, 1].sum()) == labels.numel()


def run_accumulation(device):
    seed, shape, _ = GENERATED[0]
    logits, labels, near, o = generated(seed, shape)
    C = shape[1]
    lg, lab = logits.to(device), labels.to(device)
    hist = torch.zeros(C * C, dtype=torch.int64, device=device)
    back, pair1, _ = H.seg_eval(lg, lab, hist=hist)
    assert back is hist
    _, pair2, _ = H.seg_eval(lg, lab, hist=hist)
    assert torch.equal(hist.cpu().reshape(C, C), 2 * o["hist"]), "the second call accumulates into hist"
    assert torch.equal(pair1, pair2) and float(pair2[1]) == o["count"], "the loss pair is overwritten, not accumulated"
    # only the ids
    h3, p3, ids = H.seg_eval(lg, lab, hist=None, want_loss=False, want_ids=True)
    assert h3 is None and p3 is None and torch.equal(ids.cpu().long()[~near], o["pred"][~near])
    # every label ignored: count 0, the histogram untouched, NaN from update_from_logits
    before = hist.clone()
    _, pair, _ = H.seg_eval(lg, torch.full_like(lab, IGNORE), hist=hist)
    assert float(pair[0]) == 0.0 and float(pair[1]) == 0.0 and torch.equal(hist, before)
    rs = runningScore(C)
    loss = rs.update_from_logits(torch.full_like(lab, IGNORE), lg, return_loss=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and bool(torch.isnan(loss))
    assert rs.confusion_matrix.sum() == 0


# ------------------------------------------------------------------------------------------------------------------ 3. determinism
def run_determinism(device):
    """bitwise-equal loss pairs and histograms from two calls; 2 x 19 x 32 x 64 -> 64 x 128 is 32 blocks"""
    g = torch.Generator().manual_seed(13)
    logits = (3.0 * torch.randn(2, 19, 32, 64, generator=g)).to(device)
    labels = torch.randint(0, 19, (2, 64, 128), generator=g).to(device)
    for kind in ("nchw", "cl"):
        lg = layout(logits, kind)
        h1, p1, i1 = H.seg_eval(lg, labels, n_classes=19, want_ids=True)
        h2, p2, i2 = H.seg_eval(lg, labels, n_classes=19, want_ids=True)
        assert torch.equal(h1, h2) and torch.equal(i1, i2)
        assert torch.equal(p1.view(torch.int64), p2.view(torch.int64)), (p1, p2)
        assert int(h1.sum()) == labels.numel() and float(p1[1]) == labels.numel()


# ------------------------------------------------------------------------------------------------------------------ 4. strides
def run_strides(device):
    """logits = a [::2] batch slice and a [:, 2:21] class slice of a 24-class tensor, read in place; non-contiguous labels"""
    g = torch.Generator().manual_seed(17)
    big = 3.0 * torch.randn(4, 24, 9, 14, generator=g)
    lab_big = torch.randint(0, 19, (2, 21, 2 * 31), generator=g)
    lab_big[torch.rand(lab_big.shape, generator=g) < 0.05] = IGNORE
    logits, labels = big[::2, 2:21], lab_big[:, :, ::2]
    o = oracle(logits, labels)
    labels, near = mask_near_ties(labels, o["gap"])
    o.update(score(o["up"], o["pred"], labels))
    e_ref = abs(unfused_loss_sum(logits.to(device), labels.to(device)) - o["loss_sum"])
    for kind in ("nchw", "cl"):
        bd = layout(big.to(device), kind)
        lg = bd[::2, 2:21]
        assert not lg.is_contiguous() and lg.data_ptr() != bd.data_ptr()
        lab_nc = torch.full((2, 21, 62), 3, dtype=torch.int64, device=device)[:, :, ::2]      # every other element of a wider buffer
        lab_nc.copy_(labels)
        assert not lab_nc.is_contiguous()
        hist, pair, ids = H.seg_eval(lg, lab_nc, n_classes=19, want_ids=True)
        assert torch.equal(hist.cpu().reshape(19, 19), o["hist"]), kind
        assert torch.equal(ids.cpu().long()[~near], o["pred"][~near]), kind
        check_loss(pair.cpu(), o, e_ref, "strides " + kind)


def run_large_batch_stride(device):
    """GPU only: two small images cut from one 2.2 GB buffer, a batch stride past 2^31 bytes"""
    C, Hi, Wi, Ht, Wt = 19, 12, 20, 24, 40
    sb = 540_000_000                                          # elements: 2.16e9 bytes > 2^31
    g = torch.Generator().manual_seed(19)
    logits = 3.0 * torch.randn(2, C, Hi, Wi, generator=g)
    labels = torch.randint(0, C, (2, Ht, Wt), generator=g)
    o = oracle(logits, labels)
    labels, near = mask_near_ties(labels, o["gap"])
    o.update(score(o["up"], o["pred"], labels))
    buf = torch.empty(sb + C * Hi * Wi, dtype=torch.float32, device=device)
    view = buf.as_strided((2, C, Hi, Wi), (sb, Hi * Wi, Wi, 1))
    view.copy_(logits.to(device))
    assert view.stride(0) * 4 > 2 ** 31
    hist, pair, ids = H.seg_eval(view, labels.to(device), n_classes=C, want_ids=True)
    assert torch.equal(hist.cpu().reshape(C, C), o["hist"])
    assert torch.equal(ids.cpu().long()[~near], o["pred"][~near])
    assert float(pair[1]) == o["count"] and abs(float(pair[0]) - o["loss_sum"]) <= 1e-5 * abs(o["loss_sum"])


# ------------------------------------------------------------------------------------------------------------------ 5. runningScore
def run_running_score(device):
    """a mismatched-size update, an equal-size one and a numpy one sum into confusion_matrix; the equal-size call without
    return_loss still goes through segsde_confusion_update"""
    C = 19
    lg_a, lab_a, _, o_a = generated(*GENERATED[0][:2])
    lg_b, lab_b, _, o_b = generated(*GENERATED[6][:2])
    g = np.random.RandomState(23)
    np_true, np_pred = g.randint(0, C, (2, 5, 7)), g.randint(0, C, (2, 5, 7))
    np_hist = np.bincount(C * np_true.reshape(-1) + np_pred.reshape(-1), minlength=C * C).reshape(C, C)
    L = _lib.lib()
    orig, calls = L.segsde_confusion_update, []

    def counting(*a):
        calls.append(1)
        return orig(*a)

    rs = runningScore(C)
    L.segsde_confusion_update = counting
    try:
        loss = rs.update_from_logits(lab_a.to(device), lg_a.to(device), return_loss=True)
        assert not calls
        assert rs.update_from_logits(lab_b.to(device), lg_b.to(device)) is None
        assert len(calls) == 1, "the equal-size call without return_loss keeps its kernel"
    finally:
        L.segsde_confusion_update = orig
    rs.update(np_true, np_pred)
    want = (o_a["hist"] + o_b["hist"]).numpy().astype(np.float64) + np_hist
    assert np.array_equal(rs.confusion_matrix, want)
    ref = runningScore(C)
    ref._host = want.copy()
    (s_got, iu_got), (s_want, iu_want) = rs.get_scores(), ref.get_scores()
    for k in s_want:
        np.testing.assert_allclose(s_got[k], s_want[k], rtol=1e-12)
    for k in iu_want:
        np.testing.assert_allclose(iu_got[k], iu_want[k], rtol=1e-12)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == torch.device(device).type
    mean = o_a["loss_sum"] / o_a["count"]
    assert abs(float(loss) - mean) <= 1e-6 * abs(mean), (float(loss), mean)
    # return_ids alone and with the loss
    ids = runningScore(C).update_from_logits(lab_a.to(device), lg_a.to(device), return_ids=True)
    both = runningScore(C).update_from_logits(lab_a.to(device), lg_a.to(device), return_loss=True, return_ids=True)
    assert ids.dtype == torch.uint8 and torch.equal(ids, both[1]) and torch.equal(both[0], loss)


# ------------------------------------------------------------------------------------------------------------------ 6. meters
METER_VALUES = (0.5, 1.25, 3.0, 0.125)
METER_N = (1, 2, 4, 1)
# the reference's arithmetic (sum += val * n; count += n; avg = sum / count) on that sequence
METER_SUMS = (0.5, 3.0, 15.0, 15.125)
METER_COUNTS = (1, 3, 7, 8)


def run_meters(device):
    m, t, d = AverageMeter(), AverageMeter(), AverageMeterDict()
    assert (m.val, m.avg, m.sum, m.count) == (0, 0, 0, 0) and d.avgs == {} and d.sums == {} and d.counts == {}
    for v, n, s, c in zip(METER_VALUES, METER_N, METER_SUMS, METER_COUNTS):
        m.update(v, n)
        # torch.true_divide of two Python numbers is a float32 tensor, in the reference as well
        assert m.val == v and m.sum == s and m.count == c and torch.equal(m.avg, torch.true_divide(torch.tensor(s), c))
        tv = torch.tensor(v, device=device, requires_grad=True)
        t.update(tv, n)
        assert torch.is_tensor(t.sum) and not t.sum.requires_grad and t.sum.device == tv.device and t.val is not tv
        assert float(t.sum) == s and t.count == c and torch.equal(t.avg, torch.true_divide(torch.tensor(s, device=device), c))
        d.update({"a": tv, "b": 2 * v}, n)
        assert float(d.sums["a"]) == s and d.counts == {"a": c, "b": c} and not d.sums["a"].requires_grad
        assert torch.equal(d.avgs["a"], t.avg) and torch.equal(d.avgs["b"], torch.true_divide(torch.tensor(2 * s), c))
    d.update({"late": torch.tensor(4.0, device=device)})
    assert float(d.avgs["late"]) == 4.0 and d.counts["late"] == 1 and d.counts["a"] == 8
    m.reset()
    d.reset()
    assert (m.val, m.avg, m.sum, m.count) == (0, 0, 0, 0) and d.avgs == {}


# ------------------------------------------------------------------------------------------------------------------ 7. validate
VAL_B, VAL_H, VAL_W = 1, 64, 128


@functools.lru_cache(maxsize=None)
def _validate_setup():
    import bench
    import model_cases as MC
    from oracle import nets as N
    mcfg = MC.contract_cfgs()["cfgs"]["r18_jsd"]
    sd = N.build_state_dict(mcfg, 19, seed=29, randomize_bn=True, zero_attention=False)
    batches = []
    for seed in (41, 42):
        inp = bench.synthetic_inputs(VAL_B, VAL_H, VAL_W, "cpu", seed)
        g = torch.Generator().manual_seed(seed)
        lbl = torch.randint(0, 19, (VAL_B, 2 * VAL_H, 2 * VAL_W), generator=g)
        lbl[torch.rand(lbl.shape, generator=g) < 0.05] = IGNORE
        inp["lbl"] = lbl
        batches.append(inp)
    cfg = {"model": mcfg, "data": {},
           "training": {"amp": False, "segmentation_lambda": 1.0, "monodepth_lambda": 1.0, "n_tensorboard_imgs": 3}}
    return mcfg, sd, batches, cfg


class _TinyHead(torch.nn.Module):
    """stand-in for the interpreter run, where two ResNet-18 batches take minutes: the part of the model's interface validate
    uses (a dict in, a dict with "semantics" out, parameters, the training flag); a fixed 1x1 convolution in plain torch"""

    def __init__(self):
        super().__init__()
        self.head = torch.nn.Conv2d(3, 19, 1)
        with torch.no_grad():
            g = torch.Generator().manual_seed(37)
            self.head.weight.copy_(6.0 * torch.randn(19, 3, 1, 1, generator=g))
            self.head.bias.copy_(torch.randn(19, generator=g))

    def forward(self, inputs):
        return {"semantics": self.head(inputs[("color_aug", 0, 0)])}


def _validate_model(device, kind):
    import bench
    import model_cases as MC
    mcfg, sd, batches, cfg = _validate_setup()
    if kind == "tiny":
        cfg = dict(cfg, model=dict(mcfg, disable_monodepth=True, disable_pose=True))
        return _TinyHead().to(device), None, [{k: v.to(device) for k, v in b.items()} for b in batches], cfg
    model = MC.get_model(mcfg, 19)
    model.load_state_dict(sd, strict=True)
    model.to(device)
    mono = MC.get_monodepth_loss(bench.loss_cfg(VAL_B, VAL_H, VAL_W), False)
    on_dev = [{k: v.to(device) for k, v in b.items()} for b in batches]
    return model, mono, on_dev, cfg


def run_validate(device, kind="r18"):
    """kind: "r18" = the smallest joint model of model_cases (ResNet-18 encoder) with the monodepth branch on; "tiny" = a stand-in
    head without it"""
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    model, mono, batches, cfg = _validate_model(device, kind)
    # the oracle from the very logits validate will see: the same forward, in eval mode under no_grad
    model.eval()
    total = torch.zeros(19, 19, dtype=torch.int64)
    means, preds, nears = [], [], []
    with torch.no_grad():
        for b in batches:
            logits = model(dict(b))["semantics"].float().cpu()
            assert tuple(logits.shape[-2:]) == (VAL_H, VAL_W)
            o = oracle(logits, b["lbl"].cpu())
            lbl, _ = mask_near_ties(b["lbl"].cpu(), o["gap"])
            o.update(score(o["up"], o["pred"], lbl))
            b["lbl"] = lbl.to(device)
            preds.append(o["pred"])
            nears.append(o["gap"] < GAP)
            total += o["hist"]
            means.append(o["loss_sum"] / o["count"])
    model.train()
    out = T.validate(model, [dict(b) for b in batches], cfg, 19, monodepth_loss_calculator_val=mono)
    assert model.training, "the training flag is restored"
    ref = runningScore(19)
    ref._host = total.numpy().astype(np.float64)
    s_want, iu_want = ref.get_scores()
    assert out["score"] == s_want, (out["score"], s_want)
    assert set(out["class_iou"]) == set(iu_want)
    for k in iu_want:
        assert out["class_iou"][k] == iu_want[k] or (np.isnan(out["class_iou"][k]) and np.isnan(iu_want[k])), k
    want = float(np.mean(means))
    got = out["losses"]["segmentation_loss"]
    print("validate segmentation_loss %.9g  oracle %.9g" % (got, want))
    assert isinstance(got, float) and abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert set(out["losses"]) == {"segmentation_loss", "monodepth_loss", "pseudo_depth_loss"}
    assert out["losses"]["pseudo_depth_loss"] == 0.0
    assert np.isfinite(out["losses"]["monodepth_loss"]) and (out["losses"]["monodepth_loss"] != 0.0) == (kind == "r18")
    assert out["depth"] is None
    saved = out["imgs_to_save"]
    assert len(saved) == min(3, 2 * VAL_B)
    for j, (img, label, ids, disp) in enumerate(saved):
        assert ids.dtype == torch.uint8 and tuple(ids.shape) == (2 * VAL_H, 2 * VAL_W) == tuple(label.shape)
        keep = ~nears[j // VAL_B][j % VAL_B]
        assert torch.equal(ids.cpu().long()[keep], preds[j // VAL_B][j % VAL_B][keep])
        assert tuple(img.shape) == (3, VAL_H, VAL_W)
        assert disp is None if kind == "tiny" else tuple(disp.shape[-2:]) == (VAL_H, VAL_W)
    # a custom loss_fn is called as the reference calls it; the matrix still comes from the fused pass
    seen = []

    def loss_fn(input, target):
        seen.append((tuple(input.shape), tuple(target.shape)))
        return torch.tensor(2.5, device=input.device)

    cfg2 = dict(cfg, model=dict(cfg["model"], disable_monodepth=True), training=dict(cfg["training"], n_tensorboard_imgs=0))
    model.eval()
    out2 = T.validate(model, [dict(b) for b in batches], cfg2, 19, loss_fn=loss_fn)
    assert not model.training
    assert seen == [((VAL_B, 19, VAL_H, VAL_W), (VAL_B, 2 * VAL_H, 2 * VAL_W))] * 2
    assert out2["losses"]["segmentation_loss"] == 2.5 and out2["losses"]["monodepth_loss"] == 0.0
    assert out2["score"] == s_want and out2["imgs_to_save"] == []


def run_validate_no_sync(device):
    """GPU only: with the default loss_fn and no depth_teacher the loop body never synchronises -- torch's synchronisation debug
    mode is "error" from the first batch to the exhaustion of the iterator; the copies to the host come after the loop"""
    import pytest
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    model, mono, batches, cfg = _validate_model(device, "r18")
    T.validate(model, [dict(b) for b in batches], cfg, 19, monodepth_loss_calculator_val=mono)      # loads, packs, caches
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()

    def guarded():
        try:
            torch.cuda.set_sync_debug_mode("error")
        except Exception as e:                              # noqa: BLE001
            pytest.skip("this torch build has no synchronisation debug mode on ROCm: %s" % e)
        try:
            for b in batches:
                yield dict(b)
        finally:
            torch.cuda.set_sync_debug_mode(prev)

    try:
        out = T.validate(model, guarded(), cfg, 19, monodepth_loss_calculator_val=mono)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert np.isfinite(out["losses"]["segmentation_loss"]) and len(out["imgs_to_save"]) == 2


# ------------------------------------------------------------------------------------------------------------------ 8. arguments, registry
def run_python_argument_checks(device):
    """refused in Python, before the library is looked up"""
    import pytest
    lg = torch.zeros(2, 5, 4, 6, device=device)
    gt = torch.zeros(2, 8, 12, dtype=torch.int64, device=device)
    saved = _lib._LIB, _lib.LIB_PATH
    _lib._LIB, _lib.LIB_PATH = None, "/nonexistent/libsegsde_hip.so"      # a lookup would raise RuntimeError("... not found")
    try:
        with pytest.raises(TypeError):
            H.seg_eval(lg, gt.int(), n_classes=5)
        with pytest.raises(TypeError):
            H.seg_eval(lg.long(), gt, n_classes=5)
        with pytest.raises(TypeError):
            H.seg_eval(lg[0], gt, n_classes=5)
        with pytest.raises(TypeError):
            H.seg_eval(lg, gt[0], n_classes=5)
        with pytest.raises(ValueError):
            H.seg_eval(lg, gt[:1], n_classes=5)
        with pytest.raises(ValueError):
            H.seg_eval(lg, gt, n_classes=6)
        with pytest.raises(ValueError):
            H.seg_eval(lg, gt, hist=torch.zeros(24, dtype=torch.int64, device=device))
        with pytest.raises(ValueError):
            H.seg_eval(lg, gt, hist=torch.zeros(25, dtype=torch.int32, device=device))
        with pytest.raises(ValueError):
            H.seg_eval(lg, gt, hist=torch.zeros(25, dtype=torch.int64, device="meta"))
        with pytest.raises(ValueError):
            H.seg_eval(lg, gt, hist=None, want_loss=False, want_ids=False)
        with pytest.raises(ValueError):
            H.seg_eval(torch.zeros(1, 300, 2, 2, device=device), gt[:1], n_classes=300, want_ids=True)
        with pytest.raises(ValueError):
            H.seg_eval(lg[:, :, :0], gt, n_classes=5)
    finally:
        _lib._LIB, _lib.LIB_PATH = saved


def run_torch_op(device):
    import improving_segmentation_with_selfsupervised_depth_amd.torch_ops as TO
    assert "segsde::seg_eval" in TO.names() and hasattr(torch.ops.segsde, "seg_eval")
    seed, shape, _ = GENERATED[0]
    logits, labels, near, o = generated(seed, shape)
    C = shape[1]
    hist, pair, ids = torch.ops.segsde.seg_eval(logits.to(device).half(), labels.to(device), 250, True, False)
    assert ids is None and float(pair[1]) == o["count"] and int(hist.sum()) == int(o["hist"].sum())      # half logits: .float()
    hist, pair, ids = torch.ops.segsde.seg_eval(logits.to(device), labels.to(device), want_loss=False, want_ids=True)
    assert pair is None and torch.equal(hist.cpu().reshape(C, C), o["hist"]) and ids.dtype == torch.uint8
