"""Automatic selection of the images worth annotating (the third contribution of the paper; the reference's label_selection.py)
on the HIP kernels of csrc/labelsel.hip.

Free functions over tensors and models.  What the reference's ``acquire_scores`` computes per image with about fifteen
full-resolution torch passes and three host round trips is one launch of ``hipops.labelsel_score`` per batch here; the feature
bank is filled by ``hipops.labelsel_pool`` and turned into distances by the direct-form ``hipops.labelsel_distance`` (exact zeros
for identical rows, bitwise symmetric); ``iterative_farthest_point`` is one launch of one workgroup and one device-to-host copy.
``choose_samples_from_scores`` / ``choose_samples_from_ifp`` / ``choose_initial_samples`` are host Python like the reference's.

Not here: the matplotlib dump, ``label_selection_main``, ``train_on_subset`` and ``build_trainer`` (file, TensorBoard and
dataset orchestration around the reference's Trainer; INTEGRATION.md 1d shows how the reference's script uses this module).
The reference's patch-wise distances (``ifp_args["pw"]``: a directed Chamfer distance between the pooled maps of two images)
are ``patch_feature_distance`` on ``hipops.labelsel_patch_distance``; ``acquire_scores`` calls it for ``pw: True``.
Limits: ``p`` is 1 or 2; patch-wise distances take at most ``hipops.LABELSEL_PATCH_MAX_P`` = 128 positions per image (h <= 8),
their matrix is not symmetric, and a NaN feature makes every distance it enters NaN, as ``torch.min`` does;
``_calc_feature_distance(..., patch_wise=True)`` itself still raises NotImplementedError (see its docstring); at most
``hipops.LABELSEL_FPS_MAX_N`` samples in the farthest-point loop; the selection on a distance matrix that holds NaN is
unspecified."""
import contextlib

import numpy as np
import torch

from . import hipops as H

N_TOTAL = {"cityscapes": 2975, "camvid": 367, "mapillary": 18000}
FEATURE_MODES = {"u3": "none", "u4": "none", "bn": "none", "depth": "inv_clamp", "logdepth": "log_inv_clamp"}


@contextlib.contextmanager
def np_local_seed(seed):
    """numpy's global generator seeded inside the block, its previous state restored afterwards (utils/utils.py)"""
    saved = np.random.get_state()
    np.random.seed(seed)
    try:
        yield
    finally:
        np.random.set_state(saved)


def get_n_total(cfg):
    try:
        return N_TOTAL[cfg["data"]["dataset"]]
    except KeyError:
        raise NotImplementedError


def dilate(input, kernel_size, padding):
    """[H,W] map -> clamp(window sum, 0, 1) over kernel_size x kernel_size windows with zero padding (for a 0/1 mask: the maximum).
    A utility mirror of the reference's helper; the scoring path forms its 7x7 dilation inside the score kernel."""
    pad = int(padding)
    assert pad == padding
    s = torch.nn.functional.avg_pool2d(input[None, None], kernel_size, stride=1, padding=pad, count_include_pad=True,
                                       divisor_override=1)
    return torch.clamp(s, 0, 1)[0, 0]


class FeatureBank:
    """The pooled depth features of the sample pool: a preallocated float32 [N, C*h*2h] matrix on the device plus the two
    index maps of the reference (row of the matrix <-> image index).  ``add`` pools one batch of feature maps straight into
    the next rows (``pool``: avg / max; ``mode``: u3 / u4 / bn features as they are, depth / logdepth: the pseudo-disparity
    through clamp(1/x, 0.1, 80) and its log)."""

    def __init__(self, N, C, h, pool="avg", mode="u3", device="cuda"):
        if pool not in ("avg", "max"):
            raise NotImplementedError(pool)
        if mode not in FEATURE_MODES:
            raise NotImplementedError(mode)
        self.N, self.C, self.h, self.pool, self.mode = int(N), int(C), int(h), pool, mode
        self.P = self.h * 2 * self.h
        self.bank = torch.zeros((self.N, self.C * self.P), dtype=torch.float32, device=device)
        self.n = 0
        self.dist_i_to_img_idx = {}
        self.img_idx_to_dist_i = {}

    def add(self, features, img_indices):
        """features [B,C,H,W] (either layout), img_indices: B image indices"""
        B = features.shape[0]
        if features.shape[1] != self.C or self.n + B > self.N or len(img_indices) != B:
            raise ValueError("feature batch %s does not fit the bank (C=%d, %d of %d rows used)" % (tuple(features.shape), self.C,
                                                                                                     self.n, self.N))
        H.labelsel_pool(features.detach().float(), self.h, self.bank, self.n, self.pool, FEATURE_MODES[self.mode])
        for i, idx in enumerate(img_indices):
            self.dist_i_to_img_idx[self.n + i] = int(idx)
            self.img_idx_to_dist_i[int(idx)] = self.n + i
        self.n += B

    def features(self):
        return self.bank[:self.n]


def _bank_and_bias(features, bias, bias_weight, normalize_features):
    """features: a list of [1,C,H,W] tensors or a FeatureBank -> ([N, C*P] bank, normalised on a copy when asked; C; P = H*W;
    the column bias as a float32 tensor or None)"""
    if isinstance(features, FeatureBank):
        C, P = features.C, features.P
        bank = features.features()
        if normalize_features:
            bank = bank.clone()
    else:
        assert isinstance(features, list)
        assert features[0].shape[0] == 1
        feats = torch.cat(features).float()
        N, C, Hh, W = feats.shape
        P = Hh * W
        bank = feats.reshape(N, C * P)
        if normalize_features and bank.data_ptr() == features[0].data_ptr():
            bank = bank.clone()
    if normalize_features:
        H.labelsel_normalize_(bank, C, P)
    b = None
    if bias_weight > 0:
        assert len(bias) == bank.shape[0]
        b = torch.tensor([float(v) for v in bias], dtype=torch.float32)
    return bank, C, P, b


def _calc_feature_distance(features, bias, bias_weight, p, normalize_features, patch_wise):
    """features: a list of [1,C,h,2h] tensors (the reference's argument) or a FeatureBank -> [N,N] distances between the
    flattened features, + bias[j] on column j when bias_weight > 0, zero diagonal.  The caller's features are not modified.

    ``patch_wise=True`` is refused here and lives in ``patch_feature_distance``: the refusal is part of what the package's
    test cases pin for this function, and the reference calls the function only from ``acquire_scores``, which this package
    replaces and which dispatches on ``ifp_args["pw"]`` itself."""
    if patch_wise:
        raise NotImplementedError("patch_wise feature distances: call patch_feature_distance (acquire_scores does for pw: True)")
    bank, _, _, b = _bank_and_bias(features, bias, bias_weight, normalize_features)
    return H.labelsel_distance(bank, p, b)


def patch_feature_distance(features, bias, bias_weight, p, normalize_features):
    """The reference's ``_calc_feature_distance(..., patch_wise=True)`` (label_selection.py:582-612): features: a list of
    [1,C,H,W] tensors of any H, W (P = H*W positions) or a FeatureBank -> [N,N] directed Chamfer distances
    D[i,j] = mean_a min_b ||f_i[:,a] - f_j[:,b]||_p, + bias[j] on column j when bias_weight > 0, zero diagonal.
    One launch of ``hipops.labelsel_patch_distance``: no (200 P) x (N P) intermediate.  P <= 128 and p in (1, 2), else
    NotImplementedError; D is not symmetric; NaN propagates.  The caller's features and the bank are not modified."""
    bank, C, P, b = _bank_and_bias(features, bias, bias_weight, normalize_features)
    return H.labelsel_patch_distance(bank, C, P, p, b)


def iterative_farthest_point(current_samples, feature_distances, n_new, preselected_samples=None):
    """Add up to n_new samples, each the one whose smallest distance to the current samples is largest (ties: the lowest
    row of the matrix); with ``preselected_samples`` the columns of all other samples read as 0 -- they stay in the
    competition, so a zero-distance sample can win, and the loop stops when a current sample wins.
    -> (new image indices, their distances as 0-dim tensors).  NaN in the matrix: unspecified."""
    dist = feature_distances["distances"]
    to_img, to_row = feature_distances["dist_i_to_img_idx"], feature_distances["img_idx_to_dist_i"]
    current = [to_row[s] for s in current_samples]
    pre = None if preselected_samples is None else [to_row[s] for s in preselected_samples]
    idx, d = H.labelsel_farthest_point(dist, current, n_new, pre)
    return [to_img[i] for i in idx], [d[k] for k in range(len(idx))]


def _idx(s):
    return s["idx"].item() if torch.is_tensor(s["idx"]) else int(s["idx"])


def choose_samples_from_scores(scores, n_to_add):
    """the n_to_add highest label criteria; with a list of criteria, n_to_add / n_criteria samples per criterion in turn"""
    if isinstance(scores[0]["label_criterion"], list):
        n_criteria = len(scores[0]["label_criterion"])
        per = n_to_add // n_criteria
        assert n_criteria * per == n_to_add
        chosen_samples, chosen_scores = [], []
        for c in range(n_criteria):
            for s in sorted(scores, key=lambda k: k["label_criterion"][c], reverse=True):
                if _idx(s) not in chosen_samples:
                    s["used_label_criterion"] = f"C{c}_{s['label_criterion'][c]:.4f}"
                    s["depth_error"] = s["depth_error"][c]
                    if "depth_error_map" in s:
                        s["depth_error_map"] = s["depth_error_map"][c]
                    chosen_samples.append(_idx(s))
                    chosen_scores.append(s)
                if len(chosen_samples) >= (c + 1) * per:
                    break
    else:
        chosen_scores = sorted(scores, key=lambda k: k["label_criterion"], reverse=True)[:n_to_add]
        for s in chosen_scores:
            s["used_label_criterion"] = f"{s['label_criterion']:.4f}"
        chosen_samples = [_idx(s) for s in chosen_scores]
    return chosen_samples, chosen_scores


def choose_samples_from_ifp(initial_samples, scores, feature_distances, n_to_add, preselection_multiplier):
    """farthest-point selection, optionally restricted to the int(preselection_multiplier * n_to_add) highest-scoring samples"""
    assert len(scores[0]["label_criterion"]) == 1
    preselected = None
    if preselection_multiplier is not None:
        assert preselection_multiplier > 0
        ranked = sorted(scores, key=lambda k: k["label_criterion"][0], reverse=True)
        preselected = [_idx(s) for s in ranked[:int(preselection_multiplier * n_to_add)]]
        print("LABEL_SELECTION: Preselected samples:", preselected)
    idxs, ifp_distances = iterative_farthest_point(initial_samples, feature_distances, n_to_add, preselected)
    by_idx = {}
    for s in scores:
        by_idx.setdefault(_idx(s), []).append(s)
    chosen_samples, chosen_scores = [], []
    for i, dist in zip(idxs, ifp_distances):
        if preselected is not None:
            assert i in preselected
        for s in by_idx.get(i, []):
            s.update({"label_criterion": dist, "used_label_criterion": f"{dist:.4f}", "iterative_farthest_distance": dist,
                      "depth_error": s["depth_error"][0]})
            if "depth_error_map" in s:
                s["depth_error_map"] = s["depth_error_map"][0]
            chosen_samples.append(i)
            chosen_scores.append(s)
    assert len(chosen_scores) == n_to_add
    return chosen_samples, chosen_scores


def choose_initial_samples(cfg, n, mode, feature_distances=None):
    """mode "random": the first n of the seeded permutation of the pool.  mode "ifp": its first sample, then n - 1 farthest
    points of ``feature_distances`` (the dict ``acquire_scores`` returns for the whole pool; the reference builds it with a
    scoring run without a model)."""
    with np_local_seed(cfg["seed"]):
        perm = np.random.permutation(get_n_total(cfg))
    if mode == "random":
        return perm[:n].tolist()
    if mode == "ifp":
        if feature_distances is None:
            raise ValueError("initial samples by ifp need the feature distances of the pool")
        seed_sample = perm[:1].tolist()
        new, _ = iterative_farthest_point(seed_sample, feature_distances, n - 1)
        assert len(new) == n - 1
        return seed_sample + new
    raise NotImplementedError(mode)


def _as_list(v):
    return v if isinstance(v, list) else [v]


def _device_of(*modules):
    for m in modules:
        if m is not None:
            for p in m.parameters():
                return p.device
    return None


def acquire_scores(model, batches, samples_to_score, label_selection_cfg, depth_teacher=None, depth_ifp_w=0, amp=False,
                   verbose=False, n_total=None, device=None):
    """The scoring loop of the reference (label_selection.py:383-571) over ``batches``: an iterable of input dicts (``idx`` [B],
    ("color_aug", 0, 0), ``pseudo_depth`` [B,1,H,W]) at any batch size.  ``label_selection_cfg``: the ``label_selection`` section
    of the reference's config (depth_lambda, entropy_lambda, bias_weight, ifp_args, depth_error_types).  ``depth_teacher``: the
    frozen depth model whose ("upconv", 3) / ("upconv", 4) / "bottleneck" features fill the bank in the u3 / u4 / bn modes.
    ``n_total``: rows of the bank (default: counted from ``batches``, which is then consumed into a list first).
    The batches may live on the host (a DataLoader's): every tensor of a batch except ``idx`` is moved to the device of the
    model (of the depth teacher without a model; ``device``, default "cuda", when neither has parameters) at the top of the
    loop, as ``trainer.train_step`` does; the caller's dicts are left as they are.

    Runs under no_grad with the models in eval().  Per-sample scores go to one device table that is copied to the host once
    after the loop; the dicts returned carry 0-dim tensors cut from that copy under the reference's keys.
    -> (scores, {"distances", "dist_i_to_img_idx", "img_idx_to_dist_i"})"""
    cfg = label_selection_cfg
    calc_depth_distances = depth_ifp_w > 0
    depth_lambda, entropy_lambda = cfg["depth_lambda"], cfg["entropy_lambda"]
    dist_bias_weight = cfg["bias_weight"]
    ifp_args = cfg.get("ifp_args", {})
    error_types = _as_list(cfg.get("depth_error_types", "abs"))
    T = len(error_types)
    if not verbose:
        if isinstance(depth_lambda, list):
            for dl, el in zip(depth_lambda, entropy_lambda):
                assert dl + el > 0
        else:
            assert depth_lambda + entropy_lambda > 0 or calc_depth_distances
    assert not (isinstance(depth_lambda, list) and T > 1)
    if calc_depth_distances:
        mode = ifp_args["m"]
        if mode not in FEATURE_MODES:
            raise NotImplementedError(mode)
        if ifp_args["pool"] not in ("avg", "max"):
            raise NotImplementedError(ifp_args["pool"])
        if mode in ("u3", "u4", "bn") and depth_teacher is None:
            raise ValueError("feature mode %r needs the depth teacher" % mode)
    if n_total is None:
        batches = list(batches)
        n_total = sum(int(b["idx"].numel()) for b in batches)
    score_all = set(int(s) for s in samples_to_score)
    was_training = [(m, m.training) for m in (model, depth_teacher) if m is not None]
    for m, _ in was_training:
        m.eval()
    dev = _device_of(model, depth_teacher) or torch.device(device if device is not None else "cuda")
    bank, table, row = None, None, 0
    maps = {}                      # table row -> (entropy map, error maps) in verbose mode
    order = []                     # (image index, table row or None) in loader order
    with torch.no_grad():
        for inputs in batches:
            idxs = [int(i) for i in inputs["idx"].reshape(-1).tolist()]
            B = len(idxs)
            inputs = {k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) and k != "idx" else v) for k, v in inputs.items()}
            if calc_depth_distances:
                if mode == "u3":
                    feats = depth_teacher(inputs)[("upconv", 3)]
                elif mode == "u4":
                    feats = depth_teacher(inputs)[("upconv", 4)]
                elif mode == "bn":
                    feats = depth_teacher(inputs)["bottleneck"]
                else:
                    feats = inputs["pseudo_depth"]
                if bank is None:
                    bank = FeatureBank(n_total, feats.shape[1], ifp_args["h"], ifp_args["pool"], mode, feats.device)
                bank.add(feats, idxs)
                if not verbose and dist_bias_weight == 0:
                    order.extend((i, None) for i in idxs)
                    continue
            with torch.autocast(device_type="cuda", enabled=bool(amp)):
                outputs = model(inputs)
            logits = outputs["semantics"].float()
            disp_pred = outputs[("disp", 0)][:, 0].float()
            disp_pseudo = inputs["pseudo_depth"][:, 0].float()
            if table is None:
                table = torch.zeros((n_total, 1 + T), dtype=torch.float32, device=logits.device)
            _, ent, err = H.labelsel_score(logits, disp_pred, disp_pseudo, error_types, want_maps=verbose, table=table[row:row + B])
            for k, i in enumerate(idxs):
                order.append((i, row + k))
                if verbose and i in score_all:         # own copies: a view would keep the whole batch's maps alive
                    maps[row + k] = (ent[k].clone(), [err[k, t].clone() for t in range(T)])
            row += B
    for m, t in was_training:
        m.train(t)
    host = table.cpu() if table is not None else None          # the one copy
    scores, dist_bias = [], []
    for i, r in order:
        if r is None:
            scores.append({"idx": torch.tensor(i), "label_criterion": [0], "depth_error": [0], "entropy_mean": 0})
            continue
        if i not in score_all:
            dist_bias.append(0)
            continue
        entropy_mean = host[r, 0]
        depth_errors = [host[r, 1 + t] for t in range(T)]
        depth_error_maps = list(maps[r][1]) if verbose else []
        if isinstance(depth_lambda, list):
            label_criterion = [dl * depth_errors[-1] + el * entropy_mean for dl, el in zip(depth_lambda, entropy_lambda)]
            depth_errors = depth_errors + [depth_errors[-1]] * len(depth_lambda)
            if verbose:
                depth_error_maps = depth_error_maps + [depth_error_maps[-1]] * len(depth_lambda)
        else:
            label_criterion = [depth_lambda * e + entropy_lambda * entropy_mean for e in depth_errors]
        if dist_bias_weight > 0:
            assert len(label_criterion) == 1
            dist_bias.append(dist_bias_weight * label_criterion[0])
        s = {"idx": torch.tensor(i), "label_criterion": label_criterion, "depth_error": depth_errors, "entropy_mean": entropy_mean}
        if verbose:
            s.update({"segmentation_entropy": maps[r][0], "depth_error_map": depth_error_maps})
        scores.append(s)
    distances = 0
    if calc_depth_distances:
        if ifp_args.get("pw", False):
            distances = patch_feature_distance(bank, dist_bias, dist_bias_weight, p=ifp_args["p"],
                                               normalize_features=ifp_args.get("norm", False))
        else:
            distances = _calc_feature_distance(bank, dist_bias, dist_bias_weight, p=ifp_args["p"],
                                               normalize_features=ifp_args.get("norm", False), patch_wise=False)
    return scores, {"distances": depth_ifp_w * distances,
                    "dist_i_to_img_idx": bank.dist_i_to_img_idx if bank is not None else {},
                    "img_idx_to_dist_i": bank.img_idx_to_dist_i if bank is not None else {}}
