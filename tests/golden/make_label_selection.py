#!/usr/bin/env python
"""Fixture recipe of the label-selection tests (build container only: needs the reference tree).

Feeds the seeded inputs of tests/label_selection_cases.py to the REFERENCE's own functions and writes what they return to
tests/golden/label_selection.npz (numbers only), plus ``inspect.signature`` of those functions to
tests/golden/label_selection_signatures.json.

The reference's label_selection.py imports its whole training stack at module level (datasets, TensorBoard, ray through
experiments.py).  The stubbed import that make_trainstep.py uses for train.py was not attempted here: on top of that recipe's stubs
it would need stand-ins for ray, the dataset loaders and the experiment tables, a larger surface than the seven functions wanted, and
a stub that drifts from the reference would fail silently.  So the module is not imported: the named functions are taken out of the file with ``ast`` when this script runs and
executed in a namespace of torch / numpy / math / deepcopy plus the reference's own ``pixel_wise_entropy`` (loss/loss.py) and
``np_local_seed`` (utils/utils.py), both imported from their files.  The error-map expressions live inside ``acquire_scores``:
its ``for depth_error_type in depth_error_types`` loop is taken out the same way and run per sample on (disp_pred, disp_pseudo).
Nothing of the reference's text is stored here or in the fixture.

Recorded: discrete results (farthest-point indices / distances, chosen lists, dilation masks, NaN patterns, permutations) and
e_ref = (max, rms) error of the reference's fp32 results against the float64 evaluations of label_selection_cases.py.

  --check   recompute everything and compare with the committed fixture: discrete results exactly, error figures within a factor
            of two (they depend on the CPU's vector math library, the gates take them times three)."""
import argparse
import ast
import copy
import importlib.util
import inspect
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SEGSDE_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
for p_ in (REPO, os.path.join(REPO, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
OUT = os.path.join(HERE, "label_selection.npz")
SIG = os.path.join(HERE, "label_selection_signatures.json")
WANT = ("dilate", "_calc_feature_distance", "iterative_farthest_point", "choose_samples_from_scores", "choose_samples_from_ifp",
        "choose_initial_samples", "get_n_total")


def _from_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_namespace():
    path = os.path.join(REF, "label_selection.py")
    tree = ast.parse(open(path).read())
    ns = {"torch": torch, "np": np, "math": math, "deepcopy": copy.deepcopy,
          "pixel_wise_entropy": _from_file("_ref_loss", os.path.join(REF, "loss", "loss.py")).pixel_wise_entropy,
          "np_local_seed": _from_file("_ref_utils", os.path.join(REF, "utils", "utils.py")).np_local_seed}
    loop = None
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in WANT:
            exec(compile(ast.Module([node], []), path, "exec"), ns)
        if isinstance(node, ast.FunctionDef) and node.name == "acquire_scores":
            for sub in ast.walk(node):
                if isinstance(sub, ast.For) and isinstance(sub.target, ast.Name) and sub.target.id == "depth_error_type":
                    loop = compile(ast.Module([sub], []), path, "exec")
    assert loop is not None and all(n in ns for n in WANT)
    ns["_error_loop"] = loop
    return ns


def ref_error_maps(ns, dp, ds, types):
    """one sample [H,W]: the reference's loop -> (maps, means)"""
    env = dict(ns, disp_pred=torch.from_numpy(dp), disp_pseudo=torch.from_numpy(ds), depth_error_types=list(types),
               depth_error_maps=[], depth_errors=[])
    exec(ns["_error_loop"], env)
    return [m.numpy() for m in env["depth_error_maps"]], [float(e) for e in env["depth_errors"]]


def fps_f64(d, current, n_new, pre):
    """the loop in float64 -> (indices, smallest relative lead of a winner over the runner-up)"""
    d = d.copy()
    if pre is not None:
        d[:, [i for i in range(d.shape[0]) if i not in pre]] = 0
    current, new, lead = list(current), [], math.inf
    for _ in range(n_new):
        m = d[current].min(0)
        order = np.argsort(-m, kind="stable")
        if order[0] in current:
            break
        if m[order[0]] > 0 and len(order) > 1:
            lead = min(lead, (m[order[0]] - m[order[1]]) / m[order[0]])
        else:
            lead = 0.0
        current.append(int(order[0]))
        new.append(int(order[0]))
    return new, lead


def build():
    import label_selection_cases as C
    ns = reference_namespace()
    out = {}
    # ---- farthest point
    for name, (kind, N, seed, current, n_new, pre) in C.FPS_CASES.items():
        ident = {i: i for i in range(N)}
        m = torch.from_numpy(C.fps_matrix(kind, N, seed))
        new, d = ns["iterative_farthest_point"](list(current), {"distances": m, "dist_i_to_img_idx": ident, "img_idx_to_dist_i": ident},
                                                n_new, pre)
        out["fps_%s_idx" % name] = np.asarray(new, dtype=np.int64)
        out["fps_%s_dist" % name] = np.asarray([float(x) for x in d], dtype=np.float32)
    assert out["fps_pre_complement_low_idx"].tolist()[10:] == [0] and out["fps_zeros_one_then_stop_idx"].tolist() == [0]
    assert len(out["fps_more_than_possible_idx"]) == 7 and len(out["fps_zeros_stop_at_once_idx"]) == 0
    # ---- distances: torch.cdist in fp32 against float64
    eref = []
    for N, D, p in C.DIST_CASES:
        bank = C.dist_bank(N, D)
        t = torch.from_numpy(bank)
        eref.append(C.errors(C.offdiag(torch.cdist(t, t, p=p).numpy()), C.offdiag(C.dist_f64(bank, p))))
    out["dist_eref"] = np.asarray(eref, dtype=np.float64)
    f = C.cfd_features()
    feats = [torch.from_numpy(f[i:i + 1]) for i in range(C.CFD_N)]
    eref = []
    for norm, bw, p in C.CFD_CASES:
        r = ns["_calc_feature_distance"](feats, C.cfd_bias(), bw, p, norm, False).numpy()
        eref.append(C.errors(C.offdiag(r), C.offdiag(C.cfd_f64(f, C.cfd_bias(), bw, p, norm))))
    out["cfd_eref"] = np.asarray(eref, dtype=np.float64)
    fc = C.cfd_features(const_channel=True)
    r = ns["_calc_feature_distance"]([torch.from_numpy(fc[i:i + 1]) for i in range(C.CFD_N)], [], 0, 2, True, False)
    out["cfd_const_isnan"] = torch.isnan(r).numpy().astype(np.uint8)
    # ---- scores
    pwe = ns["pixel_wise_entropy"]
    for name, (B, Cc, Hh, W, _, _, types, _) in C.SCORE_CASES.items():
        x, dp, ds = C.score_inputs(name)
        ent64, maps64, masked = C.score_f64(x, dp, ds, types)
        ent = pwe(torch.from_numpy(x))
        T = len(types)
        maps, means = np.zeros((B, T, Hh, W), dtype=np.float32), np.zeros((B, 1 + T), dtype=np.float32)
        for b in range(B):
            means[b, 0] = float(torch.mean(ent[b]))
            if T:
                mp, mn = ref_error_maps(ns, dp[b], ds[b], types)
                maps[b], means[b, 1:] = np.stack(mp), mn
                assert np.array_equal(maps[b, types.index("abs")] == 0, masked[b]), name
        rows = [C.errors(ent.numpy(), ent64)] + [C.errors(maps[:, t], maps64[:, t]) for t in range(T)]
        rows += [C.errors(means[:, 0], ent64.mean(axis=(1, 2)))] + [C.errors(means[:, 1 + t], maps64[:, t].mean(axis=(1, 2))) for t in range(T)]
        out["score_%s_eref" % name] = np.asarray(rows, dtype=np.float64)
        if name in ("s23x40_c19", "s64x128_c20_pitched"):
            out["mask_" + name] = ns["dilate"]((torch.from_numpy(ds[0]) < 0.07).float(), 7, 3).numpy().astype(np.uint8)
    x, _, _ = C.score_inputs("s23x40_c19")
    ent64, _, _ = C.score_f64(x, x[:, 0], x[:, 0], [])
    out["pwe_norm_eref"] = np.asarray(C.errors(pwe(torch.from_numpy(x), normalize=True).numpy(),
                                               (ent64 - ent64.min()) / (ent64.max() - ent64.min())), dtype=np.float64)
    # ---- pooling: torch's adaptive pools in fp32 against float64
    rows = []
    for hw, tr in C.POOL_CASES:
        x = C.pool_input(hw)
        t32, t64 = C.pool_transform_t(torch.from_numpy(x), tr), C.pool_transform_t(torch.from_numpy(x).double(), tr)
        rows.append([C.errors(fn(t32, (C.POOL_H, 2 * C.POOL_H)).numpy(), fn(t64, (C.POOL_H, 2 * C.POOL_H)).numpy())
                     for fn in (torch.nn.functional.adaptive_avg_pool2d, torch.nn.functional.adaptive_max_pool2d)])
    out["pool_eref"] = np.asarray(rows, dtype=np.float64)
    # ---- host mirrors
    chosen, sc = ns["choose_samples_from_scores"](C.toy_scores(20, 2, 0, True), 6)
    out["choose_scores_list2"], out["choose_scores_list2_used"] = np.asarray(chosen, dtype=np.int64), np.asarray([s["used_label_criterion"] for s in sc])
    flat = C.toy_scores(20, 1, 1)
    for s in flat:
        s["label_criterion"] = s["label_criterion"][0]
    chosen, sc = ns["choose_samples_from_scores"](flat, 5)
    out["choose_scores_flat"], out["choose_scores_flat_used"] = np.asarray(chosen, dtype=np.int64), np.asarray([s["used_label_criterion"] for s in sc])
    totals = []
    for k, ds_name in enumerate(("cityscapes", "camvid", "mapillary")):
        cfg = {"seed": 7 + k, "data": {"dataset": ds_name}}
        totals.append(ns["get_n_total"](cfg))
        out["initial_random_" + ds_name] = np.asarray(ns["choose_initial_samples"](cfg, 9, "random"), dtype=np.int64)
    out["n_total"] = np.asarray(totals, dtype=np.int64)
    # ---- the selection fixture: features of low intrinsic dimension, on which the reference's choice is stable
    N, D = C.IFP_N, C.IFP_C * C.IFP_H * 2 * C.IFP_H
    to_img = {i: 1000 + i for i in range(N)}
    to_row = {v: k for k, v in to_img.items()}
    for seed in range(1, 200):
        r = C.rng(11, seed)
        latent, proj = r.random((N, 2)), r.standard_normal((2, D))
        bank = (latent[:, :1] * proj[0] + latent[:, 1:] * proj[1] + 0.01 * r.standard_normal((N, D))).astype(np.float32)
        crit = r.random(N).astype(np.float32)
        bias = (np.float32(0.5) * crit).astype(np.float32)
        g = {"ifp_bank": torch.from_numpy(bank), "ifp_criterion": torch.from_numpy(crit)}
        feats = [torch.from_numpy(bank[i].reshape(1, C.IFP_C, C.IFP_H, 2 * C.IFP_H)) for i in range(N)]
        f4 = bank.reshape(N, C.IFP_C, C.IFP_H, 2 * C.IFP_H)
        initial = [0, 1]
        res, ok = {}, True
        for n_add in (C.IFP_ADD_SMALL, C.IFP_ADD):
            for tag, bw, mult in (("plain", 0, None), ("bias", 1.0, None), ("preselect", 0, 2)):
                d = ns["_calc_feature_distance"](feats, bias.tolist(), bw, 2, True, False)
                chosen, _ = ns["choose_samples_from_ifp"]([1000 + i for i in initial], C.ifp_scores(g),
                                                          {"distances": 1.0 * d, "dist_i_to_img_idx": to_img, "img_idx_to_dist_i": to_row},
                                                          n_add, mult)
                pre = None
                if mult is not None:
                    pre = [int(i) for i in np.argsort(-crit, kind="stable")[:int(mult * n_add)]]
                new64, lead = fps_f64(C.cfd_f64(f4, bias, bw, 2, True), initial, n_add, pre)
                ok = ok and lead >= 1e-4 and [1000 + i for i in new64] == chosen
                res["ifp_chosen%d_%s" % (n_add, tag)] = np.asarray(chosen, dtype=np.int64)
        if ok:
            break
    else:
        raise SystemExit("no seed gives a selection that is stable at 1e-4 relative in float64")
    print("selection fixture: seed", seed)
    out.update(res)
    out.update({"ifp_bank": bank, "ifp_criterion": crit, "ifp_bias": bias, "ifp_initial": np.asarray(initial, dtype=np.int64)})
    sigs = {n: str(inspect.signature(ns[n])) for n in WANT}
    sigs["loss.loss:pixel_wise_entropy"] = str(inspect.signature(pwe))
    return out, sigs


DISCRETE = ("fps_", "cfd_const_isnan", "mask_", "choose_", "initial_", "n_total", "ifp_")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(8)
    out, sigs = build()
    if not args.check:
        np.savez_compressed(OUT, **out)
        json.dump(sigs, open(SIG, "w"), indent=1, sort_keys=True)
        print("wrote %s (%d bytes), %d arrays" % (OUT, os.path.getsize(OUT), len(out)))
        return 0
    z = np.load(OUT, allow_pickle=False)
    bad = sorted(set(z.files) ^ set(out))
    for k in sorted(set(z.files) & set(out)):
        a, b = z[k], out[k]
        if k.startswith(DISCRETE):
            same = a.shape == b.shape and (np.array_equal(a, b) if a.dtype.kind in "US" else np.array_equal(a.view(np.uint8), b.view(np.uint8)))
        else:
            same = a.shape == b.shape and bool(np.all((b <= 2 * a + 1e-300) & (a <= 2 * b + 1e-300)))
        if not same:
            bad.append(k)
    if json.load(open(SIG)) != sigs:
        bad.append("signatures")
    print("check:", "ok" if not bad else bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
