#!/usr/bin/env python
"""Fixture recipe of the patch-wise distance tests (build container only: needs the reference tree).

Feeds the seeded inputs of tests/patch_distance_cases.py to the REFERENCE's own ``_calc_feature_distance`` with
``patch_wise=True`` on the CPU and writes what it returns to tests/golden/patch_distance.npz (numbers only).  The function is
taken out of the reference's file with ``ast`` when this script runs, by the recipe of make_label_selection.py
(``reference_namespace``, imported from there); nothing of the reference's text is stored here or in the fixture.

Recorded: ``eref`` = (max, rms) error of the reference's fp32 result against ``patch_f64`` of the cases file, off the diagonal,
per entry of ``GRID``; ``const_isnan``: the NaN pattern of the constant-channel case under normalisation; the selection case:
``sel_seed`` (0: the bank of the label-selection fixture qualifies; otherwise the seed of ``sel_inputs``), ``sel_initial`` and the
reference's chosen lists ``sel_chosen<n>_<variant>``, each asserted to be the float64 selection with a relative lead of every
winner of at least 1e-4.

  --check   recompute everything and compare with the committed fixture: discrete results exactly, error figures within a factor
            of two (they depend on the CPU's vector math library, the gates take them times three)."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for p_ in (REPO, os.path.join(REPO, "tests"), HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
OUT = os.path.join(HERE, "patch_distance.npz")


def build():
    import patch_distance_cases as C
    from make_label_selection import fps_f64, reference_namespace
    ns = reference_namespace()

    def ref(f, bias, bw, p, norm):
        with contextlib.redirect_stdout(io.StringIO()):      # the branch prints every shape
            return ns["_calc_feature_distance"]([torch.from_numpy(f[i:i + 1]) for i in range(f.shape[0])], bias, bw, p, norm, True)

    out = {}
    eref = []
    for k, p, norm in C.GRID:
        N, Cc, hw = C.CASES[k]
        f = C.features(N, Cc, hw)
        r = ref(f, [], 0, p, norm).numpy()
        assert r.shape == (N, N)
        eref.append(C.errors(C.offdiag(r), C.offdiag(C.patch_f64(f, [], 0, p, norm))))
        print("N=%-3d C=%-3d P=%dx%-2d p=%d norm=%d  e_ref max %.3e rms %.3e" % (N, Cc, hw[0], hw[1], p, norm, eref[-1][0], eref[-1][1]))
    out["eref"] = np.asarray(eref, dtype=np.float64)
    N, Cc, hw, ch = C.CONST_CASE
    out["const_isnan"] = torch.isnan(ref(C.features(N, Cc, hw, const_channel=ch), [], 0, 2, True)).numpy().astype(np.uint8)
    # ---- the selection case
    to_img = {i: 1000 + i for i in range(C.SEL_N)}
    to_row = {v: k for k, v in to_img.items()}
    initial = [0, 1]
    for seed in range(0, 200):
        f, crit, bias = C.sel_inputs(seed)
        res, ok = {}, True
        for n_add in C.SEL_ADDS:
            for tag, bw, mult in C.SEL_VARIANTS:
                d = ref(f, bias.tolist(), bw, 2, True)
                with contextlib.redirect_stdout(io.StringIO()):
                    chosen, _ = ns["choose_samples_from_ifp"]([1000 + i for i in initial], C.sel_scores(crit),
                                                              {"distances": 1.0 * d, "dist_i_to_img_idx": to_img, "img_idx_to_dist_i": to_row},
                                                              n_add, mult)
                pre = None
                if mult is not None:
                    pre = [int(i) for i in np.argsort(-crit, kind="stable")[:int(mult * n_add)]]
                new64, lead = fps_f64(C.patch_f64(f, bias, bw, 2, True), initial, n_add, pre)
                ok = ok and lead >= 1e-4 and [1000 + i for i in new64] == chosen
                res["sel_chosen%d_%s" % (n_add, tag)] = np.asarray(chosen, dtype=np.int64)
        if ok:
            break
    else:
        raise SystemExit("no seed gives a selection that is stable at 1e-4 relative in float64")
    print("selection fixture: seed", seed, "(0 = the bank of label_selection.npz)")
    out.update(res)
    out.update({"sel_seed": np.asarray(seed, dtype=np.int64), "sel_initial": np.asarray(initial, dtype=np.int64)})
    return out


DISCRETE = ("const_isnan", "sel_")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(8)
    out = build()
    if not args.check:
        np.savez_compressed(OUT, **out)
        print("wrote %s (%d bytes), %d arrays" % (OUT, os.path.getsize(OUT), len(out)))
        return 0
    z = np.load(OUT, allow_pickle=False)
    bad = sorted(set(z.files) ^ set(out))
    for k in sorted(set(z.files) & set(out)):
        a, b = z[k], out[k]
        if k.startswith(DISCRETE):
            same = a.shape == b.shape and np.array_equal(a, b)
        else:
            same = a.shape == b.shape and bool(np.all((b <= 2 * a + 1e-300) & (a <= 2 * b + 1e-300)))
        if not same:
            bad.append(k)
    print("check:", "ok" if not bad else bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
