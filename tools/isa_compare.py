#!/usr/bin/env python3
"""Pair the conv_igemm_kernel / conv_wgrad_kernel / colreduce_kernel instantiations of two builds and compare their gfx950 code.

    hipcc <build() flags> -save-temps -c csrc/conv_igemm.hip      (once per build, in a directory of its own; likewise elementwise.hip)
    tools/isa_compare.py parent/conv_igemm-hip-amdgcn-amd-amdhsa-gfx950.s branch/conv_igemm-hip-amdgcn-amd-amdhsa-gfx950.s \
                         parent/elementwise-hip-amdgcn-amd-amdhsa-gfx950.s branch/elementwise-hip-amdgcn-amd-amdhsa-gfx950.s

The parent is the build before the decided experiment variants were removed (template arguments <.., MODE, BK, VARX> and
<.., MODEX>), the branch the one after (<.., MODE, CLAMP, CMP> and <.., MODE, CMP>): parent <128,128,2,2,4,32,16> pairs with branch
<128,128,2,2,4,false,1>.  For every pair: LDS bytes equal, no scratch, VGPR / AGPR / SGPR counts not higher, occupancy not lower,
instruction count not higher; and the basic blocks that hold v_mfma (the K loops) carry the same instruction sequence, operands
included except the offsets of scalar loads from the kernel-argument segment.  Prints a markdown table; exit status 1 on a failure.

    tools/isa_compare.py --pairing wino parent/winograd_fused-...gfx950.s branch/winograd_fused-...gfx950.s  (+ winograd_wgrad, conv_igemm)

pairs the kernels around the removal of the decided Winograd switches instead: parent wino_fused_kernel<STATS, true, UPSKIP> with branch
<STATS, UPSKIP> (the planar weight layout, <., false, .>, has no successor), parent wino_wgrad_fused_kernel<H, DB, 2, UPSKIP> with
branch <H, DB, UPSKIP> (staging variant 2, <4, true, 1, .>, has none), reflect_borders_kernel and every conv_igemm_kernel /
conv_wgrad_kernel with the instantiation of the same arguments."""
import re
import sys

INFO = {"lds": r"; LDSByteSize: (\d+)", "scratch": r"; ScratchSize: (\d+)", "vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)",
        "sgpr": r"; TotalNumSgprs: (\d+)", "occ": r"; Occupancy: (\d+)"}
KERNELS = ("conv_igemm_kernel", "conv_wgrad_kernel", "colreduce_kernel")
WINO_KERNELS = ("conv_igemm_kernel", "conv_wgrad_kernel", "wino_fused_kernel", "wino_wgrad_fused_kernel", "reflect_borders_kernel")


def parse(path):
    """mangled name -> dict(info..., blocks=[[instruction line, ...], ...])"""
    out, cur, name = {}, None, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m and any(k in m.group(1) for k in KERNELS):
            name, cur = m.group(1), {"blocks": [[]]}
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur["body_done"] = True
        elif not cur.get("body_done"):
            if re.match(r"^\.LBB\d+_\d+:", line):
                cur["blocks"].append([])
            elif re.match(r"^\t[a-z]", line):
                cur["blocks"][-1].append(re.sub(r"\s*;.*$", "", line.strip()))
        else:
            for k, pat in INFO.items():
                m = re.match(pat, line)
                if m:
                    cur[k] = int(m.group(1))
            if "occ" in cur:
                out[name], cur = cur, None
    return out


def targs(name, kernel):
    """integer / bool template arguments of the instantiation (class arguments, e.g. colreduce's Op, stay in `rest`)"""
    head = name[name.index(kernel) + len(kernel):]
    args = head[1:head.index("EEv")] if head.startswith("I") else ""
    ints = [int(a or b) for a, b in re.findall(r"L[ij](\d+)E|Lb([01])E", args)]
    rest = re.sub(r"L[ij]\d+E|Lb[01]E", "", args)
    return ints, rest


def branch_key(name):
    for k in KERNELS:
        if k in name:
            ints, rest = targs(name, k)
            return (k, tuple(ints), rest)


def parent_key(name):
    """the branch instantiation a parent instantiation became, or None if it was an experiment variant"""
    if "conv_igemm_kernel" in name:
        (bm, bn, wm, wn, mode, bk, varx), rest = targs(name, "conv_igemm_kernel")
        var, cmp_ = varx & 15, varx >> 4
        if bk != 32 or var not in (0, 9) or mode == 2:
            return None
        return ("conv_igemm_kernel", (bm, bn, wm, wn, mode, int(var == 9), cmp_), rest)
    if "conv_wgrad_kernel" in name:
        (bkt, bn, wm, wn, modex), rest = targs(name, "conv_wgrad_kernel")
        if modex & 15 in (2, 4):
            return None
        return ("conv_wgrad_kernel", (bkt, bn, wm, wn, modex & 15, modex >> 4), rest)
    return branch_key(name)


def parent_key_wino(name):
    if "wino_fused_kernel" in name:
        (stats, ublk, upskip), rest = targs(name, "wino_fused_kernel")
        return ("wino_fused_kernel", (stats, upskip), rest) if ublk else None
    if "wino_wgrad_fused_kernel" in name:
        (wt_h, db, minb, upskip), rest = targs(name, "wino_wgrad_fused_kernel")
        return ("wino_wgrad_fused_kernel", (wt_h, db, upskip), rest) if minb == 2 else None
    return branch_key(name)


def norm(ins):
    ins = re.sub(r"\.LBB\d+_\d+", ".LBB", ins)
    if ins.startswith("s_load_"):      # kernel-argument offsets moved: ConvP lost a field, the kernels lost an argument
        ins = re.sub(r"(0x[0-9a-f]+|\d+)$", "OFF", ins)
    return ins


def mfma_blocks(k):
    return [[norm(i) for i in b] for b in k["blocks"] if any(i.startswith("v_mfma") for i in b)]


def main(argv):
    global KERNELS, parent_key
    if argv[:1] == ["--pairing"]:
        assert argv[1] in ("tune", "wino"), argv[1]
        if argv[1] == "wino":
            KERNELS, parent_key = WINO_KERNELS, parent_key_wino
        argv = argv[2:]
    pairs = list(zip(argv[0::2], argv[1::2]))
    rows, bad, dropped = [], [], []
    for ppath, bpath in pairs:
        par, br = parse(ppath), parse(bpath)
        bkeys = {branch_key(n): n for n in br}
        seen = set()
        for pn in sorted(par):
            key = parent_key(pn)
            if key is None:
                dropped.append(pn)
                continue
            if key not in bkeys:
                bad.append("no branch instantiation for %s" % (key,))
                continue
            seen.add(key)
            p, b = par[pn], br[bkeys[key]]
            ni_p, ni_b = sum(map(len, p["blocks"])), sum(map(len, b["blocks"]))
            mp, mb = mfma_blocks(p), mfma_blocks(b)
            checks = {"LDS": p["lds"] == b["lds"], "scratch": b["scratch"] == 0, "VGPR": b["vgpr"] <= p["vgpr"], "AGPR": b["agpr"] <= p["agpr"],
                      "SGPR": b["sgpr"] <= p["sgpr"], "occupancy": b["occ"] >= p["occ"], "instructions": ni_b <= ni_p, "K loops": mp == mb}
            label = "%s<%s%s>" % (key[0], ",".join(map(str, key[1])), (" " + key[2]) if key[2] else "")
            rows.append("| `%s` | %d / %d | %d | %d / %d | %d / %d | %d / %d | %d / %d | %d / %d | %d blocks, %d instr: %s |" % (
                label, p["lds"], b["lds"], b["scratch"], p["vgpr"], b["vgpr"], p["agpr"], b["agpr"], p["sgpr"], b["sgpr"], p["occ"], b["occ"],
                ni_p, ni_b, len(mb), sum(map(len, mb)), "identical" if mp == mb else "DIFFER"))
            bad += ["%s: %s" % (label, c) for c, ok in checks.items() if not ok]
        bad += ["branch instantiation without a parent: %s" % (k,) for k in bkeys if k not in seen]
    print("| kernel (branch template arguments) | LDS bytes | scratch | VGPR | AGPR | SGPR | occupancy | instructions | v_mfma blocks |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    print("\nEvery cell is parent / branch.  %d pairs; %d parent instantiations (experiment variants) have no successor." % (len(rows), len(dropped)))
    if bad:
        print("\nFAILED:\n" + "\n".join("- " + b for b in bad))
        return 1
    print("\nAll checks hold.")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
