"""Cross-replica BatchNorm (models.layers.SyncBatchNorm2d) measured on the GPU, per BatchNorm call, forward plus backward, at
shapes the models have: the synchronized path in a one-rank RCCL group (local stage, all-gather of one row, global stage: every
launch and both collectives of the N-rank path, no peer to wait for) against BatchNorm2d on the same tensors, the two alternating
in one process; with two or more GPUs visible also a two-rank run, one process per GPU.  Then the error ratios of the test cases
(tests/sync_bn_cases.py) on this device.  Writes a markdown report:

    python tools/sync_bn.py --out profiles/sync_bn.md

Not part of the bench.py headline (the feature is off there).  Needs the MI355X: there is no CPU path."""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, NHWC shape, activation, residual)
SHAPES = [("16 x 256 x 128 x 256 (NCHW) after a residual add", (16, 128, 256, 256), "relu", True),
          ("2 x 1024 x 64 x 128, a layer3 bottleneck output of the 1024 x 2048 workload", (2, 64, 128, 1024), "relu", True),
          ("2 x 256 x 32 x 64, an ASPP branch", (2, 32, 64, 256), "relu", False),
          ("2 x 256 x 1 x 1, the ASPP pooling branch", (2, 1, 1, 256), "relu", False)]
BN_PER_STEP = 148            # BatchNorms of a ResNet-101 joint step


def make(shape, residual, device, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen).to(device).requires_grad_(True)
    res = torch.randn(shape, generator=gen).to(device).requires_grad_(True) if residual else None
    dy = torch.randn(shape, generator=gen).to(device)
    return x, res, dy


def call(bn, x, res, dy, act):
    x.grad = None
    if res is not None:
        res.grad = None
    bn.weight.grad = bn.bias.grad = None
    bn(x, residual=res, act=act).backward(dy)


def timed(bn, x, res, dy, act, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        call(bn, x, res, dy, act)
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / steps          # us per call


def median(v):
    v = sorted(v)
    return 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])


def measure(group, device, steps, rounds, shapes=SHAPES):
    """-> [(name, [plain us per round], [sync us per round])]"""
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L
    out = []
    for i, (name, shape, act, residual) in enumerate(shapes):
        C = shape[-1]
        x, res, dy = make(shape, residual, device, 40 + i)
        plain, sync = L.BatchNorm2d(C).to(device).train(), L.SyncBatchNorm2d(C, process_group=group).to(device).train()
        n = max(steps, 5) if x.numel() >= (1 << 24) else 10 * steps      # the small shapes: a longer window
        for bn in (plain, sync, plain, sync):                            # warm-up: code objects, allocator, the communicator
            timed(bn, x, res, dy, act, 3)
        t = ([], [])
        for _ in range(rounds):
            t[0].append(timed(plain, x, res, dy, act, n))
            t[1].append(timed(sync, x, res, dy, act, n))
        out.append((name, t[0], t[1]))
        del x, res, dy
    return out


def _two_rank_worker(rank, port, steps, rounds, path):
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2,
                            timeout=datetime.timedelta(seconds=300))
    try:
        res = measure(dist.group.WORLD, "cuda", steps, rounds)
        dist.barrier()
        if rank == 0:
            torch.save(res, path)
    finally:
        dist.destroy_process_group()


def table(rows, title):
    fmt = lambda v: ", ".join("%.1f" % x for x in v)
    lines = [title, "", "| shape | BatchNorm2d, rounds (us) | median | SyncBatchNorm2d, rounds (us) | median | difference per call (us) | x %d per step (ms) |"
             % BN_PER_STEP, "|---|---|---|---|---|---|---|"]
    for name, a, b in rows:
        d = median(b) - median(a)
        lines.append("| %s | %s | %.1f | %s | %.1f | %.1f | %.2f |" % (name, fmt(a), median(a), fmt(b), median(b), d, d * BN_PER_STEP / 1e3))
    return lines + [""]


def error_ratios():
    """the cases of the test suite on this device -> {(group, tensor): worst ratio}, rows recorded"""
    import batchnorm_cases as BC
    import sync_bn_cases as SC
    first = len(BC.RECORDS)
    for case in SC.CHUNK_CASES:
        SC.run_chunks("cuda", case)
    for case in SC.PARTIAL_CASES:
        for nrows in SC.PARTIAL_ROWS:
            SC.run_partials_source("cuda", case, nrows)
    worst = {}
    for g, _, t, _, _, _, r, _ in BC.RECORDS[first:]:
        t = "dgamma" if t in ("dgamma", "sum dgamma") else ("dbeta" if t in ("dbeta", "sum dbeta") else t)
        worst[(g, t)] = max(worst.get((g, t), 0.0), r)
    return worst, len(BC.RECORDS) - first, BC.K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_bn.md"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-errors", action="store_true", help="skip the error ratios of the test cases")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    import torch.distributed as dist
    import sync_bn_cases as SC
    lines = ["# Cross-replica BatchNorm: cost per call and error ratios", "",
             "Written by `tools/sync_bn.py` on %s (%d GPU%s visible).  Per BatchNorm call, forward plus backward, device events around a"
             % (torch.cuda.get_device_name(0), torch.cuda.device_count(), "" if torch.cuda.device_count() == 1 else "s"),
             "window of calls, `BatchNorm2d` and `SyncBatchNorm2d` alternating in one process, %d rounds.  The synchronized path adds two" % a.rounds,
             "collectives (one row of 2 C + 2 doubles each way) and three small launches per call; a ResNet-101 joint step has about",
             "%d BatchNorms, so about %d collectives.  The last column extrapolates the per-call difference to such a step; it is not a"
             % (BN_PER_STEP, 2 * BN_PER_STEP),
             "measured step time, and `bench.py` does not run this path.", ""]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % SC.free_port(), rank=0, world_size=1,
                            timeout=datetime.timedelta(seconds=300))
    try:
        rows = measure(dist.group.WORLD, "cuda", a.steps, a.rounds)
    finally:
        dist.destroy_process_group()
    lines += table(rows, "## One rank (RCCL group of one process)")
    if torch.cuda.device_count() >= 2:
        import tempfile
        import torch.multiprocessing as mp
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "two.pt")
            mp.spawn(_two_rank_worker, args=(SC.free_port(), a.steps, a.rounds, path), nprocs=2, join=True)
            lines += table(torch.load(path, weights_only=False), "## Two ranks, one process per GPU (rank 0's timings; each rank holds the shape shown)")
    else:
        lines += ["## Two ranks", "", "Not measured: one GPU visible.", ""]
    if not a.no_errors:
        worst, n, K = error_ratios()
        tensors = ["mean", "invstd", "running_mean", "running_var", "y", "dgamma", "dbeta", "dx", "dres"]
        lines += ["## Error against the float64 full-batch oracle: e_kernel / max(e_fp32, 2^-23 * scale), worst channel", "",
                  "The cases of `tests/sync_bn_cases.py` on this device (%d recorded rows; dgamma / dbeta: per-rank sums and the sums over" % n,
                  "the ranks together).  K = %g (`tests/batchnorm_cases.py`)." % K, "",
                  "| group | " + " | ".join(tensors) + " |", "|---|" + "---|" * len(tensors)]
        for g in sorted({g for g, _ in worst}):
            lines.append("| %s | " % g + " | ".join("%.2f" % worst[(g, t)] if (g, t) in worst else "" for t in tensors) + " |")
        top = max(worst.values())
        lines += ["", "Worst ratio: %.2f; K / 2 = %.2f%s." % (top, K / 2, "" if top <= K / 2 else
                                                            " -- ABOVE K / 2: the rule of that file (next power of two, at most 8) applies"), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
