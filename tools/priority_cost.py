"""Diagnostic: launch times of prioritised replay's kernels next to the uniform samplers'.  HIP events around `--timed` back-to-back
launches after `--warmup` launches, `--rounds` rounds; one JSON line.

    python tools/priority_cost.py                       this tree: ssd_sample_ids / ssd_sample_windows / ssd_priority_sample / ssd_priority_update
    python tools/priority_cost.py --root PARENT_TREE    a tree without the priority exports: the uniform samplers alone

Sample launches: population 8192 (and 2^20 for the prioritised draw), counts 16 / 64 / 128, a table with 30 % zeros.  The update: the
benched shape B = 16, T = 100, n = 5, A = 9, its two launches together (k_priority_rows + k_priority_apply) on random partials.
The profiles/prioritized_replay_cost.json of the repository was assembled from these lines."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--timed", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch as th  # noqa: E402

from homophily_marl_amd import ops  # noqa: E402

SEED = 0x1234567890ABCDEF
dev = "cuda"


def timed(launch):
    for i in range(a.warmup):
        launch(i)
    per = []
    for r in range(a.rounds):
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        e0.record()
        for i in range(a.timed):
            launch(a.warmup + r * a.timed + i)
        e1.record()
        th.cuda.synchronize()
        per.append(round(1e3 * e0.elapsed_time(e1) / a.timed, 3))
    return dict(us_per_launch=per, median_us=statistics.median(per))


out = dict(root=os.path.abspath(a.root), warmup=a.warmup, timed=a.timed, rounds=a.rounds, has_priority=hasattr(ops, "priority_sample"))
for count in (16, 64, 128):
    ids, t0 = th.empty(count, dtype=th.long, device=dev), th.empty(count, dtype=th.long, device=dev)
    out["sample_ids_8192_%d" % count] = timed(lambda i: ops.sample_ids(SEED, i, 8192, count, ids))
    out["sample_windows_8192_%d" % count] = timed(lambda i: ops.sample_windows(SEED, i, 8192, count, 76, ids, t0))
if out["has_priority"]:
    g = th.Generator().manual_seed(0)
    for population in (8192, 1 << 20):
        table = th.randint(1, (1 << 24) + 1, (population,), generator=g, dtype=th.int32)
        table[th.rand(population, generator=g) < 0.3] = 0
        table = table.to(dev)
        for count in (16, 64, 128):
            ids, t0 = th.empty(count, dtype=th.long, device=dev), th.empty(count, dtype=th.long, device=dev)
            w, log = th.empty(count, device=dev), th.empty(4, device=dev)
            out["priority_sample_%d_%d" % (population, count)] = timed(
                lambda i: ops.priority_sample(SEED, i, table, population, count, 76, 0.4, ids, t0, w, log))
    B, T, n, A = 16, 100, 5, 9
    part = th.rand(B * T * n, 16, generator=g).to(dev)
    dqe, dqi = th.randn(B, T + 1, n, A, generator=g).to(dev), th.randn(B, T + 1, n, n, 3, generator=g).to(dev)
    ids, w = th.randint(0, 8192, (B,), generator=g).to(dev), th.ones(B, device=dev)        # weights 1: the seeds keep their values over the launches
    q, table = th.empty(B, dtype=th.int32, device=dev), th.zeros(8192, dtype=th.int32, device=dev)
    out["priority_update_16x100x5"] = timed(lambda i: ops.priority_update(part, ids, w, dqe, dqi, q, table, 0.6, 0.9, 1e-3))
    out["priority_update_16x100x5"].update(rows=B * T * n, workgroups_rows_kernel=B, bytes_scaled=4 * (dqe.numel() + dqi.numel()))
print(json.dumps(out), flush=True)
