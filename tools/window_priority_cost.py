"""Diagnostic: what the config key per_unit: "window" costs.  One JSON line with two parts.

(a) the draw: ssd_priority_sample over 8192 slots x S = 7 entries (k_priority_sample_seq) next to the same launch over 8192 entries
    (k_priority_sample), counts 16 / 64, a table with 30 % zeros; HIP events around `--timed` back-to-back launches after `--warmup`
    launches, `--rounds` rounds (the method of tools/priority_cost.py).
(b) the loop: the benchmark's loop (run.train_iteration) at Cleanup-5, T = 100, class-code storage, captured rollout and train step,
    prioritised replay on windows (batch 64, train_window 25, train_burn_in 0) with per_initial_priority "rollout" -- per_unit
    "episode" and "window" in ONE process, alternating, host clock around `--steps` iterations that end in a device synchronise;
    then the per-slot priority launch of either runner alone with HIP events (back-to-back launches mid-episode).

    python tools/window_priority_cost.py --n-env 4096 --steps 100 --rounds 3

profiles/window_priority_cost.json was assembled from this line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch as th  # noqa: E402

from homophily_marl_amd import ops  # noqa: E402
from homophily_marl_amd.run import load_config, setup, train_iteration  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-env", type=int, default=4096)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--window", type=int, default=25)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--loop-warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--timed", type=int, default=200)
a = ap.parse_args()
SEED = 0x1234567890ABCDEF


def timed_launches(launch):
    for i in range(a.warmup):
        launch(i)
    per = []
    for r in range(5):
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        e0.record()
        for i in range(a.timed):
            launch(a.warmup + r * a.timed + i)
        e1.record()
        th.cuda.synchronize()
        per.append(round(1e3 * e0.elapsed_time(e1) / a.timed, 3))
    return dict(us_per_launch=per, median_us=statistics.median(per))


def draw_cost():
    g = th.Generator().manual_seed(0)
    out = {}
    S, stride, last = ops.window_grid(100, a.window)
    for label, entries, segments in (("episode_8192", 8192, None), ("window_8192x%d" % S, 8192 * S, (S, stride, last))):
        table = th.randint(1, (1 << 24) + 1, (entries,), generator=g, dtype=th.int32)
        table[th.rand(entries, generator=g) < 0.3] = 0
        table = table.cuda()
        for count in (16, 64):
            ids, t0, ent = (th.empty(count, dtype=th.long, device="cuda") for _ in range(3))
            w, log = th.empty(count, device="cuda"), th.empty(4, device="cuda")
            kw = dict(segments=segments, entries_out=ent) if segments else {}
            out["%s_count_%d" % (label, count)] = timed_launches(
                lambda i: ops.priority_sample(SEED, i, table, entries, count, 76, 0.4, ids, t0, w, log, **kw))
    return out


def make(unit):
    over = dict(runner="hip_graph", train_graph=1, batch_size_run=a.n_env, batch_size=a.batch, buffer_size=2 * a.n_env, buffer_cpu_only=False,
                store_state=False, obs_storage="code", env_args=dict(num_agents=5, map="default5", episode_limit=100, seed=1), use_cuda=True,
                save_model=False, learner_log_interval=10 ** 12, strict_device_ops=True, prioritized_replay=True, per_initial_priority="rollout",
                train_window=a.window, train_burn_in=0, per_unit=unit)
    th.manual_seed(0)
    ctx = setup(load_config("cleanup", overrides=over))
    ctx.episode = 0
    for _ in range(5 + a.loop_warmup):     # both slabs twice (rollout graphs, edge graphs), the train step captured, then the warm-up
        ctx.episode = train_iteration(ctx, ctx.episode)
    th.cuda.synchronize()
    return ctx


def timed(ctx):
    t0 = time.perf_counter()
    for _ in range(a.steps):
        ctx.episode = train_iteration(ctx, ctx.episode)
    th.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / a.steps


def priority_launch_us(ctx):
    """the per-slot priority launch alone, mid-episode: median over three runs of `reps` back-to-back launches after one warm-up run"""
    r = ctx.runner
    r.begin_episode(False)
    for _ in range(30):
        r.step_once()
    th.cuda.synchronize()
    out = {}
    for name, key, fn in r.timestep_launches():
        if key != "rollout_priority":
            continue
        runs = []
        for _ in range(4):
            s, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.reps):
                fn()
            e.record()
            th.cuda.synchronize()
            runs.append(1e3 * s.elapsed_time(e) / a.reps)
        out[name] = round(statistics.median(runs[1:]), 3)
    return out


out = dict(n_env=a.n_env, batch=a.batch, window=a.window, grid=ops.window_grid(100, a.window), steps=a.steps, rounds=a.rounds, draw=draw_cost())
names = ["episode", "window"]
ctxs = {k: make(k) for k in names}
ms = {k: [] for k in names}
for _ in range(a.rounds):
    for k in names:
        ms[k].append(timed(ctxs[k]))
out["iteration_ms"] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), runs=v) for k, v in ms.items()}
out["last_draw_log"] = {k: [round(float(x), 4) for x in c.buffer._draws.log.cpu().tolist()] for k, c in ctxs.items()}
out["priority_launch_us"] = {k: priority_launch_us(c) for k, c in ctxs.items()}
print(json.dumps(out), flush=True)
for c in ctxs.values():
    c.runner.close_env()
