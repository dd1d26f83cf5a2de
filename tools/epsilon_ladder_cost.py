"""Diagnostic: what the config key epsilon_ladder_alpha costs the training loop.  The benchmark's loop (run.train_iteration: rollout,
insert, sample, train) at Cleanup-5, T = 100, class-code storage, captured rollout and train step -- with the key at 0 and at ALPHA in
ONE process, alternating, so that both see the same machine.  Host clock around `steps` iterations that end in a device synchronise;
then the launches of one timestep of either runner one by one with HIP events (back-to-back launches of one kernel), which shows what
the row load behind each pick does to the heads.  Epsilon stays at its start value's schedule: the key changes which rows explore,
not what a launch does.  One JSON line.

    python tools/epsilon_ladder_cost.py --n-env 4096 --steps 100 --warmup 10 --rounds 3 --alpha 7

profiles/epsilon_ladder_cost.json was assembled from these lines."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch as th  # noqa: E402

from homophily_marl_amd.run import load_config, setup, train_iteration  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-env", type=int, default=4096)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--alpha", type=float, default=7.0)
a = ap.parse_args()


def make(alpha):
    over = dict(runner="hip_graph", train_graph=1, batch_size_run=a.n_env, batch_size=a.batch, buffer_size=2 * a.n_env, buffer_cpu_only=False,
                store_state=False, obs_storage="code", env_args=dict(num_agents=5, map="default5", episode_limit=100, seed=1), use_cuda=True,
                save_model=False, learner_log_interval=10 ** 12, strict_device_ops=True, epsilon_ladder_alpha=alpha)
    th.manual_seed(0)
    ctx = setup(load_config("cleanup", overrides=over))
    ctx.episode = 0
    for _ in range(5 + a.warmup):          # both slabs twice (rollout graphs, edge graphs), the train step captured, then the warm-up
        ctx.episode = train_iteration(ctx, ctx.episode)
    th.cuda.synchronize()
    return ctx


def timed(ctx):
    t0 = time.perf_counter()
    for _ in range(a.steps):
        ctx.episode = train_iteration(ctx, ctx.episode)
    th.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / a.steps


def launches_us(ctx):
    """median over three runs of `reps` back-to-back launches of every launch of a timestep but the env step, mid-episode"""
    r = ctx.runner
    r.begin_episode(False)
    for _ in range(10):
        r.step_once()
    th.cuda.synchronize()
    out = {}
    for name, key, fn in r.timestep_launches():
        if key == "env":
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
        out[key] = round(statistics.median(runs[1:]), 3)      # (the first run warms up)
    return out


def refresh_us(ctx):
    """the table's refresh (one pow launch per rollout), back to back"""
    r = ctx.runner
    if r.eps_rows is None:
        return None
    runs = []
    for _ in range(4):
        s, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            th.pow(r.eps, r.expo, out=r.eps_rows)
        e.record()
        th.cuda.synchronize()
        runs.append(1e3 * s.elapsed_time(e) / a.reps)
    return round(statistics.median(runs[1:]), 3)


names = {"off": 0.0, "on": a.alpha}
ctxs = {k: make(v) for k, v in names.items()}
ms = {k: [] for k in names}
for _ in range(a.rounds):
    for k in names:
        ms[k].append(timed(ctxs[k]))
summary = lambda xs: dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)
out = dict(n_env=a.n_env, batch=a.batch, steps=a.steps, warmup=a.warmup, rounds=a.rounds, alpha=a.alpha,
           iteration_ms={k: summary(v) for k, v in ms.items()},
           per_iteration_ms_added=statistics.median(ms["on"]) - statistics.median(ms["off"]),
           refresh_us=refresh_us(ctxs["on"]), launch_us={k: launches_us(c) for k, c in ctxs.items()})
print(json.dumps(out), flush=True)
for c in ctxs.values():
    c.runner.close_env()
