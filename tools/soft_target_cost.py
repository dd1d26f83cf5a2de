"""Diagnostic: what the config key target_tau (Polyak target updates in the fused optimiser tail) costs.

  * The loop: the benchmark's loop (run.train_iteration: rollout, insert, sample, train) at Cleanup-5, T = 100, class-code storage,
    captured rollout and train step, 8 train steps per rollout -- with the key at 0 and at TAU in ONE process, alternating, so that both
    see the same machine.  Host clock around `steps` iterations that end in a device synchronise.
  * The launch: HIP events around `launch-reps` back-to-back ssd_clip_adam_step calls after `launch-warmup` calls, `launch-rounds` rounds
    alternating n_polyak = 0 and the learner's real job table (the calls keep stepping Adam on the last gradient: run LAST, the
    networks are not used afterwards).
One JSON line.

    python tools/soft_target_cost.py --n-env 4096 --steps 100 --warmup 10 --rounds 3 --tau 0.05

profiles/soft_target_cost.json was assembled from these lines."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch as th  # noqa: E402

from homophily_marl_amd import abi  # noqa: E402
from homophily_marl_amd.run import load_config, setup, train_iteration  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n-env", type=int, default=4096)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--train-steps-per-rollout", type=int, default=8)
ap.add_argument("--tau", type=float, default=0.05)
ap.add_argument("--launch-reps", type=int, default=200)
ap.add_argument("--launch-warmup", type=int, default=20)
ap.add_argument("--launch-rounds", type=int, default=5)
a = ap.parse_args()


def make(tau):
    over = dict(runner="hip_graph", train_graph=1, batch_size_run=a.n_env, batch_size=a.batch, buffer_size=2 * a.n_env, buffer_cpu_only=False,
                store_state=False, obs_storage="code", env_args=dict(num_agents=5, map="default5", episode_limit=100, seed=1), use_cuda=True,
                save_model=False, learner_log_interval=10 ** 12, strict_device_ops=True, train_steps_per_rollout=a.train_steps_per_rollout,
                target_tau=tau)
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


def launch_us(ctx):
    """us per ssd_clip_adam_step call, back to back: {"adam": without jobs, "adam_polyak": with the learner's table}, per round"""
    plan = ctx.learner._opt_plan
    with_jobs = plan.args
    assert with_jobs.n_polyak > 0
    without = abi.SsdClipAdamArgs.from_buffer_copy(bytes(with_jobs))
    without.polyak_jobs, without.n_polyak, without.target_tau, without.polyak_partials = None, 0, 0.0, None
    stream = th.cuda.current_stream().cuda_stream
    out = {"adam": [], "adam_polyak": []}

    def run(args, n):
        for _ in range(n):
            abi.check(plan.lib, plan.lib.ssd_clip_adam_step(C.byref(args), stream))
    for _ in range(a.launch_rounds):
        for key, args in (("adam", without), ("adam_polyak", with_jobs)):
            run(args, a.launch_warmup)
            s, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            s.record()
            run(args, a.launch_reps)
            e.record()
            th.cuda.synchronize()
            out[key].append(round(1e3 * s.elapsed_time(e) / a.launch_reps, 3))
    return dict(out, n_polyak=int(with_jobs.n_polyak), n_adam_jobs=int(with_jobs.n_jobs), parameters=int(with_jobs.total),
                polyak_us_added=round(statistics.median(out["adam_polyak"]) - statistics.median(out["adam"]), 3))


names = {"off": 0.0, "on": a.tau}
ctxs = {k: make(v) for k, v in names.items()}
ms = {k: [] for k in names}
for _ in range(a.rounds):
    for k in names:
        ms[k].append(timed(ctxs[k]))
summary = lambda xs: dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)
out = dict(n_env=a.n_env, batch=a.batch, steps=a.steps, warmup=a.warmup, rounds=a.rounds, tau=a.tau, train_steps_per_rollout=a.train_steps_per_rollout,
           iteration_ms={k: summary(v) for k, v in ms.items()},
           per_iteration_ms_added=statistics.median(ms["on"]) - statistics.median(ms["off"]),
           target_gap_rel=ctxs["on"].learner.target_gap_rel(), launch=launch_us(ctxs["on"]))
print(json.dumps(out), flush=True)
for c in ctxs.values():
    c.runner.close_env()
