"""Diagnostic: what the config key share_heads (heads tied across agents) costs.  Three measurements, one JSON line each:

  --launch   the tie launch alone: HIP events around `launch-reps` back-to-back ssd_tie_agent_grads calls over the learner's own job
             table and flat gradient buffer at Cleanup-5 ("both": 36 jobs) after `launch-warmup` calls, `launch-rounds` rounds; and the
             spread launch (ssd_agent_spread over the 36 per-agent tensors) the same way.  Summing a gradient buffer over and over
             changes its values, not the work: run on a context that is not used afterwards.
  --train    sample + train per call in the benchmark's loop shape (Cleanup-5, T = 100, class-code storage, captured step, batch 16):
             host clock around `steps` x (ReplayBuffer.sample into the static batch, learner.train) ending in a device synchronise, in a
             FRESH process per run, the processes alternating between this tree with the key on and --parent (a built checkout of the
             parent commit, where the key does not exist) -- or, without --parent, this tree with the key off.
  --bench    bench.py --gpus 1 with the key off (bench.py does not know the key), fresh processes alternating between this tree and
             --parent: is the tree inside the parent's spread?

    python tools/share_heads_cost.py --launch
    python tools/share_heads_cost.py --train --parent /path/to/parent --runs 3
    python tools/share_heads_cost.py --bench --parent /path/to/parent --runs 3

profiles/share_heads_cost.json was assembled from these lines."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--launch", action="store_true")
ap.add_argument("--train", action="store_true")
ap.add_argument("--bench", action="store_true")
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
ap.add_argument("--share", default="both", choices=("env", "inc", "both"))
ap.add_argument("--n-env", type=int, default=256, help="--train / --launch: envs of the rollouts that fill the buffer")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=100)
ap.add_argument("--bench-warmup", type=int, default=10)
ap.add_argument("--launch-reps", type=int, default=200)
ap.add_argument("--launch-warmup", type=int, default=20)
ap.add_argument("--launch-rounds", type=int, default=5)
ap.add_argument("--limit", type=float, default=300.0, help="seconds a child process may take")
ap.add_argument("--child", default=None, help="(internal) the tree whose package this process measures sample + train of")
ap.add_argument("--child-share", default=None)
a = ap.parse_args()
a.parent = os.path.abspath(a.parent) if a.parent else None
sys.path.insert(0, a.child or HERE)


def make(share):
    import torch as th
    from homophily_marl_amd.run import load_config, setup, train_iteration
    over = dict(runner="hip_graph", train_graph=1, batch_size_run=a.n_env, batch_size=a.batch, buffer_size=2 * a.n_env, buffer_cpu_only=False,
                store_state=False, obs_storage="code", env_args=dict(num_agents=5, map="default5", episode_limit=100, seed=1), use_cuda=True,
                save_model=False, learner_log_interval=10 ** 12, strict_device_ops=True)
    if share is not None:
        over["share_heads"] = share
    th.manual_seed(0)
    ctx = setup(load_config("cleanup", overrides=over))
    ep = 0
    for _ in range(5):                     # both slabs twice, the train step captured
        ep = train_iteration(ctx, ep)
    th.cuda.synchronize()
    assert ctx.learner._graph is not None
    return ctx, ep


def sample_train(ctx, n):
    import torch as th
    t0 = time.perf_counter()
    for _ in range(n):
        sample = ctx.buffer.sample(a.batch, out=ctx.learner.sample_out())     # (the vectorised runner fills every slot: no trim)
        ctx.learner.train(sample, ctx.runner.t_env, ctx.train_steps)
        ctx.train_steps += 1
    th.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def child():
    ctx, ep = make(a.child_share)
    sample_train(ctx, a.warmup)
    print(json.dumps(dict(ms_per_call=sample_train(ctx, a.steps))), flush=True)
    ctx.runner.close_env()


def run_child(tree, args):
    out = subprocess.run([sys.executable] + args, cwd=tree, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=a.limit)
    if out.returncode != 0:
        raise SystemExit("child in %s exited %d:\n%s" % (tree, out.returncode, out.stderr[-2000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])


def alternating(sides, measure):
    runs = []
    for r in range(a.runs):
        for side, tree, share in sides:
            runs.append(dict(side=side, run=r + 1, **measure(tree, share)))
    return runs


def launch_us():
    import torch as th
    from homophily_marl_amd import abi
    ctx, _ = make(a.share)
    learner = ctx.learner
    plan = learner._opt_plan
    assert plan.tie is not None
    stream = th.cuda.current_stream().cuda_stream
    learner.head_spreads()
    sp = learner._spread_plan
    calls = {"tie": lambda: plan.lib.ssd_tie_agent_grads(*plan.tie, stream),
             "spread": lambda: sp.lib.ssd_agent_spread(sp.host, sp.dev.data_ptr(), sp.ptrs[2], sp.out.data_ptr(), stream)}
    out = {k: [] for k in calls}
    for _ in range(a.launch_rounds):
        for key, call in calls.items():
            for _ in range(a.launch_warmup):
                abi.check(plan.lib, call())
            s, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.launch_reps):
                abi.check(plan.lib, call())
            e.record()
            th.cuda.synchronize()
            out[key].append(round(1e3 * s.elapsed_time(e) / a.launch_reps, 3))
    ctx.runner.close_env()
    return dict(what="launch", share=a.share, unit="us per call, back to back", n_tie_jobs=int(plan.tie[4]), n_spread_jobs=sp.ptrs[2],
                parameters=int(plan.args.total), tied_elements=sum(int(p.numel()) for p in learner._tied),
                tie_us=statistics.median(out["tie"]), spread_us=statistics.median(out["spread"]), rounds=out)


if a.child:
    child()
elif a.launch:
    print(json.dumps(launch_us()), flush=True)
elif a.train:
    me = os.path.abspath(__file__)
    common = ["--n-env", str(a.n_env), "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    sides = [("parent" if a.parent else "key_off", a.parent or HERE, None), ("key_on", HERE, a.share)]
    runs = alternating(sides, lambda tree, share: run_child(tree, [me, "--child", tree] + (["--child-share", share] if share else []) + common))
    med = {s[0]: statistics.median(r["ms_per_call"] for r in runs if r["side"] == s[0]) for s in sides}
    print(json.dumps(dict(what="sample + train per call", share=a.share, n_env=a.n_env, batch=a.batch, steps=a.steps, warmup=a.warmup, runs=runs,
                          median_ms=med, added_us=1e3 * (med["key_on"] - med[sides[0][0]]))), flush=True)
elif a.bench:
    if not a.parent:
        raise SystemExit("--bench compares against --parent")
    sides = [("parent", a.parent, None), ("tree", HERE, None)]

    def bench(tree, share):
        r = run_child(tree, ["bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)])
        return dict(agent_steps_per_sec=r["value"], ms_per_iteration=r["ms_per_step"])
    runs = alternating(sides, bench)
    span = {s: (min(r["ms_per_iteration"] for r in runs if r["side"] == s), max(r["ms_per_iteration"] for r in runs if r["side"] == s)) for s in ("parent", "tree")}
    print(json.dumps(dict(what="bench.py with the key off", command="bench.py --gpus 1 --steps %d --warmup %d" % (a.bench_steps, a.bench_warmup),
                          runs=runs, ms_per_iteration_min_max=span)), flush=True)
else:
    raise SystemExit("one of --launch, --train, --bench")
