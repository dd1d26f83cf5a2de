"""Diagnostic: what the config key mixer: "vdn" (the team's TD error on the env head) costs.  Three measurements, one JSON line each:

  --launch   ssd_team_td alone at the train step's shape (Cleanup-5, T = 100, batch 16: 1600 (b, t) pairs, 8000 rows): HIP events around
             `launch-reps` back-to-back calls behind one ssd_td_sim_loss on the learner's own Q-values after `launch-warmup` calls,
             `launch-rounds` rounds, at td_lambda 0 and 0.5; the launch is idempotent (it reads the loss launch's inputs, or its columns
             5 and 13, and rewrites the same seeds and column 2).  Next to it the launch's bytes, counted from the shape, and the time
             HBM would need for them at its measured copy rate: the HBM floor.
  --train    sample + train per call in the benchmark's loop shape (Cleanup-5, T = 100, class-code storage, captured step, batch 16):
             host clock around `steps` x (ReplayBuffer.sample into the static batch, learner.train) ending in a device synchronise, in a
             FRESH process per run, alternating between the key off and the key on in this tree.
  --bench    bench.py --gpus 1 with the key off (bench.py does not know the key), fresh processes alternating between this tree and
             --parent (a built checkout of the parent commit): is the tree's median inside the parent's range?

    python tools/team_mixer_cost.py --launch
    python tools/team_mixer_cost.py --train --runs 3
    python tools/team_mixer_cost.py --bench --parent /path/to/parent --runs 5

profiles/team_mixer_cost.json was assembled from these lines."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_COPY_TBS = 6.29              # measured float4 copy rate of one MI355X (spec 8.0 TB/s)

ap = argparse.ArgumentParser()
ap.add_argument("--launch", action="store_true")
ap.add_argument("--train", action="store_true")
ap.add_argument("--bench", action="store_true")
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
ap.add_argument("--n-env", type=int, default=256, help="--train / --launch: envs of the rollouts that fill the buffer")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--bench-steps", type=int, default=100)
ap.add_argument("--bench-warmup", type=int, default=10)
ap.add_argument("--launch-reps", type=int, default=200)
ap.add_argument("--launch-warmup", type=int, default=20)
ap.add_argument("--launch-rounds", type=int, default=5)
ap.add_argument("--limit", type=float, default=300.0, help="seconds a child process may take")
ap.add_argument("--child", action="store_true", help="(internal) this process measures sample + train")
ap.add_argument("--child-mixer", default=None)
a = ap.parse_args()
a.parent = os.path.abspath(a.parent) if a.parent else None
sys.path.insert(0, HERE)


def make(mixer, capture=True, **more):
    import torch as th
    from homophily_marl_amd.run import load_config, setup, train_iteration
    over = dict(runner="hip_graph", train_graph=int(capture), batch_size_run=a.n_env, batch_size=a.batch, buffer_size=2 * a.n_env, buffer_cpu_only=False,
                store_state=False, obs_storage="code", env_args=dict(num_agents=5, map="default5", episode_limit=100, seed=1), use_cuda=True,
                save_model=False, learner_log_interval=10 ** 12, strict_device_ops=True, **more)
    if mixer is not None:
        over["mixer"] = mixer
    th.manual_seed(0)
    ctx = setup(load_config("cleanup", overrides=over))
    ep = 0
    for _ in range(5):                     # both slabs twice, the train step captured
        ep = train_iteration(ctx, ep)
    th.cuda.synchronize()
    assert (ctx.learner._graph is not None) == capture
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
    ctx, ep = make(a.child_mixer)
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
        for side, tree, mixer in sides:
            runs.append(dict(side=side, run=r + 1, **measure(tree, mixer)))
            print("# %s" % json.dumps(runs[-1]), file=sys.stderr, flush=True)
    return runs


def launch_bytes(B, T, n, A, lam):
    """what one ssd_team_td must move, from the shape: per row the taken action (8), the seed and column 2 written (8); at td_lambda 0
    the availability, live and target rows of slot t + 1 (3 A f32 / i32), the chosen value and the reward (8) and the row's column of
    the n x n incentive actions (8 n); at td_lambda > 0 columns 5 and 13 (8); per (b, t) filled and two terminated flags (10)"""
    row = 8 + 8 + ((3 * A * 4 + 8 + 8 * n) if lam == 0 else 8)
    return B * T * n * row + B * T * 10


def launch_us():
    import ctypes as C
    import torch as th
    from homophily_marl_amd import abi, ops
    out = dict(what="launch", unit="us per call, back to back (HIP events)", reps=a.launch_reps, warmup=a.launch_warmup)
    for lam in (0.0, 0.5):
        ctx, _ = make("vdn", capture=False, td_lambda=lam)
        learner, args = ctx.learner, ctx.args
        batch = ctx.buffer.sample(a.batch)
        with th.no_grad():
            q_env, q_inc, tq_env, tq_inc = (x.contiguous() for x in learner.unroll_pair(batch))
        dens = learner.denominators(batch).contiguous().float()
        B, T, n, A = batch.batch_size, batch.max_seq_length - 1, args.n_agents, args.n_actions
        partials = th.zeros(B * T * n, abi.TD_LOSS_PARTIALS, device=q_env.device)
        dq_env, dq_inc = th.empty_like(q_env), th.empty_like(q_inc)
        t, keep = ops._td_loss_args(batch, args, A, partials)
        t.q_env, t.q_inc, t.tq_env, t.tq_inc = q_env.data_ptr(), q_inc.data_ptr(), tq_env.data_ptr(), tq_inc.data_ptr()
        t.dens, t.dq_env, t.dq_inc = dens.data_ptr(), dq_env.data_ptr(), dq_inc.data_ptr()
        lib = abi.load_library()
        stream = th.cuda.current_stream().cuda_stream
        abi.check(lib, lib.ssd_td_sim_loss(C.byref(t), 1, stream))
        calls = {"team_td": lambda: lib.ssd_team_td(C.byref(t), stream), "loss": lambda: lib.ssd_td_sim_loss(C.byref(t), 1, stream)}
        rounds = {k: [] for k in calls}
        for _ in range(a.launch_rounds):
            for key in ("loss", "team_td"):                 # (team_td last: it leaves the buffers as a train step leaves them)
                for _ in range(a.launch_warmup):
                    abi.check(lib, calls[key]())
                s, e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.launch_reps):
                    abi.check(lib, calls[key]())
                e.record()
                th.cuda.synchronize()
                rounds[key].append(round(1e3 * s.elapsed_time(e) / a.launch_reps, 3))
        nbytes = launch_bytes(B, T, n, A, lam)
        out["td_lambda_%g" % lam] = dict(shape=dict(batch=B, T=T, n_agents=n, n_actions=A, pairs=B * T, rows=B * T * n),
                                          team_td_us=statistics.median(rounds["team_td"]), team_td_us_min_max=[min(rounds["team_td"]), max(rounds["team_td"])],
                                          loss_launch_us=statistics.median(rounds["loss"]), rounds=rounds, bytes=nbytes,
                                          hbm_floor_us=round(nbytes / (HBM_COPY_TBS * 1e12) * 1e6, 4), hbm_rate_tb_s=HBM_COPY_TBS)
        ctx.runner.close_env()
    return out


if a.child:
    child()
elif a.launch:
    print(json.dumps(launch_us()), flush=True)
elif a.train:
    me = os.path.abspath(__file__)
    common = ["--child", "--n-env", str(a.n_env), "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    sides = [("key_off", HERE, None), ("key_on", HERE, "vdn")]
    runs = alternating(sides, lambda tree, mixer: run_child(tree, [me] + common + (["--child-mixer", mixer] if mixer else [])))
    per = {s[0]: [r["ms_per_call"] for r in runs if r["side"] == s[0]] for s in sides}
    med = {k: statistics.median(v) for k, v in per.items()}
    print(json.dumps(dict(what="sample + train per call", mixer="vdn", n_env=a.n_env, batch=a.batch, steps=a.steps, warmup=a.warmup, runs=runs,
                          median_ms=med, min_max_ms={k: [min(v), max(v)] for k, v in per.items()}, added_us=1e3 * (med["key_on"] - med["key_off"]))), flush=True)
elif a.bench:
    if not a.parent:
        raise SystemExit("--bench compares against --parent")
    sides = [("parent", a.parent, None), ("tree", HERE, None)]

    def bench(tree, mixer):
        r = run_child(tree, ["bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)])
        return dict(agent_steps_per_sec=r["value"], ms_per_iteration=r["ms_per_step"])
    runs = alternating(sides, bench)
    per = {s: [r["ms_per_iteration"] for r in runs if r["side"] == s] for s in ("parent", "tree")}
    print(json.dumps(dict(what="bench.py with the key off", command="bench.py --gpus 1 --steps %d --warmup %d" % (a.bench_steps, a.bench_warmup),
                          runs=runs, ms_per_iteration_min_max={s: [min(v), max(v)] for s, v in per.items()},
                          ms_per_iteration_median={s: statistics.median(v) for s, v in per.items()},
                          tree_median_inside_parent_range=min(per["parent"]) <= statistics.median(per["tree"]) <= max(per["parent"]))), flush=True)
else:
    raise SystemExit("one of --launch, --train, --bench")
