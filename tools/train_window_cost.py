"""Diagnostic: device time of sample + train per call, on whole episodes or on sampled time windows (config keys train_window /
train_burn_in), and of the window gather alone.  Cleanup-5, T = 100, class-code storage, the captured train step; HIP events on the
launch stream.  One JSON line.

    python tools/train_window_cost.py --batch 16                              whole episodes (today's path)
    python tools/train_window_cost.py --batch 64 --window 25 --burn-in 10     windows
    python tools/train_window_cost.py --batch 64 --window 15 --stored-state   windows from the rollout's stored recurrent state
    python tools/train_window_cost.py --batch 64 --window 25 --gather-only    ssd_gather_windows alone (captured back to back)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/train_window_cost.py ...      the kernels' own times

The sample launches (draw + gather, or ssd_sample_ids + ssd_gather_rows) and the train step are bracketed separately: event, sample,
event, train, event, `calls` times per round; the train step is far longer than the host's work per call, so the host runs ahead and
the intervals are device time.  The profiles/train_window_cost.json of the repository was assembled from these lines."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch as th  # noqa: E402

from homophily_marl_amd.run import load_config, setup  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--window", type=int, default=0)
ap.add_argument("--burn-in", type=int, default=0)
ap.add_argument("--n-env", type=int, default=512)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--gather-only", action="store_true")
ap.add_argument("--stored-state", action="store_true", help="config key train_stored_state")
a = ap.parse_args()

over = dict(runner="hip_graph", train_graph=1, batch_size_run=a.n_env, batch_size=a.batch, buffer_size=a.n_env, buffer_cpu_only=False,
            store_state=False, obs_storage="code", env_args=dict(num_agents=5, map="default5", episode_limit=100, seed=1), use_cuda=True,
            save_model=False, runner_stats=False, learner_log_interval=10 ** 12)
if a.window:
    over.update(train_window=a.window, train_burn_in=a.burn_in, train_stored_state=a.stored_state)
th.manual_seed(0)
ctx = setup(load_config("cleanup", overrides=over))
buf, learner = ctx.buffer, ctx.learner
buf.insert_episode_batch(ctx.runner.run(False))
summary = lambda xs: dict(median=statistics.median(xs), min=min(xs), max=max(xs))
ev = lambda: th.cuda.Event(enable_timing=True)
out = dict(batch=a.batch, window=a.window, burn_in=a.burn_in, stored_state=a.stored_state, slots=(a.window or 100) + 1, rounds=a.rounds, calls_per_round=a.calls)

if a.gather_only:
    buf.sample_windows(a.batch, a.window, a.burn_in)
    ids, t0 = buf.last_window_ids, buf.last_window_t0
    dst = buf.gather_windows(ids, t0, a.window, a.burn_in)
    out["bytes_copied"] = sum(v[0].numel() * v.element_size() for v in dst.data.transition_data.values()) * a.batch
    out["fields"] = len(dst.data.transition_data)
    stream = th.cuda.Stream()
    graph = th.cuda.CUDAGraph()
    th.cuda.synchronize()
    with th.cuda.graph(graph, stream=stream):
        for _ in range(a.calls):
            buf.gather_windows(ids, t0, a.window, a.burn_in, out=dst)
    for _ in range(3):
        graph.replay()
    per = []
    for _ in range(a.rounds):
        e0, e1 = ev(), ev()
        e0.record(); graph.replay(); e1.record()
        th.cuda.synchronize()
        per.append(1e3 * e0.elapsed_time(e1) / a.calls)
    out["gather_us_per_launch_back_to_back"] = summary(per)
else:
    def sample():
        if a.window:
            return buf.sample_windows(a.batch, a.window, a.burn_in, out=learner.sample_out())
        return buf.sample(a.batch, out=learner.sample_out())
    for i in range(8):                                                   # past the capture (third call) and the first replays
        learner.train(sample(), 100 * a.n_env, i)
    th.cuda.synchronize()
    assert learner._graph is not None
    s_us, t_us, n = [], [], 8
    for _ in range(a.rounds):
        marks = []
        for _ in range(a.calls):
            e0, e1, e2 = ev(), ev(), ev()
            e0.record(); batch = sample(); e1.record(); learner.train(batch, 100 * a.n_env, n); e2.record()
            n += 1
            marks.append((e0, e1, e2))
        th.cuda.synchronize()
        s_us.append(1e3 * sum(x.elapsed_time(y) for x, y, _ in marks) / a.calls)
        t_us.append(1e3 * sum(y.elapsed_time(z) for _, y, z in marks) / a.calls)
    out["sample_us_per_call"], out["train_us_per_call"] = summary(s_us), summary(t_us)
    out["rows"] = a.batch * (out["slots"] - 1)
print(json.dumps(out), flush=True)
ctx.runner.close_env()
