"""ms per training iteration (one rollout of episode_limit = 100 timesteps + one train step, run.train_iteration) of Cleanup-5 x 4096
envs with class-code storage at several views, and which timestep the hip_graph runner takes there (FastPolicy or the generic torch
timestep; pipelined or not).

    python tools/view_iters.py [--views 3,5,10,7] [--iters 20] [--warmup 4] [--root TREE] [--agents 10 --map default10] [--set KEY=VALUE ...]

--agents / --map: another team size; --set: extra config keys (YAML values), e.g. --set obs_distance=True fused_onehot_gather=True.

--root: import the package from another checkout (e.g. the parent commit's, to measure "before" with the same script).
strict_device_ops is off so that a tree without the encoder at a view can still run it (its learner then expands the codes).
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="3,5,10,7")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--n-env", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--map", default="default5")
    ap.add_argument("--set", nargs="*", default=[], metavar="KEY=VALUE")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch as th
    import yaml
    extra = {kv.split("=", 1)[0]: yaml.safe_load(kv.split("=", 1)[1]) for kv in a.set}
    from homophily_marl_amd.run import load_config, setup, train_iteration
    for view in [int(v) for v in a.views.split(",")]:
        N = a.n_env
        cfg = load_config("cleanup", overrides=dict(runner="hip_graph", train_graph=1, steps_per_graph=10, batch_size_run=N, batch_size=16,
                                                    buffer_size=2 * N, obs_storage="code", buffer_cpu_only=False, store_state=False,
                                                    env_args=dict(num_agents=a.agents, map=a.map, episode_limit=100, seed=1, view_size=view),
                                                    use_cuda=True, save_model=False, runner_stats=False, **extra))
        th.manual_seed(0)
        ctx = setup(cfg)
        ep = 0
        for _ in range(a.warmup):
            ep = train_iteration(ctx, ep)
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            ep = train_iteration(ctx, ep)
        th.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / a.iters
        r = ctx.runner
        path = "generic" if r.fast is None else ("FastPolicy pipe" if r.pipe else "FastPolicy")
        print("view %2d  V %2d  %-16s %8.2f ms / iteration  (%d iterations, N = %d, n = %d%s)" %
              (view, 2 * view + 1, path, ms, a.iters, N, a.agents, "".join(" " + kv for kv in a.set)), flush=True)
        r.close_env()
        del ctx
        th.cuda.empty_cache()


if __name__ == "__main__":
    main()
