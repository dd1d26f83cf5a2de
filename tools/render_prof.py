"""Timing of render mode on Cleanup-5 x 4096 (COUNTER mode): the fused step+observe kernel with render mode off and on, and
k_render of every env.  Run under `rocprofv3 --kernel-trace --stats -- python tools/render_prof.py` for in-situ kernel times
(k_env<2, 5, false, 0> = off, k_env<2, 5, false, 0, true> = on); standalone it prints HIP-event means per launch."""
import argparse
import json
import os
import sys

import torch as th

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from homophily_marl_amd import abi  # noqa: E402
from homophily_marl_amd.envs.native import NativeEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-env", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    N, n = a.n_env, 5
    kw = dict(map="default5", num_agents=n, n_env=N, view_size=7, episode_limit=100, rng_mode=abi.RNG_COUNTER, seed=3,
              extra_args=dict(disable_rotation_action=False, disable_fire_action=False))
    res = {}
    g = th.Generator(device="cuda").manual_seed(0)
    acts = th.randint(0, 9, (a.steps, N, n), generator=g, device="cuda", dtype=th.int32)
    for mode in ("off", "on"):
        env = NativeEnv("cleanup", device=0, **kw)
        if mode == "on":
            env.set_render(True)
        bufs = env.obs_buffers(abi.OBS_CODE)
        env.reset()
        for t in range(20):
            env.step_observe(acts[t], fmt=abi.OBS_CODE, out=bufs)
        th.cuda.synchronize()
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(a.steps):
            if t % 100 == 0:
                env.reset()
            env.step_observe(acts[t], fmt=abi.OBS_CODE, out=bufs)
        e1.record(); th.cuda.synchronize()
        res["step_obs_us_" + mode] = 1e3 * e0.elapsed_time(e1) / a.steps
        if mode == "on":
            ids = env.env_id_tensor()
            frames = th.empty(N, env.H, env.W, 3, dtype=th.uint8, device="cuda")
            for _ in range(10):
                env.render_into(ids, frames)
            th.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                env.render_into(ids, frames)
            e1.record(); th.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / a.steps
            res["render_us"] = us
            res["render_bytes"] = frames.numel()
            res["render_GBps"] = frames.numel() / us / 1e3
            assert env.poll_error() == 0
        env.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
