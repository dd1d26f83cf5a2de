"""End-to-end replay: a short Cleanup-5 training run (8 train steps per rollout) that saves a checkpoint, then run_sequential with
that checkpoint and save_replay=True, env_args.is_replay=True (the reference README's "Watching replays").  Prints the replay
directory and the size of each GIF.  usage: python tools/replay_demo.py OUT_DIR [--rollouts R] [--n-env N]"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from homophily_marl_amd.run import load_config, run_sequential  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--rollouts", type=int, default=30)
    ap.add_argument("--n-env", type=int, default=1024)
    a = ap.parse_args()
    T, N = 100, a.n_env
    common = dict(runner="hip_graph", batch_size_run=N, batch_size=16, buffer_size=N, obs_storage="code", buffer_cpu_only=False,
                  store_state=False, local_results_path=os.path.abspath(a.out), use_cuda=True)
    env = dict(num_agents=5, map="default5", episode_limit=T, seed=1)
    train = load_config("cleanup", overrides=dict(common, train_steps_per_rollout=8, t_max=a.rollouts * N * T, save_model=True,
                                                  save_model_interval=a.rollouts * N * T // 2, test_interval=10 ** 12, env_args=env))
    run_sequential(train)
    ckpt = sorted(glob.glob(os.path.join(a.out, "models", "*")))[-1]
    print("checkpoint", ckpt, sorted(os.listdir(ckpt)), flush=True)
    rep = load_config("cleanup", overrides=dict(common, checkpoint_path=ckpt, save_replay=True, test_nepisode=1,
                                                env_args=dict(env, is_replay=True, replay_envs=[0, N - 1])))
    ctx = run_sequential(rep)
    print("replay dir", ctx.replay_dir)
    for g in sorted(glob.glob(os.path.join(ctx.replay_dir, "*", "*", "replay.gif"))):
        print(g, os.path.getsize(g), "bytes", len(glob.glob(os.path.join(os.path.dirname(g), "*.png"))), "png")


if __name__ == "__main__":
    main()
