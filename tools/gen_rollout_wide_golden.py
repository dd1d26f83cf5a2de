"""Generate tests/golden/rollout_wide_cleanup10.npz FROM THE IMPORTED REFERENCE (runs only where the reference can be imported).

The reference controller with ALL SEVEN _build_inputs flags at Cleanup-10: 155 input columns (164 for the inc head), the widest row
the rollout can meet.  B = 2 episodes of 6 steps are rolled out by the reference's own runner; then every parameter of the agent is
re-drawn from a fixed seed (draw_weights: numpy's RandomState stream, which is frozen across numpy versions), so that the fixture
holds no weights at all -- ten agents' networks are 2.8 MB -- only the seed and a checksum per tensor.  Recorded: the batch and the
reference's q_env / q_inc of mac.forward(batch, t) for t = 0 .. 5 from fresh hidden states.  Numbers only.
    python tools/gen_rollout_wide_golden.py
"""
import contextlib
import io
import json
import os
import random
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "rollout_wide_cleanup10.npz")
OVERRIDES = dict(obs_others_last_action=True, obs_distance=True)
ENV_ARGS = dict(num_agents=10, map="default10", episode_limit=6)
STEPS, SEED, B = 6, 20241, 2


def draw_weights(shapes, seed=SEED):
    """{name: f32 array} for {name: shape} in the given order: uniform in +-1 / sqrt(fan_in) (the reference's init range), fan_in =
    the rows of a per-agent matrix [1, n, in, out], 64 for its bias rows [1, n, 1, out], the receptive field of the conv / Linear."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
        if len(shape) == 4 and not name.startswith("conv_to_fc"):
            fan = shape[2] if shape[2] > 1 else 64
        elif len(shape) >= 2:
            fan = int(np.prod(shape[1:]))
        else:
            fan = 64
        b = 1.0 / np.sqrt(fan)
        out[name] = rs.uniform(-b, b, size=shape).astype(np.float32)
    return out


def checksums(weights):
    return np.array([[float(v.astype(np.float64).sum()), float((v.astype(np.float64) ** 2).sum())] for v in weights.values()])


def main():
    import torch as th
    import yaml
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from oracle import ref_harness as RH
    from oracle.gen_learner_golden import install_cluster_stub, merge
    from gen_learner_options_golden import save_npz
    RH.import_reference()
    install_cluster_stub()
    cfg = {}
    for f in ("default.yaml", "envs/cleanup.yaml", "algs/homophily.yaml"):
        merge(cfg, yaml.safe_load(open(os.path.join(RH.REF_SRC, "config", f))))
    merge(cfg, dict(env_args=ENV_ARGS, batch_size=B, buffer_size=B, use_cuda=False, use_tensorboard=False, save_model=False))
    merge(cfg, OVERRIDES)
    np.random.seed(SEED); random.seed(SEED); th.manual_seed(SEED)
    args = SimpleNamespace(**cfg)
    args.device = "cpu"
    logger = SimpleNamespace(log_stat=lambda *a, **k: None, console_logger=SimpleNamespace(info=lambda *a: None))
    with contextlib.redirect_stdout(io.StringIO()):
        from runners import REGISTRY as r_REGISTRY
        from controllers import REGISTRY as mac_REGISTRY
        from components.episode_buffer import ReplayBuffer
        from components.transforms import OneHot
        runner = r_REGISTRY[args.runner](args=args, logger=logger)
    env_info = runner.get_env_info()
    args.n_agents, args.n_actions = env_info["n_agents"], env_info["n_actions"]
    args.state_shape, args.obs_shape = env_info["state_shape"], env_info["obs_shape"]
    args.state_dims, args.obs_dims = env_info["state_dims"], env_info["obs_dims"]
    n = args.n_agents
    scheme = {
        "state": {"vshape": env_info["state_shape"]}, "obs": {"vshape": env_info["obs_shape"], "group": "agents"},
        "actions": {"vshape": (1,), "group": "agents", "dtype": th.long},
        "avail_actions": {"vshape": (env_info["n_actions"],), "group": "agents", "dtype": th.int},
        "reward": {"vshape": (n,)}, "terminated": {"vshape": (1,), "dtype": th.uint8},
        "clean_num": {"vshape": (n,)}, "apple_den": {"vshape": (n,)},
        "agent_pos": {"vshape": (n, 2)}, "agent_orientation": {"vshape": (n, 2)},
        "actions_inc": {"vshape": (n, 1), "group": "agents", "dtype": th.long},
    }
    groups = {"agents": n}
    preprocess = {"actions": ("actions_onehot", [OneHot(out_dim=args.n_actions)])}
    buffer = ReplayBuffer(scheme, groups, args.buffer_size, env_info["episode_limit"] + 1, preprocess=preprocess, device="cpu")
    mac = mac_REGISTRY[args.mac](buffer.scheme, groups, args)
    runner.setup(scheme=scheme, groups=groups, preprocess=preprocess, mac=mac)
    for _ in range(B):
        buffer.insert_episode_batch(runner.run(test_mode=False))
    batch = buffer[:B]
    batch = batch[:, :batch.max_t_filled()]
    out = {}
    for k in ("obs", "actions", "actions_inc", "reward", "terminated", "clean_num", "apple_den", "agent_pos", "agent_orientation",
              "avail_actions", "filled"):
        v = batch[k].numpy()
        if k == "obs":
            v8 = np.round(v * 256)
            assert (v8 / 256 == v).all()
            v = v8.astype(np.uint8)
        out["batch_" + k] = v
    sd = mac.agent.state_dict()
    weights = draw_weights({k: v.shape for k, v in sd.items()})
    for k, v in weights.items():
        sd[k].copy_(th.as_tensor(v))
    assert sd["fc1_env_w"].shape[2] == 155 and sd["fc1_inc_w"].shape[2] == 164
    mac.init_hidden(B)
    q_env, q_inc = [], []
    with th.no_grad():
        for t in range(STEPS):
            qe, qi, _ = mac.forward(batch, t)
            q_env.append(qe.reshape(B, n, -1).numpy().copy()); q_inc.append(qi.reshape(B, n, n, -1).numpy().copy())
    out.update(q_env=np.stack(q_env, 1), q_inc=np.stack(q_inc, 1), weight_names=np.array(list(weights)), weight_sums=checksums(weights))
    out["weight_shapes"] = np.frombuffer(json.dumps({k: list(v.shape) for k, v in weights.items()}).encode(), np.uint8)
    out["meta"] = np.frombuffer(json.dumps(dict(env="cleanup", env_args=cfg["env_args"], overrides=OVERRIDES, steps=STEPS, seed=SEED,
                                                input_shape=int(sd["fc1_env_w"].shape[2]))).encode(), np.uint8)
    save_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; |q_env| up to %.3f, |q_inc| up to %.3f" % (np.abs(out["q_env"]).max(), np.abs(out["q_inc"]).max()))


if __name__ == "__main__":
    main()
