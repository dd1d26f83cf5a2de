"""Generate tests/golden/rollout_others_cleanup5.npz FROM THE IMPORTED REFERENCE (runs only where the reference can be imported).

The reference controller with obs_others_last_action: True on the batch and weights of learner_cleanup5.npz.  That fixture's fc1
layers are 50 / 59 rows wide; with the flag they are 95 / 104, so fc1_env_w / fc1_inc_w are re-drawn at the wider shape from a fixed
seed (uniform in +-1 / sqrt(fan_in), the reference's own init range) and stored.  Recorded: the reference's q_env / q_inc of
mac.forward(batch, t) for t = 0 .. STEPS - 1 from fresh hidden states.  Numbers only.
    python tools/gen_rollout_others_golden.py
"""
import contextlib
import io
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch as th
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import ref_harness as RH  # noqa: E402
from oracle.gen_learner_golden import install_cluster_stub, merge  # noqa: E402
from gen_learner_options_golden import save_npz  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = "learner_cleanup5.npz"
OUT = os.path.join(GOLDEN, "rollout_others_cleanup5.npz")
OVERRIDES = dict(obs_others_last_action=True)
STEPS, SEED = 6, 20240


def main():
    RH.import_reference()
    install_cluster_stub()
    z = np.load(os.path.join(GOLDEN, BASE))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = {}
    for f in ("default.yaml", "envs/%s.yaml" % meta["env"], "algs/homophily.yaml"):
        merge(cfg, yaml.safe_load(open(os.path.join(RH.REF_SRC, "config", f))))
    merge(cfg, dict(env_args=meta["env_args"], batch_size=4, buffer_size=8, use_cuda=False, use_tensorboard=False, save_model=False))
    merge(cfg, OVERRIDES)
    args = SimpleNamespace(**cfg)
    args.device = "cpu"
    logger = SimpleNamespace(log_stat=lambda *a, **k: None, console_logger=SimpleNamespace(info=lambda *a: None))
    with contextlib.redirect_stdout(io.StringIO()):
        from runners import REGISTRY as r_REGISTRY
        from controllers import REGISTRY as mac_REGISTRY
        from components.episode_buffer import EpisodeBatch
        from components.transforms import OneHot
        runner = r_REGISTRY[args.runner](args=args, logger=logger)            # the env's shapes only: no episode is run
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
    B, T1 = z["batch_obs"].shape[:2]
    batch = EpisodeBatch(scheme, groups, B, T1, preprocess=preprocess, device="cpu")
    data = {k: th.as_tensor(z["batch_" + k]) for k in ("actions", "actions_inc", "reward", "terminated", "clean_num", "apple_den",
                                                        "agent_pos", "agent_orientation", "avail_actions")}
    data["obs"] = th.as_tensor(z["batch_obs"]).float() / 256
    batch.update(data)
    batch.data.transition_data["filled"].copy_(th.as_tensor(z["batch_filled"]))
    mac = mac_REGISTRY[args.mac](batch.scheme, groups, args)
    sd = mac.agent.state_dict()
    g = th.Generator().manual_seed(SEED)
    wide = {}
    for name in sd:
        src = th.as_tensor(z["w_" + name])
        if tuple(src.shape) == tuple(sd[name].shape):
            sd[name].copy_(src)
        else:
            assert name in ("fc1_env_w", "fc1_inc_w"), name
            bound = 1.0 / np.sqrt(sd[name].shape[2])
            wide[name] = ((th.rand(sd[name].shape, generator=g) * 2 - 1) * bound).float()
            sd[name].copy_(wide[name])
    assert sorted(wide) == ["fc1_env_w", "fc1_inc_w"]
    mac.init_hidden(B)
    q_env, q_inc = [], []
    with th.no_grad():
        for t in range(STEPS):
            qe, qi, _ = mac.forward(batch, t)
            q_env.append(qe.reshape(B, n, -1).numpy().copy()); q_inc.append(qi.reshape(B, n, n, -1).numpy().copy())
    out = dict(fc1_env_w=wide["fc1_env_w"].numpy(), fc1_inc_w=wide["fc1_inc_w"].numpy(),
               q_env=np.stack(q_env, 1), q_inc=np.stack(q_inc, 1))
    out["meta"] = np.frombuffer(json.dumps(dict(base=BASE, overrides=OVERRIDES, steps=STEPS, seed=SEED,
                                                input_shape=int(sd["fc1_env_w"].shape[2]))).encode(), np.uint8)
    save_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; |q_env| up to %.3f" % np.abs(out["q_env"]).max())


if __name__ == "__main__":
    main()
