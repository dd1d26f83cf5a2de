"""Generate tests/golden/learner_options.npz FROM THE IMPORTED REFERENCE (runs only where the reference can be imported).

The loss flags of config/algs/homophily.yaml other than the shipped ones (double_q: False, consider_others_inc: True) against the
reference's own HomophilyMAC / HomophilyLearner.  No new rollouts: the batches and initial weights are those already committed in
learner_cleanup5.npz, learner_harvest5.npz and learner_cleanup5_w4.npz (oracle/gen_learner_golden.py), fed to a reference learner
built with the case's overrides.  The target net is made to differ from the live net by a closed-form rule that the tests apply as
well (at construction both are equal, and double_q: False would then give exactly the default numbers):

    target_k = f32(f64(live_k) + 0.05 sin(0.37 arange(numel_k) + k)),   k = index of the entry in agent.state_dict()

Per case: the nine logged values of two consecutive cal_loss_and_step calls and the parameter checksums after each step (sum, sum
of squares, first five elements).  The file holds numbers only (no weights); the meta JSON lists the cases, their base fixture and
their overrides (tests/learner_util.build(..., overrides=...) rebuilds them).  double_q: False runs the reference's branch with
the target shape its comment states (see max_keeps_action_axis).
    python tools/gen_learner_options_golden.py
"""
import contextlib
import io
import json
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch as th
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as RH  # noqa: E402
from oracle.gen_learner_golden import install_cluster_stub, merge  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "learner_options.npz")
LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")
PERTURB = "target_k = f32(f64(live_k) + 0.05 * sin(0.37 * arange(numel_k) + k)), k = state_dict index"
CASES = [
    ("cleanup5_dq1_oth0", "learner_cleanup5.npz", dict(double_q=True, consider_others_inc=False)),
    ("cleanup5_dq0_oth0", "learner_cleanup5.npz", dict(double_q=False, consider_others_inc=False)),
    ("cleanup5_dq1_oth1", "learner_cleanup5.npz", dict(double_q=True, consider_others_inc=True)),
    ("cleanup5_dq0_oth1", "learner_cleanup5.npz", dict(double_q=False, consider_others_inc=True)),
    ("harvest5_dq1_oth1", "learner_harvest5.npz", dict(double_q=True, consider_others_inc=True)),
    ("cleanup5w4_dq1_oth1", "learner_cleanup5_w4.npz", dict(double_q=True, consider_others_inc=True)),
]


def perturbed(sd):
    """The target-net rule above, on a state_dict (any framework's tensors -> numpy f32)."""
    out = {}
    for k, (name, v) in enumerate(sd.items()):
        x = np.asarray(v, dtype=np.float64)
        out[name] = (x + 0.05 * np.sin(0.37 * np.arange(x.size, dtype=np.float64) + k).reshape(x.shape)).astype(np.float32)
    return out


@contextlib.contextmanager
def max_keeps_action_axis():
    """The reference's double_q: False branch (homophily_learner.py:159-160) takes the plain max over the env actions without
    keepdim, so the target has shape [bs, t-1, n] where its comment and the double-Q branch have [bs, t-1, n, 1]; the following
    .sum(dim=-1) then adds the agents and the target does not broadcast against the rewards (the call raises).  While the loss is
    evaluated, a bare tensor.max(dim=-1) of a tensor without grad keeps the reduced axis: the env target becomes [bs, t-1, n, 1] as
    stated, and the inc target is unchanged (its .squeeze(-1) removes the kept axis again).  HomophilyLearner's tensor-op
    statement and k_td_sim_loss compute this shape."""
    orig = th.Tensor.max

    def max_(self, *a, **k):
        if not a and k == dict(dim=-1) and not self.requires_grad:
            return orig(self, dim=-1, keepdim=True)
        return orig(self, *a, **k)
    th.Tensor.max = max_
    try:
        yield
    finally:
        th.Tensor.max = orig


def build_case(base, overrides):
    """(args, batch, mac, learner) of the REFERENCE on the base fixture's batch and weights, the target net set apart by PERTURB."""
    z = np.load(os.path.join(GOLDEN, base))
    meta = json.loads(bytes(z["meta"]).decode())
    cfg = {}
    for f in ("default.yaml", "envs/%s.yaml" % meta["env"], "algs/homophily.yaml"):
        merge(cfg, yaml.safe_load(open(os.path.join(RH.REF_SRC, "config", f))))
    merge(cfg, dict(env_args=meta["env_args"], batch_size=4, buffer_size=8, use_cuda=False, use_tensorboard=False, save_model=False))
    merge(cfg, overrides)
    args = SimpleNamespace(**cfg)
    args.device = "cpu"
    logger = SimpleNamespace(log_stat=lambda *a, **k: None, console_logger=SimpleNamespace(info=lambda *a: None))
    with contextlib.redirect_stdout(io.StringIO()):
        from runners import REGISTRY as r_REGISTRY
        from controllers import REGISTRY as mac_REGISTRY
        from learners import REGISTRY as le_REGISTRY
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
    mac.agent.load_state_dict({k[2:]: th.as_tensor(z[k]) for k in z.files if k.startswith("w_")})
    learner = le_REGISTRY[args.learner](mac, batch.scheme, logger, args)   # deep-copies the controller: the target net
    tsd = learner.target_mac.agent.state_dict()
    with th.no_grad():
        for name, v in perturbed({k: v.numpy() for k, v in tsd.items()}).items():
            tsd[name].copy_(th.as_tensor(v))
    return args, batch, mac, learner


def run_case(base, overrides):
    args, batch, mac, learner = build_case(base, overrides)
    out = {}
    for step in range(2):
        with (contextlib.nullcontext() if args.double_q else max_keeps_action_axis()):
            logs = learner.cal_loss_and_step(batch)
        for k in LOG_KEYS:
            out["step%d_%s" % (step, k)] = np.float64(logs[k].item())
        sums, sqs, heads = [], [], []
        for k, v in mac.agent.state_dict().items():
            x = v.detach().double().reshape(-1)
            sums.append(x.sum().item()); sqs.append((x * x).sum().item()); heads.append(np.resize(x[:5].numpy(), 5))
        out["step%d_param_sum" % step] = np.array(sums); out["step%d_param_sq" % step] = np.array(sqs)
        out["step%d_param_head" % step] = np.stack(heads)
    return out


def main():
    RH.import_reference()
    install_cluster_stub()
    th.manual_seed(0)
    out, cases = {}, []
    for name, base, overrides in CASES:
        rec = run_case(base, overrides)
        for k, v in rec.items():
            out[name + "/" + k] = v
        cases.append(dict(name=name, base=base, overrides=overrides))
        print(name, {k: round(float(rec["step0_" + k]), 6) for k in ("loss_value_env", "loss_value_inc", "loss_sim")})
    out["meta"] = np.frombuffer(json.dumps(dict(cases=cases, target_perturbation=PERTURB)).encode(), np.uint8)
    save_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: a rerun reproduces the file byte for byte."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main()
