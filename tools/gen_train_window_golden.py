"""Generate tests/golden/learner_train_window.npz FROM THE IMPORTED REFERENCE (runs only where the reference can be imported).

Training on sampled time windows with burn-in (config keys train_window / train_burn_in) is pinned to the reference's own
cal_loss_and_step run on a time slice of a batch: window e holds slots [t0[e], t0[e] + L] of episode e, and its first K_e rows
(K_e = K if t0[e] > 0, 0 if t0[e] == 0) have filled = 0.  The reference divides the rewards by the slice's slot count, so these are
the numbers of train_window_norm: "window".

The window batches are assembled per episode into a FRESH reference EpisodeBatch (a reference slice shares storage with its batch:
zeroing `filled` on a slice would corrupt the source).  Batches and initial weights are those of learner_cleanup5.npz and
learner_harvest5.npz (B = 4, 13 slots, n = 5), the target net set apart by the PERTURB rule of tools/gen_learner_options_golden.py.
Per case, in the format of learner_options.npz: the nine logged values of two consecutive cal_loss_and_step calls and the parameter
checksums after each.  Numbers only; `meta` lists the cases (tests/test_train_window_host.py rebuilds the windows with
ReplayBuffer.gather_windows).
    python tools/gen_train_window_golden.py
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import ref_harness as RH  # noqa: E402
from oracle.gen_learner_golden import install_cluster_stub  # noqa: E402
from gen_learner_options_golden import GOLDEN, LOG_KEYS, PERTURB, build_case, max_keeps_action_axis, save_npz  # noqa: E402

OUT = os.path.join(GOLDEN, "learner_train_window.npz")
BASES = ("learner_cleanup5.npz", "learner_harvest5.npz")
# (tag, L, K, t0 per episode, extra overrides)
WINDOWS = [("L6_K2", 6, 2, [0, 3, 6, 2], {}),
           ("L3_K1", 3, 1, [9, 0, 5, 9], {}),
           ("L11_K3", 11, 3, [1, 0, 1, 0], {}),
           ("L6_K2_h3", 6, 2, [0, 3, 6, 2], dict(sim_horizon=3))]
FLAGS = [("dq1_oth0", dict(double_q=True, consider_others_inc=False)), ("dq0_oth1", dict(double_q=False, consider_others_inc=True))]


def window_batch(batch, L, K, t0):
    """The reference's EpisodeBatch of L + 1 slots with window e = slots [t0[e], t0[e] + L] of episode e, assembled per episode."""
    from components.episode_buffer import EpisodeBatch
    W = L + 1
    derived = {"filled"} | {new for new, _ in batch.preprocess.values()}
    scheme = {k: v for k, v in batch.scheme.items() if k not in derived}
    win = EpisodeBatch(scheme, batch.groups, batch.batch_size, W, preprocess=batch.preprocess, device="cpu")
    for e, s in enumerate(t0):
        assert 0 <= s and s + W <= batch.max_seq_length
        win.update({k: batch[k][e:e + 1, s:s + W].clone() for k in scheme}, bs=e, ts=slice(0, W))
        filled = batch["filled"][e, s:s + W].clone()
        filled[:K if s > 0 else 0] = 0
        win.data.transition_data["filled"][e] = filled
    return win


def record(args, win, mac, learner):
    out = {}
    for step in range(2):
        with (contextlib.nullcontext() if args.double_q else max_keeps_action_axis()):
            logs = learner.cal_loss_and_step(win)
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
    for base in BASES:
        for tag, L, K, t0, extra in WINDOWS:
            for ftag, flags in FLAGS:
                name = "%s_%s_%s" % (base[8:-4], tag, ftag)
                overrides = dict(flags, **extra)
                args, batch, mac, learner = build_case(base, overrides)
                assert batch.batch_size == len(t0) and batch.max_seq_length == 13
                win = window_batch(batch, L, K, t0)
                rec = record(args, win, mac, learner)
                for k, v in rec.items():
                    out[name + "/" + k] = v
                cases.append(dict(name=name, base=base, window=L, burn_in=K, t0=t0, k_e=[K if s > 0 else 0 for s in t0], overrides=overrides))
                print(name, {k: round(float(rec["step0_" + k]), 6) for k in ("loss_value_env", "loss_value_inc", "loss_sim")})
    out["meta"] = np.frombuffer(json.dumps(dict(cases=cases, target_perturbation=PERTURB, norm="window")).encode(), np.uint8)
    save_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
