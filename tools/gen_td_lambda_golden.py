"""Generate tests/golden/learner_td_lambda.npz FROM THE IMPORTED REFERENCE (runs only where the reference can be imported).

The learner's td_lambda option (TD(lambda) targets for both heads) is pinned to the reference's own recursion, utils/rl_utils.py:4-14
build_td_lambda_targets (PyMARL's; the reference's homophily learner never calls it).  Two groups, numbers only:

(A) the recursion: seeded synthetic inputs, B = 3, n = 3, every T of A_T x every (gamma, lambda) of A_GAMMAS x A_LAMBDAS.  Episode 0 is
    never terminated and fully filled, episode 1 is terminated at T // 3 and unfilled after, episode 2 is terminated at T - 1; the mask
    is the learner's (filled, times 1 - terminated of the step before).  Recorded: the inputs (per T) and the function's output.
        A/T<T>/{rewards [3,T,3], terminated [3,T,1], mask [3,T,1], target_qs [3,T+1,3]}      A/T<T>/g<gi>_l<li>/ret [3,T,3]

(B) the learner: the batches and weights of learner_cleanup5.npz / learner_harvest5.npz on the reference's controller, target net set
    apart by the PERTURB rule of tools/gen_learner_options_golden.py, under the four (double_q, consider_others_inc) sets.  q / target q
    come from the reference controller; the per-row bootstrap values, rewards and chosen values are formed below in a few lines, and
    at lambda = 0 they must reproduce the loss_value_env / loss_value_inc the reference's cal_loss_and_step returns (asserted here,
    |d| < 1e-7) before they are fed to build_td_lambda_targets.  Recorded for every lambda of B_LAMBDAS:
        B/<case>/l<li>/{ret_env, ret_inc [B,T,n], loss_value_env, loss_value_inc}
    python tools/gen_td_lambda_golden.py
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
from gen_learner_options_golden import GOLDEN, PERTURB, build_case, max_keeps_action_axis, save_npz  # noqa: E402

OUT = os.path.join(GOLDEN, "learner_td_lambda.npz")
A_T = [1, 2, 12, 63, 64, 65, 255, 256, 257, 513]
A_GAMMAS = [0.95, 0.995]
A_LAMBDAS = [2.0 ** -100, 0.5, 0.8, 1.0]
B_LAMBDAS = [0.5, 0.8, 1.0]
B_CASES = [("%s_dq%d_oth%d" % (base[8:-4], dq, oth), base, dict(double_q=bool(dq), consider_others_inc=bool(oth)))
           for base in ("learner_cleanup5.npz", "learner_harvest5.npz") for dq, oth in ((1, 0), (0, 0), (1, 1), (0, 1))]
NEG = -9999999


def group_a(fn):
    out = {}
    rng = np.random.default_rng(20240607)
    for T in A_T:
        B, n = 3, 3
        term = np.zeros((B, T, 1), np.float32)
        filled = np.ones((B, T, 1), np.float32)
        term[1, T // 3] = 1
        filled[1, T // 3 + 1:] = 0
        term[2, T - 1] = 1
        mask = filled.copy()
        mask[:, 1:] *= 1 - term[:, :-1]
        rewards = (rng.standard_normal((B, T, n)) * (rng.random((B, T, n)) < 0.4) / 8).astype(np.float32)
        target_qs = rng.standard_normal((B, T + 1, n)).astype(np.float32)
        pre = "A/T%d/" % T
        out[pre + "rewards"], out[pre + "terminated"], out[pre + "mask"], out[pre + "target_qs"] = rewards, term, mask, target_qs
        for gi, gamma in enumerate(A_GAMMAS):
            for li, lam in enumerate(A_LAMBDAS):
                ret = fn(th.as_tensor(rewards), th.as_tensor(term), th.as_tensor(mask), th.as_tensor(target_qs), n, gamma, lam)
                assert ret.shape == (B, T, n) and ret.dtype == th.float32
                out[pre + "g%d_l%d/ret" % (gi, li)] = ret.numpy().copy()
    return out


def rows_of(args, batch, q_env, q_inc, tq_env, tq_inc):
    """mask, live, r_env, r_inc, v_env, v_inc, chosen_env, chosen_inc [B, T, n] (mask / live [B, T, 1]) of the one-step loss: the
    quantities homophily_learner.py:94-172 forms, restated."""
    n, T1 = args.n_agents, batch.max_seq_length
    off = 1 - th.eye(n)
    acts_inc = batch["actions_inc"].squeeze(-1)                           # [B, T1, giver, receiver]
    sent = acts_inc * off.long()
    rew = batch["reward"][:, :-1] / args.reward_scale
    give = (sent[:, :-1] != 0).sum(3).float()
    recv = th.stack([th.zeros_like(sent[:, :, 0]).float(), (sent == 1).sum(2).float(), (sent == 2).sum(2).float()], -1)   # [B, T1, receiver, 3]
    recv[..., 0] = n - 1 - recv[..., 1] - recv[..., 2]
    rv = (recv[..., 1] - recv[..., 2])[:, :-1]
    r_env = (rew + rv * args.incentive_ratio * args.incentive) / T1
    r_inc = (rew - give * args.incentive_cost * args.incentive) / T1
    term = batch["terminated"][:, :-1].float()
    mask = batch["filled"][:, :-1].float()
    mask[:, 1:] = mask[:, 1:] * (1 - term[:, :-1])
    avail = batch["avail_actions"]
    tqe = tq_env[:, 1:].masked_fill(avail[:, 1:] == 0, NEG)
    pick_env = q_env.masked_fill(avail == 0, NEG)[:, 1:] if args.double_q else tqe
    v_env = tqe.gather(-1, pick_env.argmax(-1, keepdim=True)).squeeze(-1)
    tqi = tq_inc[:, 1:]
    v_ij = tqi.gather(-1, (q_inc[:, 1:] if args.double_q else tqi).argmax(-1, keepdim=True)).squeeze(-1)     # [B, T, i, j]
    chosen_ij = q_inc[:, :-1].gather(-1, acts_inc[:, :-1].unsqueeze(-1)).squeeze(-1)
    if args.consider_others_inc:
        weighed = (tqi * recv[:, 1:].unsqueeze(2)).sum(-1)                # receiver j's counts at t + 1, over the giver axis
        taken = tqi.gather(-1, acts_inc[:, 1:].unsqueeze(-1)).squeeze(-1)
        v_ij = (v_ij + weighed - taken) / (n - 1)
        chosen_ij = (q_inc[:, :-1] * recv[:, :-1].unsqueeze(2)).sum(-1) / (n - 1)
    chosen_env = q_env[:, :-1].gather(-1, batch["actions"][:, :-1]).squeeze(-1)
    return dict(mask=mask, live=1 - term, term=term, r_env=r_env, r_inc=r_inc, v_env=v_env, v_inc=(v_ij * off).sum(-1),
                chosen_env=chosen_env, chosen_inc=(chosen_ij * off).sum(-1))


def group_b(fn):
    out = {}
    for name, base, overrides in B_CASES:
        args, batch, mac, learner = build_case(base, overrides)
        with th.no_grad():
            qs = []
            for m in (learner.mac, learner.target_mac):
                m.init_hidden(batch.batch_size)
                steps = [m.forward(batch, t=t)[:2] for t in range(batch.max_seq_length)]
                qs += [th.stack([s[0] for s in steps], 1), th.stack([s[1] for s in steps], 1)]
            p = rows_of(args, batch, *qs)
        with (contextlib.nullcontext() if args.double_q else max_keeps_action_axis()):
            logs = learner.cal_loss_and_step(batch)                      # the loss of the weights the q-values above came from
        den = p["mask"].expand_as(p["r_env"]).sum()
        loss = lambda chosen, target: float((((chosen - target) * p["mask"]) ** 2).sum() / den)
        for h, gamma in (("env", args.gamma_env), ("inc", args.gamma_inc)):
            one = loss(p["chosen_" + h], p["r_" + h] + gamma * p["live"] * p["v_" + h])
            ref = float(logs["loss_value_" + h])
            assert abs(one - ref) < 1e-7, (name, h, one, ref)
        for li, lam in enumerate(B_LAMBDAS):
            for h, gamma in (("env", args.gamma_env), ("inc", args.gamma_inc)):
                v = th.cat([th.zeros_like(p["v_" + h][:, :1]), p["v_" + h]], 1)       # slot t + 1 = the bootstrap value of row t
                ret = fn(p["r_" + h], p["term"], p["mask"], v, args.n_agents, gamma, lam)
                out["B/%s/l%d/ret_%s" % (name, li, h)] = ret.numpy().copy()
                out["B/%s/l%d/loss_value_%s" % (name, li, h)] = np.float64(loss(p["chosen_" + h], ret))
        print(name, {k.split("/", 2)[2]: round(float(v), 6) for k, v in out.items() if k.startswith("B/%s/" % name) and "loss" in k})
    return out


def main():
    RH.import_reference()
    install_cluster_stub()
    from utils.rl_utils import build_td_lambda_targets as fn
    th.manual_seed(0)
    out = group_a(fn)
    out.update(group_b(fn))
    meta = dict(a_T=A_T, a_gammas=A_GAMMAS, a_lambdas=A_LAMBDAS, b_lambdas=B_LAMBDAS, target_perturbation=PERTURB,
                b_cases=[dict(name=nm, base=base, overrides=ov) for nm, base, ov in B_CASES],
                source="utils/rl_utils.py:4-14 build_td_lambda_targets")
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    save_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
