"""A float64 numpy statement of the loss kernel's rows and of the TD(lambda) recursion (a helper, no test in it).

host_rows restates what ssd_td_sim_loss forms per (episode, t, agent) from the raw arrays -- TD mask, rewards of both heads, bootstrap
values, chosen values -- under every (double_q, consider_others_inc) set; serial_returns is the recursion of include/ssd_hip.h
(td_lambda) as a plain backward loop; host_loss puts them together with the similarity gradient into what the kernel writes.  The CPU
suite holds host_rows + serial_returns to the numbers the reference recorded (tests/test_td_lambda_host.py, group B of
tests/golden/learner_td_lambda.npz); the GPU suite then holds the kernel to them on random arrays."""
import json
import os

import numpy as np

from tests.learner_util import GOLDEN

NEG = -9999999.0


def load_golden():
    z = np.load(os.path.join(GOLDEN, "learner_td_lambda.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def received(ainc):
    """[..., receiver, 3]: how many OTHER agents gave the receiver (nothing, +, -) at every slot"""
    n = ainc.shape[-1]
    off = ~np.eye(n, dtype=bool)
    p, m = ((ainc == 1) & off).sum(-2), ((ainc == 2) & off).sum(-2)
    return np.stack([n - 1 - p - m, p, m], -1).astype(np.float64)


def host_rows(q_env, q_inc, tq_env, tq_inc, avail, actions, ainc, reward, term, filled, double_q, others, reward_scale, incentive_ratio,
              incentive_cost, incentive, seq_len):
    """All arrays over the T + 1 slots (q_env [B, T1, n, A], q_inc [B, T1, n, n, 3], actions [B, T1, n], ainc [B, T1, giver, receiver],
    term / filled [B, T1]); returns f64 [B, T, n] arrays (mask, live: [B, T])."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    q_env, q_inc, tq_env, tq_inc, reward = f(q_env), f(q_inc), f(tq_env), f(tq_inc), f(reward)
    B, T1, n, A = q_env.shape
    T = T1 - 1
    off = ~np.eye(n, dtype=bool)
    termf = f(term)
    mask = f(filled)[:, :T].copy()
    mask[:, 1:] *= 1 - termf[:, :T - 1]
    r = reward[:, :T] / reward_scale
    recv = received(ainc)
    give = ((ainc != 0) & off).sum(3)[:, :T]
    rv = (recv[..., 1] - recv[..., 2])[:, :T]
    r_env = (r + rv * incentive_ratio * incentive) / seq_len
    r_inc = (r - give * incentive_cost * incentive) / seq_len
    take = lambda x, idx: np.take_along_axis(x, idx[..., None], -1)[..., 0]
    ok = np.asarray(avail)[:, 1:] != 0
    tqe = np.where(ok, tq_env[:, 1:], NEG)
    v_env = take(tqe, (np.where(ok, q_env[:, 1:], NEG) if double_q else tqe).argmax(-1))
    tqi = tq_inc[:, 1:]
    v_ij = take(tqi, (q_inc[:, 1:] if double_q else tqi).argmax(-1))                       # [B, T, i, j]
    chosen_ij = take(q_inc[:, :T], np.asarray(ainc)[:, :T])
    if others:
        v_ij = (v_ij + (tqi * recv[:, 1:, None]).sum(-1) - take(tqi, np.asarray(ainc)[:, 1:])) / (n - 1)
        chosen_ij = (q_inc[:, :T] * recv[:, :T, None]).sum(-1) / (n - 1)
    return dict(mask=mask, live=1 - termf[:, :T], term=termf[:, :T], r_env=r_env, r_inc=r_inc, v_env=v_env, v_inc=(v_ij * off).sum(-1),
                chosen_env=take(q_env[:, :T], np.asarray(actions)[:, :T]), chosen_inc=(chosen_ij * off).sum(-1),
                q_inc_taken=take(q_inc[:, :T], np.asarray(ainc)[:, :T]).sum(-1), recv=recv)


def serial_returns(r, term, mask, live, v, gamma, lam):
    """G [B, T, n]: r, v [B, T, n] (v[:, t] = the bootstrap value of row t), term / mask / live [B, T]; one step after the other from t = T - 1 down."""
    B, T, n = r.shape
    g = v[:, T - 1] * (1 - term.sum(1))[:, None]
    out = np.empty((B, T, n))
    for t in range(T - 1, -1, -1):
        g = lam * gamma * g + mask[:, t, None] * (r[:, t] + (1 - lam) * gamma * live[:, t, None] * v[:, t])
        out[:, t] = g
    return out


def sim_gradient(q_inc, ainc, reward, clean_num, reward_scale, horizon, threshold):
    """d (sum of the similarity terms) / d q_inc[:, :T] (f64 [B, T, n, n, 3]) and the terms' per-row sums [B, T, n]
    (homophily_learner.py:184-217 with the exact-value clustering rule)."""
    q = np.asarray(q_inc, dtype=np.float64)
    B, T1, n = q.shape[:3]
    T = T1 - 1
    cn, rw = np.zeros((B, T, n)), np.zeros((B, T, n))
    for t in range(T):
        lo = max(0, t - horizon + 1)
        cn[:, t] = (np.asarray(clean_num)[:, lo:t + 1] > 0).sum(1) > 0
        rw[:, t] = (np.asarray(reward, dtype=np.float64)[:, lo:t + 1] / reward_scale).sum(1) > 0
    cl, idle = 2 * rw + cn, cn + rw
    e = np.exp(q[:, :T] - q[:, :T].max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    grad, terms = np.zeros_like(p), np.zeros((B, T, n))
    for i in range(n):
        for k in range(n):
            for j in range(n):
                if i == k or i == j or k == j:
                    continue
                sm = (cl[..., i] == cl[..., k]) * idle[..., i] * idle[..., k]
                c = np.asarray(ainc)[:, :T, k, j]
                hot = np.eye(3)[c]
                nl = -np.log((p[:, :, i, j] * hot).sum(-1))
                terms[..., i] += np.maximum(nl, threshold) * sm
                grad[:, :, i, j] += (sm * (nl >= threshold))[..., None] * (p[:, :, i, j] - hot)
    return grad, terms


def host_loss(arr, cfg, lam, dens):
    """What mode 1 writes with td_lambda = lam: G_env, G_inc, the two squared-error columns [B, T, n], dq_env [B, T1, n, A], dq_inc
    [B, T1, n, n, 3].  arr: the raw arrays by the names of ssd_td_loss_args; cfg: the struct's scalars."""
    p = host_rows(arr["q_env"], arr["q_inc"], arr["tq_env"], arr["tq_inc"], arr["avail"], arr["actions"], arr["actions_inc"], arr["reward"],
                  arr["terminated"], arr["filled"], cfg["double_q"], cfg["consider_others_inc"], cfg["reward_scale"], cfg["incentive_ratio"],
                  cfg["incentive_cost"], cfg["incentive"], cfg["seq_len"])
    B, T1, n, A = arr["q_env"].shape
    T = T1 - 1
    out = {}
    dq_env, dq_inc = np.zeros((B, T1, n, A)), np.zeros((B, T1, n, n, 3))
    sim_g, _ = sim_gradient(arr["q_inc"], arr["actions_inc"], arr["reward"], arr["clean_num"], cfg["reward_scale"], cfg["sim_horizon"], cfg["sim_threshold"])
    dq_inc[:, :T] = cfg["sim_loss_weight"] / (1 + dens[1]) * sim_g
    off = ~np.eye(n, dtype=bool)
    for h, gamma in (("env", cfg["gamma_env"]), ("inc", cfg["gamma_inc"])):
        G = serial_returns(p["r_" + h], p["term"], p["mask"], p["live"], p["v_" + h], gamma, lam)
        td = p["chosen_" + h] - G
        out["G_" + h], out["sq_" + h] = G, (td * p["mask"][..., None]) ** 2
        g = 2 * td * p["mask"][..., None] ** 2 / dens[0]
        if h == "env":
            np.put_along_axis(dq_env[:, :T], np.asarray(arr["actions"])[:, :T, :, None], g[..., None], -1)
        elif cfg["consider_others_inc"]:
            dq_inc[:, :T] += g[..., None, None] * p["recv"][:, :T, None] / (n - 1) * off[..., None]
        else:
            dq_inc[:, :T] += g[..., None, None] * np.eye(3)[np.asarray(arr["actions_inc"])[:, :T]] * off[..., None]
    out["dq_env"], out["dq_inc"] = dq_env, dq_inc
    return out
