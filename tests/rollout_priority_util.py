"""Helpers of the initial-priority tests (config key per_initial_priority: "rollout"; ssd_rollout_priority): a helper, no test in it.

The priority an episode enters the table with, restated in numpy float64 from the definition (include/ssd_hip.h, and the comment
block of k_td_sim_loss) -- nothing here calls the package.  Over whole-episode arrays, T = slots - 1, rows (t < T, agent i):

    off[i, j] = (i != j);   m = actions_inc * off                      (actions_inc[.., giver, receiver])
    give[t, i] = #{j: m[t, i, j] != 0};   rp[t, i] = #{j: m[t, j, i] == 1};   rn[t, i] = #{j: m[t, j, i] == 2}
    r = reward[t, i] / reward_scale
    r_env = (r + (rp - rn) incentive_ratio incentive) / seq_len;        r_inc = (r - give incentive_cost incentive) / seq_len
    mask[t] = filled[t] (t ? 1 - terminated[t - 1] : 1);                live[t] = 1 - terminated[t]
    td_env = Q_env[t, i, a[t, i]] - (r_env + gamma_env live max_{k available} Q_env[t + 1, i, k])
    td_inc = sum_{j != i} Q_inc[t, i, j, a_inc[t, i, j]] - (r_inc + gamma_inc live sum_{j != i} max_c Q_inc[t + 1, i, j, c])
    d = sqrt((td_env mask)^2 + (td_inc mask)^2)
    p = eta max d + (1 - eta) sum d / max(1, sum mask) + eps            (max and sums over the T n rows)
    q_init = clamp(round(p^alpha ONE), 1, QMAX)
"""
from types import SimpleNamespace

import numpy as np

from tests.priority_util import ONE, QMAX

NEG = -9999999.0                 # the masked_fill value of an unavailable action

CONSTANTS = ("gamma_env", "gamma_inc", "reward_scale", "incentive_ratio", "incentive_cost", "incentive", "seq_len")


def td_rows(q_env, q_inc, actions, actions_inc, reward, terminated, filled, avail_bits, c):
    """q_env [N, T + 1, n, A], q_inc [N, T + 1, n, n, 3], actions [N, T + 1, n], actions_inc [N, T + 1, n, n], reward [N, T + 1, n],
    terminated [N, T + 1], filled [N, T + 1] or None (all ones); c: a mapping of CONSTANTS.
    Returns float64 (td_env, td_inc, mask, bound) of shape [N, T, n]; bound[h] = |chosen_h| + |r_h| + gamma_h |V_h| per row (the
    magnitudes whose f32 rounding the subtraction propagates), as a pair (env, inc)."""
    q_env, q_inc, reward = (np.asarray(x, dtype=np.float64) for x in (q_env, q_inc, reward))
    actions, actions_inc = np.asarray(actions, dtype=np.int64), np.asarray(actions_inc, dtype=np.int64)
    N, T1, n, A = q_env.shape
    T = T1 - 1
    term = np.asarray(terminated, dtype=np.float64).reshape(N, T1)
    fill = np.ones((N, T1)) if filled is None else np.asarray(filled, dtype=np.float64).reshape(N, T1)
    off = 1 - np.eye(n, dtype=np.int64)
    m = actions_inc.reshape(N, T1, n, n)[:, :T] * off
    give = (m != 0).sum(axis=3).astype(np.float64)
    rp, rn = (m == 1).sum(axis=2).astype(np.float64), (m == 2).sum(axis=2).astype(np.float64)
    r = reward[:, :T] / c["reward_scale"]
    r_env = (r + (rp - rn) * c["incentive_ratio"] * c["incentive"]) / c["seq_len"]
    r_inc = (r - give * c["incentive_cost"] * c["incentive"]) / c["seq_len"]
    mask = fill[:, :T].copy()
    mask[:, 1:] *= 1 - term[:, :T - 1]
    live = (1 - term[:, :T])[..., None]
    avail = np.array([(int(avail_bits) >> k) & 1 for k in range(A)], dtype=bool)
    chosen_env = np.take_along_axis(q_env[:, :T], actions.reshape(N, T1, n, 1)[:, :T], axis=3)[..., 0]
    v_env = np.where(avail, q_env[:, 1:], NEG).max(axis=-1)
    chosen_inc = (np.take_along_axis(q_inc[:, :T], m[..., None], axis=4)[..., 0] * off).sum(axis=-1)
    v_inc = (q_inc[:, 1:].max(axis=-1) * off).sum(axis=-1)
    td_env = chosen_env - (r_env + c["gamma_env"] * live * v_env)
    td_inc = chosen_inc - (r_inc + c["gamma_inc"] * live * v_inc)
    bound = (np.abs(chosen_env) + np.abs(r_env) + c["gamma_env"] * np.abs(v_env), np.abs(chosen_inc) + np.abs(r_inc) + c["gamma_inc"] * np.abs(v_inc))
    return td_env, td_inc, np.broadcast_to(mask[..., None], td_env.shape).copy(), bound


def aggregate(td_env, td_inc, mask, alpha, eta, eps):
    """(p [N], the unrounded p^alpha ONE clamped to [1, QMAX], its rounding as int64) of per-row errors [N, T, n]"""
    N = td_env.shape[0]
    d = np.sqrt((td_env * mask) ** 2 + (td_inc * mask) ** 2).reshape(N, -1)
    p = eta * d.max(axis=1) + (1.0 - eta) * d.sum(axis=1) / np.maximum(1.0, mask.reshape(N, -1).sum(axis=1)) + eps
    v = np.clip(p ** alpha * ONE, 1.0, float(QMAX))
    return p, v, np.rint(v).astype(np.int64)


def fixed(p, alpha):
    """p^alpha ONE clamped to [1, QMAX], unrounded (p floored at 0)"""
    return np.clip(np.maximum(p, 0.0) ** alpha * ONE, 1.0, float(QMAX))


def initial_priority(q_env, q_inc, actions, actions_inc, reward, terminated, filled, avail_bits, c, alpha, eta, eps):
    """SimpleNamespace(p, exact, q, bound): the aggregate error, the unrounded fixed-point value, its rounding [N], and the row bounds"""
    td_env, td_inc, mask, bound = td_rows(q_env, q_inc, actions, actions_inc, reward, terminated, filled, avail_bits, c)
    p, v, q = aggregate(td_env, td_inc, mask, alpha, eta, eps)
    return SimpleNamespace(p=p, exact=v, q=q, bound=bound, td_env=td_env, td_inc=td_inc, mask=mask)


def episodes(N, T, n, A, seed, exact=True, terminate=True):
    """Random whole-episode arrays for the definition above.  exact: Q-values on multiples of 2^-10 in [-2, 2] and integer rewards
    (every td is exact in f32 with dyadic constants); else normal Q-values and rewards.  terminate: env 0 terminates at slot 0, every
    third env somewhere mid-episode (`filled` is 0 behind the flag, as a runner leaves it)."""
    rng = np.random.default_rng(seed)
    if exact:
        q_env = rng.integers(-2048, 2049, (N, T + 1, n, A)) / 1024.0
        q_inc = rng.integers(-2048, 2049, (N, T + 1, n, n, 3)) / 1024.0
        reward = rng.integers(-1, 4, (N, T + 1, n)).astype(np.float64)
    else:
        q_env, q_inc = rng.normal(size=(N, T + 1, n, A)), rng.normal(size=(N, T + 1, n, n, 3))
        reward = rng.normal(size=(N, T + 1, n)) * (rng.random((N, T + 1, n)) < 0.3)
    terminated, filled = np.zeros((N, T + 1), dtype=np.uint8), np.ones((N, T + 1), dtype=np.int64)
    if terminate:
        for b in range(N):
            t_end = 0 if b == 0 else int(rng.integers(1, T)) if b % 3 == 1 else None
            if t_end is not None:                        # the flag masks the next row; the slots behind it are not filled
                terminated[b, t_end] = 1
                filled[b, t_end + 1:] = 0
    return dict(q_env=q_env.astype(np.float32), q_inc=q_inc.astype(np.float32), actions=rng.integers(0, A, (N, T + 1, n)).astype(np.int64),
                actions_inc=rng.integers(0, 3, (N, T + 1, n, n)).astype(np.int64), reward=reward.astype(np.float32), terminated=terminated,
                filled=filled)


DYADIC = dict(gamma_env=0.5, gamma_inc=0.25, reward_scale=1.0, incentive_ratio=0.5, incentive_cost=0.25, incentive=2.0, seq_len=8.0)
