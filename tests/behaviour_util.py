"""Helpers of the behaviour-statistics tests (tests/test_behaviour_host.py, tests/test_behaviour_gpu.py): no test in here.

reference_stats is a numpy int64 statement of the block table in include/ssd_hip.h (ssd_behaviour_stats), written from that table with
plain loops over agents and pairs -- it shares no code with ops.behaviour_stats or the kernels."""
import numpy as np

ROLES = ("idle", "cleaner", "harvester", "mixed")


def length(n, A):
    return 12 * n + n * A + 3 * n * n + 3


def _rounded(x):
    x = np.asarray(x, dtype=np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    return np.rint(np.clip(x, -2.0 ** 24, 2.0 ** 24)).astype(np.int64)


def reference_blocks(actions, actions_inc, reward, clean_num, A):
    """the blocks by name, int64, of fields over T + 1 slots: actions [N, T+1, n], actions_inc [N, T+1, n, n], reward / clean_num [N, T+1, n]"""
    actions, actions_inc = np.asarray(actions).astype(np.int64), np.asarray(actions_inc).astype(np.int64)
    if actions.ndim == 4:
        actions = actions[..., 0]
    if actions_inc.ndim == 5:
        actions_inc = actions_inc[..., 0]
    N, T1, n = actions.shape
    T = T1 - 1
    act, inc = actions[:, :T], actions_inc[:, :T]
    r, c = _rounded(reward)[:, :T], _rounded(clean_num)[:, :T]
    cl, hv = (c > 0).astype(np.int64), (r > 0).astype(np.int64)
    t = np.arange(T, dtype=np.int64).reshape(1, T, 1)
    out = {"reward_sum": r.sum((0, 1)), "clean_sum": c.sum((0, 1)), "clean_steps": cl.sum((0, 1)), "harvest_steps": hv.sum((0, 1)),
           "harvest_time": (t * hv).sum((0, 1))}
    out["action_count"] = np.zeros((n, A), np.int64)
    for i in range(n):
        for a in range(A):
            out["action_count"][i, a] = (act[:, :, i] == a).sum()
    out["inc_count"] = np.zeros((n, n, 3), np.int64)
    rv = np.zeros((N, T, n), np.int64)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            for k in range(3):
                out["inc_count"][i, j, k] = (inc[:, :, i, j] == k).sum()
            rv[:, :, j] += (inc[:, :, i, j] == 1).astype(np.int64) - (inc[:, :, i, j] == 2).astype(np.int64)
    out["recv_on_clean"] = (cl * rv).sum((0, 1))
    out["recv_on_reward"] = (r * rv).sum((0, 1))
    C, H = cl.sum(1), hv.sum(1)                                        # [N, n] per episode
    role = np.full((N, n), -1, np.int64)
    role[(C == 0) & (H == 0)] = 0
    role[C > H] = 1
    role[H > C] = 2
    role[(C == H) & (C > 0)] = 3
    assert (role >= 0).all()
    out["role_count"] = np.stack([(role == k).sum(0) for k in range(4)], axis=-1).astype(np.int64)
    cleaners = (role == 1).sum(1)
    out["cleaners_hist"] = np.array([(cleaners == k).sum() for k in range(n + 1)], np.int64)
    out["n_episodes"] = np.array([N], np.int64)
    out["n_steps"] = np.array([N * T], np.int64)
    return out


ORDER = ("reward_sum", "clean_sum", "clean_steps", "harvest_steps", "harvest_time", "action_count", "inc_count", "recv_on_clean",
         "recv_on_reward", "role_count", "cleaners_hist", "n_episodes", "n_steps")


def reference_stats(actions, actions_inc, reward, clean_num, A):
    """the accumulator vector (int64 [SSD_BEHAVIOUR_LEN(n, A)]) one call adds"""
    b = reference_blocks(actions, actions_inc, reward, clean_num, A)
    vec = np.concatenate([b[k].reshape(-1) for k in ORDER]).astype(np.int64)
    assert vec.size == length(np.asarray(reward).shape[2], A)
    return vec


def seeded_batch(N, T, n, A, seed, hostile=True):
    """Integer fields over T + 1 slots: rewards in -1 .. 2 (fire cost), clean_num 0 .. 2, a non-zero diagonal in actions_inc, and
    (hostile) actions of -1 and A and incentive values of 3 sprinkled in.  Slot T carries out-of-range garbage everywhere (it must not
    be counted: the kernels never read it)."""
    g = np.random.default_rng(seed)
    actions = g.integers(0, A, (N, T + 1, n)).astype(np.int64)
    inc = g.integers(0, 3, (N, T + 1, n, n)).astype(np.int64)
    reward = g.integers(-1, 3, (N, T + 1, n)).astype(np.float32)
    clean = (g.integers(0, 3, (N, T + 1, n)) * (g.random((N, T + 1, n)) < 0.4)).astype(np.float32)
    if hostile:
        bad = g.random(actions.shape) < 0.1
        actions[bad] = np.where(g.random(int(bad.sum())) < 0.5, -1, A)
        inc[g.random(inc.shape) < 0.1] = 3
        actions[0, 0, 0], actions[-1, T - 1, n - 1] = -1, A            # (the smallest shapes too hold one of each)
        inc[0, 0, 0, n - 1] = 3
    actions[:, T], inc[:, T] = 1 << 40, -7
    reward[:, T], clean[:, T] = 1.0e9, -3.0e8
    return actions, inc, reward, clean
