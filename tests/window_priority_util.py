"""Helpers of the per-window priority tests (config key per_unit: "window"): a helper, no test in it.

The window grid and the per-window aggregate restated from include/ssd_hip.h -- nothing here calls the package.  An episode of T
transitions, windows of L, stride s, burn-in K:

    S        = ceil((T - L) / s) + 1
    start_k  = min(k s, T - L)                                  (the last window is clamped onto the episode's tail)
    loss rows of window k: start_k + K_k <= row < start_k + L,  K_k = K if start_k > 0 else 0
    entry (slot, k) of the table sits at slot S + k;  a drawn entry f is ids = f // S, t0 = start_(f % S)
    q_init[env, k] = the initial priority of rollout_priority_util over the loss rows of window k, all agents
"""
import numpy as np

from tests import rollout_priority_util as U
from tests.priority_util import ONE, QMAX

# (T, L, s, K) -> starts: the clamped last window off the stride (with and without burn-in); no overlap, exact fit; overlap at the cap
# of 8 windows per row; the single-window case
GRIDS = {(9, 4, 2, 0): [0, 2, 4, 5], (9, 4, 2, 1): [0, 2, 4, 5], (12, 3, 3, 0): [0, 3, 6, 9], (10, 8, 1, 3): [0, 1, 2], (7, 7, 1, 0): [0]}
SHAPES = [(1, 2, 9), (3, 5, 9), (17, 5, 9), (67, 10, 16)]       # (N, n, A): 17 crosses a 16-env workgroup, 67 ends in a partial one


def n_windows(T, L, s):
    return -(-(T - L) // s) + 1


def starts(T, L, s):
    return [min(k * s, T - L) for k in range(n_windows(T, L, s))]


def loss_rows(T, L, s, K):
    """per window, the list of its loss rows"""
    return [list(range(st + (K if st > 0 else 0), st + L)) for st in starts(T, L, s)]


def member(T, L, s, K):
    """bool [S, T]: row t is a loss row of window k"""
    m = np.zeros((n_windows(T, L, s), T), dtype=bool)
    for k, rows in enumerate(loss_rows(T, L, s, K)):
        m[k, rows] = True
    return m


def window_priority(ep, grid, avail_bits, c, alpha, eta, eps, filled=True):
    """float64: p [N, S], the unrounded fixed-point value [N, S], and the rollout_priority_util rows it was aggregated from (with the
    per-window largest row bounds [N, S] of the general-float bar)"""
    T, L, s, K = grid
    ref = U.initial_priority(ep["q_env"], ep["q_inc"], ep["actions"], ep["actions_inc"], ep["reward"], ep["terminated"],
                             ep["filled"] if filled else None, avail_bits, c, alpha, eta, eps)
    N = ref.td_env.shape[0]
    d = np.sqrt((ref.td_env * ref.mask) ** 2 + (ref.td_inc * ref.mask) ** 2)          # [N, T, n]
    p, bound = [], []
    for rows in loss_rows(T, L, s, K):
        dw, mw = d[:, rows].reshape(N, -1), ref.mask[:, rows].reshape(N, -1)
        p.append(eta * dw.max(axis=1) + (1.0 - eta) * dw.sum(axis=1) / np.maximum(1.0, mw.sum(axis=1)) + eps)
        bound.append(ref.bound[0][:, rows].reshape(N, -1).max(axis=1) + ref.bound[1][:, rows].reshape(N, -1).max(axis=1))
    p = np.stack(p, axis=1)
    return p, np.clip(p ** alpha * ONE, 1.0, float(QMAX)), ref, np.stack(bound, axis=1)


def acc_f32(ref, grid):
    """f32 [N, n, S, 3] = (max d, sum d in rising t, sum mask) per (env, agent, window), every operation rounded to f32 as the kernel's
    -- meaningful where the TD errors are exact in f32 (rollout_priority_util.episodes(exact=True) with the dyadic constants)"""
    T, L, s, K = grid
    e, i = (ref.td_env * ref.mask).astype(np.float32), (ref.td_inc * ref.mask).astype(np.float32)
    assert np.array_equal(e.astype(np.float64), ref.td_env * ref.mask) and np.array_equal(i.astype(np.float64), ref.td_inc * ref.mask)
    d = np.sqrt(e * e + i * i)                                                        # float32 throughout
    mask = ref.mask.astype(np.float32)
    N, _, n = d.shape
    out = np.zeros((N, n, n_windows(T, L, s), 3), np.float32)
    for k, rows in enumerate(loss_rows(T, L, s, K)):
        for t in rows:
            out[:, :, k, 0] = np.maximum(out[:, :, k, 0], d[:, t])
            out[:, :, k, 1] = out[:, :, k, 1] + d[:, t]
            out[:, :, k, 2] = out[:, :, k, 2] + mask[:, t]
    return out


def entry_tables(seed=0):
    """name -> (int32 table of entries, S): the entry counts of the issue with roughly a third of the entries zero, and one all zero"""
    rng = np.random.default_rng(seed)
    out = {}
    for slots, S in ((1, 1), (5, 4), (1000, 4), (8192, 7)):
        t = rng.integers(1, QMAX + 1, slots * S).astype(np.int32)
        t[rng.random(slots * S) < 1.0 / 3.0] = 0
        out["%dx%d" % (slots, S)] = (t, S)
    out["zero_1000x4"] = (np.zeros(4000, np.int32), 4)
    return out
