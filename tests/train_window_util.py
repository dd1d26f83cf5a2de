"""Helpers of the train-window tests (a helper, no test in it).

The window draw restated from include/ssd_hip.h (ssd_sample_windows) in plain integers -- nothing here comes from the package:

    mix32p(x): x ^= x>>17; x *= 0xed5ad4bb; x ^= x>>11; x *= 0xac4c1b51; x ^= x>>15; x *= 0x31848bab; x ^= x>>14      (u32)
    draw(i)  = mix32p(mix32p(s0 ^ (call * 0x9E3779B9)) ^ (s1 + i * 0x85EBCA6B)),   s0 / s1 = the low / high 32 bits of seed
    ids:       for i < count: j = population - count + i; t = draw(i) * (j + 1) >> 32; pick[i] = t if t is new else j
               for i = count - 1 .. 1: k = draw(count + i) * (i + 1) >> 32; swap(pick[i], pick[k])
    t0[e]    = draw(2 * count + e) * n_starts >> 32

plus the numpy statement of the gather (slices and the `filled` rule), and the cases of tests/golden/learner_train_window.npz."""
import json
import os

import numpy as np
import torch as th

from tests.learner_util import GOLDEN, build, load_fixture

M32 = 0xFFFFFFFF


def mix32p(x):
    x &= M32
    x ^= x >> 17; x = (x * 0xed5ad4bb) & M32
    x ^= x >> 11; x = (x * 0xac4c1b51) & M32
    x ^= x >> 15; x = (x * 0x31848bab) & M32
    return x ^ (x >> 14)


def draw(seed, call, i):
    s0, s1 = seed & M32, (seed >> 32) & M32
    return mix32p(mix32p(s0 ^ ((call * 0x9E3779B9) & M32)) ^ ((s1 + i * 0x85EBCA6B) & M32))


def sample_windows(seed, call, population, count, n_starts):
    """(ids, t0): two lists of `count` python ints"""
    call &= M32
    pick = []
    for i in range(count):
        j = population - count + i
        t = (draw(seed, call, i) * (j + 1)) >> 32
        pick.append(j if t in pick else t)
    for i in range(count - 1, 0, -1):
        k = (draw(seed, call, count + i) * (i + 1)) >> 32
        pick[i], pick[k] = pick[k], pick[i]
    return pick, [(draw(seed, call, 2 * count + e) * n_starts) >> 32 for e in range(count)]


def _mix32p_np(x):
    x = x & np.uint64(M32)
    for shift, mul in ((17, 0xed5ad4bb), (11, 0xac4c1b51), (15, 0x31848bab)):
        x = x ^ (x >> np.uint64(shift))
        x = (x * np.uint64(mul)) & np.uint64(M32)
    return x ^ (x >> np.uint64(14))


def starts_of_calls(seed, calls, count, n_starts):
    """t0 [len(calls), count] of many calls at once (the same lines on uint64 arrays masked to 32 bits)"""
    s0, s1 = np.uint64(seed & M32), np.uint64((seed >> 32) & M32)
    calls = np.asarray(calls, dtype=np.uint64) & np.uint64(M32)
    x = _mix32p_np(s0 ^ ((calls * np.uint64(0x9E3779B9)) & np.uint64(M32)))[:, None]
    i = np.arange(2 * count, 3 * count, dtype=np.uint64)[None, :]
    d = _mix32p_np(x ^ ((s1 + i * np.uint64(0x85EBCA6B)) & np.uint64(M32)))
    return ((d * np.uint64(n_starts)) >> np.uint64(32)).astype(np.int64)


def window_slices(arr, ids, t0, win_slots):
    """arr [rows, src_slots, ...] -> [len(ids), win_slots, ...]: the plain slices"""
    return np.stack([arr[i, s:s + win_slots] for i, s in zip(ids, t0)])


def window_filled(filled, ids, t0, win_slots, burn_in):
    """the `filled` rule: the slices times (r >= K_e), K_e = burn_in if t0 > 0 else 0"""
    out = window_slices(filled, ids, t0, win_slots).copy()
    for e, s in enumerate(t0):
        out[e, :burn_in if s > 0 else 0] = 0
    return out


# ---- tests/golden/learner_train_window.npz -------------------------------------------------------------------------------------------
def load_golden():
    z = np.load(os.path.join(GOLDEN, "learner_train_window.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def golden_case(name):
    """(recorded numbers: key -> array, the case's meta entry)"""
    z, meta = load_golden()
    c = next(c for c in meta["cases"] if c["name"] == name)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}, c


CASES = [c["name"] for c in load_golden()[1]["cases"]]


def buffer_of(batch, rows=None, size=None, norm="window"):
    """A ReplayBuffer on the batch's device that holds the batch's episodes at `rows` (default 0 .. B - 1) of `size` slots; every
    other row is a decoy: the batch's episodes rolled by five slots with the rewards negated."""
    from homophily_marl_amd.components.episode_buffer import ReplayBuffer
    B = batch.batch_size
    rows = list(range(B)) if rows is None else list(rows)
    size = max(rows) + 1 if size is None else size
    derived = {"filled"} | {new for new, _ in batch.preprocess.values()}
    scheme = {k: v for k, v in batch.scheme.items() if k not in derived}
    buf = ReplayBuffer(scheme, batch.groups, size, batch.max_seq_length, preprocess=batch.preprocess, device=batch.device)
    for k, v in batch.data.transition_data.items():
        dst = buf.data.transition_data[k]
        decoy = th.roll(v, 5, dims=1)
        decoy = -decoy if k == "reward" else decoy
        for r in range(size):
            dst[r].copy_(decoy[r % B])
        dst[th.as_tensor(rows, device=dst.device)] = v
    buf.episodes_in_buffer = size
    buf.window_norm = norm
    return buf


def build_case(c, device="cpu", code_obs=False, overrides=None):
    """(args, whole-episode batch, mac, learner) of a golden case on THIS package (tests/learner_util.build)"""
    z, meta = load_fixture(c["base"])
    return build(z, meta, device=device, overrides=dict(c["overrides"], **(overrides or {})), code_obs=code_obs)
