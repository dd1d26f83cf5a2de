"""The exploration draws of the rollout restated on the host (include/ssd_hip.h, "Exploration draws"): integers only, plus the one
f32 compare.  Written from the header's contract; nothing here comes from the package (homophily_marl_amd.ops has its own generator for
the replay sampler -- another key schedule).

    mix32p(x): x ^= x>>17; x *= 0xed5ad4bb; x ^= x>>11; x *= 0xac4c1b51; x ^= x>>15; x *= 0x31848bab; x ^= x>>14      (u32)
    x0 = mix32p(seed ^ mix32p(u32(step) * 0x9E3779B9 + key));   x1 = mix32p(x0 ^ 0x85EBCA6B)
    explore  <=>  f32(x0 >> 8) * 2^-24 < eps
    pick = (u64(x1) * popcount(live)) >> 32  ->  the pick-th lowest available action
    key  = (env_id_base + b) * n + i   (env head)        ((env_id_base + b) * n + i) * n + j   (inc head)

32-bit values travel as uint64 arrays masked to 32 bits (a 32 x 32 bit product fits); results are uint32.  Keys, draws, flags and
actions are ENV-major: [N, n] for the env head, [N, n(giver), n(receiver)] for the inc head, as the kernels store their actions."""
import numpy as np

M32 = 0xFFFFFFFF
INC_SEED_XOR = 0x5bd1e995
GOLDEN, X1_XOR = 0x9E3779B9, 0x85EBCA6B


def mix32p(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> 17)
    x = (x * 0xed5ad4bb) & M32
    x = x ^ (x >> 11)
    x = (x * 0xac4c1b51) & M32
    x = x ^ (x >> 15)
    x = (x * 0x31848bab) & M32
    return x ^ (x >> 14)


def draws(seed, step, keys):
    """(x0, x1) uint32 for every key; step (an int or an array that broadcasts against keys) is taken mod 2^32, like (uint32_t)*step"""
    step = (np.asarray(step, dtype=np.int64).astype(np.uint64)) & M32
    keys = np.asarray(keys, dtype=np.uint64) & M32
    x0 = mix32p((int(seed) & M32) ^ mix32p((step * GOLDEN + keys) & M32))
    x1 = mix32p(x0 ^ X1_XOR)
    return x0.astype(np.uint32), x1.astype(np.uint32)


def explores(x0, eps):
    """the explore flag: one f32 compare against the f32 value of eps (False for NaN and for eps <= 0, True everywhere for eps >= 1)"""
    u = (np.asarray(x0, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)       # both factors exact in f32
    return u < np.float32(eps)


def avail_bits(mask, A):
    """bit k = action k available; mask: None (all) or A values, non-zero = available"""
    if mask is None:
        return (1 << A) - 1
    assert len(mask) == A
    return sum(1 << k for k, v in enumerate(mask) if v)


def pick(x1, bits, A):
    """the uniformly drawn available action per row (int64); -1 where no action is available (the kernels then keep the greedy one)"""
    live = [k for k in range(A) if (int(bits) >> k) & 1]
    x1 = np.asarray(x1, dtype=np.uint32)
    if not live:
        return np.full(x1.shape, -1, dtype=np.int64)
    p = (x1.astype(np.uint64) * np.uint64(len(live))) >> np.uint64(32)
    return np.asarray(live, dtype=np.int64)[p.astype(np.int64)]


def env_keys(N, n, base=0):
    """[N, n] uint64 (values < 2^32)"""
    b = (np.arange(N, dtype=np.uint64)[:, None] + np.uint64(int(base) & M32)) & M32
    return (b * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]) & M32


def inc_keys(N, n, base=0):
    """[N, n(i), n(j)] uint64 (values < 2^32)"""
    return (env_keys(N, n, base)[:, :, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, None, :]) & M32


def first_max(q, bits, A):
    """the first maximum of q[..., A] over the available actions (action 0 when none is available): `q > best` from -inf, in order"""
    q = np.asarray(q)
    assert q.shape[-1] == A
    ok = np.array([(int(bits) >> k) & 1 for k in range(A)], dtype=bool)
    return np.where(ok, q, -np.inf).argmax(axis=-1).astype(np.int64)       # argmax returns the first of equal maxima


def expected_actions(seed, step, keys, eps, bits, A, q, zero_diagonal=False):
    """(actions int64, explore flags) for keys [...] and a Q array [..., A]: the pick where the flag is set (and an action is
    available), the first maximum of q over the available actions elsewhere; zero_diagonal: the inc head's i == j entries are 0."""
    x0, x1 = draws(seed, step, keys)
    flag = explores(x0, eps)
    p = pick(x1, bits, A)
    act = np.where(flag & (p >= 0), p, first_max(q, bits, A))
    if zero_diagonal:
        n = act.shape[-1]
        assert act.shape[-2] == n
        act[..., np.arange(n), np.arange(n)] = 0
    return act, flag
