"""Helpers of the prioritised-replay tests (a helper, no test in it).

The draw, the weights, a trained sample's new priority and the write-back restated from include/ssd_hip.h (ssd_priority_sample /
ssd_priority_update) in plain Python integers and numpy float64 -- nothing here comes from the package:

    mix32p(x): x ^= x>>17; x *= 0xed5ad4bb; x ^= x>>11; x *= 0xac4c1b51; x ^= x>>15; x *= 0x31848bab; x ^= x>>14      (u32)
    draw(i)  = mix32p(mix32p(s0 ^ (call * 0x9E3779B9)) ^ (s1 + i * 0x85EBCA6B)),   s0 / s1 = the low / high 32 bits of seed
    qmax     = max table[k] (k < population) or ONE if that is 0;   qeff[k] = table[k] or qmax;   total = sum qeff
    lo, hi   = total * e // count, total * (e + 1) // count;   x = lo + (draw(e) * (hi - lo) >> 32)
    ids[e]   = the smallest k with qeff[0] + .. + qeff[k] > x;   t0[e] = draw(2 * count + e) * n_starts >> 32
    w_raw[e] = (population * qeff[ids[e]] / total) ** -beta;   weights = w_raw / max w_raw
    d_row    = sqrt(col2 + col3);  p = eta max d + (1 - eta) sum d / max(1, sum col0) + eps;  q_new = clamp(round(p ** alpha * ONE), 1, MAX)
    table[k] = max of the q_new of the samples with ids[e] == k
"""
import numpy as np

M32 = 0xFFFFFFFF
ONE = 65536
QMAX = 1 << 24
SEED = 0x1234567890ABCDEF


def mix32p(x):
    x &= M32
    x ^= x >> 17; x = (x * 0xed5ad4bb) & M32
    x ^= x >> 11; x = (x * 0xac4c1b51) & M32
    x ^= x >> 15; x = (x * 0x31848bab) & M32
    return x ^ (x >> 14)


def draw(seed, call, i):
    s0, s1 = seed & M32, (seed >> 32) & M32
    return mix32p(mix32p(s0 ^ (((call & M32) * 0x9E3779B9) & M32)) ^ ((s1 + i * 0x85EBCA6B) & M32))


def effective(table, population):
    """(qeff as an int64 array, qmax, total as a Python int)"""
    q = np.asarray(table[:population], dtype=np.int64)
    qmax = int(q.max()) or ONE
    qeff = np.where(q == 0, qmax, q)
    return qeff, qmax, int(qeff.sum())


def sample(seed, call, table, population, count, n_starts, beta):
    """dict(ids, t0: lists of Python ints; weights: float64 array; log: the four log values in float64)"""
    qeff, qmax, total = effective(table, population)
    cum = np.cumsum(qeff)                                    # int64: total < 2^44
    ids = []
    for e in range(count):
        lo, hi = total * e // count, total * (e + 1) // count
        x = lo + ((draw(seed, call, e) * (hi - lo)) >> 32)
        ids.append(int(np.searchsorted(cum, x, side="right")))           # the first k with cum[k] > x
    t0 = [(draw(seed, call, 2 * count + e) * n_starts) >> 32 for e in range(count)]
    w = (population * qeff[ids].astype(np.float64) / total) ** (-float(beta))
    w = w / w.max()
    log = [total / population / ONE, int(qeff.max()) / ONE, float(w.min()), float(len(set(ids)))]
    return dict(ids=ids, t0=t0, weights=w, log=log)


def q_new(partials, B, alpha, eta, eps):
    """float64 evaluation over partials [B * rows, 16]: (the unrounded p ** alpha * ONE clamped to [1, MAX], its rounding as int64)"""
    rows = np.asarray(partials, dtype=np.float64).reshape(B, -1, partials.shape[-1])
    d = np.sqrt(rows[..., 2] + rows[..., 3])
    p = eta * d.max(axis=1) + (1.0 - eta) * d.sum(axis=1) / np.maximum(1.0, rows[..., 0].sum(axis=1)) + eps
    v = np.clip(p ** alpha * ONE, 1.0, float(QMAX))
    return v, np.rint(v).astype(np.int64)


def within_q(got, exact):
    """the bar of the issue: |got - exact| <= 1 + exact * 2^-20 (f32 rounding of a sqrt / sum / pow chain against float64)"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    return bool((np.abs(got - exact) <= 1.0 + exact * 2.0 ** -20).all())


def write_back(table, ids, q):
    """the table after the train step: every named slot holds the largest q_new of its samples; ids outside the table are skipped"""
    out = np.array(table, dtype=np.int64)
    best = {}
    for k, v in zip(ids, q):
        if 0 <= k < out.size:
            best[k] = max(best.get(k, 0), int(v))
    for k, v in best.items():
        out[k] = v
    return out


def tables(population, seed=0):
    """name -> int32 table of the cases the issue lists"""
    rng = np.random.default_rng(seed + population)
    out = {"zero": np.zeros(population, np.int32), "max": np.full(population, QMAX, np.int32), "ones": np.ones(population, np.int32)}
    for name, k in (("dominant_first", 0), ("dominant_last", population - 1), ("dominant_mid", population // 2)):
        t = np.ones(population, np.int32)
        t[k] = QMAX
        out[name] = t
    t = rng.integers(1, QMAX + 1, population).astype(np.int32)
    t[rng.random(population) < 0.3] = 0
    out["random_30pct_zero"] = t
    return out


def _mix32p_np(x):
    x = x & np.uint64(M32)
    for shift, mul in ((17, 0xed5ad4bb), (11, 0xac4c1b51), (15, 0x31848bab)):
        x = x ^ (x >> np.uint64(shift))
        x = (x * np.uint64(mul)) & np.uint64(M32)
    return x ^ (x >> np.uint64(14))


def ids_of_calls(seed, calls, table, population, count):
    """ids [len(calls), count] of many calls at once: the same lines on uint64 arrays.  draw * (hi - lo) passes 64 bits, so the
    product is split at bit 32 of the width (d * wh is a whole multiple of 2^32 once shifted: the floor is exact)."""
    qeff, qmax, total = effective(table, population)
    cum = np.cumsum(qeff).astype(np.uint64)
    s0, s1 = np.uint64(seed & M32), np.uint64((seed >> 32) & M32)
    calls = np.asarray(calls, dtype=np.uint64) & np.uint64(M32)
    x0 = _mix32p_np(s0 ^ ((calls * np.uint64(0x9E3779B9)) & np.uint64(M32)))[:, None]
    e = np.arange(count, dtype=np.uint64)[None, :]
    d = _mix32p_np(x0 ^ ((s1 + e * np.uint64(0x85EBCA6B)) & np.uint64(M32)))
    lo = np.array([total * k // count for k in range(count)], dtype=np.uint64)[None, :]
    hi = np.array([total * (k + 1) // count for k in range(count)], dtype=np.uint64)[None, :]
    w = hi - lo
    x = lo + d * (w >> np.uint64(32)) + ((d * (w & np.uint64(M32))) >> np.uint64(32))
    return np.searchsorted(cum, x, side="right").astype(np.int64)
