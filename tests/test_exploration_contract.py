"""The exploration-draw contract of include/ssd_hip.h ("Exploration draws"), tested on its host restatement (tests/explore_util.py) alone:
no GPU, no library.  tests/test_exploration_draws.py holds every pick site of the kernels to the restatement bit for bit, so what is
measured here at 10^6 rows per configuration is what the rollout draws.

Every input is fixed, so each statistic is a constant of the contract; the bars are conditions on it, not measurements of it:
|z| < 4 for every binomial count and every correlation (sqrt(R) r of two flag or value arrays is standard normal under independence), and
the 0.9999 quantile of chi-square with the matching degrees of freedom.  Every observed statistic is printed.

Configurations: both key layouts, env_id_base 0 / 4096 * 7 + 3 / one that wraps the 32-bit key, the runner's seed formula
(cfg.seed * 2654435761 + 12345, the inc head's xor on top) for four config seeds, 40 consecutive steps from 1 (the rollout's first
draw) and one run across the 2^32 wrap of the step."""
import functools

import numpy as np
import pytest

from tests import explore_util as xu

Z_BAR = 4.0
CHI2_9999 = {1: 15.136705, 2: 18.420681, 4: 23.512742, 5: 25.744832, 8: 31.827628}      # scipy.stats.chi2.ppf(0.9999, df)
STEPS = 40
BASE_MID, BASE_WRAP = 4096 * 7 + 3, 0xFFFFF000


def runner_seed(cfg_seed, inc):
    s = (cfg_seed * 2654435761 + 12345) & xu.M32
    return s ^ xu.INC_SEED_XOR if inc else s


#          id                 layout  N     n   base       config seed  first step
CONFIGS = [("env-base0",      "env", 2500, 10, 0,         1,           1),
           ("env-mid",        "env", 5000, 5,  BASE_MID,  1,           1),
           ("env-wrap",       "env", 2500, 10, BASE_WRAP, 21,          1),
           ("env-seed3-wrapstep", "env", 2500, 10, 0,     3,           2 ** 32 - 20),
           ("inc-base0",      "inc", 250,  10, 0,         1,           1),
           ("inc-mid",        "inc", 1000, 5,  BASE_MID,  1,           1),
           ("inc-wrap",       "inc", 250,  10, BASE_WRAP, 21,          1),
           ("inc-seed12345",  "inc", 250,  10, 0,         12345,       1)]
IDS = [c[0] for c in CONFIGS]


@functools.lru_cache(maxsize=None)
def _draws(layout, N, n, base, cfg_seed, step0, inc_seed=None):
    """(x0, x1) [STEPS, N, n(, n)] of a configuration; read-only"""
    keys = (xu.inc_keys if layout == "inc" else xu.env_keys)(N, n, base)
    seed = runner_seed(cfg_seed, layout == "inc" if inc_seed is None else inc_seed)
    steps = (step0 + np.arange(STEPS, dtype=np.int64)).reshape((STEPS,) + (1,) * keys.ndim)
    x0, x1 = xu.draws(seed, steps, keys[None])
    x0.setflags(write=False); x1.setflags(write=False)
    return x0, x1


def _cfg(c):
    x0, x1 = _draws(*c[1:])
    assert x0.size >= 10 ** 6 and x0.shape == x1.shape
    return x0, x1


def _z_count(count, R, p):
    return (count - R * p) / np.sqrt(R * p * (1 - p))


def _z_corr(a, b):
    """sqrt(R) times the sample correlation of two equally shaped arrays"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(np.sqrt(a.size) * (a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def _chi2_uniform(picks, live):
    counts = np.array([(picks == k).sum() for k in live], dtype=np.float64)
    assert counts.sum() == picks.size                      # nothing outside the available actions
    e = picks.size / len(live)
    return float(((counts - e) ** 2 / e).sum())


def _chi2_table(flag, picks, live):
    """chi-square of the 2 x k table flag x pick against the product of its margins (k - 1 degrees of freedom)"""
    t = np.array([[((picks == k) & (flag == f)).sum() for k in live] for f in (False, True)], dtype=np.float64)
    e = t.sum(1, keepdims=True) * t.sum(0, keepdims=True) / t.sum()
    return float(((t - e) ** 2 / e).sum())


def test_the_tabulated_quantiles_are_chi_squares():
    try:
        from scipy import stats
    except ImportError:           # the table stands on its own
        return
    for df, q in CHI2_9999.items():
        assert abs(stats.chi2.ppf(0.9999, df) - q) < 1e-5
    assert abs(2 * stats.norm.sf(Z_BAR) - 6.334e-5) < 1e-7


def test_mix32p_and_the_draws_are_the_header_arithmetic_on_plain_integers():
    """the vectorised restatement against the same lines in Python integers, at the edges of the 32-bit range"""
    def mix(x):
        x ^= x >> 17; x = x * 0xed5ad4bb & xu.M32; x ^= x >> 11; x = x * 0xac4c1b51 & xu.M32; x ^= x >> 15; x = x * 0x31848bab & xu.M32
        return x ^ (x >> 14)
    xs = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x9E3779B9, 123456789]
    assert [int(v) for v in xu.mix32p(np.array(xs, dtype=np.uint64))] == [mix(x) for x in xs]
    assert mix(0) == 0 and len({mix(x) for x in xs}) == len(xs)
    for seed, step, key in [(0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (runner_seed(21, True), 17, 4096 * 7 + 3), (5, 2 ** 32 + 17, 9)]:
        x0, x1 = xu.draws(seed, step, np.array([key]))
        e0 = mix(seed ^ mix(((step & xu.M32) * 0x9E3779B9 + key) & xu.M32))
        assert (int(x0[0]), int(x1[0])) == (e0, mix(e0 ^ 0x85EBCA6B))
    a, b = xu.draws(5, 17, np.arange(100)), xu.draws(5, 2 ** 32 + 17, np.arange(100))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()                       # step mod 2^32
    assert (xu.env_keys(3, 5, 7) == [[35 + i for i in range(5)], [40 + i for i in range(5)], [45 + i for i in range(5)]]).all()
    assert (xu.inc_keys(2, 3, 1)[1] == [[(6 + i) * 3 + j for j in range(3)] for i in range(3)]).all()
    assert int(xu.env_keys(1, 10, 0xFFFFFFFF)[0, 3]) == (0xFFFFFFFF * 10 + 3) & xu.M32          # the key wraps like the kernel's uint32
    # the pick: floor(x1 * live / 2^32) counted over the AVAILABLE actions, lowest first
    x1 = np.array([0, 0x33333333, 0x33333334, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    shipped9 = xu.avail_bits([1, 1, 1, 1, 1, 0, 0, 0, 1], 9)
    assert shipped9 == 0b100011111
    assert xu.pick(x1, shipped9, 9).tolist() == [0, 1, 1, 2, 3, 8] and xu.pick(x1, 0, 9).tolist() == [-1] * 6
    assert xu.pick(x1, xu.avail_bits(None, 2), 2).tolist() == [0, 0, 0, 0, 1, 1]
    q = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 1.0, 5.0]])
    assert xu.first_max(q, 0b1111, 4).tolist() == [1, 0] and xu.first_max(q, 0b0100, 4).tolist() == [2, 2]
    assert xu.first_max(q, 0b1101, 4).tolist() == [2, 0] and xu.first_max(q, 0b1110, 4).tolist() == [1, 1]
    assert xu.first_max(q, 0b1100, 4).tolist() == [2, 3] and xu.first_max(q, 0, 4).tolist() == [0, 0]


@pytest.mark.parametrize("c", CONFIGS, ids=IDS)
def test_explored_fraction_is_epsilon(c):
    x0, _ = _cfg(c)
    R = x0.size
    for eps in (2.0 ** -24, 0.05, 0.3, 0.999):
        count = int(xu.explores(x0, eps).sum())
        z = _z_count(count, R, eps)
        print("%s eps %.3g: %d of %d explore, z = %+.2f" % (c[0], eps, count, R, z))
        assert abs(z) < Z_BAR, (eps, count, z)
    for eps in (1.0, 1.5, np.inf):
        assert xu.explores(x0, eps).all(), eps
    for eps in (0.0, -0.0, -1.0, np.nan):
        assert not xu.explores(x0, eps).any(), eps
    # the flag is monotone in epsilon: a row that explores at 0.05 explores at 0.3
    assert not (xu.explores(x0, 0.05) & ~xu.explores(x0, 0.3)).any()


#        id             A  mask (None = all)
MASKS = [("A3-all",     3, None),
         ("A8-shipped", 8, [1, 1, 1, 1, 1, 0, 0, 0]),
         ("A9-shipped", 9, [1, 1, 1, 1, 1, 0, 0, 0, 1]),
         ("A9-first",   9, [1] + [0] * 8),
         ("A9-last",    9, [0] * 8 + [1])]


@pytest.mark.parametrize("c", CONFIGS, ids=IDS)
def test_picks_are_uniform_over_the_available_actions_and_independent_of_the_flag(c):
    x0, x1 = _cfg(c)
    for name, A, mask in MASKS:
        bits = xu.avail_bits(mask, A)
        live = [k for k in range(A) if (bits >> k) & 1]
        picks = xu.pick(x1, bits, A)
        if len(live) == 1:
            assert (picks == live[0]).all(), name
            continue
        df = len(live) - 1
        c_all = _chi2_uniform(picks, live)
        print("%s %s: chi2_%d of the picks over all rows %.2f (bar %.2f)" % (c[0], name, df, c_all, CHI2_9999[df]))
        assert c_all < CHI2_9999[df], (name, c_all)
        for eps in (0.05, 0.3):
            flag = xu.explores(x0, eps)
            c_exp, c_tab = _chi2_uniform(picks[flag], live), _chi2_table(flag, picks, live)
            print("%s %s eps %.2f: chi2_%d among the %d explored rows %.2f, of the flag x pick table %.2f" % (c[0], name, eps, df, flag.sum(), c_exp, c_tab))
            assert c_exp < CHI2_9999[df] and c_tab < CHI2_9999[df], (name, eps, c_exp, c_tab)
    # the two words of a draw as numbers
    z = _z_corr(x0, x1)
    print("%s: corr(x0, x1) z = %+.2f" % (c[0], z))
    assert abs(z) < Z_BAR


@pytest.mark.parametrize("c", CONFIGS, ids=IDS)
def test_flags_are_independent_across_steps_and_keys(c):
    """a row at step t against step t + 1 and t + 2; neighbouring keys at one step (the last axis: agents of an env, receivers of a
    giver -- at every distance, so the inc flags of (b, i, j) against every (b, i, j')), and neighbouring envs"""
    x0, _ = _cfg(c)
    u = x0 >> np.uint32(8)
    for eps in (0.05, 0.3):
        f = xu.explores(x0, eps)
        out = {"t+1": _z_corr(f[:-1], f[1:]), "t+2": _z_corr(f[:-2], f[2:]), "env+1": _z_corr(f[:, :-1], f[:, 1:])}
        for d in range(1, f.shape[-1]):
            out["key+%d" % d] = _z_corr(f[..., :-d], f[..., d:])
        if f.ndim == 4:
            n = f.shape[-1]
            out["giver+1"] = _z_corr(f[:, :, :-1], f[:, :, 1:])
            lo, hi = np.triu_indices(n, 1)
            out["transpose"] = _z_corr(f[..., lo, hi], f[..., hi, lo])          # (b, i, j) against (b, j, i), every pair once
            # all receivers of a giver exploring together (a key that drops j) would put every row sum at 0 or n: the variance of the
            # explored receivers per giver against a Binomial(n, eps) count's, n p q, with the sample variance's own spread
            # sqrt((mu4 - (n p q)^2) / m), mu4 = n p q (1 + 3 (n - 2) p q)
            sums = f.sum(-1).astype(np.float64)
            npq = n * eps * (1 - eps)
            mu4 = npq * (1 + 3 * (n - 2) * eps * (1 - eps))
            out["row-variance"] = float((sums.var() - npq) / np.sqrt((mu4 - npq * npq) / sums.size))
        print("%s eps %.2f flag correlations (z): %s" % (c[0], eps, "  ".join("%s %+.2f" % kv for kv in out.items())))
        assert max(abs(z) for z in out.values()) < Z_BAR, out
    out = {"t+1": _z_corr(u[:-1], u[1:]), "key+1": _z_corr(u[..., :-1], u[..., 1:]), "env+1": _z_corr(u[:, :-1], u[:, 1:])}
    print("%s serial correlation of the 24-bit uniforms (z): %s" % (c[0], "  ".join("%s %+.2f" % kv for kv in out.items())))
    assert max(abs(z) for z in out.values()) < Z_BAR, out


@pytest.mark.parametrize("N,n,base,cfg_seed", [(250, 10, 0, 1), (1000, 5, BASE_MID, 1), (250, 10, BASE_WRAP, 21), (250, 10, 0, 12345)])
def test_env_head_and_inc_head_draw_from_separate_streams(N, n, base, cfg_seed):
    """the env-head flag (and pick) of (b, i) against the inc-head flags (and picks) of (b, i, .), same steps, same config seed; and
    the inc layout under the ENV seed (what the inc head would draw without its xor) is another stream than the inc head's own."""
    e0, e1 = _draws("env", N, n, base, cfg_seed, 1)
    i0, i1 = _draws("inc", N, n, base, cfg_seed, 1)
    assert i0.size >= 10 ** 6 and e0.shape == i0.shape[:-1]
    for eps in (0.05, 0.3):
        fe, fi = xu.explores(e0, eps), xu.explores(i0, eps)
        z = _z_corr(np.broadcast_to(fe[..., None], fi.shape), fi)
        print("N %d n %d base %d seed %d eps %.2f: env flag x inc flags z = %+.2f" % (N, n, base, cfg_seed, eps, z))
        assert abs(z) < Z_BAR
    z = _z_corr(np.broadcast_to((e1 >> np.uint32(8))[..., None], i1.shape), i1 >> np.uint32(8))
    assert abs(z) < Z_BAR, z
    s0, _ = _draws("inc", N, n, base, cfg_seed, 1, False)
    assert runner_seed(cfg_seed, True) == runner_seed(cfg_seed, False) ^ 0x5bd1e995
    same = float((s0 == i0).mean())
    z = _z_corr(s0 >> np.uint32(8), i0 >> np.uint32(8))
    print("inc keys under the env seed against the inc seed: equal words %.2e, z = %+.2f" % (same, z))
    assert same < 1e-5 and abs(z) < Z_BAR
