"""The law of the env's random draws, restated from the reference's source, and the statistics that hold a COUNTER-mode run to it
(numpy only; nothing here comes from csrc or from the library's probability tables).

Bit equality of the device with the CPU oracle cannot see a mistake both sides share (a threshold off by one, a draw index used
twice in one call, a call index or an episode that never enters the key, a tie-break that leans one way): it cancels.  What is
stated here is what the reference's own lines make of np.random / random, whichever generator stands behind them:

  Cleanup   cleanup.py:189-204 (compute_probabilities), constants cleanup.py:31-54        -> cleanup_probabilities
            cleanup.py:168-174  every apple site without an apple and without an agent grows with p_apple(current)
            cleanup.py:177-186  at most one waste cell per step; the free sites are tried in a uniformly shuffled order, each with
                                p_waste:  P(none) = (1 - p)^nfree,  P(J = j) = p (1 - p)^j,  the site is uniform over the free ones
  Harvest   harvest.py:107-120  SPAWN_PROB[min(#apples with j^2 + k^2 <= APPLE_RADIUS, 3)], harvest.py:8,22; the comparison is with
                                APPLE_RADIUS = 2, not its square, so the neighbourhood is the 3 x 3 block      -> harvest_neighbours
  Contests  map_env.py:540-542  the movers are shuffled and the first of them in a contested free cell gets it: 1 / k each
  Spawns    map_env.py:776-777  the spawn list is shuffled for every agent, which takes the last free point of it: uniform over
                                the free points, so the team's placement is uniform over the permutations of the points
            map_env.py:789      the rotation is uniform over 4

tests/golden/env_law.npz (oracle/gen_env_law_golden.py) holds the reference's own numbers for the first two blocks; the restatement
equals them to the last bit (tests/test_env_law_host.py).

`sweep_run` / `contest_run` / `spawn_run` drive any env with OracleEnv's interface (the oracle, or the device
through tests.hip_adapter.HipEnv) and read only that env's own exported states and step outputs.  The event counts come from
tests/env_state_util.census; `site_events` adds the per-site masks the census sums over and asserts that they sum to it.

Every statistic takes `scale`: the restated probabilities times `scale`.  1.0 is the law; 1.03 is the deliberately wrong law of the
power checks, under which a statistic has to exceed its bar, or the sample was too small to see a 3 % error."""
import itertools

import numpy as np

from tests import env_state_util as U

Z_BAR = 4.0
# scipy.stats.chi2.ppf(0.9999, df) for the degrees of freedom used: 1 / 2 / 4 contestants - 1, 3 rotations, 5 J classes, 7 rank bins,
# 12 / 103 / 206 apple sites of Cleanup default3 / 5 / 10, 119 permutations
CHI2_9999 = {1: 15.136705, 2: 18.420681, 3: 21.107513, 4: 23.512742, 5: 25.744832, 7: 29.877504, 12: 39.134404,
             103: 165.099657, 119: 185.085983, 206: 290.166076}
WRONG = 1.03                    # the power checks' law: every probability times this
TILT = 0.03                     # contests: one contestant at 1 / k + TILT

# ---- the law --------------------------------------------------------------------------------------------------------------------
# cleanup.py:31-54: thresholdDepletion, thresholdRestoration, wasteSpawnProbability, appleRespawnProbability of each map
CLEANUP_CONSTANTS = {"default3": (0.4, 0.0, 0.5, 0.3), "default5": (0.99, 0.0, 0.5, 0.05), "default10": (0.99, 0.0, 0.5, 0.05)}
HARVEST_SPAWN_PROB = (0, 0.05, 0.08, 0.1)           # harvest.py:22
APPLE_RADIUS = 2                                    # harvest.py:8


def cleanup_probabilities(map_name, n_waste, current):
    """(p_apple, p_waste) after compute_probabilities with `current` of the `n_waste` waste sites holding waste (cleanup.py:189-212)"""
    depletion, restoration, waste_prob, apple_prob = CLEANUP_CONSTANTS[map_name]
    waste_density = 0
    if n_waste > 0:
        waste_density = 1 - (n_waste - current) / n_waste
    if waste_density >= depletion:
        return 0.0, 0.0
    if waste_density <= restoration:
        return apple_prob, waste_prob
    return (1 - (waste_density - restoration) / (depletion - restoration)) * apple_prob, waste_prob


def cleanup_tables(map_name, n_waste):
    """(p_apple [n_waste + 1], p_waste [n_waste + 1]) by the waste count"""
    t = np.array([cleanup_probabilities(map_name, n_waste, c) for c in range(n_waste + 1)], np.float64)
    return t[:, 0].copy(), t[:, 1].copy()


def harvest_neighbours(L, grid):
    """[N, n_apple]: for every apple site the number of apples at the offsets (j, k), |j|, |k| <= APPLE_RADIUS, with
    j^2 + k^2 <= APPLE_RADIUS, inside the map (harvest.py:107-116).  grid [N, H * W]"""
    R = APPLE_RADIUS
    a = np.zeros((len(grid), L.H + 2 * R, L.W + 2 * R), np.int64)
    a[:, R:R + L.H, R:R + L.W] = (grid == U.APPLE).reshape(-1, L.H, L.W)
    cnt = np.zeros((len(grid), L.H, L.W), np.int64)
    for j in range(-R, R + 1):
        for k in range(-R, R + 1):
            if j ** 2 + k ** 2 <= APPLE_RADIUS:
                cnt += a[:, R + j:R + j + L.H, R + k:R + k + L.W]
    return cnt.reshape(len(grid), -1)[:, L.apple]


# ---- statistics -----------------------------------------------------------------------------------------------------------------
def z_events(observed, p, weight=1):
    """z of a count against independent events of probability p (array), `weight` events at each p: (O - sum p) / sqrt(sum p (1 - p))"""
    p = np.asarray(p, np.float64)
    e, v = float((weight * p).sum()), float((weight * p * (1 - p)).sum())
    return (float(observed) - e) / np.sqrt(v), e


def chi2_counts(observed, expected, variance=None):
    """sum (O - E)^2 / V over the cells with V > 0 (V = E unless given); a cell with V == 0 has to hold exactly E"""
    o, e = np.asarray(observed, np.float64), np.asarray(expected, np.float64)
    v = e if variance is None else np.asarray(variance, np.float64)
    live = v > 0
    assert (o[~live] == e[~live]).all(), (o[~live], e[~live])
    return float(((o[live] - e[live]) ** 2 / v[live]).sum())


def z_corr(a, b, mask=None):
    """sqrt(R) times the sample correlation of two equally shaped arrays (over the entries of `mask`)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if mask is not None:
        a, b = a[mask], b[mask]
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float(np.sqrt(a.size) * (a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def residual(count, e, v):
    """(count - E) / sqrt(V) where V > 0, else 0; and the mask V > 0"""
    live = v > 0
    return np.where(live, (count - e) / np.sqrt(np.where(live, v, 1.0)), 0.0), live


# ---- runs -----------------------------------------------------------------------------------------------------------------------
STAY = 4
# N is what it takes for every statistic of the case to see a 3 % error (tests/test_env_law_host.py): 4096 where that is enough.
# default10 has 110 waste sites, so 1 env-step in 20 has the <= 5 free sites at which (1 - p)^nfree moves visibly; default3 has 12
# apple sites and 4 waste counts with p > 0, and at least 5 free sites wherever p_waste > 0, which spreads its few waste spawns
# over the rank bins (its map is 10 x 10, so an env costs a fifth of a default5 one).
#         id               env        map          n   seed   step-and-observe with class codes   N
SWEEPS = {"cleanup5":      ("cleanup", "default5",  5,  1105, False, 4096),
          "cleanup10":     ("cleanup", "default10", 10, 1110, False, 16384),
          "cleanup3":      ("cleanup", "default3",  3,  1103, False, 32768),
          "harvest5":      ("harvest", "default10", 5,  1205, False, 4096),
          "cleanup5_code": ("cleanup", "default5",  5,  1305, True,  4096)}
T_EPISODE, EPISODES, EVERY = 20, 2, 8                         # 40 steps per env, the state re-imported every 8
N_CONTEST, CONTESTS = 16384, [(k, earlier) for k in (3, 2, 5) for earlier in (0, 3)]          # one step per env
N_SPAWN, SPAWN_SEED = 8192, 1405


def make_sweep(name, constructor):
    env_name, map_name, n, seed, code, N = SWEEPS[name]
    L = U.shipped(env_name, map_name)
    return constructor(env_name, **law_kwargs(map_name, n, N, seed, T_EPISODE)), L, seed, code


def make_contest(k, earlier, constructor):
    seed = 1500 + 10 * k + earlier
    return constructor("cleanup", **law_kwargs("default5", 5, N_CONTEST, seed, 20)), U.shipped("cleanup", "default5"), seed


def make_spawn(constructor):
    ea = dict(random_spawn_point=True, random_spawn_rotation=None)
    return constructor("cleanup", **law_kwargs("default5", 5, N_SPAWN, SPAWN_SEED, 20, ea)), U.shipped("cleanup", "default5")


def law_kwargs(map_name, n, N, seed, episode_limit, extra_args=None):
    from homophily_marl_amd import abi
    return dict(map=map_name, num_agents=n, n_env=N, view_size=7, episode_limit=episode_limit, extra_args=extra_args,
                rng_mode=abi.RNG_COUNTER, seed=seed, env_id_base=(seed * 31) & 0xFFFF)


def site_events(L, steps, cen):
    """(eligible, grown) bool [S, N, n_apple] and free bool [S, N, n_waste] (the sites the waste draw may choose from): the masks
    whose sums the census reports.  No beam is fired in a law run, so the free sites are the ones without waste before the step."""
    S, N = len(steps), len(steps[0]["pre_grid"])
    elig, grown = np.zeros((S, N, L.n_apple), bool), np.zeros((S, N, L.n_apple), bool)
    free = np.zeros((S, N, L.n_waste), bool)
    rows = np.arange(N)[:, None]
    for s, st in enumerate(steps):
        assert not st["clean_num"].any()
        cells = st["pos"][:, :, 0].astype(np.int64) * L.W + st["pos"][:, :, 1]
        occ = np.zeros(st["pre_grid"].shape, bool)
        occ[rows, cells] = True
        before = st["pre_grid"][:, L.apple] == U.APPLE
        assert not (occ[:, L.apple] & before).any()                    # nobody stands on an apple: nothing is eaten in a law run
        elig[s] = ~before & ~occ[:, L.apple]
        grown[s] = (st["post_grid"][:, L.apple] == U.APPLE) & ~before
        free[s] = st["pre_grid"][:, L.waste] != U.WASTE
    assert (elig.sum(2) == cen["apple_eligible"]).all() and (grown.sum(2) == cen["apple_grown"]).all()
    assert (free.sum(2) == cen["nfree"]).all() and not (grown & ~elig).any()
    return elig, grown, free


def _step(env, acts, code_obs):
    if code_obs:                   # the step-and-observe request with class codes: the instantiation the rollout launches
        from homophily_marl_amd import abi
        return env.step_observe(acts, fmt=abi.OBS_CODE)
    return env.step(acts)


def step_events(L, step):
    """the census of one env step with the per-site masks next to it: dict of arrays [1, N, ...] (census keys, elig, grown, free, and
    for Harvest cls: min(neighbour count, 3) of every apple site, counted on the grid before the step: nobody eats in a law run)"""
    ev = U.census(L, [step])
    ev["elig"], ev["grown"], ev["free"] = site_events(L, [step], ev)
    if L.env == "harvest":
        ev["cls"] = np.minimum(harvest_neighbours(L, step["pre_grid"]), 3).astype(np.int8)[None]
    return ev


def sweep_run(env, L, seed, episodes=2, t_ep=20, every=8, code_obs=False):
    """Every agent stays; the grid is re-imported every `every` steps of each episode: `waste_sweep` with the apples cleared (Cleanup:
    the waste count uniform over 0 .. n_waste, so it does not drift to full), `harvest_sweep` (Harvest: the orchard's density varies
    per env).  Every state is the env's own export; each step is counted as it is made, so no grid outlives it.
    Returns dict(cen, elig, grown, free[, cls], t_ep, episodes)."""
    N, n = env.n_env, env.n
    rng = np.random.default_rng(seed)
    acts = np.full((N, n), STAY, np.int32)
    events = []
    for ep in range(episodes):
        env.reset()
        for t in range(t_ep):
            recount = t % every == 0
            if recount:
                if L.env == "cleanup":
                    grid = U.waste_sweep(N, L, rng)
                    grid[:, L.apple] = U.EMPTY
                else:
                    grid = U.harvest_sweep(N, L, rng)
                env.import_state(grid=grid)
                pre = env.export_state()["grid"]
                assert (pre == grid).all()
            b = _step(env, acts, code_obs)
            so = env.export_state()
            events.append(step_events(L, dict(recount=recount, pre_grid=pre, post_grid=so["grid"], pos=so["pos"],
                                              clean_num=b["clean_num"], n_draws=b["n_draws"])))
            pre = so["grid"]
        assert b["terminated"].all()
    return _gather(events, t_ep, episodes)


def _gather(events, t_ep, episodes):
    cen = {k: np.concatenate([ev[k] for ev in events]) for k in events[0]}
    run = {k: cen.pop(k) for k in ("elig", "grown", "free", "cls") if k in cen}
    return dict(run, cen=cen, t_ep=t_ep, episodes=episodes)


CONTEST_CELL = (4, 9)              # Cleanup default5: an empty cell with four empty neighbours
# (row offset, column offset, action): with every agent facing UP the moves are unrotated (map_env.py:826-829), 0 / 1 = row -/+ 1,
# 2 / 3 = column -/+ 1.  The fifth contestant shares the first one's cell.
CONTESTANTS = [(-1, 0, 1), (1, 0, 0), (0, -1, 3), (0, 1, 2), (-1, 0, 1)]
BYSTANDERS = [(12, 7), (12, 8), (12, 9), (12, 10)]
UP = 2


def contest_run(env, L, k, seed, earlier_steps):
    """k of the 5 agents are imported around CONTEST_CELL and all move into it; the others stay far away.  The step is call index
    1 + earlier_steps of the episode.  The grid is a `waste_sweep` with the apples cleared, so the same call draws apples too.
    Returns dict(winner [N] (index of the contestant), cen, elig, grown, free)."""
    N, n = env.n_env, env.n
    assert n == 5 and 2 <= k <= 5
    rng = np.random.default_rng(seed)
    r0, c0 = CONTEST_CELL
    pos = np.array([(r0 + dr, c0 + dc) for dr, dc, _ in CONTESTANTS[:k]] + BYSTANDERS[:n - k], np.int16)
    acts = np.array([a for _, _, a in CONTESTANTS[:k]] + [STAY] * (n - k), np.int32)
    assert (L.base[[r0 * L.W + c0] + (pos[:, 0].astype(int) * L.W + pos[:, 1]).tolist()] == U.EMPTY).all()
    env.reset()
    for _ in range(earlier_steps):
        env.step(np.full((N, n), STAY, np.int32))
    grid = U.waste_sweep(N, L, rng)
    grid[:, L.apple] = U.EMPTY
    env.import_state(grid=grid, pos=np.tile(pos, (N, 1, 1)), orient=np.full((N, n), UP, np.uint8))
    pre = env.export_state()
    assert (pre["grid"] == grid).all() and (pre["pos"] == pos).all() and (pre["ep_step"] == earlier_steps).all()
    b = env.step(np.tile(acts, (N, 1)))
    so = env.export_state()
    at_cell = (so["pos"][:, :k] == np.array(CONTEST_CELL, np.int16)).all(2)
    assert (at_cell.sum(1) == 1).all(), "every env has exactly one winner"
    stayed = (so["pos"] == pre["pos"]).all(2)
    assert (stayed[:, :k] == ~at_cell).all(), "the losers did not move"
    assert stayed[:, k:].all() and (so["orient"] == UP).all()
    step = dict(recount=True, pre_grid=pre["grid"], post_grid=so["grid"], pos=so["pos"], clean_num=b["clean_num"], n_draws=b["n_draws"])
    return dict(_gather([step_events(L, step)], 1, 1), winner=at_cell.argmax(1))


def spawn_run(env, L, episodes=2):
    """`episodes` consecutive resets under random_spawn_point / random rotation.  Returns (perm [episodes, N]: the lexicographic
    index of the team's placement among the permutations of the spawn points, orient [episodes, N, n])."""
    n, P = env.n, len(L.spawn)
    assert n == P, "the placement is a permutation only with as many agents as points"
    index = {p: i for i, p in enumerate(itertools.permutations(range(P)))}
    perm, orient = [], []
    for _ in range(episodes):
        env.reset()
        s = env.export_state()
        cells = s["pos"][:, :, 0].astype(np.int64) * L.W + s["pos"][:, :, 1]
        assert np.isin(cells, L.spawn).all()
        point = np.searchsorted(L.spawn, cells)
        perm.append(np.array([index[tuple(row)] for row in point.tolist()]))           # KeyError: two agents on one point
        orient.append(s["orient"].astype(np.int64))
    return np.stack(perm), np.stack(orient)


# ---- the statistics of the table (A .. F) ---------------------------------------------------------------------------------------
def _tables(map_name, L, scale):
    pa, pw = cleanup_tables(map_name, L.n_waste)
    return pa * scale, pw * scale


def strata_of(count, weight, parts=5):
    """Stratum 0 .. parts - 1 of every entry of `count` (waste counts, so waste densities): quintiles of the waste density over the
    expected events `weight`, so that every stratum sees the same share of them.  A count goes where the midpoint of its share
    falls; a stratum may stay empty when few counts carry the events (default3 has four counts with p_apple > 0)."""
    values = np.unique(count)
    w = np.array([weight[count == v].sum() for v in values], np.float64)
    mid = (np.cumsum(w) - w / 2) / w.sum()
    which = np.minimum((mid * parts).astype(np.int64), parts - 1)
    return which[np.searchsorted(values, count)]


def apple_statistics(map_name, L, run, scale=1.0):
    """A: dict(pooled z, expected, eligible, grown, strata [(z, expected)], site chi2, df)"""
    pa, _ = _tables(map_name, L, scale)
    cen = run["cen"]
    p = pa[cen["waste_lookup"]]                                          # [S, N]
    n_el, n_gr = cen["apple_eligible"], cen["apple_grown"]
    assert (n_gr[p == 0] == 0).all()
    z, e = z_events(n_gr.sum(), p, n_el)
    true_pa = cleanup_tables(map_name, L.n_waste)[0][cen["waste_lookup"]]
    stratum = strata_of(cen["waste_lookup"], n_el * true_pa)             # the strata are the law's, whatever is tested against
    strata = []
    for q in range(5):
        m = (stratum == q) & (p > 0)
        if m.any():
            strata.append((q,) + z_events(n_gr[m].sum(), p[m], n_el[m]))
    e_s, v_s = np.zeros(L.n_apple), np.zeros(L.n_apple)
    for s, el in enumerate(run["elig"]):                                 # step by step: [N, n_apple] doubles at a time
        el = el.astype(np.float64)
        e_s += p[s] @ el
        v_s += (p[s] * (1 - p[s])) @ el
    return dict(z=z, expected=e, eligible=int(n_el.sum()), grown=int(n_gr.sum()), strata=strata,
                site_chi2=chi2_counts(run["grown"].sum((0, 1)), e_s, v_s), df=L.n_apple)


RANK_BINS, J_CLASSES = 8, 6


def tilt_lowest(share, tilt):
    """share [bins, ...]: probabilities over the bins (summing to 1, or all 0).  The lowest bin times (1 + tilt), the others scaled
    by one common factor so that the sum stays; where the lowest bin is the only one, nothing can move."""
    if not tilt:
        return share
    rest = share[1:].sum(0)
    some = rest > 0
    low = np.where(some, share[0] * (1 + tilt), share[0])
    return np.concatenate([low[None], share[1:] * np.where(some, (share.sum(0) - low) / np.where(some, rest, 1), 1)])


def waste_statistics(map_name, L, run, scale=1.0, rank_tilt=0.0):
    """B: dict(z of 'no waste spawned', none, expected_none, rank chi2 (8 bins of the spawned site's rank among the free ones),
    J chi2 over {0, 1, 2, 3, 4, >= 5}).  The rank of the site does not depend on p_waste, so `scale` cannot move that statistic; its
    wrong law is `rank_tilt`: the sites of the lowest bin are drawn (1 + rank_tilt) times as often as the law says, the others less."""
    _, pw = _tables(map_name, L, scale)
    cen = run["cen"]
    p, nfree, spawned = pw[cen["waste_lookup"]], cen["nfree"], cen["spawned"] == 1
    none = (1 - p) ** nfree
    z, e = z_events((~spawned).sum(), none)
    # rank of the spawned site among the free sites, in the row-major order of the sites
    site = cen["spawn_site"]
    assert (site[spawned] >= 0).all() and (site[~spawned] == -1).all()
    below = np.cumsum(run["free"], 2) - run["free"]                      # free sites before each site
    rank = np.take_along_axis(below, np.maximum(site, 0)[:, :, None], 2)[:, :, 0]
    assert (rank[spawned] < nfree[spawned]).all() and np.take_along_axis(run["free"], np.maximum(site, 0)[:, :, None], 2)[:, :, 0][spawned].all()
    edges = np.arange(RANK_BINS + 1) * L.n_waste // RANK_BINS
    obs = np.array([((rank >= lo) & (rank < hi) & spawned).sum() for lo, hi in zip(edges[:-1], edges[1:])])
    assert obs.sum() == spawned.sum()
    share = np.stack([np.clip(nfree, lo, hi) - lo for lo, hi in zip(edges[:-1], edges[1:])]) / np.maximum(nfree, 1)   # |bin & [0, nfree)| / nfree
    exp = (tilt_lowest(share, rank_tilt) * (1 - none)).sum((1, 2))
    # J: the index of the successful draw
    J = cen["J"]
    obs_j = np.array([(J == j).sum() for j in range(J_CLASSES - 1)] + [(J >= J_CLASSES - 1).sum()])
    exp_j = [(p * (1 - p) ** j * (nfree > j)).sum() for j in range(J_CLASSES - 1)]
    exp_j.append((((1 - p) ** (J_CLASSES - 1) - none) * (nfree > J_CLASSES - 1)).sum())
    return dict(z=z, none=int((~spawned).sum()), expected_none=e, spawns=int(spawned.sum()),
                rank_chi2=chi2_counts(obs, exp), J_chi2=chi2_counts(obs_j, exp_j))


def harvest_statistics(L, run, scale=1.0):
    """C: dict(z [4] per neighbour class (class 0: nan), eligible [4], grown [4]); the classes are those of the law's own neighbourhood
    (step_events) and have to give the census's counts"""
    cen = run["cen"]
    el = np.array([(run["elig"] & (run["cls"] == c)).sum() for c in range(4)])
    gr = np.array([(run["grown"] & (run["cls"] == c)).sum() for c in range(4)])
    assert (el == cen["class_eligible"].sum((0, 1))).all() and (gr == cen["class_grown"].sum((0, 1))).all(), (el, gr)
    z = [float("nan")] + [z_events(gr[c], np.array([HARVEST_SPAWN_PROB[c] * scale]), el[c])[0] for c in (1, 2, 3)]
    return dict(z=z, eligible=el.tolist(), grown=gr.tolist())


def contest_chi2(winner, k, tilt=0.0):
    """D: chi-square of the winner over the k contestants against 1 / k each (tilt: contestant 0 at 1 / k + tilt)"""
    p = np.full(k, (1 - (1 / k + tilt)) / (k - 1))
    p[0] = 1 / k + tilt
    obs = np.bincount(winner, minlength=k)
    assert len(obs) == k
    return chi2_counts(obs, len(winner) * p), obs.tolist()


def uniform_chi2(values, cells):
    obs = np.bincount(np.asarray(values).ravel(), minlength=cells)
    assert len(obs) == cells
    return chi2_counts(obs, np.full(cells, obs.sum() / cells))


def apple_residual(map_name, L, run):
    """per (step, env): ((grown - E) / sqrt(V), V > 0) of the apple draws, and the same of 'a waste cell spawned'"""
    pa, pw = _tables(map_name, L, 1.0)
    cen = run["cen"]
    p, q = pa[cen["waste_lookup"]], 1 - (1 - pw[cen["waste_lookup"]]) ** cen["nfree"]
    n_el = cen["apple_eligible"]
    return residual(cen["apple_grown"], n_el * p, n_el * p * (1 - p)), residual(cen["spawned"], q, q * (1 - q))


def independence_statistics(map_name, L, run):
    """F on a sweep run: sqrt(R) r of the apple residual between step t and t + 1 of one env (inside an episode), env e and e + 1 at
    one step, episode 1 and episode 2 of one env at equal step, the apple residual against the waste residual of the same call, and
    two single apple draws against the first waste draw of the call"""
    (ra, la), (rw, lw) = apple_residual(map_name, L, run)
    E, T = run["episodes"], run["t_ep"]
    ra4, la4 = ra.reshape(E, T, -1), la.reshape(E, T, -1)
    out = {"step t, t+1": z_corr(ra4[:, :-1], ra4[:, 1:], la4[:, :-1] & la4[:, 1:]),
           "env e, e+1": z_corr(ra[:, :-1], ra[:, 1:], la[:, :-1] & la[:, 1:]),
           "apple, waste": z_corr(ra, rw, la & lw)}
    if E > 1:
        out["episode 1, 2"] = z_corr(ra4[0], ra4[1], la4[0] & la4[1])
    out.update(single_draw_statistics(run["elig"], run["grown"], run["cen"]["J"], la & lw))
    return out


def single_draw_statistics(elig, grown, J, both):
    """Single draws of one call: the first and the last apple draw (the first and the last eligible site of the scan) against the first
    waste draw, which succeeds (J == 0) with p_waste whatever the state.  A draw index used for both would make every grown apple of
    that draw a success of the waste draw (p_apple < p_waste).  `both`: the env-steps with apple draws and waste draws."""
    first, last = elig.argmax(2), elig.shape[2] - 1 - elig[:, :, ::-1].argmax(2)
    out = {}
    for what, site in (("first apple draw, first waste draw", first), ("last apple draw, first waste draw", last)):
        assert np.take_along_axis(elig, site[:, :, None], 2)[:, :, 0][both].all()
        out[what] = z_corr(np.take_along_axis(grown, site[:, :, None], 2)[:, :, 0], J == 0, both)
    return out


# ---- the bars: conditions, not measurements (seeds, N and T are fixed by the callers, so every statistic is a constant) ---------------
def show(tag, what, value, bar, power=False):
    print("%s: %s = %+.2f (%s %.2f)" % (tag, what, value, "wrong law, has to exceed" if power else "bar", bar))


def hold_z(tag, what, z):
    show(tag, "z of " + what, z, Z_BAR)
    assert abs(z) < Z_BAR, (tag, what, z)


def hold_chi2(tag, what, value, df):
    show(tag, "chi2_%d of %s" % (df, what), value, CHI2_9999[df])
    assert value < CHI2_9999[df], (tag, what, value)


def hold_cleanup(tag, map_name, L, run):
    """A, B and the sweep's part of F"""
    a, b = apple_statistics(map_name, L, run), waste_statistics(map_name, L, run)
    print("%s: %d eligible apple draws, %d grown against %.1f; %d waste spawns, %d env-steps without against %.1f"
          % (tag, a["eligible"], a["grown"], a["expected"], b["spawns"], b["none"], b["expected_none"]))
    hold_z(tag, "grown apples, pooled", a["z"])
    for q, z, e in a["strata"]:
        hold_z(tag, "grown apples, waste-density quintile %d (%.0f expected)" % (q + 1, e), z)
    hold_chi2(tag, "grown apples by site", a["site_chi2"], a["df"])
    hold_z(tag, "'no waste spawned'", b["z"])
    hold_chi2(tag, "the spawned site's rank among the free sites", b["rank_chi2"], RANK_BINS - 1)
    hold_chi2(tag, "the successful draw's index J", b["J_chi2"], J_CLASSES - 1)
    for what, z in independence_statistics(map_name, L, run).items():
        hold_z(tag, "residuals, " + what, z)
    return a, b


def hold_harvest(tag, L, run):
    """C"""
    c = harvest_statistics(L, run)
    print("%s: eligible by neighbour class %s, grown %s" % (tag, c["eligible"], c["grown"]))
    assert c["grown"][0] == 0 and c["eligible"][0] > 0, "class 0 never grows"
    for k in (1, 2, 3):
        hold_z(tag, "grown apples, neighbour class %d" % k, c["z"][k])
    return c


def hold_contest(tag, map_name, L, run, k):
    """D (the winner, the losers and the bystanders are asserted by contest_run) and its part of F"""
    value, obs = contest_chi2(run["winner"], k)
    print("%s: wins by contestant %s" % (tag, obs))
    hold_chi2(tag, "the winner over %d contestants" % k, value, k - 1)
    (ra, la), _ = apple_residual(map_name, L, run)
    hold_z(tag, "apple residual against 'contestant 0 wins'", z_corr(ra, (run["winner"] == 0)[None], la))
    return value


def hold_spawns(tag, perm, orient):
    """E"""
    cells = 120
    for ep in range(len(perm)):
        hold_chi2(tag, "the placements of episode %d over the permutations" % (ep + 1), uniform_chi2(perm[ep], cells), cells - 1)
        hold_chi2(tag, "the rotations of episode %d" % (ep + 1), uniform_chi2(orient[ep], 4), 3)
    same = perm[0] == perm[1]
    z, e = z_events(same.sum(), np.array([1 / cells]), same.size)
    print("%s: %d of %d envs drew episode 1's placement again, %.1f expected" % (tag, same.sum(), same.size, e))
    hold_z(tag, "'episode 2 drew episode 1's placement'", z)
    hold_z(tag, "rotation of agent a against agent a + 1", z_corr(orient[:, :, :-1], orient[:, :, 1:]))
    hold_z(tag, "rotation of episode 1 against episode 2", z_corr(orient[0], orient[1]))
