"""CPU suite: the CPU oracle's COUNTER-mode draws against the law of the reference (tests/env_law_util.py), and that law against the
reference's own numbers (tests/golden/env_law.npz).

The device and the oracle are equal bit for bit in COUNTER mode (test_env_domain, test_hip_parity, test_env_states_gpu), so what holds
here at the same seeds, N and T holds for tests/test_env_law_gpu.py before a GPU is involved; that file measures the device's own
exports all the same.  Seeds, N and T are fixed (env_law_util.SWEEPS, CONTESTS, N_*), so every statistic is a constant: the bars are
conditions on it.  |z| < 4 for every binomial count and every sqrt(R) r; the 0.9999 quantile of chi-square for every table.  Every
statistic is printed next to its bar (pytest -s).

    A  Cleanup sweeps: grown apples against sum p_apple(current), pooled, per quintile of the waste density and by site
    B  the same runs: 'no waste spawned' against sum (1 - p)^nfree, the spawned site's rank among the free ones, the index J
    C  Harvest sweep: grown apples by neighbour class 1 / 2 / 3; class 0 never grows
    D  2 / 3 / 5 agents moving into one free cell, at call index 1 and 4: the winner over the contestants
    E  random spawn points and rotations over two resets: the 120 placements, the 4 rotations, the repeat rate
    F  residuals of A across steps, envs and episodes, apples against waste in one call (the residuals, and the first and the last
       apple draw against the first waste draw), apples against the contest's winner

The quintiles of A are taken over the expected grown apples, not over the env-steps (env_law_util.strata_of): p_apple falls to 0 with
the density, so a fifth of the env-steps at the dense end would hold a twentieth of the events and could not see a 3 % error.

Power.  Every binomial and chi-square statistic is evaluated again against a wrong law and has to exceed its bar: every probability
times 1.03 (A-C), one contestant at 1 / k + 0.03 (D).  The rank of the spawned site does not depend on any probability the law
names, so its wrong law is the lowest rank bin drawn 1.03 times as often (env_law_util.tilt_lowest).  Where 4096 envs x 40 steps
cannot see that, the case has more envs (env_law_util.SWEEPS, with the reason), never a coarser wrong law.  The wrong law is applied
to the restated expectation, never to the code under test."""
import numpy as np
import pytest

from tests import env_law_util as W

HOST_SWEEPS = [k for k, v in W.SWEEPS.items() if not v[4]]         # the oracle has no step-and-observe request


def _golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_law.npz"))


def test_the_tabulated_quantiles_are_chi_squares():
    try:
        from scipy import stats
    except ImportError:           # the table stands on its own
        return
    for df, q in W.CHI2_9999.items():
        assert abs(stats.chi2.ppf(0.9999, df) - q) < 1e-5, df
    assert abs(2 * stats.norm.sf(W.Z_BAR) - 6.334e-5) < 1e-7


@pytest.mark.parametrize("map_name", ["default3", "default5", "default10"])
def test_cleanup_probabilities_equal_the_references_at_every_waste_count(map_name):
    z = _golden()
    L = W.U.shipped("cleanup", map_name)
    pa, pw = W.cleanup_tables(map_name, L.n_waste)
    ra, rw = z["cleanup_%s_p_apple" % map_name], z["cleanup_%s_p_waste" % map_name]
    assert ra.dtype == np.float64 and ra.shape == (L.n_waste + 1,) and rw.shape == ra.shape
    assert (pa == ra).all() and (pw == rw).all()                         # exact doubles
    assert ra[0] == W.CLEANUP_CONSTANTS[map_name][3] and ra[-1] == 0 and rw[0] == 0.5 and rw[-1] == 0 and (np.diff(ra) <= 0).all()


def test_harvest_table_and_neighbour_counts_equal_the_references():
    z = _golden()
    L = W.U.shipped("harvest", "default10")
    assert (np.array(W.HARVEST_SPAWN_PROB, np.float64) == z["harvest_spawn_prob"]).all()
    grid, pos, count, klass = z["harvest_grid"], z["harvest_pos"], z["harvest_count"], z["harvest_class"]
    assert grid.shape == (len(grid), L.H * L.W) and count.shape == (len(grid), L.n_apple) and count.max() >= 4
    mine = W.harvest_neighbours(L, grid)
    cells = pos[:, :, 0].astype(np.int64) * L.W + pos[:, :, 1]
    reached = (grid[:, L.apple] != W.U.APPLE) & ~(L.apple[None, :, None] == cells[:, None, :]).any(2)
    assert (reached == (count >= 0)).all() and reached.sum() >= 300
    assert (mine[reached] == count[reached]).all() and (np.minimum(mine, 3)[reached] == klass[reached]).all()
    # the census of tests/env_state_util.py classes by the 3 x 3 block: the same neighbourhood
    block = sum(np.roll(np.roll((grid == W.U.APPLE).reshape(-1, L.H, L.W), j, 1), k, 2) for j in (-1, 0, 1) for k in (-1, 0, 1))
    assert (block.reshape(len(grid), -1)[:, L.apple] == mine).all()


def test_strata_and_statistics_on_hand_made_numbers():
    count = np.array([0, 0, 1, 2, 3, 3])
    assert W.strata_of(count, np.array([1.0, 1.0, 2.0, 2.0, 2.0, 2.0])).tolist() == [0, 0, 1, 2, 4, 4]
    assert W.strata_of(count, np.array([5.0, 5.0, 0.0, 0.0, 0.0, 0.0])).tolist() == [2, 2, 4, 4, 4, 4]
    z, e = W.z_events(30, np.array([0.5, 0.1]), np.array([40, 100]))
    assert e == 30 and z == 0 and W.z_events(34, np.array([0.5]), 64)[0] == 0.5
    assert W.chi2_counts([12, 8, 0], [10, 10, 0]) == 0.8 and W.chi2_counts([12], [10], [4]) == 1.0
    assert abs(W.z_corr([1, 2, 3, 4], [2, 4, 6, 8]) - 2) < 1e-12 and abs(W.z_corr([1, 2, 3, 4, 9], [8, 6, 4, 2, 9], np.arange(5) < 4) + 2) < 1e-12
    # the rank statistic's wrong law: columns are env-steps with 4, 1 and 0 free sites over 4 one-rank bins
    share = np.array([[0.25, 1.0, 0.0], [0.25, 0.0, 0.0], [0.25, 0.0, 0.0], [0.25, 0.0, 0.0]])
    tilted = W.tilt_lowest(share, 0.2)
    assert np.allclose(tilted, [[0.3, 1.0, 0.0], [0.7 / 3, 0.0, 0.0], [0.7 / 3, 0.0, 0.0], [0.7 / 3, 0.0, 0.0]], rtol=0, atol=1e-15)
    assert W.tilt_lowest(share, 0.0) is share
    assert W.contest_chi2(np.array([0, 1, 2, 0, 1, 2]), 3) == (0.0, [2, 2, 2])
    assert abs(W.contest_chi2(np.array([0, 1] * 50), 2, 0.03)[0] - (9 / 53 + 9 / 47)) < 1e-12


def test_a_draw_index_shared_by_apples_and_waste_is_seen():
    """F's single-draw statistics on made-up draws (numpy's generator, no env): 10 eligible sites at p_apple 0.05, 3 free waste sites
    at p_waste 0.5.  With the waste draws on uniforms of their own every z is below the bar; with the first waste draw on the first
    (or the last) apple draw's uniform that pair is far above it and the other pair stays below."""
    rng = np.random.default_rng(5)
    S, N, sites = 4, 4096, 10
    ua, uw = rng.random((S, N, sites)), rng.random((S, N, 3))
    elig, grown, both = np.ones((S, N, sites), bool), ua < 0.05, np.ones((S, N), bool)
    def J(u):
        hit = u < 0.5
        return np.where(hit.any(2), hit.argmax(2), -1)
    for shared, pair in ((None, None), (0, "first apple draw, first waste draw"), (sites - 1, "last apple draw, first waste draw")):
        u = uw.copy()
        if shared is not None:
            u[:, :, 0] = ua[:, :, shared]
        z = W.single_draw_statistics(elig, grown, J(u), both)
        print("first waste draw on apple draw %s: %s" % (shared, z))
        for what, v in z.items():
            assert (abs(v) > 4 * W.Z_BAR) if what == pair else (abs(v) < W.Z_BAR), (shared, what, v)


def _sweep(name):
    from oracle.oracle_py import OracleEnv
    env, L, seed, code = W.make_sweep(name, OracleEnv)
    try:
        return L, W.sweep_run(env, L, seed, W.EPISODES, W.T_EPISODE, W.EVERY, code)
    finally:
        env.close()


def _contest(k, earlier):
    from oracle.oracle_py import OracleEnv
    env, L, seed = W.make_contest(k, earlier, OracleEnv)
    try:
        return L, W.contest_run(env, L, k, seed, earlier)
    finally:
        env.close()


def _exceeds(tag, what, value, bar):
    W.show(tag, what, value, bar, power=True)
    assert abs(value) > bar, (tag, what, value, bar)


@pytest.mark.parametrize("name", [k for k in HOST_SWEEPS if W.SWEEPS[k][0] == "cleanup"])
def test_cleanup_sweep_follows_the_law_and_a_wrong_law_is_seen(name):
    """A, B and the sweep's part of F; then the power of each statistic"""
    L, run = _sweep(name)
    map_name = W.SWEEPS[name][1]
    W.hold_cleanup(name, map_name, L, run)
    assert len(np.unique(run["cen"]["waste_lookup"])) == L.n_waste + 1                 # every entry of the table was drawn at
    a, b = W.apple_statistics(map_name, L, run, W.WRONG), W.waste_statistics(map_name, L, run, W.WRONG, W.TILT)
    how = "p x %.2f" % W.WRONG
    _exceeds(name, "z of grown apples, pooled, " + how, a["z"], W.Z_BAR)
    for q, z, _ in a["strata"]:
        _exceeds(name, "z of grown apples, quintile %d, %s" % (q + 1, how), z, W.Z_BAR)
    _exceeds(name, "chi2 of grown apples by site, " + how, a["site_chi2"], W.CHI2_9999[L.n_apple])
    _exceeds(name, "z of 'no waste spawned', " + how, b["z"], W.Z_BAR)
    _exceeds(name, "chi2 of the rank, lowest bin x %.2f" % (1 + W.TILT), b["rank_chi2"], W.CHI2_9999[W.RANK_BINS - 1])
    _exceeds(name, "chi2 of J, " + how, b["J_chi2"], W.CHI2_9999[W.J_CLASSES - 1])


def test_harvest_sweep_follows_the_law_and_a_wrong_law_is_seen():
    """C"""
    L, run = _sweep("harvest5")
    W.hold_harvest("harvest5", L, run)
    assert len(np.unique(run["cen"]["apple_before"][run["cen"]["recount"]])) == L.n_apple + 1      # every orchard size was imported
    wrong = W.harvest_statistics(L, run, W.WRONG)
    for k in (1, 2, 3):
        _exceeds("harvest5", "z of grown apples, neighbour class %d, p x %.2f" % (k, W.WRONG), wrong["z"][k], W.Z_BAR)


@pytest.mark.parametrize("k,earlier", W.CONTESTS)
def test_a_move_contest_is_won_uniformly_and_a_leaning_one_is_seen(k, earlier):
    """D and its part of F"""
    L, run = _contest(k, earlier)
    tag = "%d contestants at call %d" % (k, earlier + 1)
    W.hold_contest(tag, "default5", L, run, k)
    _exceeds(tag, "chi2 of the winner, contestant 0 at 1 / %d + %.2f" % (k, W.TILT), W.contest_chi2(run["winner"], k, W.TILT)[0],
             W.CHI2_9999[k - 1])


def test_spawn_points_and_rotations_are_uniform_and_episodes_independent():
    """E"""
    from oracle.oracle_py import OracleEnv
    env, L = W.make_spawn(OracleEnv)
    try:
        perm, orient = W.spawn_run(env, L)
    finally:
        env.close()
    W.hold_spawns("spawns", perm, orient)
