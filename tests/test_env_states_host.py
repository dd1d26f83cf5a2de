"""CPU suite: the state builders, layouts, rule-constant override and census of tests/env_state_util.py, and every case of
tests/test_env_states_gpu.py run on the oracle alone against the same census minimums -- so the conditions the GPU cases assert are
known to hold for their seeds before a GPU is involved."""
import numpy as np
import pytest

from homophily_marl_amd.envs import maps
from tests import env_state_util as U

LAYOUTS = {
    "default3": lambda: U.shipped("cleanup", "default3"),
    "default5": lambda: U.shipped("cleanup", "default5"),
    "default10": lambda: U.shipped("cleanup", "default10"),
    "harvest": lambda: U.shipped("harvest", "default10"),
    "apple_256": lambda: U.Layout("cleanup", U.layout_apple_256()),
    "waste_256": lambda: U.Layout("cleanup", U.layout_waste_256()),
    "one_waste": lambda: U.Layout("cleanup", U.layout_one_waste()),
}


def _legal(L, grid):
    ok = L.legal()
    assert ok[np.arange(grid.shape[1])[None, :], grid].all()


def test_custom_layout_site_counts():
    a, w, o = LAYOUTS["apple_256"](), LAYOUTS["waste_256"](), LAYOUTS["one_waste"]()
    assert (a.H, a.W, a.n_apple, a.n_waste) == (22, 24, 256, 0)
    assert (w.H, w.W, w.n_apple, w.n_waste) == (22, 24, 0, 256)
    assert (o.H, o.W, o.n_apple, o.n_waste) == (5, 7, 3, 1) and len(o.spawn) == 2
    for L in (a, w, o):
        border = [i for i in range(L.H * L.W) if i // L.W in (0, L.H - 1) or i % L.W in (0, L.W - 1)]
        assert (L.base[border] == U.WALL).all()


@pytest.mark.parametrize("name", ["default3", "default5", "default10", "waste_256", "one_waste", "apple_256"])
def test_waste_sweep_counts_and_codes(name):
    L = LAYOUTS[name]()
    N = 2 * (L.n_waste + 1) + 3
    grid = U.waste_sweep(N, L, np.random.default_rng(1))
    assert grid.shape == (N, L.H * L.W) and grid.dtype == np.uint8
    assert ((grid == U.WASTE).sum(1) == np.arange(N) % (L.n_waste + 1)).all()
    assert (grid[:, L.waste] != U.WASTE).sum(1).tolist() == ((grid[:, L.waste] == U.RIVER).sum(1)).tolist()
    _legal(L, grid)
    others = np.setdiff1d(np.arange(L.H * L.W), np.concatenate([L.waste, L.apple]))
    assert (grid[:, others] == L.base[others]).all()
    if L.n_apple:
        filled = (grid[:, L.apple] == U.APPLE).mean(1)
        assert filled.min() < 0.2 and filled.max() > 0.8             # the per-env fraction spans sparse to dense


def test_harvest_sweep_counts_and_codes():
    L = LAYOUTS["harvest"]()
    N = 2 * (L.n_apple + 1) + 3
    grid = U.harvest_sweep(N, L, np.random.default_rng(2))
    assert ((grid == U.APPLE).sum(1) == np.arange(N) % (L.n_apple + 1)).all()
    _legal(L, grid)
    others = np.setdiff1d(np.arange(L.H * L.W), L.apple)
    assert (grid[:, others] == L.base[others]).all()


@pytest.mark.parametrize("name,n", [("default10", 10), ("default3", 3)])
def test_orchard_counts_and_agents(name, n):
    L = LAYOUTS[name]()
    grid, pos = U.orchard(37, L, np.random.default_rng(3), n)
    assert ((grid == U.APPLE).sum(1) == L.n_apple).all() and ((grid == U.WASTE).sum(1) == L.n_waste).all()
    _legal(L, grid)
    cells = pos[:, :, 0].astype(np.int64) * L.W + pos[:, :, 1]
    assert pos.dtype == np.int16 and np.isin(cells, L.apple).all() and not np.isin(cells, L.wall).any()
    assert all(len(set(c.tolist())) == n for c in cells)


def test_rule_constants_reach_both_constructors_and_are_restored():
    from homophily_marl_amd.envs.config import make_config
    orig = maps.get_spec
    before = make_config("cleanup", map="default5")[0]
    with U.rule_constants("cleanup", "default5", waste_spawn_prob=0.01, threshold_depletion=1.5):
        cfg, spec = make_config("cleanup", map="default5", ascii_map=U.layout_waste_256())
        assert (cfg.waste_spawn_prob, cfg.threshold_depletion) == (0.01, 1.5) and spec.waste_spawn_prob == 0.01
        assert cfg.apple_respawn_prob == before.apple_respawn_prob                      # the others stay
        assert make_config("cleanup", map="default10")[0].threshold_depletion == 0.99    # and so do the other maps
    assert maps.get_spec is orig
    with pytest.raises(RuntimeError):
        with U.rule_constants("harvest", "default10", harvest_spawn_prob=(0.0, 1.0, 0.0, 1.0)):
            assert tuple(make_config("harvest", map="default10")[0].harvest_spawn_prob) == (0.0, 1.0, 0.0, 1.0)
            raise RuntimeError
    assert maps.get_spec is orig
    assert make_config("cleanup", map="default5")[0].waste_spawn_prob == before.waste_spawn_prob


def test_census_of_a_hand_made_step():
    """One env, 3 x 3 interior: the agent eats, one waste cell is cleaned and another spawns, one apple grows."""
    L = U.Layout("cleanup", ["@@@@@", "@HHB@", "@ PB@", "@  B@", "@@@@@"])
    pre = L.base.copy()
    pre[L.waste[1]] = U.RIVER; pre[L.apple[0]] = U.APPLE                       # waste count 1, apple at (1, 3)
    post = pre.copy()
    post[L.waste[0]] = U.RIVER; post[L.waste[1]] = U.WASTE                     # site 0 cleaned, site 1 spawned
    post[L.apple[0]] = U.EMPTY; post[L.apple[2]] = U.APPLE                     # eaten at (1, 3); (3, 3) grows
    step = dict(recount=True, pre_grid=pre[None], post_grid=post[None], pos=np.array([[[1, 3]]], np.int16),
                clean_num=np.array([[1.0]], np.float32), n_draws=np.array([2 + 2], np.int32))
    cen = U.census(L, [step, dict(step, recount=False)])
    assert cen["recount"][:, 0].tolist() == [True, False]
    for k, v in dict(waste_before=1, waste_lookup=0, apple_before=1, apple_change=0, spawned=1, spawn_site=1, spawn_chunk=0,
                     apple_eligible=2, apple_grown=1, waste_draws=2, nfree=2, J=1).items():
        assert cen[k][0, 0] == v, (k, cen[k][0, 0], v)


@pytest.mark.parametrize("name", list(U.CASES))
def test_case_reaches_its_regime_on_the_oracle(name):
    from oracle.oracle_py import OracleEnv
    orc, = U.make_envs(name, OracleEnv)
    try:
        fig = U.require(name, U.run_case(name, orc))
    finally:
        orc.close()
    print(name, fig)
