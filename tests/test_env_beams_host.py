"""CPU suite: the beam tracer, the frame composer, the builders and the census of tests/beam_util.py.

`trace_beams` and `frame_of` are first held to the reference's own recordings (tests/golden/render_*.npz: clean_num, the number of
beam cells and the rendered frame of every step call), so the restatement is pinned to the reference before the device is
compared with it.  Then every case of tests/test_env_beams_gpu.py runs on the oracle alone against the same census minimums, and
the all-at-once mutant rule is shown to fail the comparison the sequential rule passes."""
import glob
import json
import os

import numpy as np
import pytest

from tests import beam_util as B
from tests import env_state_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_RUNS = {}


def render_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "render_*.npz")))


def oracle_run(name):
    """the steps and the census of the case on the oracle, computed once"""
    if name not in _RUNS:
        from oracle.oracle_py import OracleEnv
        orc, = B.make_envs(name, OracleEnv)
        try:
            steps = B.run_case(name, orc)
        finally:
            orc.close()
        _RUNS[name] = steps, B.beam_census(B.CASES[name].the_layout(), steps)
    return _RUNS[name]


# ---- the restatement against the reference's recordings ----------------------------------------------------------------------------
def test_render_fixtures_are_the_four():
    assert [os.path.basename(p)[7:-4] for p in render_files()] == ["cleanup10_allact", "cleanup5_beams", "cleanup5_simplified",
                                                                   "harvest5_fire"]


@pytest.mark.parametrize("path", render_files(), ids=lambda p: os.path.basename(p)[7:-4])
def test_tracer_and_frames_equal_the_reference_recordings(path):
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    colours = dict(zip(json.loads(bytes(z["color_chars"]).decode()), z["color_rgb"]))
    H, W = z["grid"].shape[1:]
    n = meta["num_agents"]
    stops = np.zeros(4, np.int64)
    shots = cleaned = 0
    for c in range(len(z["kind"])):
        if z["kind"][c] == 0:
            continue
        pos = z["pos"][c][None]
        mid, _ = B.eaten(z["grid"][c - 1].reshape(1, -1), pos, W)       # the previous call's map, the eaten apples removed
        tr = B.trace_beams(mid, pos, z["orient"][c][None], z["actions"][c][None], H, W, meta["env"])
        assert (tr["clean_num"][0] == z["clean_num"][c]).all(), (path, c, tr["clean_num"][0].tolist(), z["clean_num"][c].tolist())
        assert tr["covered"][tr["reason"] != B.NO_SHOT].sum() == z["n_beam_cells"][c], (path, c)
        assert ((tr["cells"] >= 0).sum(-1) == tr["covered"]).all(), (path, c)
        frame = B.frame_of(z["grid"][c], pos, tr, colours, H, W)[0]
        assert (frame == z["frames"][c]).all(), (path, c, np.argwhere((frame != z["frames"][c]).any(-1))[:4].tolist())
        # the map after the step: the tracer's, plus what spawned
        waste = tr["grid"][0] == B.WASTE
        got = z["grid"][c].reshape(-1) == B.WASTE
        assert not (waste & ~got).any() and (got & ~waste).sum() <= 1, (path, c)
        m = tr["reason"] != B.NO_SHOT
        stops += np.bincount(tr["reason"][m], minlength=4)
        shots += int((tr["kind"] != B.K_NONE).sum()); cleaned += int(tr["clean_num"].sum())
    assert shots >= 40 and stops[B.R_WALL] and stops[B.R_AGENT] and stops[B.R_FREE], (path, shots, stops.tolist())
    if meta["env"] == "cleanup":
        assert cleaned >= 10 and stops[B.R_WASTE] >= 10, (path, cleaned, stops.tolist())
    assert n == z["pos"].shape[1]


# ---- the tracer on hand-made steps --------------------------------------------------------------------------------------------------
ROWS = ["@@@@@@@@@",
        "@HHHHH B@",
        "@HHHHH P@",
        "@HHHHH P@",
        "@@@@@@@@@"]


def _hand(pos, orient, actions, grid=None):
    L = U.Layout("cleanup", ROWS)
    g = (L.base if grid is None else grid)[None]
    args = (g, np.array([pos], np.int16), np.array([orient], np.uint8), np.array([actions], np.int32), L.H, L.W, "cleanup")
    return L, B.trace_beams(*args), B.trace_all_at_once(*args)


def test_the_second_shooter_sees_what_the_first_left():
    """Two agents in one row face the waste (orientation UP: towards column 0).  Agent 0 at column 7 cleans column 5 of the rows
    beside it; agent 1 at column 6 cleans column 5 of its own row, then its side beams run over the cleaned cells and clean
    column 4.  All at once, its side beams would stop at column 5 and clean it a second time."""
    L, tr, mu = _hand([[2, 7], [2, 6]], [2, 2], [B.CLEAN, B.CLEAN])
    assert tr["clean_num"].tolist() == [[2, 3]] and mu["clean_num"].tolist() == [[2, 3]]
    cell = lambda r, c: r * L.W + c
    assert all(tr["grid"][0, cell(r, c)] == U.RIVER for r, c in ((1, 5), (2, 5), (3, 5), (1, 4), (3, 4)))
    assert (tr["grid"][0] == U.WASTE).sum() == 15 - 5 and (mu["grid"][0] == U.WASTE).sum() == 15 - 3
    assert all(mu["grid"][0, cell(r, 4)] == U.WASTE for r in (1, 2, 3))
    # agent 0: the centre beam stops at agent 1 (index 0), the side beams at the waste in column 5 (index 2)
    assert tr["reason"][0, 0].tolist() == [B.R_AGENT, B.R_WASTE, B.R_WASTE] and tr["stop"][0, 0].tolist() == [0, 2, 2]
    assert tr["covered"][0, 0].tolist() == [1, 3, 3]
    # agent 1: the centre beam finds column 5 still waste, the side beams run over the cleaned cells to column 4
    assert tr["stop"][0, 1].tolist() == [0, 2, 2] and tr["covered"][0, 1].tolist() == [1, 3, 3]
    assert (tr["pass_through"][0], tr["clean_behind"][0], tr["waste_under_agent"][0]) == (2, 2, 0)
    assert mu["stop"][0, 1].tolist() == [0, 1, 1] and mu["pass_through"][0] == 0


def test_waste_under_an_agent_is_cleaned_and_walls_are_not_covered():
    """A side beam that starts in the wall covers nothing; a FIRE beam runs over waste, changes no cell and stops at the wall, which
    it does not cover; waste under an agent is covered, cleaned and counted."""
    L, tr, _ = _hand([[1, 7], [1, 4]], [2, 0], [B.CLEAN, B.FIRE])
    # agent 0 in row 1 faces column 0: the centre beam meets waste at index 1; the beam on its right hand runs in row 2 (it starts a
    # cell further back: index 2), the one on its left in row 0, the wall
    assert tr["reason"][0, 0].tolist() == [B.R_WASTE, B.R_WASTE, B.R_WALL] and tr["stop"][0, 0].tolist() == [1, 2, 0]
    assert tr["covered"][0, 0].tolist() == [2, 3, 0] and tr["clean_num"][0].tolist() == [2, 0]
    # agent 1 faces LEFT (up the rows): the centre beam meets the wall at once, the side beams cover one cell of row 1 each
    assert tr["reason"][0, 1].tolist() == [B.R_WALL] * 3 and tr["stop"][0, 1].tolist() == [0, 1, 1]
    assert tr["covered"][0, 1].tolist() == [0, 1, 1] and tr["cells"][0, 1, 1:, 0].tolist() == [1 * L.W + 3, 1 * L.W + 5]
    assert (tr["grid"][0] == U.WASTE).sum() == 15 - 2 and tr["grid"][0, 1 * L.W + 3] == U.WASTE
    L, tr, _ = _hand([[2, 7], [2, 3]], [2, 2], [B.CLEAN, B.FIRE])
    assert tr["reason"][0, 0, 0] == B.R_WASTE and tr["stop"][0, 0, 0] == 1                         # (2, 5) before the agent at (2, 3)
    L, tr, _ = _hand([[2, 7], [2, 5]], [2, 2], [B.CLEAN, B.FIRE])
    assert tr["reason"][0, 0, 0] == B.R_AGENT and tr["waste_under_agent"][0] == 1 and tr["clean_num"][0].tolist() == [3, 0]
    assert tr["grid"][0, 2 * L.W + 5] == U.RIVER
    # FIRE from (2, 5): four cells over waste to the wall in the centre, five cells free on either side (they start a cell back)
    assert tr["reason"][0, 1].tolist() == [B.R_WALL, B.R_FREE, B.R_FREE] and tr["stop"][0, 1].tolist() == [4, 5, 5]
    assert tr["covered"][0, 1].tolist() == [4, 5, 5] and (tr["grid"][0] == U.WASTE).sum() == 15 - 3


def test_builders():
    L = U.shipped("cleanup", "default10")
    rng = np.random.default_rng(5)
    grid, pos, orient = B.squad(64, L, 10, rng)
    assert grid.dtype == np.uint8 and pos.dtype == np.int16 and orient.dtype == np.uint8
    ok = L.legal()
    assert ok[np.arange(L.H * L.W)[None, :], grid].all()
    cells = pos[:, :, 0].astype(np.int64) * L.W + pos[:, :, 1]
    assert (L.base[cells] != U.WALL).all()
    frac = (grid[:, L.waste] == U.WASTE).mean(1)
    assert frac.min() < 0.2 and frac.max() > 0.8
    assert (orient[::4] == orient[::4, :1]).all() and not (orient[1::4] == orient[1::4, :1]).all()
    spread = pos.max(1) - pos.min(1)
    assert (spread[0::3] <= 2).all() and (spread[1::3] <= 4).all() and (spread <= 6).all() and spread.max() > 4
    assert any(len(set(c.tolist())) < 10 for c in cells) and (grid[np.arange(64)[:, None], cells] == U.WASTE).any()
    acts = B.squad_actions(258, 10, 9, B.CLEAN, rng)
    assert (acts[-8:] == B.CLEAN).all() and 0.6 < (acts[:-8] == B.CLEAN).mean() < 0.7 and set(np.unique(acts)) == set(range(9))
    rate = [(acts[:-8][(np.arange(250) // 3) % 3 == k] == B.CLEAN).mean() for k in range(3)]
    assert rate[0] < 0.4 < rate[1] < 0.75 < rate[2]
    W = U.Layout("cleanup", B.layout_waste_block())
    assert (W.H, W.W, W.n_waste, W.n_apple, len(W.spawn)) == (13, 15, 105, 10, 8)
    held = (W.base == U.WASTE).reshape(W.H, W.W)
    assert held.any(1).sum() >= 3 and held.any(0).sum() >= 3 and (W.base.reshape(W.H, W.W)[1:-1, 1:-1] == U.WALL).sum() == 20


# ---- the cases on the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.CASES))
def test_case_reaches_its_beam_regimes_on_the_oracle(name):
    print(name, B.require(name, oracle_run(name)[1]))


def test_every_beam_of_every_orientation_meets_walls_over_the_cases():
    print(B.require_union({k: oracle_run(k)[1] for k in B.CLEANUP_CASES}))


@pytest.mark.parametrize("name", B.CLEANUP_CASES)
def test_the_all_at_once_rule_fails_the_same_comparison(name):
    """the net can fail: checked against the mutant rule instead of the sequential one, the oracle's run mismatches"""
    steps, cen = oracle_run(name)
    L = B.CASES[name].the_layout()
    assert sum(int(B.against_oracle(L, st, "trace").sum()) for st in steps) == 0
    first = next(t for t, st in enumerate(steps) if B.against_oracle(L, st, "mutant").any())
    assert first <= 1 and cen["mutant_mismatch"] >= 200, (name, first, cen["mutant_mismatch"])
    bad = dict(cen, oracle_mismatch=cen["mutant_mismatch"])
    with pytest.raises(AssertionError):
        B.require(name, bad)
