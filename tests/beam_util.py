"""The beams of one env step where they meet: a sequential restatement of the reference's beam rule, states in which the order of
the shooters decides the result, and the census that proves a run reached them (numpy only).

k_env applies the CLEAN beams of a step one shooter after the other (ssd_env.hip, the `fire` loop around clean_beams); the next
shooter sees the map the earlier ones left.  That order is all that separates the result from evaluating every shooter on the
pre-beam map, and a walk of uniform random actions almost never decides it: over 10 320 env-steps from reset a later shooter's
beam crosses a cell an earlier one cleaned 6 to 15 times, and on Cleanup-5 it never cleans a cell behind it.

`trace_beams` restates update_custom_moves / update_map_fire / custom_action of the reference (map_env.py:663-769,
cleanup.py:127-144, harvest.py:79-84) -- written from those, not from the kernel or the C oracle -- and `frame_of` restates
MapEnv._render / get_map_with_agents_beam (map_env.py:381-404, 448-475).  tests/test_env_beams_host.py holds both to the
reference's recordings (tests/golden/render_*.npz) before anything is compared with them.  `trace_all_at_once` is the mutant rule
(every shooter sees the pre-beam map); it exists so that the census can count the env-steps in which the order decides.

`squad` / `squad_harvest` build the states: the team within 1 to 3 cells of a random waste (apple) site, 60 % of the actions CLEAN
(FIRE).  `run_case` drives one case on the oracle, or on the oracle and a device env in lockstep; `beam_census` counts, from the
ORACLE's side of the run and the tracer alone, which beam regimes were reached; `require` asserts the case's minimums, so that a
run that missed a regime fails instead of passing empty.
"""
import dataclasses

import numpy as np

from homophily_marl_amd import abi
from tests.env_state_util import APPLE, EMPTY, RIVER, WALL, WASTE, Layout, shipped
from tests.test_env_domain import ALL, FORMATS, FULL, _place, _text, _walled

FIRE, CLEAN = 7, 8                                   # agent.py:153-154, 207-209 (Harvest has FIRE only)
BEAM_LEN = 5                                         # ACTIONS['FIRE'] (cleanup.py:10-11, harvest.py:11)
DIRS = np.array([[-1, 0], [1, 0], [0, -1], [0, 1]])  # ORIENTATIONS in the order LEFT, RIGHT, UP, DOWN (map_env.py:28-31), as (row, col)
NO_SHOT, R_WALL, R_AGENT, R_WASTE, R_FREE = -1, 0, 1, 2, 3
REASONS = ("wall", "agent", "waste", "free")
K_NONE, K_CLEAN, K_FIRE = 0, 1, 2
CELL_CHARS = " @AHRS"                                # the chars of the cell codes 0..5


# ---- the reference's beam rule ------------------------------------------------------------------------------------------------------
def _trace(pre_grid, pos, orient, actions, H, W, env_kind, sequential):
    pre_grid = np.asarray(pre_grid, np.uint8).reshape(-1, H * W)
    N, n = pre_grid.shape[0], np.asarray(pos).reshape(pre_grid.shape[0], -1, 2).shape[1]
    pos = np.asarray(pos).reshape(N, n, 2).astype(np.int64)
    orient = np.asarray(orient).reshape(N, n).astype(np.int64)
    actions = np.asarray(actions).reshape(N, n).astype(np.int64)
    rows = np.arange(N)
    grid = pre_grid.copy()                                       # world_map: updated after every shooter (map_env.py:670-671)
    occ = np.zeros((N, H * W), bool)                             # self.agent_pos: every agent, the shooter included
    occ[rows[:, None], pos[:, :, 0] * W + pos[:, :, 1]] = True
    out = dict(clean_num=np.zeros((N, n), np.int64), kind=np.zeros((N, n), np.int64),
               reason=np.full((N, n, 3), NO_SHOT, np.int64), stop=np.zeros((N, n, 3), np.int64),
               covered=np.zeros((N, n, 3), np.int64), cells=np.full((N, n, 3, BEAM_LEN), -1, np.int64),
               pass_through=np.zeros(N, np.int64), clean_behind=np.zeros(N, np.int64), waste_under_agent=np.zeros(N, np.int64))
    cleaned_before = np.zeros((N, H * W), bool)                  # cells an earlier shooter of this step cleaned
    for f in range(n):                                           # update_custom_moves: agents in id order (map_env.py:664)
        clean = (actions[:, f] == CLEAN) if env_kind == "cleanup" else np.zeros(N, bool)
        shoot = clean | (actions[:, f] == FIRE)
        out["kind"][:, f] = np.where(clean, K_CLEAN, np.where(shoot, K_FIRE, K_NONE))
        seen = grid if sequential else pre_grid
        d = DIRS[orient[:, f]]                                   # firing_direction
        right = np.stack([-d[:, 1], d[:, 0]], 1)                 # rotate_right: np.dot([[0, -1], [1, 0]], direction)
        starts = (pos[:, f], pos[:, f] + right - d, pos[:, f] - right - d)        # map_env.py:729-730
        updates = np.zeros((N, H * W), bool)
        for b, start in enumerate(starts):
            alive = shoot.copy()
            crossed = np.zeros(N, bool)
            cell_rc = start.copy()
            for k in range(BEAM_LEN):
                cell_rc = cell_rc + d                            # next_cell
                inb = (cell_rc[:, 0] >= 0) & (cell_rc[:, 0] < H) & (cell_rc[:, 1] >= 0) & (cell_rc[:, 1] < W)
                cell = np.where(inb, cell_rc[:, 0] * W + cell_rc[:, 1], 0)
                g = seen[rows, cell]

                def stops(m, reason, covers):
                    out["reason"][m, f, b], out["stop"][m, f, b], out["covered"][m, f, b] = reason, k, k + covers
                    if covers:
                        out["cells"][m, f, b, k] = cell[m]

                wall = alive & (~inb | (g == WALL))              # :736-737, :765-766: neither covered nor updated
                stops(wall, R_WALL, 0)
                alive &= ~wall
                agent = alive & occ[rows, cell]                  # :741-749: covered, updated if in cell_types, then break
                stops(agent, R_AGENT, 1)
                under = agent & clean & (g == WASTE)
                updates[rows[under], cell[under]] = True
                out["waste_under_agent"] += under
                alive &= ~agent
                waste = alive & clean & (g == WASTE)             # :752-760: cell_types = blocking_cells = ['H'] for CLEAN only
                stops(waste, R_WASTE, 1)
                updates[rows[waste], cell[waste]] = True
                out["clean_behind"] += waste & crossed
                alive &= ~waste
                out["cells"][alive, f, b, k] = cell[alive]       # :756: a free cell is covered and the beam goes on
                through = alive & clean & cleaned_before[rows, cell]
                out["pass_through"] += through & ~crossed
                crossed |= through
            out["reason"][alive, f, b], out["stop"][alive, f, b], out["covered"][alive, f, b] = R_FREE, BEAM_LEN, BEAM_LEN
        grid[updates] = RIVER                                    # update_map after the shooter's three beams (:669-671)
        out["clean_num"][:, f] = updates.sum(1)                  # len(updates) (:672-673)
        cleaned_before |= updates
    out["grid"] = grid
    return out


def trace_beams(pre_grid, pos, orient, actions, H, W, env_kind):
    """The beams of one env step, shooter after shooter in id order.  pre_grid [N, H * W] is the map after the move and the consume
    loop, pos [N, n, 2] / orient [N, n] the agents after the move, actions [N, n].  Returns a dict of
      clean_num [N, n], grid [N, H * W] (after the beams, before anything spawns), kind [N, n] (K_NONE / K_CLEAN / K_FIRE),
      reason [N, n, 3] (NO_SHOT, or R_WALL / R_AGENT / R_WASTE / R_FREE), stop [N, n, 3] (index 0..4 of the cell the beam stopped
      at, 5 when it ran free), covered [N, n, 3] (cells the beam covers: up to and including a first agent or waste cell, a wall
      not covered), cells [N, n, 3, 5] (the covered cells, -1 elsewhere), and the events per env
      pass_through (CLEAN beams that ran on over a cell an earlier shooter of the step had cleaned), clean_behind (those that
      then cleaned a cell) and waste_under_agent (waste cells cleaned under an agent)."""
    return _trace(pre_grid, pos, orient, actions, H, W, env_kind, True)


def trace_all_at_once(pre_grid, pos, orient, actions, H, W, env_kind):
    """The MUTANT rule: every shooter traces its beams on the pre-beam map.  Only for counting where the order decides."""
    return _trace(pre_grid, pos, orient, actions, H, W, env_kind, False)


def agent_char(a):
    return str(a + 1)[0]              # world-map arrays are '<U1': agent index 9 writes '10', stored as '1'


def frame_of(post_grid, pos, traces, colours, H, W):
    """u8 [N, H, W, 3]: the map after the step, then the agents in id order (the highest id on a cell wins), then every shooter's
    covered cells in id order, 'C' for a CLEAN beam and 'F' for a FIRE beam; colours {char: rgb}."""
    post_grid = np.asarray(post_grid).reshape(-1, H * W)
    N = post_grid.shape[0]
    pos = np.asarray(pos).reshape(N, -1, 2).astype(np.int64)
    n = pos.shape[1]
    rows = np.arange(N)
    table = [colours[ch] for ch in CELL_CHARS[:6 if "H" in colours else 3]]
    table += [(0, 0, 0)] * (6 - len(table)) + [colours[agent_char(a)] for a in range(n)] + [colours.get("C", (0, 0, 0)), colours["F"]]
    lut = np.array(table, np.uint8)
    cls = post_grid.astype(np.int64)
    for a in range(n):
        cls[rows, pos[:, a, 0] * W + pos[:, a, 1]] = 6 + a
    for f in range(n):
        code = np.where(traces["kind"][:, f] == K_CLEAN, 6 + n, 6 + n + 1)
        for b in range(3):
            for k in range(BEAM_LEN):
                cell = traces["cells"][:, f, b, k]
                m = cell >= 0
                cls[rows[m], cell[m]] = code[m]
    return lut[cls].reshape(N, H, W, 3)


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def _squad(N, L, n, rng, sites, fill):
    grid = np.tile(L.base, (N, 1))
    pos = np.zeros((N, n, 2), np.int16)
    orient = rng.integers(0, 4, (N, n)).astype(np.uint8)
    orient[::4] = orient[::4, :1]                                  # every fourth env: the whole team faces one way
    for e in range(N):
        fill(grid[e])
        r0, c0 = divmod(int(sites[rng.integers(len(sites))]), L.W)
        rad = 1 + e % 3
        a = 0
        while a < n:                                               # shared cells and cells that hold waste are allowed
            r, c = r0 + rng.integers(-rad, rad + 1), c0 + rng.integers(-rad, rad + 1)
            if 0 <= r < L.H and 0 <= c < L.W and L.base[r * L.W + c] != WALL:
                pos[e, a] = r, c
                a += 1
    return grid, pos, orient


def squad(N, layout, n, rng):
    """(grid [N, H * W], pos [N, n, 2], orient [N, n]): a per-env random fraction of the 'H' sites holds waste, the rest is river
    (the apple sites likewise, apples or empty); the agents stand on non-wall cells within 1 + e % 3 cells of a random waste site."""
    def fill(g):
        g[layout.waste] = np.where(rng.random(layout.n_waste) < rng.random(), WASTE, RIVER)
        g[layout.apple] = np.where(rng.random(layout.n_apple) < rng.random(), APPLE, EMPTY)
    return _squad(N, layout, n, rng, layout.waste, fill)


def squad_harvest(N, layout, n, rng):
    """the same around apple sites"""
    def fill(g):
        g[layout.apple] = np.where(rng.random(layout.n_apple) < rng.random(), APPLE, EMPTY)
    return _squad(N, layout, n, rng, layout.apple, fill)


def squad_actions(N, n, n_actions, shot, rng):
    """[N, n] int32: 60 % `shot` over the envs -- 25 %, 60 % and 95 % in turn, so that steps with no shooter and steps with a whole
    team of ten shooting both occur -- otherwise uniform over all actions; the last 8 envs all shoot."""
    p = np.array([0.25, 0.6, 0.95])[(np.arange(N) // 3) % 3][:, None]
    acts = np.where(rng.random((N, n)) < p, shot, rng.integers(0, n_actions, (N, n))).astype(np.int32)
    acts[-8:] = shot
    return acts


def layout_waste_block():
    """13 x 15: wall pillars every 7th interior cell, eight spawn points and ten apple sites among them, and every other interior
    cell an 'H' site -- a waste field 11 deep both ways, so that every beam of a shooter can clean, and a beam of any orientation
    can meet a wall at any index."""
    rows = _place(_walled(13, 15), "@", 20, start=3, step=7)
    _place(rows, "P", 8, start=5, step=13)
    _place(rows, "B", 10, start=2, step=11)
    return _text(_place(rows, "H", 105))


# ---- cases --------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    env: str
    map: str
    n: int
    layout: list = None            # rows of a custom layout, None: the map's own
    three: bool = True             # a shooter that cleans 3 cells is required (on default3 none does: its waste field is too thin)
    low_counts: bool = True        # 0 and 1 shooters are required (rare at n = 10 under the 60 % rule)
    N: int = 258
    T: int = 16
    view: int = 7

    def the_layout(self):
        return Layout(self.env, self.layout) if self.layout is not None else shipped(self.env, self.map)


CASES = {
    "default3_n3": Case("cleanup", "default3", 3, three=False),        # the compile-time team sizes
    "default5_n5": Case("cleanup", "default5", 5),
    "default10_n10": Case("cleanup", "default10", 10, low_counts=False),
    "default5_n4": Case("cleanup", "default5", 4),                     # the run-time instantiation
    "default10_n7": Case("cleanup", "default10", 7),
    "default10_n2": Case("cleanup", "default10", 2),
    "waste_block_n6": Case("cleanup", "default5", 6, layout=layout_waste_block()),
    "harvest_n5": Case("harvest", "default10", 5),
}
CLEANUP_CASES = [k for k, c in CASES.items() if c.env == "cleanup"]
RENDER_CASES = ["default5_n5", "default10_n10", "harvest_n5"]
FULL_COLOUR_CASE = "default5_n4"


def env_kwargs(name, full_colour=False):
    c = CASES[name]
    k = sorted(CASES).index(name)
    kw = dict(map=c.map, num_agents=c.n, n_env=c.N, view_size=c.view, episode_limit=c.T, extra_args=dict(FULL if full_colour else ALL),
              rng_mode=abi.RNG_COUNTER, seed=0xBEA305 + 1009 * k, env_id_base=2000 * k + c.n)
    if c.layout is not None:
        kw["ascii_map"] = c.layout
    return kw


def make_envs(name, *constructors, full_colour=False):
    return [make(CASES[name].env, **env_kwargs(name, full_colour)) for make in constructors]


def eaten(pre, pos, W):
    """pre [N, H * W] with the apples under the agents removed (the consume loop, map_env.py:253-256), and who ate [N, n]: the
    lowest id on a cell."""
    N, n = pos.shape[:2]
    rows = np.arange(N)
    mid = pre.copy()
    ate = np.zeros((N, n), bool)
    for a in range(n):
        cell = pos[:, a, 0].astype(np.int64) * W + pos[:, a, 1]
        ate[:, a] = mid[rows, cell] == APPLE
        mid[rows, cell] = np.where(ate[:, a], EMPTY, mid[rows, cell])
    return mid, ate


def run_case(name, orc, dev=None, compare=None, render=False, full_colour=False):
    """Drive the case on the oracle (and on `dev` in lockstep, compared through `compare` = (step, obs, state) after every call;
    with `render` the device's frame of every env is compared with frame_of after every step).  Returns one dict per env step of
    the ORACLE's run: pre_grid (after the move and the consume loop), pos, orient, actions, post_grid, clean_num, reward, ate and
    the two traces."""
    c = CASES[name]
    L = c.the_layout()
    rng = np.random.default_rng(env_kwargs(name)["seed"])
    n_actions, shot = (9, CLEAN) if c.env == "cleanup" else (8, FIRE)
    build = squad if c.env == "cleanup" else squad_harvest
    fmts = FORMATS[1:] if full_colour else FORMATS                  # class codes exist for the simplified palette only
    both = lambda f: [f(x) for x in ((orc, dev) if dev is not None else (orc,))]
    if render:
        from homophily_marl_amd.utils.replay import full_color_table
        colours = full_color_table(c.env)
        dev.e.set_render(True)
    r = both(lambda x: x.reset())
    if dev is not None:
        compare[0]("reset", r[1], r[0], keys=("n_draws",))
        compare[2]("reset", dev, orc)
    steps = []
    for t in range(c.T):
        if t % 2 == 0:                                              # every second step starts from a squad, the other follows a move
            grid, pos, orient = build(c.N, L, c.n, rng)
            both(lambda x: x.import_state(grid=grid, pos=pos, orient=orient))
            if dev is not None:
                compare[2](("import", t), dev, orc)
        acts = squad_actions(c.N, c.n, n_actions, shot, rng)
        pre = orc.export_state()["grid"]
        b = orc.step(acts)
        so = orc.export_state()
        mid, ate = eaten(pre, so["pos"], L.W)
        args = (mid, so["pos"], so["orient"], acts, L.H, L.W, c.env)
        st = dict(pre_grid=mid, pos=so["pos"], orient=so["orient"], actions=acts, post_grid=so["grid"], clean_num=b["clean_num"],
                  reward=b["reward"], ate=ate, trace=trace_beams(*args), mutant=trace_all_at_once(*args))
        steps.append(st)
        if dev is not None:
            fmt = fmts[(t + t // 4) % len(fmts)]                      # both call shapes meet every format
            if t % 4 < 2:
                a = dev.step_observe(acts, fmt=fmt)
            else:
                a = dev.step(acts)
                a.update(dev.observe(fmt))
            compare[0](t, a, b)
            compare[1]((t, fmt), a, orc.observe(fmt))
            compare[2](t, dev, orc)
            if render:
                got = dev.e.get_frames().cpu().numpy()
                want = frame_of(so["grid"], so["pos"], st["trace"], colours, L.H, L.W)
                bad = np.flatnonzero((got != want).any((1, 2, 3)))
                assert not len(bad), (name, t, "frames", bad[:4].tolist(), np.argwhere((got[bad[0]] != want[bad[0]]).any(-1))[:4].tolist())
    assert b["terminated"].all(), name
    return steps


# ---- census -------------------------------------------------------------------------------------------------------------------------
def against_oracle(L, st, rule="trace"):
    """[N] bool: the env-steps in which the rule (`trace`: sequential, `mutant`: all at once) disagrees with the ORACLE's step --
    in clean_num, or in the waste cells: after the step the oracle's map holds the rule's post-beam waste and at most one more
    cell (the step's waste spawn), and nothing else on the 'H' sites; a Harvest map changes on grown apples only."""
    tr = st[rule]
    bad = (tr["clean_num"] != st["clean_num"]).any(1)
    want, got = tr["grid"] == WASTE, st["post_grid"] == WASTE
    bad |= (want & ~got).any(1) | ((got & ~want).sum(1) > 1)
    other = np.ones(L.H * L.W, bool)
    other[L.apple] = False; other[L.waste] = False
    bad |= (st["post_grid"][:, other] != st["pre_grid"][:, other]).any(1)
    a0, a1 = st["pre_grid"][:, L.apple], st["post_grid"][:, L.apple]
    bad |= ((a0 == APPLE) & (a1 != APPLE)).any(1)
    fires = (st["actions"] == FIRE).astype(np.int64)
    bad |= (st["reward"] != st["ate"].astype(np.int64) - fires).any(1)                # fire_beam: -1 per shot (agent.py:188-190,239-241)
    if L.env == "harvest":
        bad |= (tr["grid"] != st["pre_grid"]).any(1)
    return bad


def beam_census(layout, steps):
    """The figures `require` holds to its minimums, over all env-steps of a run (see run_case)."""
    L = layout
    cen = dict(env_steps=0, oracle_mismatch=0, mutant_mismatch=0, mutant_differs=0, pass_through=0, clean_behind=0, waste_under_agent=0,
               shots=0, stops=np.zeros((4, BEAM_LEN + 1), np.int64), by_beam=np.zeros((3, 4, 4), np.int64),
               shooters=np.zeros(steps[0]["actions"].shape[1] + 1, np.int64), cleaned_by_shot=np.zeros(4, np.int64))
    for st in steps:
        tr, mu = st["trace"], st["mutant"]
        cen["env_steps"] += len(st["actions"])
        cen["oracle_mismatch"] += int(against_oracle(L, st, "trace").sum())
        cen["mutant_mismatch"] += int(against_oracle(L, st, "mutant").sum())
        cen["mutant_differs"] += int(((tr["clean_num"] != mu["clean_num"]).any(1) | (tr["grid"] != mu["grid"]).any(1)).sum())
        for k in ("pass_through", "clean_behind", "waste_under_agent"):
            cen[k] += int(tr[k].sum())
        shot = tr["kind"] != K_NONE
        cen["shots"] += int(shot.sum())
        cen["shooters"] += np.bincount(shot.sum(1), minlength=len(cen["shooters"]))
        cen["cleaned_by_shot"] += np.bincount(tr["clean_num"][tr["kind"] == K_CLEAN], minlength=4)[:4]
        m = tr["reason"] != NO_SHOT
        np.add.at(cen["stops"], (tr["reason"][m], tr["stop"][m]), 1)
        beam = np.broadcast_to(np.arange(3), tr["reason"].shape)
        ori = np.broadcast_to(st["orient"].astype(np.int64)[:, :, None], tr["reason"].shape)
        np.add.at(cen["by_beam"], (beam[m], ori[m], tr["reason"][m]), 1)
    return cen


def require(name, cen):
    """Assert the census minimums of the case (conditions, not measurements) and return the figures reached, for the log.  The wall
    stops per (beam, orientation) are held over the union of the cases: see require_union."""
    c = CASES[name]
    assert cen["env_steps"] == c.N * c.T and cen["oracle_mismatch"] == 0, (name, cen["env_steps"], cen["oracle_mismatch"])
    fig = dict(env_steps=cen["env_steps"], shots=cen["shots"], agent_stops=cen["stops"][R_AGENT, :BEAM_LEN].tolist())
    if c.env == "harvest":
        assert cen["shots"] >= 1000, (name, cen["shots"])
        assert cen["stops"][R_AGENT, :BEAM_LEN].min() >= 1, (name, fig["agent_stops"])
        assert cen["stops"][R_WASTE].sum() == 0 and cen["mutant_differs"] == 0, name       # a FIRE beam stops at no waste, cleans nothing
        return fig
    fig.update(mutant_differs=cen["mutant_differs"], pass_through=cen["pass_through"], clean_behind=cen["clean_behind"],
               waste_under_agent=cen["waste_under_agent"], min_stop_bin=int(cen["stops"][:R_FREE, :BEAM_LEN].min()),
               min_agent_waste_bin=int(cen["by_beam"][:, :, R_AGENT:R_WASTE + 1].min()), wall_bins=cen["by_beam"][:, :, R_WALL].tolist(),
               shooters=cen["shooters"].tolist(), cleaned_by_shot=cen["cleaned_by_shot"].tolist())
    assert cen["mutant_differs"] >= 200 and cen["mutant_mismatch"] >= 200, (name, fig)
    assert cen["pass_through"] >= 200 and cen["clean_behind"] >= 50 and cen["waste_under_agent"] >= 100, (name, fig)
    assert fig["min_stop_bin"] >= 20, (name, cen["stops"].tolist())
    assert fig["min_agent_waste_bin"] >= 50, (name, cen["by_beam"].tolist())
    lo = 0 if c.low_counts else 2
    assert cen["shooters"][lo:].min() >= 20, (name, fig["shooters"])
    assert cen["cleaned_by_shot"][:4 if c.three else 3].min() >= 50, (name, fig["cleaned_by_shot"])
    return fig


def require_union(censuses):
    """Every (beam, orientation) meets a wall at least 50 times over the Cleanup cases together.  On default5 and default10 a centre
    beam fired away from the river meets no wall within five cells; the waste_block layout fills that bin."""
    assert set(censuses) >= set(CLEANUP_CASES)
    walls = sum(censuses[k]["by_beam"][:, :, R_WALL] for k in CLEANUP_CASES)
    assert walls.min() >= 50, walls.tolist()
    return walls.tolist()
