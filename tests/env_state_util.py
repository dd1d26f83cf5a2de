"""States of the env step (k_env) that a walk from `reset` never reaches, and the census that proves a run reached them (numpy only).

A rollout that starts at reset and takes 40 random steps keeps the waste count near n_waste, the orchard dense and the one-step
change of the apple count small, so most of the kernel's probability table, both out-of-window branches of its density lookup and
the far end of its waste draw stay unread.  The builders below make such states directly (import_state(grid=...) exists on the
device, in the oracle and in the reference harness), the layouts and the rule-constant override reach what the shipped maps
cannot, and `census` measures, from the ORACLE's side of a run alone, which regime every env-step was in.  `run_case` drives one
case on the oracle, or on the oracle and a device env side by side; `require` asserts the case's census minimums, so a run that
missed its regime fails instead of passing empty.  tests/test_env_states_host.py runs all of it without a GPU.

Overridden rule constants have no counterpart in the reference (its constructors hard-code them per map): those cases pin the
device to the oracle only.
"""
import contextlib
import dataclasses

import numpy as np

from homophily_marl_amd import abi
from homophily_marl_amd.envs import maps
from tests.test_env_domain import ALL, CUSTOM, FORMATS, _place, _text, _walled

EMPTY, WALL, APPLE, WASTE, RIVER, STREAM = 0, 1, 2, 3, 4, 5
CHUNK = 64                     # the kernel deals sites to lanes 64 at a time


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
class Layout:
    """Site lists of a layout by the row-major scan every implementation uses, and the grid `reset` starts from."""

    def __init__(self, env_name, rows):
        rows = [r.decode("ascii") if isinstance(r, bytes) else r for r in rows]
        self.env, self.rows = env_name, rows
        self.H, self.W = len(rows), len(rows[0])
        assert all(len(r) == self.W for r in rows)
        ch = np.frombuffer("".join(rows).encode("ascii"), np.uint8)
        self.chars = ch
        site = lambda c: np.flatnonzero(ch == ord(c))
        self.wall, self.spawn = site("@"), site("P")
        self.apple = site("B") if env_name == "cleanup" else site("A")
        self.waste = site("H") if env_name == "cleanup" else np.zeros(0, np.int64)
        self.n_apple, self.n_waste = len(self.apple), len(self.waste)
        base = np.zeros(self.H * self.W, np.uint8)
        base[self.wall] = WALL
        if env_name == "cleanup":
            base[self.waste] = WASTE; base[site("R")] = RIVER; base[site("S")] = STREAM
        else:
            base[self.apple] = APPLE
        self.base = base

    def legal(self):
        """[H * W, 6] bool: the codes each cell may ever hold (an 'H' site holds waste or, once cleaned, river)."""
        ok = np.zeros((self.H * self.W, 6), bool)
        ok[np.arange(self.H * self.W), self.base] = True
        ok[self.apple, EMPTY] = ok[self.apple, APPLE] = True
        ok[self.waste, RIVER] = True
        return ok


def shipped(env_name, map_name):
    return Layout(env_name, maps.get_spec(env_name, map_name).rows)


def layout_apple_256():
    """22 x 24, 256 'B' sites, no 'H' site: n_waste == 0 (waste density 0 for ever), and a reset that grows a third of 256 apples"""
    return _text(_place(_place(_walled(22, 24), "P", 6, start=3, step=61), "B", 256))


def layout_waste_256():
    """22 x 24, 256 'H' sites, no 'B' site: every draw of a step is a waste draw"""
    return _text(_place(_place(_walled(22, 24), "P", 6, start=3, step=61), "H", 256))


def layout_one_waste():
    """5 x 7 with exactly one 'H' site, two spawn points and three 'B' sites: the waste count is 0 or 1"""
    rows = _place(_walled(5, 7), "H", 1)
    return _text(_place(_place(rows, "P", 2, start=5, step=2), "B", 3, start=9))


# ---- state builders -----------------------------------------------------------------------------------------------------------------
def _as_layout(env_name, layout):
    return layout if isinstance(layout, Layout) else Layout(env_name, layout)


def waste_sweep(N, layout, rng):
    """grid [N, H * W]: env e holds exactly e mod (n_waste + 1) waste cells on randomly chosen 'H' sites, the other 'H' sites are
    cleaned (river), and a per-env random fraction of the apple sites is filled."""
    L = _as_layout("cleanup", layout)
    grid = np.tile(L.base, (N, 1))
    for e in range(N):
        k = e % (L.n_waste + 1)
        grid[e, L.waste] = RIVER
        grid[e, L.waste[rng.permutation(L.n_waste)[:k]]] = WASTE
        grid[e, L.apple] = np.where(rng.random(L.n_apple) < rng.random(), APPLE, EMPTY)
    return grid


def harvest_sweep(N, layout, rng):
    """grid [N, H * W]: env e holds exactly e mod (n_apple + 1) apples on randomly chosen sites"""
    L = _as_layout("harvest", layout)
    grid = np.tile(L.base, (N, 1))
    for e in range(N):
        k = e % (L.n_apple + 1)
        grid[e, L.apple] = EMPTY
        grid[e, L.apple[rng.permutation(L.n_apple)[:k]]] = APPLE
    return grid


def orchard(N, layout, rng, n_agents):
    """(grid [N, H * W], pos [N, n, 2]): every 'B' site holds an apple, every 'H' site waste, the agents stand on distinct 'B' cells"""
    L = _as_layout("cleanup", layout)
    grid = np.tile(L.base, (N, 1))
    grid[:, L.apple] = APPLE
    pos = np.zeros((N, n_agents, 2), np.int16)
    for e in range(N):
        cells = L.apple[rng.permutation(L.n_apple)[:n_agents]]
        pos[e, :, 0], pos[e, :, 1] = cells // L.W, cells % L.W
    return grid, pos


# ---- rule constants -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def rule_constants(env_name, map_name, **over):
    """Override rule constants of one map for every constructor that goes through envs.config.make_config (NativeEnv and OracleEnv
    both do) while the block runs.  Test-side only; the reference has no counterpart."""
    orig = maps.get_spec

    def get_spec(env, name):
        spec = orig(env, name)
        return dataclasses.replace(spec, **over) if (env, name) == (env_name, map_name) else spec

    maps.get_spec = get_spec
    try:
        yield
    finally:
        maps.get_spec = orig


# ---- census -------------------------------------------------------------------------------------------------------------------------
def census(layout, steps):
    """steps: one dict per env step of the ORACLE's run -- recount (bool: import_state was given grid or pos since the previous step,
    so the device recounts its cells; otherwise it carries the counts), pre_grid / post_grid [N, H * W], pos [N, n, 2] after the
    step, clean_num [N, n], n_draws [N].  Returns arrays [S, N] (S steps):
      recount, waste_before, waste_lookup (= before - cleaned: the count the probability table is read at), apple_before,
      apple_change, spawned, spawn_site (-1: none, or a site cleaned and refilled in the same step), spawn_chunk,
      apple_eligible, apple_grown, waste_draws, nfree, J (index of the successful waste draw, -1 without a spawn),
      and for Harvest class_eligible / class_grown [S, N, 4] by neighbour class min(#apples in the 3 x 3 block, 3)."""
    L = layout
    S, N = len(steps), len(steps[0]["pre_grid"])
    out = {k: np.zeros((S, N), np.int64) for k in ("waste_before", "waste_lookup", "apple_before", "apple_change", "spawned",
                                                   "spawn_site", "spawn_chunk", "apple_eligible", "apple_grown", "waste_draws",
                                                   "nfree", "J")}
    out["recount"] = np.zeros((S, N), bool)
    out["class_eligible"] = np.zeros((S, N, 4), np.int64)
    out["class_grown"] = np.zeros((S, N, 4), np.int64)
    rows = np.arange(N)[:, None]
    for s, st in enumerate(steps):
        pre, post = st["pre_grid"], st["post_grid"]
        cells = st["pos"][:, :, 0].astype(np.int64) * L.W + st["pos"][:, :, 1]
        occ = np.zeros(pre.shape, bool)
        occ[rows, cells] = True
        mid = np.where(occ & (pre == APPLE), EMPTY, pre)               # after the move and the consume loop
        w0 = (pre == WASTE).sum(1)
        cleaned = st["clean_num"].sum(1).astype(np.int64)
        look = w0 - cleaned
        spawned = (post == WASTE).sum(1) - look
        assert ((spawned == 0) | (spawned == 1)).all(), (s, np.unique(spawned))
        new = (post[:, L.waste] == WASTE) & (pre[:, L.waste] != WASTE)
        assert (new.sum(1) <= spawned).all(), s
        site = np.where(new.any(1), new.argmax(1), -1) if L.n_waste else np.full(N, -1)
        elig = (mid[:, L.apple] != APPLE) & ~occ[:, L.apple]
        grown = (post[:, L.apple] == APPLE) & (mid[:, L.apple] != APPLE)
        assert not (grown & ~elig).any(), s
        assert ((post == APPLE).sum(1) == (mid == APPLE).sum(1) + grown.sum(1)).all(), s
        wd = st["n_draws"].astype(np.int64) - elig.sum(1)
        nfree = L.n_waste - look
        # the draws end at the first success: J + 1 of them; without one, all nfree free sites were tried, or none was (p ~ 0)
        assert (wd[spawned == 1] >= 1).all() and (wd <= nfree).all(), s
        assert ((wd == 0) | (wd == nfree))[spawned == 0].all(), s
        out["recount"][s] = st["recount"]
        out["waste_before"][s], out["waste_lookup"][s] = w0, look
        out["apple_before"][s] = (pre == APPLE).sum(1)
        out["apple_change"][s] = (post == APPLE).sum(1) - out["apple_before"][s]
        out["spawned"][s], out["spawn_site"][s] = spawned, site
        out["spawn_chunk"][s] = np.where(site >= 0, site // CHUNK, -1)
        out["apple_eligible"][s], out["apple_grown"][s] = elig.sum(1), grown.sum(1)
        out["waste_draws"][s], out["nfree"][s] = wd, nfree
        out["J"][s] = np.where(spawned == 1, wd - 1, -1)
        if L.env == "harvest":
            a = np.zeros((N, L.H + 2, L.W + 2), np.int64)
            a[:, 1:-1, 1:-1] = (mid == APPLE).reshape(N, L.H, L.W)
            cnt = sum(a[:, 1 + j:1 + j + L.H, 1 + k:1 + k + L.W] for j in (-1, 0, 1) for k in (-1, 0, 1)).reshape(N, -1)
            cls = np.minimum(cnt[:, L.apple], 3)
            for c in range(4):
                out["class_eligible"][s, :, c] = (elig & (cls == c)).sum(1)
                out["class_grown"][s, :, c] = (grown & (cls == c)).sum(1)
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    env: str
    map: str
    n: int
    view: int
    builder: str = None            # None: run from reset (the first step carries the counts reset wrote)
    layout: list = None            # rows of a custom layout, None: the map's own
    moves_only: bool = False       # actions from the four moves, otherwise from all of them
    constants: dict = None         # rule constants overridden for both constructors (device against oracle only)
    N: int = 258
    T: int = 40
    episodes: int = 1

    def the_layout(self):
        return Layout(self.env, self.layout) if self.layout is not None else shipped(self.env, self.map)


_H256 = dict(env="cleanup", map="default5", n=2, view=7, builder="waste_sweep", layout=layout_waste_256())
CASES = {
    "tables_default3": Case("cleanup", "default3", 3, 7, "waste_sweep"),
    "tables_default5": Case("cleanup", "default5", 5, 7, "waste_sweep"),
    "tables_default10": Case("cleanup", "default10", 10, 7, "waste_sweep", episodes=2),
    "count0_carried": Case("cleanup", "default3", 2, 3, layout=layout_one_waste()),
    "waste_sites_256": Case("cleanup", "default5", 2, 15, "waste_sweep", layout=CUSTOM["waste_sites_256"][1]),
    "density_fall": Case("cleanup", "default10", 10, 7, "orchard", moves_only=True, T=20),
    "density_rise": Case("cleanup", "default3", 3, 7, layout=layout_apple_256(), T=8, episodes=2),
    "waste_draw_index": Case(**_H256, constants=dict(threshold_depletion=1.5, waste_spawn_prob=0.01)),
    "p_waste_1": Case(**_H256, constants=dict(threshold_depletion=1.5, waste_spawn_prob=1.0), T=16),
    "p_waste_1e-9": Case(**_H256, constants=dict(threshold_depletion=1.5, waste_spawn_prob=1e-9), T=16),
    "p_waste_2e-8": Case(**_H256, constants=dict(threshold_depletion=1.5, waste_spawn_prob=2e-8), T=16),
    "p_apple_1": Case("cleanup", "default5", 5, 7, "waste_sweep", constants=dict(apple_respawn_prob=1.0, threshold_restoration=0.5), T=16),
    "p_apple_0": Case("cleanup", "default5", 5, 7, "waste_sweep", constants=dict(apple_respawn_prob=0.0, threshold_restoration=0.5), T=16),
    "harvest_swept_5v7": Case("harvest", "default10", 5, 7, "harvest_sweep"),
    "harvest_swept_2v15": Case("harvest", "default10", 2, 15, "harvest_sweep"),
    "harvest_p_0101": Case("harvest", "default10", 5, 7, "harvest_sweep", constants=dict(harvest_spawn_prob=(0.0, 1.0, 0.0, 1.0)), T=16),
}


def env_kwargs(name):
    c = CASES[name]
    k = sorted(CASES).index(name)
    kw = dict(map=c.map, num_agents=c.n, n_env=c.N, view_size=c.view, episode_limit=c.T // c.episodes, extra_args=dict(ALL),
              rng_mode=abi.RNG_COUNTER, seed=0x57A7E5 + 977 * k, env_id_base=1000 * k + c.n)
    if c.layout is not None:
        kw["ascii_map"] = c.layout
    return kw


def make_envs(name, *constructors):
    """one env per constructor, all built under the case's rule constants"""
    c = CASES[name]
    with rule_constants(c.env, c.map, **(c.constants or {})):
        return [make(c.env, **env_kwargs(name)) for make in constructors]


def run_case(name, orc, dev=None, compare=None):
    """Drive the case on the oracle (and on `dev` in lockstep, compared through `compare` = (step, obs, state) after every call).
    Returns the census of the oracle's run, with `import_apples` / `import_waste`: the counts of every imported grid."""
    c = CASES[name]
    L = c.the_layout()
    rng = np.random.default_rng(env_kwargs(name)["seed"])
    n_actions = 9 if c.env == "cleanup" else 8
    steps, imp_a, imp_w = [], [], []
    t_ep = c.T // c.episodes
    both = lambda f: [f(x) for x in ((orc, dev) if dev is not None else (orc,))]
    for ep in range(c.episodes):
        r = both(lambda x: x.reset())
        if dev is not None:
            compare[0](("reset", ep), r[1], r[0], keys=("n_draws",))
            compare[2](("reset", ep), dev, orc)
        recount = False
        if c.builder is not None:
            if c.builder == "orchard":
                grid, pos = orchard(c.N, L, rng, c.n)
                both(lambda x: x.import_state(grid=grid, pos=pos))
            else:
                grid = {"waste_sweep": waste_sweep, "harvest_sweep": harvest_sweep}[c.builder](c.N, L, rng)
                both(lambda x: x.import_state(grid=grid))
            imp_a.append((grid == APPLE).sum(1)); imp_w.append((grid == WASTE).sum(1))
            recount = True
            if dev is not None:
                compare[2](("import", ep), dev, orc)
        for t in range(t_ep):
            acts = rng.integers(0, 4 if c.moves_only else n_actions, size=(c.N, c.n)).astype(np.int32)
            pre = orc.export_state()["grid"]
            b = orc.step(acts)
            so = orc.export_state()
            steps.append(dict(recount=recount, pre_grid=pre, post_grid=so["grid"], pos=so["pos"], clean_num=b["clean_num"],
                              n_draws=b["n_draws"]))
            recount = False
            if dev is not None:
                fmt = FORMATS[(ep * t_ep + t) % len(FORMATS)]
                a = dev.step_observe(acts, fmt=fmt)
                compare[0]((ep, t), a, b)
                compare[1]((ep, t, fmt), a, orc.observe(fmt))
                compare[2]((ep, t), dev, orc)
        assert b["terminated"].all(), (name, ep)
    cen = census(L, steps)
    cen["import_apples"] = np.concatenate(imp_a) if imp_a else np.zeros(0, np.int64)
    cen["import_waste"] = np.concatenate(imp_w) if imp_w else np.zeros(0, np.int64)
    return cen


# ---- what each case must have reached ----------------------------------------------------------------------------------------------
def _seen(values, lo, hi):
    """the counts lo..hi missing from values"""
    return sorted(set(range(lo, hi + 1)) - set(np.unique(values).tolist()))


def require(name, cen):
    """Assert the census minimums of the case (conditions, not measurements) and return the figures reached, for the log."""
    c = CASES[name]
    L = c.the_layout()
    rc, carry = cen["recount"], ~cen["recount"]
    spawned = cen["spawned"] == 1
    fig = dict(env_steps=int(rc.size), spawns=int(spawned.sum()))
    if name.startswith("tables_"):
        # the table is read at the count left after the beams; the count before the step is what the device's window is built around
        for key in ("waste_before", "waste_lookup"):
            assert not _seen(cen[key][rc], 0, L.n_waste), (name, key, "recounting", _seen(cen[key][rc], 0, L.n_waste))
            assert not _seen(cen[key][carry], 1, L.n_waste), (name, key, "carrying", _seen(cen[key][carry], 1, L.n_waste))
        fig.update(recount_counts=len(np.unique(cen["waste_lookup"][rc])), carry_counts=len(np.unique(cen["waste_lookup"][carry])))
    elif name == "count0_carried":
        assert L.n_waste == 1 and L.n_apple == 3
        for key in ("waste_before", "waste_lookup"):
            assert not _seen(cen[key][carry], 0, 1), (name, key)
        fig.update(carry_at_0=int((cen["waste_lookup"][carry] == 0).sum()), carry_at_1=int((cen["waste_lookup"][carry] == 1).sum()))
    elif name == "waste_sites_256":
        assert L.n_waste == 256
        per = [int((cen["spawn_chunk"] == ch).sum()) for ch in range(4)]
        assert min(per) >= 500, (name, per)
        assert not _seen(cen["waste_before"][carry], 1, 254), (name, _seen(cen["waste_before"][carry], 1, 254))
        fig.update(spawns_per_chunk=per)
    elif name == "density_fall":
        k = int((cen["apple_change"][carry] <= -9).sum())
        assert k >= 20, (name, k)
        fig.update(carry_fall_ge_9=k, min_change=int(cen["apple_change"][carry].min()))
    elif name == "density_rise":
        assert L.n_waste == 0 and L.n_apple == 256
        assert carry.all()
        k = int((cen["apple_change"] >= 56).sum())
        assert k >= 20, (name, k)
        fig.update(carry_rise_ge_56=k, max_change=int(cen["apple_change"].max()))
    elif name == "waste_draw_index":
        assert L.n_waste == 256 and L.n_apple == 0
        j64, j192 = int((cen["J"] >= 64).sum()), int((cen["J"] >= 192).sum())
        dry = int(((cen["waste_draws"] > 0) & ~spawned).sum())
        assert j64 >= 100 and j192 >= 10 and dry >= 100, (name, j64, j192, dry)
        fig.update(J_ge_64=j64, J_ge_192=j192, draws_without_spawn=dry)
    elif name == "p_waste_1":
        assert spawned.sum() >= 1000 and (cen["J"][spawned] == 0).all(), name
        assert (spawned == (cen["nfree"] > 0)).all(), name
    elif name == "p_waste_1e-9":
        assert (cen["nfree"] > 0).sum() >= 1000 and (cen["waste_draws"] == 0).all() and not spawned.any(), name
    elif name == "p_waste_2e-8":
        tried = cen["nfree"] > 0
        assert tried.sum() >= 1000 and (cen["waste_draws"] == cen["nfree"]).all() and not spawned.any(), name
        fig.update(draws=int(cen["waste_draws"].sum()))
    elif name in ("p_apple_1", "p_apple_0"):
        # threshold_restoration 0.5: wd <= 0.5 takes the flat branch at every count up to n_waste / 2 (wd = 1 - (n - c) / n)
        wd = 1 - (L.n_waste - cen["waste_lookup"]) / L.n_waste
        flat = wd <= 0.5
        for m, tag in ((rc, "recounting"), (carry, "carrying")):
            assert len(np.unique(cen["waste_lookup"][flat & m])) >= 20, (name, tag)
        some = cen["apple_eligible"] > 0
        assert (flat & some).sum() >= 200 and (~flat & some).sum() >= 200, name      # (at 1.0 a flat env is full after one step)
        if name == "p_apple_1":
            assert (cen["apple_grown"] == cen["apple_eligible"])[flat].all() and cen["apple_grown"][flat].sum() >= 1000, name
            sloped = ~flat & (wd < 0.99) & (cen["apple_eligible"] >= 20)
            assert (cen["apple_grown"] < cen["apple_eligible"])[sloped].any() and (cen["apple_grown"] > 0)[sloped].any(), name
        else:
            assert (cen["apple_grown"] == 0).all(), name
        fig.update(flat_counts=len(np.unique(cen["waste_lookup"][flat])), flat_grown=int(cen["apple_grown"][flat].sum()))
    elif name.startswith("harvest_swept"):
        assert L.n_apple >= 57
        assert not _seen(cen["import_apples"], 0, L.n_apple), (name, _seen(cen["import_apples"], 0, L.n_apple))
        el, gr = cen["class_eligible"].sum((0, 1)), cen["class_grown"].sum((0, 1))
        assert (el >= 1000).all() and (gr[1:] >= 500).all() and gr[0] == 0, (name, el.tolist(), gr.tolist())
        fig.update(eligible=el.tolist(), grown=gr.tolist())
    elif name == "harvest_p_0101":
        el, gr = cen["class_eligible"].sum((0, 1)), cen["class_grown"].sum((0, 1))
        assert (el >= 500).all(), (name, el.tolist())
        assert gr[0] == 0 and gr[2] == 0 and gr[1] == el[1] and gr[3] == el[3], (name, el.tolist(), gr.tolist())
        fig.update(eligible=el.tolist(), grown=gr.tolist())
    else:
        raise KeyError(name)
    return fig
