"""GPU suite: the env kernel (k_env) against the CPU oracle over the whole domain ssd_create accepts, not only the benchmark's
shapes -- every team size 1..10 (3 / 5 / 10 have compile-time instantiations, the others run with NT = 0), windows from 1 x 1 (view 0:
the observation is shorter than one 16-byte vector) to the largest view that fits LDS (above 32 x 32 the gather deals one window row
per pass), env counts that leave the last workgroup partly filled or give every wave live neighbours in LDS, custom layouts at the
map-size and site-list limits, and render mode.  COUNTER RNG; every step compares the step outputs, the observation, positions,
orientations and the whole exported state; HipEnv.close() asserts that the device error bits are 0."""
import numpy as np
import pytest

from homophily_marl_amd import abi

pytestmark = pytest.mark.gpu

ALL = dict(disable_rotation_action=False, disable_fire_action=False)
FULL = dict(ALL, obs_color="full", random_spawn_rotation=None)
FORMATS = (abi.OBS_CODE, abi.OBS_F32, abi.OBS_U8, abi.OBS_BF16)


def _envs(env_name, **kw):
    from oracle.oracle_py import OracleEnv
    from tests.hip_adapter import HipEnv
    return HipEnv(env_name, **kw), OracleEnv(env_name, **kw)


def _compare_step(tag, a, b, keys=("reward", "clean_num", "apple_den", "terminated", "n_draws")):
    for k in keys:
        assert (a[k] == b[k]).all(), (tag, k, np.argwhere(a[k] != b[k])[:4].tolist())


def _compare_state(tag, dev, orc):
    sa, sb = dev.export_state(), orc.export_state()
    for k in ("grid", "pos", "orient", "ep_reward", "ep_step", "epoch"):
        assert (sa[k] == sb[k]).all(), (tag, k, np.argwhere(sa[k] != sb[k])[:4].tolist())


def _compare_obs(tag, a, b, keys=("obs", "pos", "orient")):
    for k in keys:
        assert a[k].shape == b[k].shape, (tag, k, a[k].shape, b[k].shape)
        assert (a[k] == b[k]).all(), (tag, k, np.argwhere(a[k] != b[k])[:4].tolist())


def run_vs_oracle(env_name, n, view, N, T, extra_args=None, render=False, seed=0, **kw):
    """Two episodes of T / 2 steps of random actions through step_observe, the requested format rotating over the four; the device
    against the oracle after every call, one observe(want_state=True) per episode."""
    opts = dict(extra_args or {})
    kw = dict(kw, num_agents=n, n_env=N, view_size=view, episode_limit=T // 2, extra_args=opts, rng_mode=abi.RNG_COUNTER,
              seed=0x5EED00 + 131 * n + 7 * view + seed, env_id_base=N * n + view)
    dev, orc = _envs(env_name, **kw)
    try:
        if render:
            dev.e.set_render(True)
        assert dev.V == orc.V == 2 * view + 1
        full_palette = opts.get("obs_color") == "full"
        fmts = FORMATS[1:] if full_palette else FORMATS                   # class codes exist for the simplified palette only
        every = not opts.get("disable_rotation_action", True)
        avail = list(range(dev.n_actions)) if every else [a for a in range(dev.n_actions) if a not in (5, 6, 7)]
        rng = np.random.default_rng(kw["seed"])
        for ep in range(2):
            _compare_step(("reset", ep), dev.reset(), orc.reset(), keys=("n_draws",))
            _compare_state(("reset", ep), dev, orc)
            for t in range(ep * (T // 2), (ep + 1) * (T // 2)):
                acts = rng.choice(avail, size=(N, n)).astype(np.int32)
                fmt = fmts[t % len(fmts)]
                a, b = dev.step_observe(acts, fmt=fmt), orc.step(acts)
                _compare_step(t, a, b)
                _compare_obs((t, fmt), a, orc.observe(fmt))
                _compare_state(t, dev, orc)
                if t % (T // 2) == T // 4:
                    fmt = fmts[(t + 1) % len(fmts)]
                    _compare_obs((t, fmt, "observe"), dev.observe(fmt, want_state=True), orc.observe(fmt, want_state=True),
                                 keys=("obs", "state", "pos", "orient"))
            assert a["terminated"].all() and b["terminated"].all(), ep
    finally:
        dev.close(); orc.close()


# ---- team sizes x views -------------------------------------------------------------------------------------------------------------
_VMAX = {}


def v_max(env_name, mapname, n):
    """The largest view ssd_create accepts for this map and team size (found by creating, not by restating the LDS formula); the
    next view up must be refused as an invalid configuration."""
    key = (env_name, mapname, n)
    if key not in _VMAX:
        from homophily_marl_amd.envs.native import NativeEnv
        for v in range(31, -1, -1):
            try:
                e = NativeEnv(env_name, device=0, map=mapname, num_agents=n, n_env=1, view_size=v)
            except abi.SsdError:
                continue
            e.close()
            _VMAX[key] = v
            break
    return _VMAX[key]


def _map_of(env_name, n):
    return "default10" if env_name == "harvest" or n > 5 else "default5"


SWEEP = [("cleanup", n) for n in range(1, 11)] + [("harvest", n) for n in (1, 2, 9)]


@pytest.mark.parametrize("env_name,n", SWEEP, ids=["%s%d" % c for c in SWEEP])
def test_team_sizes_and_views(env_name, n):
    """Views {0, 1, 3, 7, 16, v_max(n)}; env counts 1, 4k + 1 and 33; both palettes across the set (the simplified one takes the
    grouped class-code gather)."""
    from homophily_marl_amd.envs.native import NativeEnv
    mapname = _map_of(env_name, n)
    vm = v_max(env_name, mapname, n)
    assert vm >= 16, (env_name, n, vm)
    with pytest.raises(abi.SsdError, match="ssd error -1:"):
        NativeEnv(env_name, device=0, map=mapname, num_agents=n, n_env=1, view_size=vm + 1)
    views = sorted({0, 1, 3, 7, 16, vm})
    for i, view in enumerate(views):
        N = (1, 5, 33, 9)[(i + n) % 4]
        full_palette = (i + n) % 3 == 2 and view != vm
        run_vs_oracle(env_name, n, view, N, 32 if view < 16 else 20, extra_args=FULL if full_palette else ALL, seed=i,
                      map=mapname)


# ---- env counts: many workgroups, every wave with live neighbours in LDS -----------------------------------------------------------
MANY = [(env_name, n, view) for env_name in ("cleanup", "harvest") for n in (1, 2) for view in (7, 15)]


@pytest.mark.parametrize("env_name,n,view", MANY, ids=["%s%d_v%d" % c for c in MANY])
def test_small_teams_in_many_workgroups(env_name, n, view):
    """One- and two-agent envs, 130 / 258 of them: a wave whose class-code gather overran its LDS slice would corrupt a live
    neighbour's grid (the state comparison covers every env every step)."""
    run_vs_oracle(env_name, n, view, 130 if view == 7 else 258, 40, extra_args=ALL, map=_map_of(env_name, n))


# ---- custom layouts (ascii_map: the oracle and the kernel, the reference has no layout argument) ------------------------------------
def _walled(H, W, fill=" "):
    rows = [["@"] * W] + [["@"] + [fill] * (W - 2) + ["@"] for _ in range(H - 2)] + [["@"] * W]
    return rows


def _place(rows, ch, k, start=0, step=1):
    """k cells of ch on interior blanks, row-major from the start-th blank, every step-th"""
    cells = [(r, c) for r in range(len(rows)) for c in range(len(rows[0])) if rows[r][c] == " "][start::step]
    assert len(cells) >= k
    for r, c in cells[:k]:
        rows[r][c] = ch
    return rows


def _text(rows):
    return ["".join(r) for r in rows]


def _sites_map(env_name, sites):
    """22 x 24: `sites` apple (Harvest) or waste (Cleanup) sites, spread over the interior, plus spawn points (and apple, river and
    stream cells on Cleanup)"""
    rows = _walled(22, 24)
    _place(rows, "P", 6, start=3, step=61)
    _place(rows, "A" if env_name == "harvest" else "H", sites)
    if env_name == "cleanup":
        _place(rows, "B", 40); _place(rows, "R", 6); _place(rows, "S", 4)
    return _text(rows)


CUSTOM = {
    "smallest": ("cleanup", ["@@@", "@P@", "@@@"], 1, 7),
    "smallest_harvest": ("harvest", ["@@@", "@P@", "@@@"], 1, 3),
    "tall_3wide": ("cleanup", _text(_place(_place(_place(_walled(120, 3), "P", 4, step=29), "H", 30, step=3), "B", 20)), 4, 5),
    "wide_3high": ("harvest", _text(_place(_place(_walled(3, 255), "P", 2, step=97), "A", 120, step=2)), 2, 9),
    "cells_1024": ("cleanup", _text(_place(_place(_place(_walled(32, 32), "P", 5, step=151), "H", 120, step=5), "B", 150, step=3)), 5, 7),
    "cells_1023": ("harvest", _text(_place(_place(_walled(31, 33), "P", 3, step=200), "A", 200, step=3)), 3, 16),
    "apple_sites_256": ("harvest", _sites_map("harvest", 256), 6, 7),
    "waste_sites_256": ("cleanup", _sites_map("cleanup", 256), 2, 15),
}


@pytest.mark.parametrize("name", list(CUSTOM))
def test_custom_layouts(name):
    """The smallest legal map (3 x 3, one spawn cell), a 3-wide tall and a 3-high wide one, 1024 cells (the limit; 32 x 32) and 1023
    cells (31 x 33: a cell count that is not a multiple of 4), and the site-list limit of 256 apple / waste sites."""
    env_name, rows, n, view = CUSTOM[name]
    H, W = len(rows), len(rows[0])
    assert H * W <= 1024 and min(H, W) >= 3
    if name.startswith("cells_"):
        assert H * W == int(name[6:])
    if name.endswith("_256"):
        assert sum(r.count("A" if env_name == "harvest" else "H") for r in rows) == 256
    for N, opts in ((5, ALL), (66, FULL)):
        run_vs_oracle(env_name, n, view, N, 32, extra_args=opts, map=_map_of(env_name, 1), ascii_map=rows)


def test_layouts_past_the_limits_are_refused():
    """1025 cells, 257 apple sites (Harvest) and 257 waste sites (Cleanup): an invalid configuration, on the device and in the oracle."""
    from homophily_marl_amd.envs.native import NativeEnv
    from oracle.oracle_py import OracleEnv
    big = _text(_place(_walled(25, 41), "P", 2))
    assert len(big) * len(big[0]) == 1025
    bad = [("cleanup", big), ("harvest", _sites_map("harvest", 257)), ("cleanup", _sites_map("cleanup", 257))]
    for env_name, rows in bad:
        with pytest.raises(abi.SsdError, match="ssd error -1:"):
            NativeEnv(env_name, device=0, map=_map_of(env_name, 1), num_agents=1, n_env=4, ascii_map=rows)
        with pytest.raises(abi.SsdError, match="ssd error -1:"):
            OracleEnv(env_name, map=_map_of(env_name, 1), num_agents=1, n_env=4, ascii_map=rows)
    # and the last legal size of each is accepted (the refusals are the limits, not the layouts)
    for env_name, rows in (("harvest", _sites_map("harvest", 256)), ("cleanup", _sites_map("cleanup", 256))):
        NativeEnv(env_name, device=0, map=_map_of(env_name, 1), num_agents=1, n_env=4, ascii_map=rows).close()


# ---- render mode at a large window -------------------------------------------------------------------------------------------------
RENDER_VIEWS = [(1, 20), (2, 16)]


@pytest.mark.parametrize("n,view", RENDER_VIEWS)
def test_render_mode_at_large_views(n, view):
    """Render mode runs the run-time team size for every team but 5, and every observation format: its observations still match
    the oracle above 32 x 32 windows."""
    run_vs_oracle("cleanup", n, view, 130, 32, extra_args=ALL, render=True, map="default10")
