"""GPU suite: the HIP kernels (through the C ABI) against the golden vectors and against the CPU oracle."""
import numpy as np
import pytest

from homophily_marl_amd import abi
from tests import golden_util as GU

pytestmark = pytest.mark.gpu

ALL = dict(disable_rotation_action=False, disable_fire_action=False)
CONFIGS = {
    "cleanup3": dict(env="cleanup", map="default3", num_agents=3, view_size=7),
    "cleanup5": dict(env="cleanup", map="default5", num_agents=5, view_size=7),
    "cleanup10": dict(env="cleanup", map="default10", num_agents=10, view_size=7),
    "harvest5": dict(env="harvest", map="default10", num_agents=5, view_size=15),
    "harvest10": dict(env="harvest", map="default10", num_agents=10, view_size=7),
}


def _hip():
    from tests.hip_adapter import HipEnv, hip_tape
    return HipEnv, hip_tape


@pytest.mark.parametrize("path", GU.traj_files(), ids=lambda p: p.split("traj_")[-1][:-4])
def test_golden_trajectory(path):
    HipEnv, hip_tape = _hip()
    assert GU.replay(HipEnv, hip_tape, path, n_env=1) > 50


def test_golden_trajectory_batched():
    HipEnv, hip_tape = _hip()
    for key in ("cleanup5_cluster", "harvest5_allact"):
        path = [p for p in GU.traj_files() if key in p][0]
        GU.replay(HipEnv, hip_tape, path, n_env=7)      # 7: a partially filled workgroup (4 envs per workgroup)


@pytest.mark.parametrize("name", GU.FUSED_TAPE_TRAJ)
def test_golden_trajectory_through_step_observe(name):
    """The TAPE instantiation of the step-and-observe request (k_env<2, 0, true, 0, false>), which the replays above never launch (they
    step, then observe): the reference's recording with every step as one step_observe, 5 envs (a second, partly filled workgroup),
    the four formats in turn; outputs and state against the recording and the oracle, the observation against the oracle's."""
    from oracle.oracle_py import OracleEnv, make_tape
    HipEnv, hip_tape = _hip()
    path = [p for p in GU.traj_files() if p.endswith(name)][0]
    fmts = (abi.OBS_CODE, abi.OBS_F32, abi.OBS_U8, abi.OBS_BF16)
    assert GU.replay_fused(HipEnv, hip_tape, OracleEnv, lambda *a: make_tape(*a)[0], path, fmts) >= 40


def test_move_kats():
    HipEnv, hip_tape = _hip()
    assert GU.replay_kats(HipEnv, hip_tape) > 2000


def _cluster(rng, grid, N, n, HW_shape):
    H, W = HW_shape
    free = np.argwhere(grid.reshape(H, W) != 1)
    pos = np.zeros((N, n, 2), np.int16)
    for e in range(N):
        c = free[rng.integers(len(free))]
        k = 0
        while k < n:
            p = c + rng.integers(-2, 3, 2)
            if 0 < p[0] < H - 1 and 0 < p[1] < W - 1 and grid.reshape(H, W)[p[0], p[1]] != 1:
                pos[e, k] = p; k += 1
    return pos


def _compare_step(tag, a, b, keys=("reward", "clean_num", "apple_den", "terminated", "n_draws")):
    for k in keys:
        assert (a[k] == b[k]).all(), (tag, k, np.argwhere(a[k] != b[k])[:4].tolist())


def _compare_state(tag, dev, orc):
    sa, sb = dev.export_state(), orc.export_state()
    for k in ("grid", "pos", "orient", "ep_reward", "ep_step", "epoch"):
        assert (sa[k] == sb[k]).all(), (tag, k, np.argwhere(sa[k] != sb[k])[:4].tolist())


OTHER_TEAMS = [("cleanup", 4, "default5", 7), ("cleanup", 7, "default10", 7), ("cleanup", 5, "default5", 7), ("cleanup", 10, "default10", 7),
               ("harvest", 6, "default10", 7)]


@pytest.mark.parametrize("env_name,n,mapname,view", OTHER_TEAMS)
def test_counter_mode_other_team_sizes_and_the_class_code_request(env_name, n, mapname, view):
    """The step kernel has instantiations per team size (3 / 5 / 10 at compile time, anything else at run time) and per observation
    request (class-code windows and f32 planes have their own, everything else takes the all-formats kernel): team sizes that take
    the run-time instantiation, and the fused step + class-code observation the rollout issues, against the oracle every step."""
    from oracle.oracle_py import OracleEnv
    HipEnv, _ = _hip()
    N, T = 130, 24
    kw = dict(map=mapname, num_agents=n, n_env=N, view_size=view, episode_limit=T, rng_mode=abi.RNG_COUNTER, seed=0xBEEF + n, env_id_base=77)
    dev, orc = HipEnv(env_name, **kw), OracleEnv(env_name, **kw)
    rng = np.random.default_rng(n)
    avail = [a for a in range(dev.n_actions) if a not in (5, 6)]
    _compare_step("reset", dev.reset(), orc.reset(), keys=("n_draws",))
    for t in range(T):
        acts = rng.choice(avail, size=(N, n)).astype(np.int32)
        fmt = (abi.OBS_CODE, abi.OBS_F32, abi.OBS_U8)[t % 3]
        a = dev.step_observe(acts, fmt=fmt)
        b = orc.step(acts)
        _compare_step(t, a, b)
        ob = orc.observe(fmt)
        for k in ("obs", "pos", "orient"):
            assert (a[k] == ob[k]).all(), (t, fmt, k)
        _compare_state(t, dev, orc)
    dev.close(); orc.close()


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("opts", [None, dict(ALL, random_spawn_rotation=None, obs_color="full"),
                                  dict(ALL, random_spawn_point=True, random_spawn_rotation=None)], ids=["default", "allact_full", "randspawn"])
def test_counter_mode_vs_oracle(name, opts):
    """Random actions, COUNTER RNG, 258 envs, 2 episodes of 40 steps; everything compared every step."""
    from oracle.oracle_py import OracleEnv
    HipEnv, _ = _hip()
    cfg = CONFIGS[name]
    N, T = 258, 40
    kw = dict(map=cfg["map"], num_agents=cfg["num_agents"], n_env=N, view_size=cfg["view_size"], episode_limit=T,
              extra_args=opts, rng_mode=abi.RNG_COUNTER, seed=0xC0FFEE + len(name), env_id_base=1000)
    dev, orc = HipEnv(cfg["env"], **kw), OracleEnv(cfg["env"], **kw)
    n = cfg["num_agents"]
    rng = np.random.default_rng(len(name))
    avail = list(range(dev.n_actions)) if opts else [a for a in range(dev.n_actions) if a not in (5, 6, 7)]
    simplified = not opts or opts.get("obs_color", "simplified") == "simplified"
    for ep in range(2):
        _compare_step(("reset", ep), dev.reset(), orc.reset(), keys=("n_draws",))
        _compare_state(("reset", ep), dev, orc)
        for t in range(T):
            if t % 9 == 4:   # teleport half of the envs into tight clusters: dense move conflicts
                g = orc.export_state()["grid"][0]
                pos = orc.export_state()["pos"]
                cl = _cluster(rng, g, N, n, (dev.H, dev.W))
                pos[::2] = cl[::2]
                dev.import_state(pos=pos); orc.import_state(pos=pos)
            acts = rng.choice(avail, size=(N, n)).astype(np.int32)
            if t % 3 == 0:
                a = dev.step_observe(acts)
                b = orc.step(acts)
                _compare_step((ep, t), a, b)
                ob = orc.observe(abi.OBS_F32)
                for k in ("obs", "pos", "orient"):
                    assert (a[k] == ob[k]).all(), (ep, t, k)
            else:
                _compare_step((ep, t), dev.step(acts), orc.step(acts))
            _compare_state((ep, t), dev, orc)
            if t % 10 == 5:
                fmts = [abi.OBS_F32, abi.OBS_U8, abi.OBS_BF16] + ([abi.OBS_CODE] if simplified else [])
                for fmt in fmts:
                    a, b = dev.observe(fmt, want_state=True), orc.observe(fmt, want_state=True)
                    for k in ("obs", "state", "pos", "orient"):
                        assert (a[k] == b[k]).all(), (ep, t, fmt, k)
    dev.close(); orc.close()


FULL_SIZE = {   # BASELINE.json configs[1], [2] and [3] at their full env counts and window sizes
    "cleanup5": dict(env="cleanup", map="default5", num_agents=5, view_size=7, n_env=4096),
    "harvest5": dict(env="harvest", map="default10", num_agents=5, view_size=15, n_env=4096),
    "cleanup10": dict(env="cleanup", map="default10", num_agents=10, view_size=7, n_env=8192),
}


@pytest.mark.parametrize("name", list(FULL_SIZE))
def test_full_size_episode_vs_oracle(name):
    """BASELINE.json sizes (4096 x 5 Cleanup, 4096 x 5 Harvest with 31 x 31 windows, 8192 x 10 Cleanup): one full 100-step
    episode, rewards / info scalars / draw counts compared at every step, observations and the whole state every 25 steps."""
    from oracle.oracle_py import OracleEnv
    HipEnv, _ = _hip()
    cfg = FULL_SIZE[name]
    N, n, T = cfg["n_env"], cfg["num_agents"], 100
    kw = dict(map=cfg["map"], num_agents=n, n_env=N, view_size=cfg["view_size"], episode_limit=T, rng_mode=abi.RNG_COUNTER, seed=1)
    dev, orc = HipEnv(cfg["env"], **kw), OracleEnv(cfg["env"], **kw)
    rng = np.random.default_rng(0x5D5D)
    avail = np.array([a for a in range(dev.n_actions) if a not in (5, 6, 7)])     # the shipped action set (no rotation, no FIRE)
    dev.reset(); orc.reset()
    for t in range(T):
        acts = avail[rng.integers(0, len(avail), (N, n))].astype(np.int32)
        a, b = dev.step_observe(acts, fmt=abi.OBS_U8), orc.step(acts)
        _compare_step(t, a, b)
        if t % 25 == 24:
            ob = orc.observe(abi.OBS_U8)
            for k in ("obs", "pos", "orient"):
                assert (a[k] == ob[k]).all(), (t, k)
            _compare_state(t, dev, orc)
    assert a["terminated"].all()
    assert (a["collective_return"] == b["collective_return"]).all() and (a["equality"] == b["equality"]).all()
    # domain invariants that hold for any size (checked on the full batch)
    st = dev.export_state()
    H, W = dev.H, dev.W
    grid = st["grid"].reshape(N, H, W)
    base = np.frombuffer(dev.e.spec.ascii, np.uint8)[:H * W].reshape(H, W)
    assert (grid[:, base == ord("@")] == 1).all()                     # walls stay walls
    if cfg["env"] == "cleanup":
        assert np.isin(grid[:, base == ord("B")], (0, 2)).all()          # apple sites hold ' ' or 'A'
        assert np.isin(grid[:, base == ord("H")], (3, 4)).all()          # waste sites hold 'H' or 'R'
        assert (grid[:, base == ord("R")] == 4).all() and (grid[:, base == ord("S")] == 5).all()
        assert (grid[:, (base == ord(" ")) | (base == ord("P"))] == 0).all()
    else:
        assert np.isin(grid[:, base == ord("A")], (0, 2)).all()          # apples regrow only on the map's apple sites
        assert (grid[:, (base == ord(" ")) | (base == ord("P"))] == 0).all()
    r, c = st["pos"][..., 0].astype(int), st["pos"][..., 1].astype(int)
    assert (base[r, c] != ord("@")).all()                            # nobody stands in a wall
    assert (st["ep_step"] == T).all()
    dev.close(); orc.close()


def test_sharding_reproduces_the_unsharded_job():
    """Env streams are keyed by global env id: 2 shards of 64 == one job of 128 (the multi-GPU decomposition)."""
    HipEnv, _ = _hip()
    kw = dict(map="default5", num_agents=5, view_size=7, episode_limit=30, rng_mode=abi.RNG_COUNTER, seed=5)
    full = HipEnv("cleanup", n_env=128, **kw)
    sh = [HipEnv("cleanup", n_env=64, env_id_base=64 * i, **kw) for i in range(2)]
    rng = np.random.default_rng(3)
    full.reset(); [s.reset() for s in sh]
    for t in range(30):
        acts = rng.integers(0, 9, (128, 5)).astype(np.int32)
        a = full.step_observe(acts)
        for i, s in enumerate(sh):
            b = s.step_observe(acts[64 * i:64 * (i + 1)])
            for k in ("reward", "clean_num", "apple_den", "obs", "terminated"):
                assert (a[k][64 * i:64 * (i + 1)] == b[k]).all(), (t, i, k)
    full.close(); [s.close() for s in sh]


def test_partial_reset_and_error_paths():
    import torch
    HipEnv, _ = _hip()
    e = HipEnv("cleanup", map="default5", num_agents=5, n_env=6, rng_mode=abi.RNG_COUNTER, seed=2)
    e.reset()
    for _ in range(5):
        e.step(np.full((6, 5), 1))
    before = e.export_state()
    mask = np.array([1, 0, 0, 1, 0, 0], np.uint8)
    e.reset(env_mask=mask)
    after = e.export_state()
    assert (after["ep_step"] == np.where(mask, 0, 5)).all()
    assert (after["pos"][1] == before["pos"][1]).all() and (after["pos"][0] != before["pos"][0]).any()
    # invalid action: sticky device-side flag (KeyError in the reference's action_map)
    e.step(np.full((6, 5), 9))
    assert e.e.poll_error() & 1
    assert e.e.poll_error() == 0
    # misaligned obs buffer is rejected on the host
    buf = torch.empty(6 * 5 * 3 * 15 * 15 + 1, dtype=torch.float32, device="cuda")[1:]
    with pytest.raises(abi.SsdError):
        e.e.observe(abi.OBS_F32, out=dict(obs=buf))
    # TAPE mode without a tape
    t = HipEnv("cleanup", map="default5", num_agents=5, n_env=2, rng_mode=abi.RNG_TAPE)
    with pytest.raises(abi.SsdError):
        t.reset()
    with pytest.raises(abi.SsdError):
        HipEnv("cleanup", map="default3", num_agents=5, n_env=2)
    e.close(); t.close()


@pytest.mark.parametrize("fmt,n", [(abi.OBS_F32, 5), (abi.OBS_U8, 3), (abi.OBS_BF16, 5)])
def test_obs_written_into_episode_storage(fmt, n):
    """ssd_obs_out.obs_env_stride / obs_slot_stride: the env kernel places obs at storage[b, ep_step] (ragged 16-byte
    alignment per block: 37 envs, odd block sizes) -- bit-identical to the dense output of the same state."""
    import torch
    from homophily_marl_amd.envs.native import NativeEnv
    N, T = 37, 5
    env = NativeEnv("cleanup", device=0, map="default%d" % n, num_agents=n, n_env=N, view_size=7, episode_limit=50,
                    rng_mode=abi.RNG_COUNTER, seed=11)
    dt = {abi.OBS_F32: torch.float32, abi.OBS_U8: torch.uint8, abi.OBS_BF16: torch.bfloat16}[fmt]
    storage = torch.zeros(N, T + 1, n, 3, 15, 15, dtype=dt, device="cuda")
    bufs = env.storage_obs_buffers(storage, fmt)
    g = torch.Generator().manual_seed(1)
    env.reset()
    env.observe(fmt, out=bufs)
    assert (storage[:, 0] == env.observe(fmt)["obs"]).all()
    for t in range(T - 1):
        acts = torch.randint(0, 9, (N, n), generator=g, dtype=torch.int32).cuda()
        r = env.step_observe(acts, fmt=fmt, out=bufs)
        assert r["obs"] is storage
        dense = env.observe(fmt)["obs"]
        assert (storage[:, t + 1] == dense).all(), t
        assert (storage[:, t + 2:] == 0).all()          # later slots untouched
    assert env.poll_error() == 0
