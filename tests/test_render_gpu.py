"""GPU suite: render mode -- the beam record of the step kernels and k_render against the reference's frames
(tests/golden/render_*.npz), render mode against plain mode, frames of a large batch, and replay recording in HipGraphRunner."""
import glob
import json
import os

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from tests import golden_util as GU

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = dict(disable_rotation_action=False, disable_fire_action=False)
F_RGB, C_RGB = (255, 255, 0), (100, 255, 255)


def render_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "render_*.npz")))


def _rep(a, n_env):
    return np.repeat(np.asarray(a)[None], n_env, 0)


@pytest.mark.parametrize("n_env", [1, 7])
@pytest.mark.parametrize("path", render_files(), ids=lambda p: os.path.basename(p)[7:-4])
def test_frames_match_the_reference(path, n_env):
    """Every recorded call replayed in TAPE mode: the frame of every env equals the reference's, reset frames included.  With
    n_env = 7 the second episode's reset is split into two partial resets (env_mask): in between, the reset envs show the fixture's
    reset frame and the others still show their last step's frame, beams included."""
    from tests.hip_adapter import HipEnv, hip_tape
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    n = meta["num_agents"]
    env = HipEnv(meta["env"], map=meta["map"], num_agents=n, n_env=n_env, view_size=meta["view_size"],
                 episode_limit=meta["episode_limit"], extra_args=meta["extra_args"], rng_mode=abi.RNG_TAPE)
    env.e.set_render(True)
    U, Wn = z["uniforms"].shape[1], z["waste_order"].shape[1]
    resets = 0
    for c in range(len(z["kind"])):
        tape = hip_tape(n_env, n, U, Wn, _rep(z["move_order"][c], n_env), _rep(z["uniforms"][c], n_env),
                        _rep(z["waste_order"][c], n_env), _rep(z["spawn_rot"][c], n_env))
        if z["kind"][c] == 0:
            if resets and n_env > 1:
                before = env.e.get_frames().cpu().numpy()
                mask = (np.arange(n_env) % 2).astype(np.uint8)
                env.reset(tape, env_mask=mask)
                mid = env.e.get_frames().cpu().numpy()
                for e in range(n_env):
                    want = z["frames"][c] if mask[e] else before[e]
                    assert (mid[e] == want).all(), (path, c, e, "partial reset")
                env.reset(tape, env_mask=1 - mask)
            else:
                env.reset(tape)
            resets += 1
        else:
            env.import_state(pos=_rep(z["pre_pos"][c], n_env), orient=_rep(z["pre_orient"][c], n_env))
            o = env.step(_rep(z["actions"][c], n_env), tape)
            assert (o["reward"] == z["reward"][c].astype(np.float32)).all(), (path, c)
        fr = env.e.get_frames().cpu().numpy()
        for e in range(n_env):
            assert (fr[e] == z["frames"][c]).all(), (path, c, e, int((fr[e] != z["frames"][c]).any(-1).sum()))
    st = env.export_state()
    assert (st["grid"][0] == z["grid"][-1].reshape(-1)).all()
    env.close()


@pytest.mark.parametrize("name", GU.FUSED_TAPE_RENDER)
def test_frames_match_the_reference_through_step_observe(name):
    """The beam-recording TAPE instantiation of the step-and-observe request (k_env<2, 0, true, 0, true>; the replay above steps
    without observing): every step of the recording as one step_observe in render mode, 5 envs -- frames, rewards and state against the
    reference's recording, the observation of every call (the four formats in turn) against the CPU oracle replaying the same tapes."""
    from oracle.oracle_py import OracleEnv, make_tape
    from tests.hip_adapter import HipEnv, hip_tape
    assert set(GU.FUSED_TAPE_RENDER) <= {os.path.basename(p) for p in render_files()}
    fmts = (abi.OBS_CODE, abi.OBS_F32, abi.OBS_U8, abi.OBS_BF16)
    steps = GU.replay_fused(HipEnv, hip_tape, OracleEnv, lambda *a: make_tape(*a)[0], os.path.join(GOLDEN, name), fmts, render=True)
    assert steps >= 40


@pytest.mark.parametrize("n", [1, 2, 5, 10])
def test_render_mode_changes_no_dynamics(n):
    """COUNTER mode, 258 envs, every action: the render-mode kernels (step and step+observe) against the shipped ones, same seed."""
    from homophily_marl_amd.envs.native import NativeEnv
    kw = dict(map="default5" if n == 5 else "default10", num_agents=n, n_env=258, view_size=7, episode_limit=100,
              extra_args=ALL, rng_mode=abi.RNG_COUNTER, seed=5)
    plain, rend = NativeEnv("cleanup", device=0, **kw), NativeEnv("cleanup", device=0, **kw)
    rend.set_render(True)
    for e in (plain, rend):
        e.reset()
    g = th.Generator().manual_seed(3)
    keys = ("reward", "clean_num", "apple_den", "terminated", "n_draws")
    for t in range(100):
        a = th.randint(0, 9, (258, n), generator=g, dtype=th.int32)
        if t % 3 == 0:
            outs = [dict((k, v.clone()) for k, v in e.step(a).items()) for e in (plain, rend)]
            obs = [e.observe(abi.OBS_CODE)["obs"].clone() for e in (plain, rend)]
        else:
            outs = [dict((k, v.clone()) for k, v in e.step_observe(a, fmt=abi.OBS_U8).items()) for e in (plain, rend)]
            obs = [o["obs"] for o in outs]
        for k in keys:
            assert th.equal(outs[0][k], outs[1][k]), (t, k)
        assert th.equal(obs[0], obs[1]), t
        s0, s1 = plain.export_state(), rend.export_state()
        for k in ("grid", "pos", "orient", "ep_reward"):
            assert th.equal(s0[k], s1[k]), (t, k)
    assert rend.poll_error() == 0 and plain.poll_error() == 0
    plain.close(); rend.close()


def _beam_footprint(r, c, o, H, W):
    """cells of the three beams of an agent at (r, c) with orientation o (LEFT, RIGHT, UP, DOWN), 5 cells each, in order"""
    dr, dc = {0: (-1, 0), 1: (1, 0), 2: (0, -1), 3: (0, 1)}[int(o)]
    rr, rc = -dc, dr
    starts = [(r, c), (r + rr - dr, c + rc - dc), (r - rr - dr, c - rc - dc)]
    return [[(sr + (k + 1) * dr, sc + (k + 1) * dc) for k in range(5)] for sr, sc in starts]


def test_frames_of_4096_envs_are_the_state_plus_straight_beams():
    from homophily_marl_amd.envs.native import NativeEnv
    from homophily_marl_amd.utils.replay import full_color_table, CELL_CHARS
    N, n = 4096, 5
    env = NativeEnv("cleanup", device=0, map="default5", num_agents=n, n_env=N, view_size=7, episode_limit=100, extra_args=ALL,
                    rng_mode=abi.RNG_COUNTER, seed=9)
    env.set_render(True)
    env.reset()
    assert not (env.get_frames() == th.tensor(F_RGB, dtype=th.uint8, device=env.device)).all(-1).any()
    g = th.Generator().manual_seed(1)
    table = full_color_table("cleanup")
    lut = np.zeros((16, 3), np.uint8)
    for i, ch in enumerate(CELL_CHARS):
        lut[i] = table[ch]
    for a in range(9):
        lut[6 + a] = table[str(a + 1)]
    for step in range(12):
        a = th.randint(0, 9, (N, n), generator=g, dtype=th.int32)
        a[::3] = 4                                            # every third env: nobody fires
        env.step(a)
    mask = np.zeros(N, np.uint8); mask[1::6] = 1              # some envs freshly reset
    env.reset(env_mask=mask)
    fr = env.get_frames().cpu().numpy()
    st = {k: v.cpu().numpy() for k, v in env.export_state().items()}
    acts = a.numpy()
    H, W = env.H, env.W
    cls = st["grid"].reshape(N, H, W).astype(np.int64)
    for ag in range(n):                                       # agents in id order: the highest id on a cell wins
        r, c = st["pos"][:, ag, 0].astype(np.int64), st["pos"][:, ag, 1].astype(np.int64)
        cls[np.arange(N), r, c] = 6 + ag
    base = lut[cls]
    is_f = (fr == F_RGB).all(-1)
    is_c = (fr == C_RGB).all(-1)
    beam = is_f | is_c
    assert (fr[~beam] == base[~beam]).all()
    n_fired = 0
    for e in range(N):
        cells = set(map(tuple, np.argwhere(beam[e]).tolist()))
        if mask[e] or e % 3 == 0:
            assert not cells, (e, "no beams")
            continue
        allowed = set()
        for ag in range(n):
            if acts[e, ag] >= 7:
                for run in _beam_footprint(st["pos"][e, ag, 0], st["pos"][e, ag, 1], st["orient"][e, ag], H, W):
                    allowed |= set(run)
        assert cells <= allowed, e
        n_fired += bool(cells)
        firing = [ag for ag in range(n) if acts[e, ag] >= 7]
        if len(firing) == 1:                                  # nothing overwrites: each run is covered from its first cell on
            ag = firing[0]
            for run in _beam_footprint(st["pos"][e, ag, 0], st["pos"][e, ag, 1], st["orient"][e, ag], H, W):
                on = [p in cells for p in run]
                assert on == sorted(on, reverse=True), (e, ag, on)
    assert n_fired > N // 3
    assert env.poll_error() == 0
    env.close()


def test_graph_runner_records_test_episodes_and_keeps_its_graphs(tmp_path):
    """Cleanup-5 x 4096 in render mode through HipGraphRunner: training episodes run the beam-recording k_env inside the captured
    rollout / episode-edge graphs and every rollout replays on the CPU oracle (rewards, clean_num, terminated); a recorded test
    episode of envs [0, 4095] yields T + 1 frames per env equal to get_frames() at the same steps; training then replays its graph."""
    from homophily_marl_amd.run import load_config, setup
    from oracle.oracle_py import OracleEnv
    T, N = 50, 4096
    th.manual_seed(0)
    np.random.seed(0)
    cfg = load_config("cleanup", overrides=dict(
        runner="hip_graph", train_graph=1, steps_per_graph=10, batch_size_run=N, batch_size=16, buffer_size=N, obs_storage="code",
        buffer_cpu_only=False, store_state=False, strict_device_ops=True, local_results_path=str(tmp_path),
        env_args=dict(num_agents=5, map="default5", episode_limit=T, seed=1, view_size=7, is_replay=True, replay_envs=[0, N - 1]),
        use_cuda=True, save_model=False))
    ctx = setup(cfg)
    runner = ctx.runner
    assert runner.env.native.render_on and runner.replay_envs == [0, N - 1]
    orc = OracleEnv("cleanup", map="default5", num_agents=5, n_env=N, view_size=7, episode_limit=T, rng_mode=abi.RNG_COUNTER, seed=1)
    try:
        for it in range(4):
            batch = runner.run(test_mode=False)
            assert it == 0 or runner._graph is not None
            orc.reset()
            acts = batch["actions"].squeeze(-1).cpu().numpy()
            rew, cln = batch["reward"].cpu().numpy(), batch["clean_num"].cpu().numpy()
            term = batch["terminated"][:, :, 0].cpu().numpy()
            for t in range(T):
                o = orc.step(acts[:, t])
                assert (rew[:, t] == o["reward"]).all() and (cln[:, t] == o["clean_num"]).all() and (term[:, t] == o["terminated"]).all(), (it, t)
            ctx.buffer.insert_episode_batch(batch)
        b = runner._bundle
        assert b.graph is not None and b.begin_graph is not None and b.finish_graph is not None
        assert runner.replays == []
        # a recorded test episode, stepped by hand so that the eager frames can be taken at the same steps
        runner.begin_episode(test_mode=True)
        ids = [0, N - 1]
        eager = [runner.env.native.get_frames(ids).cpu()]
        while not runner.step_once():
            eager.append(runner.env.native.get_frames(ids).cpu())
        eager.append(runner.env.native.get_frames(ids).cpu())
        runner.finish_episode()
        assert len(runner.replays) == 1
        rec = runner.replays[0]
        assert rec["frames"].shape == (2, T + 1, runner.env.native.H, runner.env.native.W, 3)
        want = th.stack(eager, 1).numpy()
        assert (rec["frames"] == want).all()
        assert (rec["frames"][:, 1:] != rec["frames"][:, :1]).any()
        assert rec["collective"].shape == (2, T + 1) and (rec["collective"][:, 0] == 0).all()
        # training resumes on its captured graphs
        calls = []
        orig = th.cuda.CUDAGraph.replay
        th.cuda.CUDAGraph.replay = lambda self: (calls.append(1), orig(self))[1]
        try:
            runner.run(test_mode=False)
        finally:
            th.cuda.CUDAGraph.replay = orig
        assert len(calls) >= T // 10
        out = runner.save_replay(str(tmp_path / "rp"))
        d = os.path.join(out, "episode_0", "env_%d" % (N - 1))
        assert sorted(os.listdir(d)) == sorted(["%d.png" % k for k in range(T + 1)] + ["frames.npz", "replay.gif"])
    finally:
        runner.close_env()
