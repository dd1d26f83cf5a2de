"""CPU suite: replay rendering -- the render fixtures (tests/golden/render_*.npz, generated from the reference by
tools/gen_render_golden.py), the package's full-colour table, the replay writer and the save_replay path of run_sequential."""
import glob
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CELL_CHARS = " @AHRS"


def render_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "render_*.npz")))


def load(path):
    z = np.load(path)
    return z, json.loads(bytes(z["meta"]).decode()), dict(zip(json.loads(bytes(z["color_chars"]).decode()), z["color_rgb"]))


def agent_char(a):
    return str(a + 1)[0]        # '<U1' truncation: agent index 9 writes '10', stored as '1'


def map_to_colors(grid, pos, color_map):
    """numpy restatement of map_to_colors(get_map_with_agents(), color_map) (no beams)."""
    chars = np.array(list(CELL_CHARS))[grid]
    for a, (r, c) in enumerate(pos):
        chars[r, c] = agent_char(a)
    out = np.zeros(grid.shape + (3,), np.uint8)
    for ch, rgb in color_map.items():
        out[chars == ch] = rgb
    return out


def test_render_fixtures_exist():
    names = {os.path.basename(p) for p in render_files()}
    assert {"render_cleanup5_beams.npz", "render_harvest5_fire.npz", "render_cleanup10_allact.npz",
            "render_cleanup5_simplified.npz"} <= names


@pytest.mark.parametrize("path", render_files(), ids=lambda p: os.path.basename(p)[7:-4])
def test_fixture_frames_are_the_map_agents_and_beams(path):
    z, meta, cm = load(path)
    beam = [np.array(cm["F"])] + ([np.array(cm["C"])] if "C" in cm else [])
    n_beam = 0
    for c in range(len(z["kind"])):
        f = z["frames"][c]
        base = map_to_colors(z["grid"][c], z["pos"][c], cm)
        is_beam = np.zeros(f.shape[:2], bool)
        for rgb in beam:
            is_beam |= (f == rgb).all(-1)
        assert (f[~is_beam] == base[~is_beam]).all(), (path, c)
        n_beam += int(is_beam.sum())
        if z["kind"][c] == 0:
            assert not is_beam.any(), (path, c, "a reset frame carries no beams")
    assert n_beam > 50                                        # the fixtures do exercise beams
    if meta["num_agents"] == 10:
        assert (z["kind"] == 1).sum() > 0 and "1" in cm      # agent index 9 is drawn with the colour of '1'


@pytest.mark.parametrize("path", render_files(), ids=lambda p: os.path.basename(p)[7:-4])
def test_package_colour_table_is_the_reference_color_map(path):
    from homophily_marl_amd.utils import replay
    z, meta, cm = load(path)
    table = replay.full_color_table(meta["env"])
    for ch, rgb in table.items():
        assert tuple(int(x) for x in cm[ch]) == tuple(rgb), (meta["env"], ch)
    # every char a frame of this env kind can hold (Harvest: no waste / river / stream, no CLEAN beam) is in both tables
    for ch in (CELL_CHARS + "123456789FC" if meta["env"] == "cleanup" else " @A123456789F"):
        assert ch in cm and ch in table, ch
    for i in range(meta["num_agents"]):                       # the legend: color_map[str(i + 1)], untruncated
        assert tuple(int(x) for x in cm[str(i + 1)]) == replay.AGENT_LEGEND_RGB[i]


def test_writer_produces_pngs_npz_and_gif(tmp_path):
    from PIL import Image
    from homophily_marl_amd.utils import replay
    T, n, H, W = 4, 3, 6, 7
    rng = np.random.default_rng(0)
    rec = dict(frames=rng.integers(0, 256, (2, T + 1, H, W, 3)).astype(np.uint8),
               pos=rng.integers(1, 5, (2, T + 1, n, 2)).astype(np.float32),
               actions_inc=rng.integers(0, 3, (2, T + 1, n, n)).astype(np.int32),
               collective=np.cumsum(rng.integers(0, 3, (2, T + 1)), 1).astype(np.float32))
    dirs = replay.write_replay(str(tmp_path), rec, "cleanup", env_ids=[0, 17])
    assert [os.path.basename(d) for d in dirs] == ["env_0", "env_17"]
    for i, d in enumerate(dirs):
        assert sorted(os.listdir(d)) == sorted(["%d.png" % k for k in range(T + 1)] + ["frames.npz", "replay.gif"])
        back = np.load(os.path.join(d, "frames.npz"))
        for k in ("frames", "pos", "actions_inc", "collective"):
            assert (back[k] == rec[k][i]).all(), k
        with Image.open(os.path.join(d, "replay.gif")) as g:
            assert g.n_frames == T + 1


def test_run_sequential_save_replay_reaches_the_recorder(tmp_path, monkeypatch):
    from homophily_marl_amd import run as R
    calls = []

    class FakeRunner:
        t_env = 0

        def run(self, test_mode=False):
            calls.append(("run", test_mode))

        def save_replay(self):
            calls.append(("save_replay",))
            return str(tmp_path / "replays" / "replay-x")

        def close_env(self):
            calls.append(("close",))

    class FakeLearner:
        def load_models(self, path):
            calls.append(("load", os.path.basename(path)))

    ck = tmp_path / "ckpt"
    (ck / "8").mkdir(parents=True)
    args = SimpleNamespace(checkpoint_path=str(ck), load_step=0, evaluate=False, save_replay=True, test_nepisode=3, t_max=10 ** 9)
    ctx = SimpleNamespace(args=args, runner=FakeRunner(), learner=FakeLearner(), logger=None)
    monkeypatch.setattr(R, "setup", lambda config, logger=None: ctx)
    out = R.run_sequential({})
    assert calls == [("load", "8"), ("run", True), ("run", True), ("run", True), ("save_replay",), ("close",)]
    assert out.replay_dir.endswith("replay-x")
