"""Generate tests/golden/render_*.npz FROM THE IMPORTED REFERENCE (through oracle/ref_harness.py, as oracle/gen_golden.py does).

Build-container tool (needs the reference sources).  Usage: python tools/gen_render_golden.py [names...]
A fixture is data only.  Schema of traj_*.npz (one env, calls c = 0..C-1, kind 0 = reset / 1 = step; the recorded draws, the
actions and the teleports fed to every call, the state after it), plus

    frames[C,H,W,3] u8   map_to_colors(get_map_with_agents_beam(), color_map) after every call (what MapEnv._render shows)
    color_chars         json list of the keys of the reference's color_map, color_rgb[K,3] u8 their colours
"""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from oracle import ref_harness as RH  # noqa: E402
from oracle.check_vs_reference import cluster_positions  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ALL = dict(disable_rotation_action=False, disable_fire_action=False)

RENDER = [
    # name, cfg, episodes, episode_limit, extra_args, seed, teleport prob (clustered teleports: beams hit agents)
    ("cleanup5_beams", dict(env="cleanup", map="default5", num_agents=5, view_size=7), 2, 40, dict(ALL, obs_color="full"), 61, 0.3),
    ("harvest5_fire", dict(env="harvest", map="default10", num_agents=5, view_size=7), 2, 40, ALL, 62, 0.2),
    ("cleanup10_allact", dict(env="cleanup", map="default10", num_agents=10, view_size=7), 2, 30, ALL, 63, 0.2),
    ("cleanup5_simplified", dict(env="cleanup", map="default5", num_agents=5, view_size=7), 2, 30,
     dict(ALL, obs_color="simplified"), 64, 0.2),
]


def frame(ref):
    e = ref.env
    return np.asarray(e.map_to_colors(e.get_map_with_agents_beam(), e.color_map)).astype(np.uint8)


def gen(name, cfg, episodes, limit, ea, seed, p_tele):
    np.random.seed(seed); random.seed(seed)
    rng = np.random.default_rng(seed)
    ref = RH.RefEnv(cfg["env"], cfg["map"], cfg["num_agents"], cfg["view_size"], limit, ea)
    n = cfg["num_agents"]
    n_actions = ref.env.n_actions
    maxu, nw = ref.n_apple + ref.n_waste, ref.n_waste
    rows = []

    def add(kind, acts, pre_pos, pre_orient, rec, reward, info):
        ta = RH.tape_arrays(rec, n, maxu, nw, ref.spawn_len)
        rows.append(dict(kind=kind, actions=acts, pre_pos=pre_pos, pre_orient=pre_orient, move_order=ta["move_order"],
                         uniforms=ta["uniforms"], n_uniforms=ta["n_uniforms"], waste_order=ta["waste_order"], spawn_rot=ta["spawn_rot"],
                         grid=ref.grid(), pos=ref.pos(), orient=ref.orient(),
                         reward=np.zeros(n) if reward is None else np.array(reward, copy=True),
                         clean_num=np.zeros(n) if info is None else np.array(info["clean_num"], copy=True),
                         n_beam_cells=len(ref.env.beam_pos), frames=frame(ref)))

    for ep in range(episodes):
        pre_pos = ref.pos() if ep else np.zeros((n, 2), np.int16)
        pre_ori = ref.orient() if ep else np.zeros(n, np.uint8)
        rec = ref.reset()
        add(0, np.zeros(n, np.int32), pre_pos, pre_ori, rec, None, None)
        term = False
        while not term:
            if rng.random() < p_tele:
                ref.set_state(pos=cluster_positions(rng, ref.grid(), n, int(rng.integers(1, 3))),
                              orient=rng.integers(0, 4, n).astype(np.uint8))
            pre_pos, pre_ori = ref.pos(), ref.orient()
            acts = rng.integers(0, n_actions, n).astype(np.int32)
            reward, term, info, rec = ref.step(acts)
            add(1, acts, pre_pos, pre_ori, rec, reward, info)
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    out["kind"] = out["kind"].astype(np.uint8)
    out["n_uniforms"] = out["n_uniforms"].astype(np.int32)
    out["n_beam_cells"] = out["n_beam_cells"].astype(np.int32)
    out["uniforms"] = out["uniforms"][:, :max(1, int(out["n_uniforms"].max()))]
    cm = ref.env.color_map
    chars = sorted(cm)
    out["color_chars"] = np.frombuffer(json.dumps(chars).encode(), np.uint8)
    out["color_rgb"] = np.array([cm[c] for c in chars], np.uint8)
    meta = dict(cfg, episode_limit=limit, extra_args=ea, n_actions=int(n_actions), generator="tools/gen_render_golden.py", seed=seed)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(OUT, "render_%s.npz" % name)
    np.savez_compressed(path, **out)
    firing = (out["actions"][out["kind"] == 1] >= 7).sum(1)
    print("wrote", path, dict(calls=len(rows), beam_cells=int(out["n_beam_cells"].sum()), max_firing_in_a_step=int(firing.max()),
                              kb=os.path.getsize(path) // 1024), flush=True)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for row in RENDER:
        if not only or row[0] in only:
            gen(*row)
