"""Generate tests/golden/env_law.npz FROM THE IMPORTED REFERENCE: the numbers its own lines give for the law that
tests/env_law_util.py restates.  No sampling: nothing here draws.

TEST INFRASTRUCTURE; runs only in the build container (needs /root/reference).  Usage: python oracle/gen_env_law_golden.py
The fixture is data only:

    cleanup_<map>_p_apple[n_waste + 1] f64, cleanup_<map>_p_waste[n_waste + 1] f64     for map = default3 / default5 / default10:
        current_apple_spawn_prob / current_waste_spawn_prob after compute_probabilities() (cleanup.py:189-204) with c = 0 .. n_waste
        of the waste sites holding 'H' and the others 'R'
    harvest_spawn_prob[4] f64                   HarvestEnv.SPAWN_PROB of map default10 (harvest.py:22)
    harvest_grid[G, H * W] u8, harvest_pos[G, n, 2] i16
        G hand-made orchards on the default10 layout and the agents' cells
    harvest_count[G, n_apple] i32               num_apples of spawn_apples' loop (harvest.py:107-116) at every apple site it
        reaches, -1 where the site holds an apple or an agent (harvest.py:106)
    harvest_class[G, n_apple] i32               the index spawn_apples reads SPAWN_PROB at (harvest.py:118), -1 likewise
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import ref_harness as RH  # noqa: E402
from tests import env_state_util as U  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "env_law.npz")


def cleanup_tables(map_name, n):
    ref = RH.RefEnv("cleanup", map_name, n)
    ref.reset()
    L = U.shipped("cleanup", map_name)
    assert L.n_waste == ref.n_waste and ref.env.potential_waste_area == L.n_waste
    pa, pw = [], []
    for c in range(L.n_waste + 1):
        g = ref.grid().reshape(-1)
        g[L.waste] = U.RIVER
        g[L.waste[:c]] = U.WASTE
        ref.set_state(grid=g.reshape(L.H, L.W))
        ref.env.compute_probabilities()
        pa.append(float(ref.env.current_apple_spawn_prob)); pw.append(float(ref.env.current_waste_spawn_prob))
    return np.array(pa, np.float64), np.array(pw, np.float64)


class _Recorder:
    """stands in for SPAWN_PROB: records the index it is read at and never lets an apple grow"""

    def __init__(self):
        self.read = []

    def __getitem__(self, i):
        self.read.append(int(i))
        return 0.0


def harvest_orchards(L, rng):
    """hand-made orchards: empty, full, every other site, single rows, the left half, and random fills of 10 % .. 90 %"""
    grids = []
    def make(mask):
        g = L.base.copy()
        g[L.apple] = np.where(mask, U.APPLE, U.EMPTY)
        grids.append(g)
    k = np.arange(L.n_apple)
    make(k < 0); make(k >= 0); make(k % 2 == 0); make(k % 3 == 0)
    for r in np.unique(L.apple // L.W):
        make(L.apple // L.W == r)
    make(L.apple % L.W < L.W // 2)
    for f in (0.1, 0.3, 0.5, 0.7, 0.9):
        make(rng.random(L.n_apple) < f)
    return np.stack(grids)


def harvest_counts(n=5):
    ref = RH.RefEnv("harvest", "default10", n)
    ref.reset()
    L = U.shipped("harvest", "default10")
    assert [tuple(p) for p in ref.env.apple_points] == [(int(c) // L.W, int(c) % L.W) for c in L.apple]
    spawn_prob = np.array(ref.env.SPAWN_PROB, np.float64)
    harvest = sys.modules[type(ref.env).__module__]
    rng = np.random.default_rng(2024)
    grids = harvest_orchards(L, rng)
    pos = np.zeros((len(grids), n, 2), np.int16)
    count = np.full((len(grids), L.n_apple), -1, np.int32)
    klass = np.full((len(grids), L.n_apple), -1, np.int32)
    for g, grid in enumerate(grids):
        cells = L.apple[rng.permutation(L.n_apple)[:n]]          # the agents stand on apple sites, with or without an apple
        pos[g, :, 0], pos[g, :, 1] = cells // L.W, cells % L.W
        ref.set_state(grid=grid.reshape(L.H, L.W), pos=pos[g])
        reached = [i for i, c in enumerate(L.apple) if grid[c] != U.APPLE and c not in cells]
        for out, clip in ((klass, None), (count, lambda a, b: a)):       # the second pass reads the count before min(., 3)
            rec = _Recorder()
            ref.env.SPAWN_PROB = rec
            # spawn_apples looks `min` up in its module's globals before the builtins: a module attribute of that name shadows
            # the builtin for the call, and deleting the attribute uncovers the builtin again
            if clip is not None:
                harvest.min = clip
            try:
                assert ref.env.spawn_apples() == []
            finally:
                if clip is not None:
                    del harvest.min
            assert len(rec.read) == len(reached)
            out[g, reached] = rec.read
        assert (np.minimum(count[g], 3) == klass[g]).all()
    return spawn_prob, grids, pos, count, klass


if __name__ == "__main__":
    out = {}
    for map_name, n in (("default3", 3), ("default5", 5), ("default10", 10)):
        out["cleanup_%s_p_apple" % map_name], out["cleanup_%s_p_waste" % map_name] = cleanup_tables(map_name, n)
    out["harvest_spawn_prob"], out["harvest_grid"], out["harvest_pos"], out["harvest_count"], out["harvest_class"] = harvest_counts()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()}, "bytes", os.path.getsize(OUT))
    print("neighbour counts seen:", sorted(set(out["harvest_count"].ravel().tolist())))
