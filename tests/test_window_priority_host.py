"""CPU suite of a priority per training window (config keys per_unit: "window" / per_window_stride; the n_segments members of
ssd_priority_sample_args and ssd_rollout_priority_args -- "ssd_priority_sample", "ssd_rollout_priority", "ssd_priority_update" gain no
sibling export and "ssd_abi_version" stays): the grid helper, ops' host restatement of the draw over entries, the buffer's table of
buffer_size * S entries, the setup refusals, and the two exports' refusals (the library loads without a device)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops, run
from homophily_marl_amd.components.episode_buffer import EpisodeBatch, ReplayBuffer
from tests import priority_util as P
from tests import window_priority_util as W
from tests.test_priority_host import _sample_args
from tests.test_rollout_priority_host import _args as _rollout_args

INV = abi.SSD_ERR_INVALID


# ---- 1. the grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(W.GRIDS))
def test_grid_helper_gives_the_starts_and_covers_every_row(grid):
    T, L, s, K = grid
    S, stride, last = ops.window_grid(T, L, s)
    assert (S, stride, last) == (len(W.GRIDS[grid]), s, T - L) == (W.n_windows(T, L, s), s, T - L)
    assert ops.window_starts((S, stride, last)) == W.GRIDS[grid] == W.starts(T, L, s)
    per_row = W.member(T, L, s, 0).sum(axis=0)
    assert per_row.min() >= 1 and per_row.max() <= -(-L // s) + 1            # K = 0: every row trains somewhere; at most ceil(L / s) + 1 windows
    assert W.member(T, L, s, K).sum(axis=0).max() <= -(-L // s) + 1
    for k, st in enumerate(W.GRIDS[grid]):                                    # slots [start, start + L] stay inside the episode
        assert 0 <= st and st + L <= T


def test_grid_default_stride_is_the_half_overlap_and_gaps_are_refused():
    assert ops.window_grid(100, 25, 0) == (7, 13, 75) and ops.window_grid(100, 25) == (7, 13, 75)
    assert ops.window_grid(12, 4, 0) == (5, 2, 8) and ops.window_grid(7, 7, 0) == (1, 4, 0)
    for T, L, s in ((10, 4, 5), (10, 0, 1), (10, 11, 1), (10, 4, -1)):
        with pytest.raises(ValueError, match="window_grid"):
            ops.window_grid(T, L, s)


# ---- 2. the host draw over entries --------------------------------------------------------------------------------------------------
def _host(table, population, count, n_starts=1, beta=0.4, segments=None, call=3):
    ids, t0, ent = (th.full((count,), -7, dtype=th.long) for _ in range(3))
    w, log = th.full((count,), -7.0), th.full((4,), -7.0)
    ops.priority_sample(P.SEED, call, th.as_tensor(table), population, count, n_starts, beta, ids, t0, w, log,
                        **(dict(segments=segments, entries_out=ent) if segments else {}))
    return ids, t0, ent, w, log


@pytest.mark.parametrize("name", list(W.entry_tables()))
def test_host_draw_over_entries_is_the_flat_draw_mapped(name):
    table, S = W.entry_tables()[name]
    s = 2
    last = max(0, (S - 1) * s - 1)                                            # a clamped last window wherever S > 1
    grid_starts = [min(k * s, last) for k in range(S)]
    for count in (1, 16, 64, 1024):
        flat_ids, flat_t0, _, flat_w, flat_log = _host(table, table.size, count)
        ids, t0, ent, w, log = _host(table, table.size, count, n_starts=999, segments=(S, s, last))
        assert ent.tolist() == flat_ids.tolist() == P.sample(P.SEED, 3, table, table.size, count, 1, 0.4)["ids"]
        assert ids.tolist() == [f // S for f in ent.tolist()] and t0.tolist() == [grid_starts[f % S] for f in ent.tolist()]
        assert th.equal(w, flat_w) and th.equal(log, flat_log) and float(log[3]) == len(set(ent.tolist()))


def test_host_draw_refuses_a_grid_that_cannot_be():
    table = th.ones(12, dtype=th.int32)
    o = lambda: (th.zeros(4, dtype=th.long), th.zeros(4, dtype=th.long), th.zeros(4), th.zeros(4))
    for seg, pop, ent in (((0, 1, 0), 12, th.zeros(4, dtype=th.long)), ((257, 1, 0), 12, th.zeros(4, dtype=th.long)), ((4, 0, 0), 12, th.zeros(4, dtype=th.long)),
                          ((4, 1, -1), 12, th.zeros(4, dtype=th.long)), ((4, 2, 7), 12, th.zeros(4, dtype=th.long)), ((5, 1, 0), 12, th.zeros(4, dtype=th.long)),
                          ((4, 1, 3), 12, None), ((4, 1, 3), 12, th.zeros(3, dtype=th.long)), ((4, 1, 3), 12, th.zeros(4, dtype=th.int32))):
        with pytest.raises(ValueError, match="priority_sample"):
            ops.priority_sample(1, 0, table, pop, 4, 1, 0.4, *o(), segments=seg, entries_out=ent)


# ---- 3. the buffer ----------------------------------------------------------------------------------------------------------------------
SCHEME = {"reward": {"vshape": (2,)}, "terminated": {"vshape": (1,), "dtype": th.uint8}}


def _buffer(size, T=12, L=4, s=2):
    buf = ReplayBuffer(SCHEME, {}, size, T + 1, device="cpu")
    S = W.n_windows(T, L, s)
    buf.enable_priorities(segments=S, stride=s, window=L)
    return buf, S


def _episodes(n, first, slots=13):
    b = EpisodeBatch(SCHEME, {}, n, slots, device="cpu")
    b.update({"reward": th.arange(first, first + n, dtype=th.float32).reshape(n, 1, 1).expand(n, slots, 2)})
    return b


def test_table_holds_s_entries_per_slot_and_inserts_zero_exactly_their_slots():
    buf, S = _buffer(5)
    table = buf.priority_table
    assert S == 5 and table.numel() == 25 and table.dtype == th.int32 and not table.any() and buf.priority_grid == (5, 2, 8)
    assert buf.enable_priorities(segments=S, stride=2, window=4) is table
    fresh = lambda: table.copy_(th.arange(25, dtype=th.int32) + 100)
    fresh()
    buf.insert_episode_batch(_episodes(3, 0))                                # slots 0 .. 2
    assert table.tolist() == [0] * 15 + list(range(115, 125))
    fresh()
    buf.insert_episode_batch(_episodes(4, 10))                               # slots 3, 4, 0, 1: around the ring's end
    assert table.tolist() == [0] * 10 + list(range(110, 115)) + [0] * 10 and buf.buffer_index == 2


def test_insert_with_window_priorities_writes_them_and_splits_on_wrap_around():
    buf, S = _buffer(5)
    table = buf.priority_table
    table.fill_(7)
    pr = (th.arange(15, dtype=th.int32) + 1).reshape(3, S)
    buf.insert_episode_batch(_episodes(3, 0), priorities=pr)
    assert table.tolist() == list(range(1, 16)) + [7] * 10
    calls = []
    write = buf._write_priorities
    buf._write_priorities = lambda start, p: (calls.append((start, tuple(p.shape))), write(start, p))
    pr2 = (th.arange(20, dtype=th.int32) + 50).reshape(4, S)
    buf.insert_episode_batch(_episodes(4, 10), priorities=pr2)               # slots 3, 4 | 0, 1
    assert calls == [(3, (2, S)), (0, (2, S))]
    assert table.tolist() == list(range(60, 70)) + list(range(11, 16)) + list(range(50, 60))
    for bad in (th.ones(2, dtype=th.int32), th.ones(2, S, dtype=th.int64), th.ones(2, S + 1, dtype=th.int32), th.ones(3, S, dtype=th.int32)):
        with pytest.raises(ValueError, match="insert_episode_batch: priorities"):
            buf.insert_episode_batch(_episodes(2, 50), priorities=bad)


def test_buffer_draws_entries_and_hands_them_to_the_learner():
    buf, S = _buffer(6)
    buf.insert_episode_batch(_episodes(4, 0))
    table = buf.priority_table
    table[:4 * S].copy_(th.tensor(np.random.default_rng(1).integers(0, 1 << 20, 4 * S), dtype=th.int32))
    np.random.seed(3)
    b = buf.sample_prioritized(4, window=4, burn_in=1, beta=0.5)
    tab, ent, w = b.priority
    ref = P.sample(buf._sample_seed, 0, table.numpy(), 4 * S, 4, 1, 0.5)      # the filled prefix is episodes_in_buffer * S entries
    assert tab is table and ent.tolist() == ref["ids"] and ent is buf._draws.entries
    st = W.starts(12, 4, 2)
    assert buf.last_window_ids.tolist() == [f // S for f in ref["ids"]] and buf.last_window_t0.tolist() == [st[f % S] for f in ref["ids"]]
    assert np.array_equal(b["reward"][:, 0, 0].numpy(), np.array([f // S for f in ref["ids"]], np.float32)) and b.max_seq_length == 5
    b2 = buf.sample_prioritized(4, window=4, burn_in=1, beta=0.5)
    assert b2.priority[1].data_ptr() == ent.data_ptr()                        # a persistent tensor: a captured train step bakes the address in
    with pytest.raises(ValueError, match="window"):
        buf.sample_prioritized(4, window=5, burn_in=1)
    with pytest.raises(ValueError, match="window"):
        buf.sample_prioritized(4)


def test_enable_priorities_refuses_what_is_not_the_grid():
    for kw in (dict(segments=4, stride=2, window=4), dict(segments=5, stride=5, window=4), dict(segments=2)):
        with pytest.raises(ValueError):
            ReplayBuffer(SCHEME, {}, 5, 13, device="cpu").enable_priorities(**kw)
    big = ReplayBuffer.__new__(ReplayBuffer)                                  # (only the size check is reached)
    big.buffer_size, big.max_seq_length, big.priority_table = abi.PRIORITY_POP_MAX // 5 + 1, 13, None
    with pytest.raises(ValueError, match="PRIORITY_POP_MAX"):
        big.enable_priorities(segments=5, stride=2, window=4)
    buf, S = _buffer(5)
    with pytest.raises(ValueError, match="exists"):
        buf.enable_priorities()


# ---- 4. setup ---------------------------------------------------------------------------------------------------------------------------
def _ctx(T=100, buffer_size=64, **keys):
    a = SimpleNamespace(**dict(dict(runner="hip_graph", batch_size=16, prioritized_replay=True, train_window=25, train_burn_in=0, per_unit="window"), **keys))
    enabled = []
    buf = SimpleNamespace(device="cuda:0", max_seq_length=T + 1, buffer_size=buffer_size, enable_priorities=lambda **kw: enabled.append(kw))
    return a, buf, SimpleNamespace(fixed_length_episodes=True), enabled


@pytest.mark.parametrize("keys,match", [
    (dict(per_unit="row"), "per_unit"), (dict(per_unit=None), "per_unit"), (dict(per_unit=True), "per_unit"),
    (dict(prioritized_replay=False), "per_unit.*prioritized_replay"), (dict(train_window=0), "per_unit.*train_window"),
    (dict(per_window_stride=26), "per_window_stride"), (dict(per_window_stride=-1), "per_window_stride"),
    (dict(per_window_stride=3), "per_window_stride.*over 8"),                          # ceil(25 / 3) = 9
    (dict(train_window=2, per_window_stride=1, T=300), "per_window_stride.*SSD_PRIORITY_SEGMENTS_MAX"),      # 299 windows
    (dict(buffer_size=(1 << 20) // 7 + 1), "buffer_size.*SSD_PRIORITY_POP_MAX")])
def test_setup_refuses_with_the_keys_name(keys, match):
    keys = dict(keys)
    geo = {k: keys.pop(k) for k in ("T", "buffer_size") if k in keys}
    a, buf, runner, enabled = _ctx(**geo, **keys)
    with pytest.raises(ValueError, match=match):
        run._check_prioritized(a, buf, runner)
    assert not enabled


def test_setup_resolves_the_stride_and_sizes_the_table():
    a, buf, runner, enabled = _ctx()
    assert run._check_prioritized(a, buf, runner) is True
    assert (a.per_unit, a.per_window_stride) == ("window", 13) and enabled == [dict(segments=7, stride=13, window=25)]
    a, buf, runner, enabled = _ctx(per_window_stride=5, train_window=10, T=12)
    assert run._check_prioritized(a, buf, runner) is True and enabled == [dict(segments=2, stride=5, window=10)]


def test_defaults_leave_the_setup_as_it_was():
    cfg = run.load_config("cleanup")
    assert (cfg["per_unit"], cfg["per_window_stride"]) == ("episode", 0)
    for keys in ({}, dict(per_unit="episode"), dict(per_unit="episode", per_window_stride=0)):
        a = SimpleNamespace(runner="r", batch_size=16, prioritized_replay=True, train_window=25, **keys)
        plain = []
        buf = SimpleNamespace(device="cuda:0", enable_priorities=lambda *args, **kw: plain.append((args, kw)))
        assert run._check_prioritized(a, buf, SimpleNamespace(fixed_length_episodes=True)) is True
        assert plain == [((), {})]                                            # one entry per slot, as before
        rest = {k: v for k, v in vars(a).items() if k not in ("per_unit", "per_window_stride")}
        assert (a.per_unit, a.per_window_stride) == ("episode", 0)
        assert rest == dict(runner="r", batch_size=16, prioritized_replay=True, train_window=25, per_alpha=0.6, per_beta=0.4, per_eta=0.9, per_eps=1e-3,
                            per_beta_anneal_steps=0, per_initial_priority="max")
    off = SimpleNamespace(runner="r", batch_size=16)
    assert run._check_prioritized(off, SimpleNamespace(device="cpu"), SimpleNamespace()) is False and off.per_unit == "episode"


# ---- 5. the library's refusals ----------------------------------------------------------------------------------------------------------
PTR = 1 << 20
SEQ = dict(n_segments=4, seg_stride=2, last_start=5, entries=PTR, population=2000)
SAMPLE_REFUSALS = [dict(n_segments=-1), dict(n_segments=257, population=257 * 4), dict(entries=None), dict(seg_stride=0), dict(seg_stride=-2), dict(last_start=-1),
                   dict(last_start=7), dict(population=2001), dict(n_segments=3, population=2000)]
# t_slots 8 (T = 7) in the base block: (L, s, K) = (3, 2, 1) has S = 3
ROLL = dict(n_segments=3, win_len=3, seg_stride=2, burn_in=1)
ROLLOUT_REFUSALS = [dict(n_segments=-1), dict(n_segments=257), dict(win_len=0, n_segments=1), dict(win_len=8), dict(seg_stride=0), dict(seg_stride=4),
                    dict(win_len=7, seg_stride=0, n_segments=1), dict(burn_in=-1), dict(burn_in=3), dict(n_segments=2), dict(n_segments=4),
                    dict(t_slots=101, win_len=25, seg_stride=3, n_segments=26, burn_in=0)]      # ceil(25 / 3) = 9 windows per row


def test_abi_version_stays():
    assert abi.load_library().ssd_abi_version() == abi.ABI_VERSION == 10      # members appended, no export added


@pytest.mark.parametrize("over", SAMPLE_REFUSALS, ids=[",".join("%s=%s" % kv for kv in o.items()) for o in SAMPLE_REFUSALS])
def test_draw_refuses_a_bad_grid_with_a_message(over):
    lib = abi.load_library()
    lib.ssd_rollout_priority(None, None)                                      # another name in ssd_last_error before the case
    rc = lib.ssd_priority_sample(C.byref(_sample_args(**dict(SEQ, **over))), None)
    msg = lib.ssd_last_error()
    assert rc == INV and b"ssd_priority_sample" in msg and any(w in msg for w in (b"n_segments", b"entries", b"seg_stride", b"last_start", b"population")), (over, msg)


@pytest.mark.parametrize("over", ROLLOUT_REFUSALS, ids=[",".join("%s=%s" % kv for kv in o.items()) for o in ROLLOUT_REFUSALS])
def test_rollout_priority_refuses_a_bad_grid_with_a_message(over):
    lib = abi.load_library()
    lib.ssd_priority_sample(None, None)
    rc = lib.ssd_rollout_priority(C.byref(_rollout_args(**dict(ROLL, **over))), None)
    msg = lib.ssd_last_error()
    assert rc == INV and b"ssd_rollout_priority" in msg and any(w in msg for w in (b"n_segments", b"win_len", b"seg_stride", b"burn_in")), (over, msg)


def test_zero_segments_ignore_the_members_behind():
    """n_segments 0 is today's launch: the other new members are not looked at (a refusal that belongs to the old checks still names
    the old member)"""
    lib = abi.load_library()
    assert lib.ssd_priority_sample(C.byref(_sample_args(seg_stride=-5, last_start=-5, count=0)), None) == INV and b"count" in lib.ssd_last_error()
    assert lib.ssd_rollout_priority(C.byref(_rollout_args(win_len=-5, seg_stride=-5, burn_in=-5, n_env=0)), None) == INV and b"n_env" in lib.ssd_last_error()
