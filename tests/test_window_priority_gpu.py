"""GPU suite of a priority per training window (config key per_unit: "window"):
  1. k_priority_sample_seq against ssd_priority_sample without segments on the same flat table, bit for bit, the integer mapping of
     entries to (ids, t0), and the host restatement;
  2. k_rollout_priority_seq, driven slot by slot: on exact TD inputs the accumulators against an f32 restatement bit for bit and q_init
     against float64 (the bar of tests/test_rollout_priority_gpu.py); with S = 1 against k_rollout_priority bit for bit; on general
     floats within the propagated rounding, per window;
  3. every operand in the poisoned arena: only carry, the accumulators of the windows that hold row t - 1 and (at slot T) q_init change;
  4. the training loop with the key on ("max", "rollout", stored state, captured) and the key off against its absence."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests import priority_util as P
from tests import rollout_priority_util as U
from tests import window_priority_util as W
from tests.arena_util import Arena

pytestmark = pytest.mark.gpu

FIELDS = ("actions", "actions_inc", "reward", "terminated", "filled")
GUARD = 8


# ---- 1. the draw ------------------------------------------------------------------------------------------------------------------------
def _guarded(count, dtype, fill):
    buf = th.full((count + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + count]


def _device_sample(call, table, count, beta, segments=None):
    """one launch; host copies of (ids, t0, weights, log, entries) after checking the guard words around every output"""
    bufs = [_guarded(count, th.long, -7), _guarded(count, th.long, -7), _guarded(count, th.float32, -7.0), _guarded(4, th.float32, -7.0),
            _guarded(count, th.long, -7)]
    views = [v for _, v in bufs]
    ops.priority_sample(P.SEED, call, table, table.numel(), count, 1, beta, *views[:4],
                        **(dict(segments=segments, entries_out=views[4]) if segments else {}))
    out = []
    for (buf, view), n in zip(bufs, (count, count, count, 4, count)):
        host = buf.cpu()
        assert (host[:GUARD] == -7).all() and (host[GUARD + n:] == -7).all()
        out.append(host[GUARD:GUARD + n])
    return out


@pytest.mark.parametrize("name", list(W.entry_tables()))
def test_draw_over_entries_is_the_flat_draw_bit_for_bit(name):
    host_table, S = W.entry_tables()[name]
    table = th.as_tensor(host_table).cuda()
    s = 2
    last = max(0, (S - 1) * s - 1)                                            # a clamped last window wherever S > 1
    grid_starts = [min(k * s, last) for k in range(S)]
    for count in (1, 16, 64, 1024):
        for beta in (0.4, 1.0):
            flat_ids, flat_t0, flat_w, flat_log, untouched = _device_sample(count, table, count, beta)
            ids, t0, w, log, ent = _device_sample(count, table, count, beta, segments=(S, s, last))
            where = (name, count, beta)
            assert (untouched == -7).all() and not flat_t0.any()
            assert ent.tolist() == flat_ids.tolist(), where
            assert w.numpy().tobytes() == flat_w.numpy().tobytes() and log.numpy().tobytes() == flat_log.numpy().tobytes(), where
            e = ent.tolist()
            assert ids.tolist() == [f // S for f in e] and t0.tolist() == [grid_starts[f % S] for f in e], where
            assert float(log[3]) == len(set(e))
            # the host restatement, compared as tests/test_priority_gpu.py compares the flat draw
            ho = [th.zeros(count, dtype=th.long), th.zeros(count, dtype=th.long), th.zeros(count), th.zeros(4), th.zeros(count, dtype=th.long)]
            ops.priority_sample(P.SEED, count, th.as_tensor(host_table), host_table.size, count, 1, beta, *ho[:4], segments=(S, s, last), entries_out=ho[4])
            assert ho[4].tolist() == e and ho[0].tolist() == ids.tolist() and ho[1].tolist() == t0.tolist(), where
            ref = P.sample(P.SEED, count, host_table, host_table.size, count, 1, beta)
            assert e == ref["ids"], where
            err = np.abs(w.numpy().astype(np.float64) - ref["weights"]) / ref["weights"]
            assert err.max() <= 1e-5 and float(w.max()) == 1.0, (where, float(err.max()))
            assert np.allclose(log.numpy()[:2], ref["log"][:2], rtol=1e-6, atol=0) and abs(float(log[2]) - ref["log"][2]) <= 1e-5 * ref["log"][2], where


# ---- 2. the rollout priority --------------------------------------------------------------------------------------------------------------
def _layout(q, layout):
    return np.ascontiguousarray(np.swapaxes(q, 0, 1)) if layout == "agent_major" else np.ascontiguousarray(q)


def _strides(N, n, A, layout):
    return (N * A, A, N * n * 3, n * 3) if layout == "agent_major" else (A, n * A, n * 3, n * n * 3)


def _drive(ep, N, n, A, layout, c, alpha, eta, eps, avail_bits, grid=None, filled=True):
    """the T + 1 launches of an episode; grid = (T, L, s, K): per window (q_init [N, S], acc [N, n, S, 3]), None: per episode"""
    lib = abi.load_library()
    T = ep["reward"].shape[1] - 1
    dev = {k: th.as_tensor(ep[k]).cuda() for k in FIELDS}
    q_env, q_inc = th.zeros(_layout(ep["q_env"][:, 0], layout).shape, device="cuda"), th.zeros(_layout(ep["q_inc"][:, 0], layout).shape, device="cuda")
    t_index = th.zeros(1, dtype=th.long, device="cuda")
    S = W.n_windows(*grid[:3]) if grid else None
    carry = th.full((N, n, 2), float("nan"), device="cuda")
    acc = th.full((N, n, S, 3) if grid else (N, n, 3), float("nan"), device="cuda")
    q_init = th.zeros((N, S) if grid else (N,), dtype=th.int32, device="cuda")
    a = abi.SsdRolloutPriorityArgs()
    a.t_index, a.n_env, a.n_agents, a.n_actions, a.t_slots, a.avail_bits = t_index.data_ptr(), N, n, A, T + 1, avail_bits
    a.q_env, a.q_inc, a.carry, a.acc, a.q_init = q_env.data_ptr(), q_inc.data_ptr(), carry.data_ptr(), acc.data_ptr(), q_init.data_ptr()
    a.q_env_agent_stride, a.q_env_env_stride, a.q_inc_agent_stride, a.q_inc_env_stride = _strides(N, n, A, layout)
    for k in FIELDS:
        setattr(a, k, dev[k].data_ptr() if (k != "filled" or filled) else None)
    for k, v in dict(c, alpha=alpha, eta=eta, eps=eps).items():
        setattr(a, k, v)
    if grid:
        assert grid[0] == T
        a.n_segments, a.win_len, a.seg_stride, a.burn_in = S, grid[1], grid[2], grid[3]
    st = th.cuda.current_stream().cuda_stream
    for t in range(T + 1):
        q_env.copy_(th.as_tensor(_layout(ep["q_env"][:, t], layout)))
        q_inc.copy_(th.as_tensor(_layout(ep["q_inc"][:, t], layout)))
        t_index.fill_(t)
        assert lib.ssd_rollout_priority(C.byref(a), st) == 0, lib.ssd_last_error()
    th.cuda.synchronize()
    return q_init.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, acc.cpu().numpy()


def _exact_case(N, T, n, A):
    ep = U.episodes(N, T, n, A, seed=100 * N + 10 * n + A + T, exact=True)
    ep["q_env"][..., 0] = 2.0                                                 # the largest Q-value of every row: excluded by avail_bits below
    if N > 2:
        ep["filled"][N - 1] = 0                                               # an env without a loss row: p = eps in every window
    return ep


@pytest.mark.parametrize("layout", ["agent_major", "env_major"])
@pytest.mark.parametrize("N,n,A", W.SHAPES)
def test_window_kernel_is_the_restatement_on_exact_td_inputs(N, n, A, layout):
    c = dict(U.DYADIC)
    eps = 2.0 ** -10
    bits = (1 << A) - 2
    for grid, want_starts in W.GRIDS.items():
        T, L, s, K = grid
        ep = _exact_case(N, T, n, A)
        for alpha, eta in ((0.6, 0.9), (1.0, 0.0)):
            got, acc = _drive(ep, N, n, A, layout, c, alpha, eta, eps, bits, grid)
            p, exact, ref, _ = W.window_priority(ep, grid, bits, c, alpha, eta, eps)
            assert got.shape == (N, len(want_starts)) == exact.shape
            err = np.abs(got - exact)
            print("N %d n %d A %d %s grid %s alpha %.1f eta %.1f: q in [%d, %d], largest |got - exact| %.3f (bar 1 + exact 2^-20)"
                  % (N, n, A, layout, grid, alpha, eta, got.min(), got.max(), err.max()))
            assert P.within_q(got, exact), (grid, alpha, eta, got, exact)
            assert acc.tobytes() == W.acc_f32(ref, grid).tobytes(), (grid, alpha, eta)     # max, sums in rising t, counts: bit for bit
            if N > 2:
                assert (got[N - 1] == int(np.rint(np.clip(eps ** alpha * P.ONE, 1, P.QMAX)))).all()
        if len(want_starts) > 1:
            assert (exact.max(axis=1) - exact.min(axis=1) > 2).any()          # the windows of an episode do not all carry one value


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("N,n,A", W.SHAPES)
def test_one_window_is_the_per_episode_kernel_bit_for_bit(N, n, A, exact):
    grid = (7, 7, 1, 0)
    ep = U.episodes(N, 7, n, A, seed=3 * N + n + int(exact), exact=exact)
    from homophily_marl_amd.run import load_config
    c = dict(U.DYADIC) if exact else ops.td_constants(SimpleNamespace(**load_config("cleanup")), 8)
    for layout in ("agent_major", "env_major"):
        for alpha, eta, eps in ((0.6, 0.9, 1e-3), (0.3, 1.0, 1e-6)):
            q_seq, acc_seq = _drive(ep, N, n, A, layout, c, alpha, eta, eps, (1 << A) - 1, grid)
            q_ep, acc_ep = _drive(ep, N, n, A, layout, c, alpha, eta, eps, (1 << A) - 1, None)
            assert q_seq.shape == (N, 1) and np.array_equal(q_seq[:, 0], q_ep), (layout, alpha)
            assert acc_seq.shape == (N, n, 1, 3) and acc_seq.tobytes() == acc_ep.tobytes(), (layout, alpha)
            assert not np.isnan(acc_ep).any() and len(set(q_ep.tolist())) > min(1, N - 1)


@pytest.mark.parametrize("layout", ["agent_major", "env_major"])
@pytest.mark.parametrize("N,n,A", [(3, 5, 9), (67, 10, 16)])
def test_window_kernel_on_general_floats_within_the_propagated_rounding(N, n, A, layout):
    """the bar of tests/test_rollout_priority_gpu.py (derived there), per window: delta = 2^-22 (max M_env + max M_inc) over the window's
    loss rows, |got - exact| <= 1 + exact 2^-20 + ONE alpha max(p - delta, eps)^(alpha - 1) delta"""
    from homophily_marl_amd.run import load_config
    cfg = load_config("cleanup")
    for grid in W.GRIDS:
        T = grid[0]
        c = ops.td_constants(SimpleNamespace(**cfg), T + 1)
        ep = U.episodes(N, T, n, A, seed=7 * N + n + T, exact=False)
        bits = (1 << A) - 1 - 4
        for alpha, eta, eps in ((0.6, 0.9, 1e-3), (1.0, 0.0, 1e-3), (0.3, 1.0, 1e-6)):
            got, _ = _drive(ep, N, n, A, layout, c, alpha, eta, eps, bits, grid)
            p, exact, ref, bound = W.window_priority(ep, grid, bits, c, alpha, eta, eps)
            delta = 2.0 ** -22 * bound
            bar = 1.0 + exact * 2.0 ** -20 + P.ONE * alpha * np.maximum(p - delta, eps) ** (alpha - 1.0) * delta
            err = np.abs(got - exact)
            print("N %d n %d A %d %s grid %s alpha %.1f eta %.1f: largest |got - exact| %.3f at a bar of %.3f"
                  % (N, n, A, layout, grid, alpha, eta, err.max(), bar.reshape(-1)[np.argmax(err)]))
            assert (err <= bar).all(), (grid, alpha, eta, err.max())


# ---- 3. bounds --------------------------------------------------------------------------------------------------------------------------
def _arena_case(ep, N, n, A, layout, t, grid, c, rng):
    T, L, s, K = grid
    S = W.n_windows(T, L, s)
    ar = Arena()
    reg = dict(t_index=ar.place("t_index", np.array([t], np.int64), align=8, fill=0))
    tq = min(max(t, 0), T)
    reg["q_env"] = ar.place("q_env", _layout(ep["q_env"][:, tq], layout))
    reg["q_inc"] = ar.place("q_inc", _layout(ep["q_inc"][:, tq], layout), offset_in_16=4)
    reg["actions"] = ar.place("actions", ep["actions"], align=8, fill=0)
    reg["actions_inc"] = ar.place("actions_inc", ep["actions_inc"], align=8, fill=0)
    reg["reward"] = ar.place("reward", ep["reward"], offset_in_16=12)
    reg["terminated"] = ar.place("terminated", ep["terminated"], align=1, fill=0)
    reg["filled"] = ar.place("filled", ep["filled"], align=8, fill=1)
    carry0, acc0 = rng.uniform(-1, 1, (N, n, 2)).astype(np.float32), rng.uniform(0, 1, (N, n, S, 3)).astype(np.float32)
    reg["carry"] = ar.place("carry", carry0, offset_in_16=8, inout=True)
    reg["acc"] = ar.place("acc", acc0, offset_in_16=4, inout=True)
    reg["q_init"] = ar.reserve("q_init", (N, S), np.uint32, written=(t == T))
    a = abi.SsdRolloutPriorityArgs()
    for k, r in reg.items():
        setattr(a, k, r.ptr)
    a.n_env, a.n_agents, a.n_actions, a.t_slots, a.avail_bits = N, n, A, T + 1, (1 << A) - 1
    a.q_env_agent_stride, a.q_env_env_stride, a.q_inc_agent_stride, a.q_inc_env_stride = _strides(N, n, A, layout)
    for k, v in dict(c, alpha=0.6, eta=0.9, eps=1e-3).items():
        setattr(a, k, v)
    a.n_segments, a.win_len, a.seg_stride, a.burn_in = S, L, s, K
    return ar, a, reg, carry0, acc0


@pytest.mark.parametrize("layout", ["agent_major", "env_major"])
@pytest.mark.parametrize("N,n,A", W.SHAPES)
def test_window_launch_stays_inside_its_operands_and_touches_only_its_windows(N, n, A, layout):
    lib = abi.load_library()
    st = th.cuda.current_stream().cuda_stream
    c = dict(U.DYADIC)
    rng = np.random.default_rng(N)
    for grid in W.GRIDS:
        T, L, s, K = grid
        member = W.member(T, L, s, K)                                         # [S, T]
        ep = U.episodes(N, T, n, A, seed=N + n + A + T, exact=True, terminate=False)
        for t in sorted({0, 1, T // 2, T - 1, T, -1, T + 1}):
            ar, a, reg, carry0, acc0 = _arena_case(ep, N, n, A, layout, t, grid, c, rng)
            assert lib.ssd_rollout_priority(C.byref(a), st) == 0, lib.ssd_last_error()
            ar.check()                                                        # bands, slack and inputs bit-identical; q_init written iff t == T
            carry, acc = reg["carry"].array(), reg["acc"].array()
            if not 0 <= t <= T:
                assert carry.tobytes() == carry0.tobytes() and acc.tobytes() == acc0.tobytes(), (grid, t)
                continue
            assert not np.isnan(carry).any() and not np.isnan(acc).any(), (grid, t)
            assert (carry.tobytes() == carry0.tobytes()) == (t == T)
            if t == 0:
                assert not acc.any()
                continue
            hit = member[:, t - 1]                                            # the windows whose loss rows contain row t - 1
            assert acc[:, :, ~hit].tobytes() == acc0[:, :, ~hit].tobytes(), (grid, t)          # no other accumulator moved
            assert np.array_equal(acc[:, :, hit, 2], acc0[:, :, hit, 2] + np.float32(1.0)), (grid, t)      # (no termination: every row counts)
            assert (acc[:, :, hit, 0] >= acc0[:, :, hit, 0]).all() and (acc[:, :, hit, 1] >= acc0[:, :, hit, 1]).all()
            d = acc[:, :, hit, 1] - acc0[:, :, hit, 1]
            assert hit.sum() <= -(-L // s) + 1 and (not hit.any() or d.max() > 0)
            if t == T:                                                        # q_init is the aggregate of the state the launch left
                a64 = acc.astype(np.float64)
                p = 0.9 * a64[..., 0].max(axis=1) + 0.1 * a64[..., 1].sum(axis=1) / np.maximum(1.0, a64[..., 2].sum(axis=1)) + 1e-3
                assert P.within_q(reg["q_init"].array().astype(np.int64), np.clip(p ** 0.6 * P.ONE, 1.0, P.QMAX)), grid


def test_refused_grids_launch_nothing():
    lib = abi.load_library()
    st = th.cuda.current_stream().cuda_stream
    grid = (9, 4, 2, 1)
    ep = U.episodes(3, 9, 5, 9, seed=1, exact=True)
    for field, value in (("n_segments", 3), ("n_segments", 257), ("n_segments", -1), ("win_len", 10), ("seg_stride", 5), ("seg_stride", 0), ("burn_in", 4)):
        ar, a, reg, carry0, acc0 = _arena_case(ep, 3, 5, 9, "agent_major", 9, grid, dict(U.DYADIC), np.random.default_rng(0))
        reg["q_init"].written = False
        setattr(a, field, value)
        assert lib.ssd_rollout_priority(C.byref(a), st) == abi.SSD_ERR_INVALID, field
        assert b"ssd_rollout_priority" in lib.ssd_last_error(), field
        ar.check()
        assert reg["carry"].array().tobytes() == carry0.tobytes() and reg["acc"].array().tobytes() == acc0.tobytes(), field


# ---- 4. the loop --------------------------------------------------------------------------------------------------------------------------
N_ENV, T_EP, L_WIN, STRIDE, BURN, BATCH, SLOTS, ITERS = 32, 12, 4, 2, 1, 8, 64, 6
S_WIN = W.n_windows(T_EP, L_WIN, STRIDE)


def _loop_ctx(drop=(), np_seed=11, **over):
    """Cleanup-5, hip_graph runner, 32 envs of 12 transitions written into the buffer's own slots, a buffer of two rollouts (every
    third insert wraps), windows of 4 at stride 2 (S = 5) with one burn-in row"""
    from homophily_marl_amd.run import load_config, setup
    th.manual_seed(0)
    np.random.seed(np_seed)
    cfg = load_config("cleanup", overrides=dict(dict(
        runner="hip_graph", batch_size_run=N_ENV, batch_size=BATCH, buffer_size=SLOTS, buffer_cpu_only=False, store_state=False, obs_storage="code",
        env_args=dict(num_agents=5, map="default5", episode_limit=T_EP, seed=3), use_cuda=True, save_model=False, runner_stats=False,
        learner_log_interval=10 ** 12, strict_device_ops=True, train_graph=False, train_steps_per_rollout=4, prioritized_replay=True,
        train_window=L_WIN, train_burn_in=BURN), **over))
    for k in drop:
        del cfg[k]
    return setup(cfg)


def _run_window_loop(initial, **over):
    from homophily_marl_amd.run import train_iteration
    ctx = _loop_ctx(per_unit="window", per_window_stride=STRIDE, per_initial_priority=initial, **over)
    try:
        buf, learner, runner = ctx.buffer, ctx.learner, ctx.runner
        table = buf.priority_table
        assert table.numel() == SLOTS * S_WIN and not table.any() and buf.priority_grid == (S_WIN, STRIDE, T_EP - L_WIN)
        grid_starts = W.starts(T_EP, L_WIN, STRIDE)
        host = lambda: table.cpu().numpy().astype(np.int64)
        inserts, steps = [], []
        inner_insert, inner_train = buf.insert_episode_batch, learner.train

        def insert(batch, priorities=None):
            before, lo = host(), buf.buffer_index
            inner_insert(batch, priorities=priorities)
            th.cuda.synchronize()
            want = before.copy()
            if initial == "rollout":
                assert priorities.dtype == th.int32 and tuple(priorities.shape) == (N_ENV, S_WIN)
                want[lo * S_WIN:(lo + N_ENV) * S_WIN] = priorities.cpu().numpy().astype(np.int64).reshape(-1)
                assert (priorities > 0).all() and len(set(priorities.cpu().numpy().reshape(-1).tolist())) > N_ENV
            else:
                assert priorities is None
                want[lo * S_WIN:(lo + N_ENV) * S_WIN] = 0
            assert np.array_equal(host(), want), len(inserts)                 # the rollout's S entries per slot, and no other entry
            inserts.append(lo)
        buf.insert_episode_batch = insert

        def train(sample, t_env, episode):
            tab, ent_t, w_t = sample.priority
            before = host()
            ent, ids, t0 = ent_t.cpu().tolist(), buf.last_window_ids.cpu().tolist(), buf.last_window_t0.cpu().tolist()
            assert tab is table and ent_t is buf._draws.entries and sample.max_seq_length == L_WIN + 1
            assert ids == [f // S_WIN for f in ent] and t0 == [grid_starts[f % S_WIN] for f in ent], (len(steps), ent, ids, t0)
            ref = P.sample(buf._sample_seed, buf._sample_calls - 1, before, buf.episodes_in_buffer * S_WIN, BATCH, 1, sample_beta)
            assert ent == ref["ids"] and np.abs(w_t.cpu().numpy() - ref["weights"]).max() <= 1e-5, (len(steps), ent, ref["ids"])
            inner_train(sample, t_env, episode)
            th.cuda.synchronize()
            q = learner.last_q_new.cpu().numpy().astype(np.int64)
            assert q.min() >= 1 and np.array_equal(host(), P.write_back(before, ent, q)), (len(steps), ent, q)
            pairs = set(zip(ids, t0))
            steps.append(dict(ent=ent, two_windows=any(len({t for i, t in pairs if i == e}) > 1 for e in set(ids))))
        sample_beta = ctx.args.per_beta
        learner.train = train
        ep = 0
        for _ in range(ITERS):
            ep = train_iteration(ctx, ep)
        th.cuda.synchronize()
        assert inserts == [0, 32, 0, 32, 0, 32] and len(steps) == 4 * ITERS
        assert runner.priority_windows == ((S_WIN, L_WIN, STRIDE, BURN) if initial == "rollout" else None)     # (allocated by the first rollout)
        hits = [k for k, s in enumerate(steps) if s["two_windows"]]
        print("%s %s: train steps of the loop that drew two different windows of one episode: %s" % (initial, over, hits))
        # Several windows of one episode in a train step.  In the loop above that is left to chance (with a mostly unset table the eight
        # strata are four whole episodes each), so one more step is taken on a table the test writes: windows 1 and 3 of episode 40
        # hold nearly all of the mass.  The CPU restatement of the coming call says which entries it draws.
        f1, f3 = 40 * S_WIN + 1, 40 * S_WIN + 3
        table.fill_(1)
        table[f1], table[f3] = P.QMAX, P.QMAX
        coming = P.sample(buf._sample_seed, buf._sample_calls, host(), buf.episodes_in_buffer * S_WIN, BATCH, 1, sample_beta)["ids"]
        assert {f1, f3} <= set(coming), coming
        sample = buf.sample_prioritized(BATCH, L_WIN, BURN, beta=sample_beta, out=learner.sample_out() if hasattr(learner, "sample_out") else None)
        learner.train(sample, runner.t_env, ctx.train_steps)                  # (the wrapper above: the same checks)
        assert steps[-1]["ent"] == coming and steps[-1]["two_windows"] and len(steps) == 4 * ITERS + 1
        assert (learner._graph is not None) == bool(over.get("train_graph"))
        assert all(bool(th.isfinite(p).all()) for p in ctx.mac.parameters())
        name = dict((key, kernel) for kernel, key, _ in runner.timestep_launches()).get("rollout_priority")
        assert name == ("ssd::k_rollout_priority_seq" if initial == "rollout" else None)
        return [s["ent"] for s in steps]
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


@pytest.mark.parametrize("case", ["max", "rollout", "rollout_stored_state", "rollout_captured"])
def test_loop_draws_trains_and_writes_windows(case):
    """six iterations of run.train_iteration, four train steps each.  After every insert the inserted slots' entries are zero ("max") or
    the runner's [N, S] values and no other entry moved; at every train step the drawn entries are the restatement's draw from the
    flat table as it stands, every (ids, t0) is the entry's window on the grid, and the table after the step is the restated
    write-back at the drawn entries.  One more train step, on a table written so that the restatement draws two different windows of
    one episode, passes the same checks."""
    over = dict(rollout_stored_state=dict(train_stored_state=True), rollout_captured=dict(train_graph=True)).get(case, {})
    _run_window_loop("max" if case == "max" else "rollout", **over)


def test_key_off_is_the_loop_without_the_key():
    """per_unit absent against "episode": stored bytes, drawn ids / t0 of every call, the table and the parameters after four
    iterations bit for bit; one entry per slot; the per-slot launch is k_rollout_priority"""
    from homophily_marl_amd.run import train_iteration
    runs = []
    for drop, over in ((("per_unit", "per_window_stride"), {}), ((), dict(per_unit="episode"))):
        ctx = _loop_ctx(drop=drop, per_initial_priority="rollout", train_graph=True, **over)
        try:
            drawn = []
            inner = ctx.learner.train

            def train(sample, t_env, episode, ctx=ctx, drawn=drawn, inner=inner):
                assert sample.priority[1] is ctx.buffer._draws.ids and ctx.buffer._draws.entries is None
                drawn.append((ctx.buffer._draws.ids.cpu().tolist(), ctx.buffer._draws.t0.cpu().tolist()))
                inner(sample, t_env, episode)
            ctx.learner.train = train
            ep = 0
            for _ in range(4):
                ep = train_iteration(ctx, ep)
            th.cuda.synchronize()
            assert ctx.args.per_unit == "episode" and ctx.buffer.priority_table.numel() == SLOTS and ctx.runner.priority_windows is None
            assert tuple(ctx.runner.initial_priorities().shape) == (N_ENV,)
            launches = [(kernel, key) for kernel, key, _ in ctx.runner.timestep_launches()]
            assert ("ssd::k_rollout_priority", "rollout_priority") in launches
            runs.append((drawn, {k: v.cpu().clone() for k, v in ctx.buffer.data.transition_data.items()}, ctx.buffer.priority_table.cpu().clone(),
                         [p.detach().cpu().clone() for p in ctx.mac.parameters()], launches))
        finally:
            ops.set_strict(False)
            ctx.runner.close_env()
    (drawn_a, data_a, tab_a, par_a, launches_a), (drawn_b, data_b, tab_b, par_b, launches_b) = runs
    assert len(drawn_a) == 16 and drawn_a == drawn_b and launches_a == launches_b and th.equal(tab_a, tab_b) and bool((tab_a != 0).any())
    assert any(len(set(t0)) > 1 for _, t0 in drawn_a)                         # starts drawn uniformly inside the episode, as before
    for k in data_a:
        assert th.equal(data_a[k], data_b[k]), k
    assert all(th.equal(a, b) for a, b in zip(par_a, par_b)) and len(par_a) > 0
