"""GPU suite of training on sampled time windows with burn-in: the device draws against the restatement of
tests/train_window_util.py bit for bit, ssd_gather_windows in the poisoned arena of tests/arena_util.py against numpy slices byte for
byte, the fused learner on gathered windows against the numbers the reference recorded on time slices
(tests/golden/learner_train_window.npz), eager and captured, and the training loop under train_window (and train_window: 0 against
the keys' absence, bit for bit)."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests import td_lambda_util as U
from tests import train_window_util as W
from tests.arena_util import Arena
from tests.test_learner_options import check_step, perturb_target

pytestmark = pytest.mark.gpu

SHAPES = [(7, 3, 1), (7, 7, 2), (40, 16, 8), (8192, 64, 76), (5000, 16, 976)]      # (population, count, n_starts)
SEED = 0x1234567890ABCDEF


# ---- 7. the device draws -----------------------------------------------------------------------------------------------------------------
# beyond the shapes of the host test: every register-slot count of k_sample_draw (count up to 64, 128, 256, SSD_SAMPLE_IDS_MAX) and its edges
MORE_SHAPES = [(64, 64, 1), (65, 65, 2), (300, 128, 89), (129, 129, 3), (2000, 200, 5), (256, 256, 7), (257, 257, 2), (5000, 1024, 3), (1, 1, 4)]


@pytest.mark.parametrize("population,count,n_starts", SHAPES + MORE_SHAPES)
def test_device_draws_are_the_restatement(population, count, n_starts):
    for seed, call in ((SEED, 0), (SEED, 5), (3, 2 ** 32 - 1), (2 ** 64 - 1, 77)):
        draws = th.full((2, count + 8), -7, dtype=th.long, device="cuda")
        ids, t0 = ops.sample_windows(seed, call, population, count, n_starts, draws[0], draws[1])
        ref_ids, ref_t0 = W.sample_windows(seed, call, population, count, n_starts)
        got = draws.cpu()
        assert got[0, :count].tolist() == ref_ids and got[1, :count].tolist() == ref_t0, (seed, call)
        assert (got[:, count:] == -7).all()                                  # nothing past `count`
        assert th.equal(got[0, :count], ops.sample_ids(seed, call, population, count, th.empty(count, dtype=th.long, device="cuda")).cpu())


# ---- 8. the device gather in the arena -------------------------------------------------------------------------------------------------------
ROWS = 6
# (name, dtype, elements per slot, align of src, offset_in_16 of src, align of dst, offset_in_16 of dst): slot bytes 1, 12, 27, 1125, 4 * 45
FIELDS = [("terminated", np.uint8, 1, 1, 0, 1, 0), ("pos", np.float32, 3, 4, 4, 16, 0), ("odd27", np.uint8, 27, 1, 0, 1, 0),
          ("codes", np.uint8, 1125, 1, 0, 16, 0), ("onehot", np.float32, 45, 4, 12, 4, 8), ("codes_b", np.uint8, 1125, 1, 0, 1, 0)]


def _window_case(src_slots, win_slots):
    span = src_slots - win_slots
    t0 = [0, span] + [(5 * k + 1) % (span + 1) for k in range(10)]
    ids = [0, ROWS - 1, 2, 0, ROWS - 1, 3, 1, 4, ROWS - 1, 5, 0, 2]
    return ids, t0


def _arena_gather(src_slots, win_slots, burn_in, ids, t0, call=True):
    """every operand in an arena; returns (arena, {name: (source array, output region)}, filled source, filled region, rc)"""
    rng = np.random.default_rng(100 * src_slots + win_slots)
    ar, n_ids = Arena(), len(ids)
    regs = {}
    for name, dtype, per, sa, so, da, do in FIELDS:
        x = (rng.integers(0, 256, (ROWS, src_slots, per)).astype(np.uint8) if dtype == np.uint8 else rng.standard_normal((ROWS, src_slots, per)).astype(np.float32))
        src = ar.place(name, x, align=sa, offset_in_16=so, fill=0xA5 if dtype == np.uint8 else None, row_bytes=x[0, 0].nbytes)
        dst = ar.reserve(name + "_out", (n_ids, win_slots, per), dtype, align=da, offset_in_16=do, row_bytes=x[0, 0].nbytes,
                         written=(True if call else False) if dtype == np.float32 else None)
        regs[name] = (x, src, dst)
    filled = (rng.random((ROWS, src_slots)) < 0.8).astype(np.int64)
    filled[:, 0] = 1
    f_src = ar.place("filled", filled, align=8, fill=7)
    f_dst = ar.reserve("filled_out", (n_ids, win_slots), np.int64, align=8, written=None)
    p_ids = ar.place("ids", np.asarray(ids, dtype=np.int64), align=8, fill=0)
    p_t0 = ar.place("t0", np.asarray(t0, dtype=np.int64), align=8, fill=0)
    tab = (abi.SsdWindowField * (len(FIELDS) + 1))()
    order = list(FIELDS[:3]) + [None] + list(FIELDS[3:])                     # the filled field in the middle of the table
    for e, f in zip(tab, order):
        if f is None:
            e.src, e.dst, e.slot_bytes, e.filled = f_src.ptr, f_dst.ptr, 8, 1
        else:
            x, src, dst = regs[f[0]]
            e.src, e.dst, e.slot_bytes, e.filled = src.ptr, dst.ptr, x[0, 0].nbytes, 0
    return ar, regs, filled, f_dst, (tab, len(tab), p_ids.ptr, p_t0.ptr, n_ids, src_slots, win_slots, burn_in, None)


GATHER_CASES = [(13, 2, 0), (13, 7, 0), (13, 7, 5), (13, 13, 0), (13, 13, 11), (101, 2, 0), (101, 7, 5), (101, 13, 0), (101, 26, 0), (101, 26, 24)]


@pytest.mark.parametrize("src_slots,win_slots,burn_in", GATHER_CASES)
def test_gather_windows_in_the_arena(src_slots, win_slots, burn_in):
    """one launch for six copied fields (slot bytes 1, 12, 27, 1125 twice, 180; sources and destinations at byte, 4-, 8- and 16-byte
    alignments) and the filled field: outputs equal the numpy slices byte for byte, bands / slack / inputs untouched, no poison in an
    output; ids with row 0 and the last row, t0 with 0 and src_slots - win_slots"""
    ids, t0 = _window_case(src_slots, win_slots)
    assert 0 in ids and ROWS - 1 in ids and 0 in t0 and src_slots - win_slots in t0 and max(t0) + win_slots <= src_slots
    if src_slots - win_slots >= 7:
        for sb in (1, 27, 1125):
            assert len({(s * sb) % 16 for s in t0}) >= 8, sb             # the source lands on at least eight alignments
    ar, regs, filled, f_dst, args = _arena_gather(src_slots, win_slots, burn_in, ids, t0)
    assert any(dst.ptr % 16 for _, _, dst in regs.values()) and any(dst.ptr % 16 == 0 for _, _, dst in regs.values())
    lib = abi.load_library()
    abi.check(lib, lib.ssd_gather_windows(*args))
    ar.check()
    for name, (x, src, dst) in regs.items():
        got, ref = dst.array(), W.window_slices(x, ids, t0, win_slots)
        assert got.tobytes() == ref.tobytes(), (name, int(np.flatnonzero(got.view(np.uint8).ravel() != ref.view(np.uint8).ravel())[0]))
    assert np.array_equal(f_dst.array(), W.window_filled(filled, ids, t0, win_slots, burn_in))
    if burn_in:
        f = f_dst.array()
        assert all(not f[e, :burn_in].any() for e, s in enumerate(t0) if s > 0) and any(f[e, :burn_in].any() for e, s in enumerate(t0) if s == 0)


def test_refused_gathers_launch_nothing():
    """invalid arguments with every operand in the arena: SSD_ERR_INVALID with a message, and every output keeps its pre-fill"""
    ids, t0 = _window_case(13, 7)
    ar, regs, filled, f_dst, args = _arena_gather(13, 7, 2, ids, t0, call=False)
    lib = abi.load_library()
    prefill = f_dst.array().copy()
    bad = [args[:1] + (0,) + args[2:], args[:4] + (0,) + args[5:], args[:6] + (14,) + args[7:], args[:6] + (1, 0) + args[8:], args[:7] + (6,) + args[8:],
           args[:7] + (-1,) + args[8:], args[:2] + (None,) + args[3:], args[:3] + (None,) + args[4:]]
    for a in bad:
        rc = lib.ssd_gather_windows(*a)
        assert rc == abi.SSD_ERR_INVALID and b"ssd_gather_windows" in lib.ssd_last_error(), (a[1:], rc)
    th.cuda.synchronize()
    ar.check()
    assert np.array_equal(f_dst.array(), prefill)
    for name, (x, src, dst) in regs.items():
        assert dst.array().tobytes() == ar.mirror[dst.start:dst.start + dst.nbytes].tobytes(), name


def test_ops_gather_windows_on_tensors_and_strict_fallback():
    """ops.gather_windows on torch tensors (u8 codes at 1125-byte slots, i64, f32, the filled mask) against indexing; a pair that does
    not qualify returns False, and ReplayBuffer.gather_windows then refuses the tensor-op branch under strict_device_ops"""
    g = th.Generator().manual_seed(3)
    src = [th.randint(0, 255, (9, 13, 5, 15, 15), generator=g, dtype=th.uint8), th.randint(0, 9, (9, 13, 5, 1), generator=g), th.randn(9, 13, 5, 2, generator=g),
           (th.rand(9, 13, 1, generator=g) < 0.7).long()]
    src = [s.cuda() for s in src]
    ids, t0 = th.tensor([8, 0, 3, 8, 5], device="cuda"), th.tensor([0, 6, 3, 1, 6], device="cuda")
    dst = [th.empty((5, 7) + tuple(s.shape[2:]), dtype=s.dtype, device="cuda") for s in src]
    assert ops.gather_windows(list(zip(src, dst)), ids, t0, 13, 7, 3, 3)
    slots = t0.unsqueeze(1) + th.arange(7, device="cuda")
    for k, (s, d) in enumerate(zip(src, dst)):
        ref = s[ids.unsqueeze(1), slots]
        if k == 3:
            ref = ref * (th.arange(7, device="cuda").view(1, 7, 1) >= th.where(t0 > 0, 3, 0).view(5, 1, 1))
        assert th.equal(d, ref), k
    assert not ops.gather_windows([(src[2], dst[2][:, :6])], ids, t0, 13, 7, 3, None)          # a destination of another shape
    assert not ops.gather_windows([(src[2], dst[2])], ids, t0, 13, 7, 3, 0)                    # a filled field that is not int64 slots
    assert not ops.gather_windows([(src[2].transpose(0, 1).contiguous().transpose(0, 1), dst[2])], ids, t0, 13, 7, 3, None)   # a strided source
    from homophily_marl_amd.components.episode_buffer import ReplayBuffer
    buf = ReplayBuffer({"reward": {"vshape": (1,)}}, {}, 2, 3, device="cuda")
    buf["reward"].copy_(th.arange(6.0).view(2, 3, 1))
    many = th.ones(65536, dtype=th.long, device="cuda")                    # more ids than one launch takes: indexing, field by field
    win = buf.gather_windows(many, many, 1, 0)
    assert win["reward"].shape == (65536, 2, 1) and win["reward"][-1].flatten().tolist() == [4.0, 5.0]
    ops.set_strict(True)
    try:
        with pytest.raises(RuntimeError, match="strict_device_ops"):
            buf.gather_windows(many, many, 1, 0)
    finally:
        ops.set_strict(False)


# ---- 9. the learner on the device ----------------------------------------------------------------------------------------------------------
ROWS_OF_EPISODES = [4, 1, 6, 3]


@pytest.mark.parametrize("train_graph,storage", [(False, "f32"), (True, "f32"), (False, "code"), (True, "code")])
@pytest.mark.parametrize("name", W.CASES)
def test_fused_learner_on_gathered_windows_matches_the_reference(name, train_graph, storage):
    """A device ReplayBuffer holds the fixture's four episodes among decoy rows; gather_windows with the golden's (ids, t0) feeds the
    fused learner, norm "window": two optimisation steps within 1e-5 of what the reference recorded on the slices, eagerly and
    replayed from the step captured on the window's shape (graph at the third call, the windows gathered straight into sample_out())."""
    th.backends.cuda.matmul.allow_tf32 = False
    rec, c = W.golden_case(name)
    args, batch, mac, learner = W.build_case(c, device="cuda:0", code_obs=storage == "code", overrides=dict(train_graph=train_graph))
    buf = W.buffer_of(batch, rows=ROWS_OF_EPISODES, size=8, norm="window")
    ids = th.tensor(ROWS_OF_EPISODES, device="cuda:0")
    t0 = th.tensor(c["t0"], device="cuda:0")
    ops.set_strict(True)
    try:
        win = buf.gather_windows(ids, t0, c["window"], c["burn_in"])
        assert learner._fused(win) and learner.use_graph == train_graph and win.reward_norm == c["window"] + 1.0
        assert [int((win["filled"][e] == 0).sum()) for e in range(4)] == c["k_e"]
        if train_graph:
            # past the capture (third call) on a scratch copy of the weights, then rewind weights, target net and optimiser state
            sd0 = {k: v.clone() for k, v in mac.agent.state_dict().items()}
            for _ in range(3):
                learner.train(win, 0, 0)
            assert learner._graph is not None
            out = learner.sample_out()
            assert (out.batch_size, out.max_seq_length, out.reward_norm) == (4, c["window"] + 1, c["window"] + 1.0)
            with pytest.raises(ValueError):
                learner.train(batch, 0, 0)                                   # whole episodes into the step captured for windows
            assert buf.gather_windows(ids, t0, c["window"], c["burn_in"], out=out) is out
            win = out
            mac.agent.load_state_dict(sd0)
            learner.target_mac.load_state(mac)
            for opt in (learner.optimiser_env, learner.optimiser_inc):
                for st in opt.state.values():
                    st["step"].zero_(); st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
        perturb_target(learner)
        for step in range(2):
            if train_graph:
                learner.train(win, 0, 0)
                logs = learner._static_logs
            else:
                logs = learner.cal_loss_and_step(win)
            check_step(logs, mac, rec, step)
    finally:
        ops.set_strict(False)


@pytest.mark.parametrize("name", ["cleanup5_L6_K2_dq1_oth0", "harvest5_L3_K1_dq0_oth1"])
def test_loss_kernel_on_windows_with_lambda_returns_and_the_episode_norm(name):
    """td_lambda 0.8, norm "episode": one mode-1 launch on the device learner's own Q-values of the gathered windows against
    tests/td_lambda_util.host_loss at the window's shape with seq_len = 13 (the tolerances of tests/test_td_lambda_gpu.py)."""
    th.backends.cuda.matmul.allow_tf32 = False
    lam = 0.8
    rec, c = W.golden_case(name)
    args, batch, mac, learner = W.build_case(c, device="cuda:0", code_obs=True, overrides=dict(td_lambda=lam))
    buf = W.buffer_of(batch, rows=ROWS_OF_EPISODES, size=8, norm="episode")
    win = buf.gather_windows(th.tensor(ROWS_OF_EPISODES, device="cuda:0"), th.tensor(c["t0"], device="cuda:0"), c["window"], c["burn_in"])
    assert win.reward_norm == 13.0 and learner._fused(win)
    perturb_target(learner)
    with th.no_grad():
        qs = [x.contiguous() for x in learner.unroll_pair(win)]
    dens = learner.denominators(win).contiguous().float()
    B, T, n = win.batch_size, win.max_seq_length - 1, args.n_agents
    partials = th.zeros(B * T * n, abi.TD_LOSS_PARTIALS, device="cuda:0")
    dq_env, dq_inc = th.empty_like(qs[0]), th.empty_like(qs[1])
    t, keep = ops._td_loss_args(win, args, args.n_actions, partials)
    assert t.seq_len == 13.0 and t.t_slots == c["window"] + 1
    t.q_env, t.q_inc, t.tq_env, t.tq_inc = (q.data_ptr() for q in qs)
    t.dens, t.dq_env, t.dq_inc = dens.data_ptr(), dq_env.data_ptr(), dq_inc.data_ptr()
    lib = abi.load_library()
    abi.check(lib, lib.ssd_td_sim_loss(C.byref(t), 1, th.cuda.current_stream().cuda_stream))
    th.cuda.synchronize()
    part = partials.reshape(B, T, n, -1).cpu().numpy()
    sq = lambda k: win[k].squeeze(-1).cpu().numpy()
    arr = dict(zip(("q_env", "q_inc", "tq_env", "tq_inc"), (q.cpu().numpy() for q in qs)))
    arr.update(avail=win["avail_actions"].cpu().numpy(), actions=sq("actions"), actions_inc=sq("actions_inc"), reward=win["reward"].cpu().numpy(),
               clean_num=win["clean_num"].cpu().numpy(), terminated=sq("terminated"), filled=sq("filled"))
    r32 = lambda x: float(np.float32(x))
    cfg = dict(double_q=int(args.double_q), consider_others_inc=int(args.consider_others_inc), reward_scale=r32(args.reward_scale),
               incentive_ratio=r32(args.incentive_ratio), incentive_cost=r32(args.incentive_cost), incentive=r32(args.incentive), seq_len=13.0,
               sim_horizon=int(args.sim_horizon), sim_threshold=r32(args.sim_threshold), sim_loss_weight=r32(args.sim_loss_weight),
               gamma_env=r32(args.gamma_env), gamma_inc=r32(args.gamma_inc))
    ref = U.host_loss(arr, cfg, lam, dens.cpu().numpy().astype(np.float64))
    for col, key in ((13, "G_env"), (14, "G_inc"), (2, "sq_env"), (3, "sq_inc")):
        err = np.abs(part[..., col] - ref[key])
        print(key, "max err %.3e, max |ref| %.3e" % (err.max(), np.abs(ref[key]).max()))
        assert (err <= 1e-5 * np.maximum(1.0, np.abs(ref[key]))).all(), (key, float(err.max()))
    for got, key in ((dq_env.cpu().numpy(), "dq_env"), (dq_inc.cpu().numpy(), "dq_inc")):
        err, top = float(np.abs(got - ref[key]).max()), float(np.abs(ref[key]).max())
        print(key, "max err %.3e, max |g| %.3e" % (err, top))
        assert top > 0 and err < 2e-6 * max(1.0, top), (key, err, top)


# ---- 10. the loop --------------------------------------------------------------------------------------------------------------------------
N_ENV, T_EP, BATCH = 32, 12, 16


def _loop_ctx(drop=(), **over):
    from homophily_marl_amd.run import load_config, setup
    th.manual_seed(0)
    np.random.seed(11)
    cfg = load_config("cleanup", overrides=dict(dict(
        runner="hip_graph", batch_size_run=N_ENV, batch_size=BATCH, buffer_size=2 * N_ENV, buffer_cpu_only=False, store_state=False, obs_storage="code",
        env_args=dict(num_agents=5, map="default5", episode_limit=T_EP, seed=3), use_cuda=True, save_model=False, runner_stats=False,
        learner_log_interval=10 ** 12, strict_device_ops=True, train_graph=True, train_steps_per_rollout=2), **over))
    for k in drop:
        del cfg[k]
    return setup(cfg)


def test_loop_trains_on_the_windows_the_buffer_recorded():
    """four iterations of run.train_iteration under train_window 5 / burn-in 2 (two train steps each; the step is captured at the third):
    every train step's batch equals the buffer's slices at the buffer's recorded (ids, t0) with the filled rule; after the capture the
    batch IS the learner's static batch (gathered in place: train copies nothing); losses finite"""
    from homophily_marl_amd.run import train_iteration
    ctx = _loop_ctx(train_window=5, train_burn_in=2)
    try:
        buf, learner = ctx.buffer, ctx.learner
        assert buf.window_norm == "episode"
        seen = []
        inner = learner.train

        def train(sample, t_env, episode):
            ids, t0 = buf.last_window_ids.cpu().tolist(), buf.last_window_t0.cpu().tolist()
            assert (sample.batch_size, sample.max_seq_length, sample.reward_norm) == (BATCH, 6, T_EP + 1.0)
            assert len(set(ids)) == BATCH and max(ids) < buf.episodes_in_buffer and 0 <= min(t0) and max(t0) <= T_EP - 5
            for k, v in buf.data.transition_data.items():
                x = v.cpu().numpy()
                ref = W.window_filled(x, ids, t0, 6, 2) if k == "filled" else W.window_slices(x, ids, t0, 6)
                assert np.array_equal(sample[k].cpu().numpy(), ref), (len(seen), k)
            static = learner.sample_out()
            seen.append((static is not None, sample is static, ids, t0))
            inner(sample, t_env, episode)
            if static is not None:
                assert all(sample[k].data_ptr() == learner._static_data[k].data_ptr() for k in learner._static_data)
        learner.train = train
        ep = 0
        for _ in range(4):
            ep = train_iteration(ctx, ep)
        th.cuda.synchronize()
        assert len(seen) == 8 and buf._sample_calls == 8 and ctx.train_steps == 8
        assert [s[0] for s in seen] == [False] * 3 + [True] * 5 and all(s[1] for s in seen[3:])      # captured at the third call
        assert len({tuple(s[3]) for s in seen}) > 1 and len({tuple(s[2]) for s in seen}) > 1         # the draws move with the call
        assert learner._graph is not None and learner._static_batch.max_seq_length == 6
        logs = learner._static_logs
        assert all(np.isfinite(float(logs[k])) for k in ("loss_value_env", "loss_value_inc", "loss_sim"))
        assert all(bool(th.isfinite(p).all()) for p in ctx.mac.parameters())
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


def test_window_zero_is_the_loop_without_the_keys():
    """the same setup with the three keys absent against train_window: 0: the stored bytes, the sampled ids of every call and the
    learner's parameters after four iterations are equal bit for bit"""
    from homophily_marl_amd.run import train_iteration
    runs = []
    for drop, over in ((("train_window", "train_burn_in", "train_window_norm"), {}), ((), dict(train_window=0))):
        ctx = _loop_ctx(drop=drop, **over)
        try:
            ids = []
            inner = ctx.learner.train

            def train(sample, t_env, episode, ctx=ctx, ids=ids, inner=inner):
                assert sample.max_seq_length == T_EP + 1 and ctx.buffer.last_window_ids is None
                ids.append(None if ctx.buffer._draws.ids is None else ctx.buffer._draws.ids.cpu().tolist())
                inner(sample, t_env, episode)
            ctx.learner.train = train
            ep = 0
            for _ in range(4):
                ep = train_iteration(ctx, ep)
            th.cuda.synchronize()
            runs.append((ids, {k: v.cpu().clone() for k, v in ctx.buffer.data.transition_data.items()},
                         [p.detach().cpu().clone() for p in ctx.mac.parameters()], ctx.buffer._sample_calls))
        finally:
            ops.set_strict(False)
            ctx.runner.close_env()
    (ids_a, data_a, par_a, calls_a), (ids_b, data_b, par_b, calls_b) = runs
    assert len(ids_a) == 8 and ids_a == ids_b and calls_a == calls_b and any(i is not None for i in ids_a)
    for k in data_a:
        assert th.equal(data_a[k], data_b[k]), k
    assert all(th.equal(a, b) for a, b in zip(par_a, par_b)) and len(par_a) > 0
