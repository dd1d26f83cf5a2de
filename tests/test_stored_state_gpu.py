"""GPU suite of training windows from the rollout's stored recurrent state (config key train_stored_state): the sequence kernels from
a given state (ssd_gru_seq_fwd_h0 / _bwd_h0) against a float64 stepwise unroll with a constant h0, the chain identity on the device
(a window evaluated from the stored state is the same slice of the whole unroll), h0 read in place from a strided field, and every
operand of the new launches -- ssd_store_hidden included -- in the poisoned arena of tests/arena_util.py; the rollout files the
states the learner's whole-episode unroll computes on the stored episode (three timestep forms; every other field as with the key
off), and the training loop starts every window from the buffer's stored state (eager and captured; the key absent = False).

Bars (tests/test_hip_learner_path.py): states 1e-5 absolute, gradients 2e-5 * max(1, max|ref|), bf16 BF16_Q_TOL."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests.arena_util import Arena
from tests.stored_state_util import gru_unroll_ref, gru_case

pytestmark = pytest.mark.gpu

BF16_Q_TOL = 2e-2            # tests/test_hip_learner_path.py: the bf16 variant's bar
INV = abi.SSD_ERR_INVALID


def _grad_ok(got, ref, name, tol=2e-5):
    err, scale = float((got.detach().double().cpu() - ref).abs().max()), max(1.0, float(ref.abs().max()))
    print("%s: max error %.3e (bar %.1e x %.3g)" % (name, err, tol, scale))
    assert err < tol * scale, (name, err)


# ---- 4. the kernels against a stepwise unroll with a constant h0 ---------------------------------------------------------------------------
@pytest.mark.parametrize("G,B", [(2, 16), (3, 32), (10, 21)])                # the last: ragged, through the time-major launch that pads
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 9])                             # the forward's prefetch groups of 4, the backward's of 2, T = 1
def test_kernels_from_a_given_state_match_the_stepwise_unroll(T, G, B):
    gi, wh, bh, h0, wout = gru_case(T, G, B, seed=1000 * T + 10 * G + B)
    ref, grads = gru_unroll_ref(gi, wh, bh, h0, wout)
    d = [x.cuda().requires_grad_() for x in (gi, wh, bh)]
    hs = ops.gru_sequence(d[0], d[1], d[2], h0=h0.cuda())
    err = float((hs.detach().double().cpu() - ref).abs().max())
    print("states: max error %.3e" % err)
    assert err < 1e-5
    assert th.equal(hs[:, 0].cpu(), h0)                                       # step 0 is loaded, bit for bit
    (hs * wout.cuda()).sum().backward()
    for x, r, name in zip(d, grads, ("d_gi", "d_wh", "d_bh")):
        _grad_ok(x.grad, r, name)
    assert not d[0].grad[0].any()                                             # d_gi[0] is exactly zero
    if T == 1:
        assert not d[1].grad.any() and not d[2].grad.any()
    with th.no_grad():                                                        # the no_grad form (no saved gates)
        hs2 = ops.gru_sequence(d[0], d[1], d[2], h0=h0.cuda())
    assert th.equal(hs2, hs)


def _parts_case(T, n, B, seed):
    """4 projection parts [n, T * B, 192], 2 weight parts over 2 n sets each, h0 [4 n, B, 64]"""
    gi, wh, bh, h0, wout = gru_case(T, 4 * n, B, seed=seed)
    parts = [gi[:, k * n:(k + 1) * n].permute(1, 0, 2, 3).reshape(n, T * B, 192).contiguous() for k in range(4)]
    return gi, wh, bh, h0, wout, parts


def test_parts_form_with_a_gradient_for_the_first_two_parts_only():
    T, n, B = 6, 5, 32
    gi, wh, bh, h0, wout, parts = _parts_case(T, n, B, seed=7)
    ref, grads = gru_unroll_ref(gi, wh, bh, h0, wout, grad_sets=2 * n)
    parts = [p.cuda().requires_grad_(k < 2) for k, p in enumerate(parts)]
    whs = [wh[:2 * n].cuda().requires_grad_(), wh[2 * n:].cuda()]
    bhs = [bh[:2 * n].cuda().requires_grad_(), bh[2 * n:].cuda()]
    hs = ops.gru_sequence_parts(parts, T, B, whs, bhs, h0=h0.cuda())
    full = th.cat(hs, dim=0)
    err = float((full.detach().double().cpu() - ref).abs().max())
    print("states: max error %.3e" % err)
    assert err < 1e-5 and th.equal(full[:, 0].cpu(), h0)
    sum((h * wout[k * n:(k + 1) * n].cuda()).sum() for k, h in enumerate(hs[:2])).backward()
    d_gi = th.stack([p.grad.reshape(n, T, B, 192) for p in parts[:2]]).reshape(2 * n, T, B, 192).permute(1, 0, 2, 3)
    _grad_ok(d_gi, grads[0][:, :2 * n], "d_gi")
    _grad_ok(whs[0].grad, grads[1][:2 * n], "d_wh")
    _grad_ok(bhs[0].grad, grads[2][:2 * n], "d_bh")
    assert not d_gi[0].any() and parts[2].grad is None and parts[3].grad is None


def test_bf16_instantiations_at_the_bf16_bar():
    T, G, B = 5, 4, 16
    gi, wh, bh, h0, wout = gru_case(T, G, B, seed=5)
    ref, grads = gru_unroll_ref(gi, wh, bh, h0, wout)
    d = [x.cuda().requires_grad_() for x in (gi, wh, bh)]
    f32 = ops.gru_sequence(d[0], d[1], d[2], h0=h0.cuda()).detach()
    ops.set_learner_precision(1)
    try:
        hs = ops.gru_sequence(d[0], d[1], d[2], h0=h0.cuda())
        (hs * wout.cuda()).sum().backward()
        with th.no_grad():                                                    # the bf16 form without saved gates (the target net's unroll)
            hs2 = ops.gru_sequence(d[0], d[1], d[2], h0=h0.cuda())
    finally:
        ops.set_learner_precision(2)
    err2 = float((hs2.double().cpu() - ref).abs().max())
    print("bf16 states without saved gates: max error %.3e" % err2)
    assert err2 < BF16_Q_TOL and th.equal(hs2[:, 0].cpu(), h0) and not th.equal(hs2, f32)
    err = float((hs.detach().double().cpu() - ref).abs().max())
    print("bf16 states: max error %.3e" % err)
    assert err < BF16_Q_TOL and th.equal(hs[:, 0].cpu(), h0)
    assert not th.equal(hs.detach(), f32)                                     # not the f32 instantiation
    for x, r, name in zip(d, grads, ("d_gi", "d_wh", "d_bh")):
        _grad_ok(x.grad, r, "bf16 " + name, tol=BF16_Q_TOL)
    assert not d[0].grad[0].any()


# ---- 5. chain identity on the device ----------------------------------------------------------------------------------------------------
def test_a_window_from_the_stored_state_is_the_slice_of_the_whole_unroll():
    T, G, B = 9, 3, 32
    gi, wh, bh, _, _ = gru_case(T, G, B, seed=11)
    gi, wh, bh = gi.cuda(), wh.cuda(), bh.cuda()
    with th.no_grad():
        hs = ops.gru_sequence(gi, wh, bh)
        for t0 in (0, 1, 4, 8):
            win = ops.gru_sequence(gi[t0:].contiguous(), wh, bh, h0=hs[:, t0].contiguous())
            err = float((win - hs[:, t0:]).abs().max())
            print("t0 = %d: max difference %.3e, bit for bit: %s" % (t0, err, th.equal(win, hs[:, t0:])))
            assert err < 1e-5


# ---- 6. h0 read in place ------------------------------------------------------------------------------------------------------------------
def test_strided_h0_is_read_in_place():
    T, n, B, Wn = 4, 5, 16, 6
    gi, wh, bh, h0, wout, parts = _parts_case(T, n, B, seed=13)
    field = th.zeros(B, Wn, n, 128)
    field.uniform_(-0.9, 0.9, generator=th.Generator().manual_seed(2))
    field = field.cuda()
    h = field[:, 0]
    views = [h[..., :64].transpose(0, 1), h[..., 64:].transpose(0, 1)] * 2   # live env / inc, target env / inc
    assert ops._gru_h0_in_place(views) == (128, Wn * n * 128)
    parts = [p.cuda() for p in parts]
    whs, bhs = [wh[:2 * n].cuda(), wh[2 * n:].cuda()], [bh[:2 * n].cuda(), bh[2 * n:].cuda()]
    with th.no_grad():
        got = th.cat(ops.gru_sequence_parts(parts, T, B, whs, bhs, h0=views), dim=0)
        ref = th.cat(ops.gru_sequence_parts(parts, T, B, whs, bhs, h0=th.cat([v.contiguous() for v in views], dim=0)), dim=0)
    assert th.equal(got, ref) and th.equal(got[:, 0], th.cat(views, dim=0))


# ---- 7. bounds: every operand in the poisoned arena ------------------------------------------------------------------------------------
def _ptrs(*regs):
    return (C.c_void_p * len(regs))(*[r.ptr for r in regs])


@pytest.mark.parametrize("strided", [False, True])
def test_sequence_launches_from_a_given_state_stay_inside_their_operands(strided):
    lib = abi.load_library()
    T, n, B, Wn = 3, 2, 32, 3
    G = 2 * n
    gi, wh, bh, h0, wout = gru_case(T, G, B, seed=17)
    parts = [gi[:, k * n:(k + 1) * n].permute(1, 0, 2, 3).contiguous().numpy() for k in range(2)]        # [n, T, B, 192] each
    if strided:       # [B, W, n, 128] cut at the last element the launch addresses: the field's slot 0 of the last row, exactly
        full = np.zeros((B, Wn, n, 128), np.float32)
        full[:, 0, :, :64], full[:, 0, :, 64:] = h0[:n].permute(1, 0, 2).numpy(), h0[n:].permute(1, 0, 2).numpy()
        h0_arr = full.reshape(-1)[:(B - 1) * Wn * n * 128 + n * 128]
        strides = (128, Wn * n * 128)
    else:
        h0_arr, strides = h0.numpy(), (B * 64, 64)
    st = th.cuda.current_stream().cuda_stream
    for train in (True, False):
        ar = Arena()
        rp = [ar.place("gi%d" % k, p, align=16) for k, p in enumerate(parts)]
        rw, rb = ar.place("wh", wh.numpy(), align=16), ar.place("bh", bh.numpy(), align=16)
        rh = ar.place("h0", h0_arr, align=16)
        hs = ar.reserve("hs", (G, T, B, 64), align=16)
        rzn = ar.reserve("rzn", (T, G, B, 192), align=16) if train else None
        ghn = ar.reserve("ghn", (T, G, B, 64), align=16) if train else None
        hp = (C.c_void_p * 2)(rh.ptr, rh.ptr + (256 if strided else n * B * 64 * 4))
        rc = lib.ssd_gru_seq_fwd_h0(_ptrs(*rp), 2, _ptrs(rw), _ptrs(rb), 1, hp, strides[0], strides[1], hs.ptr, rzn.ptr if train else None,
                                    ghn.ptr if train else None, T, G, B, st)
        assert rc == 0, lib.ssd_last_error()
        ar.check()
        assert np.array_equal(hs.array()[:, 0], h0.numpy())
        if train:
            assert not rzn.array()[0].any() and not ghn.array()[0].any()
            saved = hs.array().copy(), rzn.array().copy(), ghn.array().copy()
    ar = Arena()
    dhs = [ar.place("dhs%d" % k, wout[k * n:(k + 1) * n].numpy(), align=16) for k in range(2)]
    rin = [ar.place(name, a, align=16) for name, a in zip(("hs", "rzn", "ghn"), saved)]
    rw = ar.place("wh", wh.numpy(), align=16)
    dgi = [ar.reserve("d_gi%d" % k, (n, T, B, 192), align=16) for k in range(2)]
    dgh, dwh, dbh = ar.reserve("dgh", (G, T, B, 192), align=16), ar.reserve("d_wh", (G, 64, 192), align=16), ar.reserve("d_bh", (G, B // 16, 192), align=16)
    rc = lib.ssd_gru_seq_bwd_h0(_ptrs(*dhs), rin[0].ptr, rin[1].ptr, rin[2].ptr, _ptrs(rw), 1, _ptrs(*dgi), 2, dgh.ptr, dwh.ptr, dbh.ptr, T, G, G, B, st)
    assert rc == 0, lib.ssd_last_error()
    ar.check()
    assert not dgh.array()[:, 0].any() and not any(r.array()[:, 0].any() for r in dgi)
    _, grads = gru_unroll_ref(gi, wh, bh, h0, wout)
    got = np.concatenate([r.array() for r in dgi]).transpose(1, 0, 2, 3)
    _grad_ok(th.from_numpy(got.copy()), grads[0], "d_gi (arena)")
    _grad_ok(th.from_numpy(dwh.array().copy()), grads[1], "d_wh (arena)")


def _store_case(N, n, slots, layout, t):
    """ssd_store_hidden with every operand in an arena; returns (arena, dst region, the storage before, h_env, h_inc, rc)"""
    rng = np.random.default_rng(N * 100 + n * 10 + slots)
    shape = (n, N, 64) if layout == "agent_major" else (N, n, 1, 64)
    he, hi = rng.uniform(-1, 1, shape).astype(np.float32), rng.uniform(-1, 1, shape).astype(np.float32)
    before = rng.uniform(-1, 1, (N, slots, n, 128)).astype(np.float32)
    ar = Arena()
    rt = ar.place("t_index", np.array([t], np.int64), align=8, fill=0)
    re_, ri = ar.place("h_env", he, align=16), ar.place("h_inc", hi, align=16)
    dst = ar.place("dst", before, align=16, inout=True)
    a = abi.SsdStoreHiddenArgs()
    a.t_index, a.n_env, a.n_agents, a.t_slots, a.h_env, a.h_inc, a.dst = rt.ptr, N, n, slots, re_.ptr, ri.ptr, dst.ptr
    a.src_agent_stride, a.src_env_stride = (N * 64, 64) if layout == "agent_major" else (64, n * 64)
    return ar, a, dst, before, he, hi


@pytest.mark.parametrize("layout", ["agent_major", "env_major"])
@pytest.mark.parametrize("N,n,slots", [(3, 5, 4), (258, 10, 3)])
def test_store_hidden_writes_its_slot_and_nothing_else(N, n, slots, layout):
    lib = abi.load_library()
    st = th.cuda.current_stream().cuda_stream
    for t in (0, slots - 1, -1, slots):
        ar, a, dst, before, he, hi = _store_case(N, n, slots, layout, t)
        assert lib.ssd_store_hidden(C.byref(a), st) == 0, lib.ssd_last_error()
        ar.check()
        exp = before.copy()
        if 0 <= t < slots:
            env_major = (lambda h: h.transpose(1, 0, 2)) if layout == "agent_major" else (lambda h: h[:, :, 0])
            exp[:, t, :, :64], exp[:, t, :, 64:] = env_major(he), env_major(hi)
        assert dst.array().tobytes() == exp.tobytes(), (t, layout)         # the slot, and every other slot byte-identical


def test_store_hidden_refusals_launch_nothing():
    lib = abi.load_library()
    st = th.cuda.current_stream().cuda_stream
    assert lib.ssd_store_hidden(None, st) == INV and b"ssd_store_hidden" in lib.ssd_last_error()
    bad = [("t_index", 0), ("h_env", 0), ("h_inc", 0), ("dst", 0), ("n_env", 0), ("n_agents", 0), ("t_slots", 0), ("n_env", -1),
           ("dst", "+4"), ("h_env", "+8"), ("src_agent_stride", 6), ("src_env_stride", 66), ("src_env_stride", -64)]
    for field, value in bad:
        ar, a, dst, before, he, hi = _store_case(3, 5, 4, "agent_major", 1)
        setattr(a, field, getattr(a, field) + int(value) if isinstance(value, str) else value)
        assert lib.ssd_store_hidden(C.byref(a), st) == INV, field
        assert b"ssd_store_hidden" in lib.ssd_last_error(), field
        ar.check()
        assert dst.array().tobytes() == before.tobytes(), field


# ---- 8. the rollout files the state after every slot -----------------------------------------------------------------------------------
N_ENV, T_EP, BATCH = 32, 12, 16


def _ctx(drop=(), **over):
    from homophily_marl_amd.run import load_config, setup
    th.manual_seed(0)
    np.random.seed(11)
    cfg = load_config("cleanup", overrides=dict(dict(
        runner="hip_graph", batch_size_run=N_ENV, batch_size=BATCH, buffer_size=2 * N_ENV, buffer_cpu_only=False, store_state=False, obs_storage="code",
        env_args=dict(num_agents=5, map="default5", episode_limit=T_EP, seed=3), use_cuda=True, save_model=False, runner_stats=False,
        learner_log_interval=10 ** 12, strict_device_ops=True, train_graph=True, train_steps_per_rollout=2, train_window=5), **over))
    for k in drop:
        del cfg[k]
    return setup(cfg)


def _four_episodes(**over):
    """four rollouts with frozen weights (eager, rollout-graph capture, edge-graph capture, pure replays): the stored fields of each,
    the learner's whole-episode states on each stored episode, and the launch keys of a timestep"""
    ctx = _ctx(**over)
    try:
        episodes, states = [], []
        for _ in range(4):
            batch = ctx.runner.run(test_mode=False)
            th.cuda.synchronize()
            episodes.append({k: v.cpu().clone() for k, v in batch.data.transition_data.items()})
            with th.no_grad():
                shared = ctx.mac.unroll_shared(batch)
                parts, wh, bh = ctx.mac.unroll_pre(batch, shared)
                he, hi = ops.gru_sequence_parts(parts, T_EP + 1, N_ENV, wh, bh)               # [n, T + 1, N, 64] from zeros
            states.append((he.cpu(), hi.cpu()))
            ctx.buffer.insert_episode_batch(batch)
        keys = [k for _, k, _ in ctx.runner.timestep_launches()]
        plan = (ctx.runner.fast is not None, ctx.runner.pipe)
        return episodes, states, keys, plan
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


@pytest.mark.parametrize("form,over", [("pipelined", {}), ("four_launch", dict(pipeline_encode=False)), ("generic", dict(fast_policy=False))])
def test_rollout_files_the_state_the_learner_computes_on_the_stored_episode(form, over):
    on, states, keys_on, plan = _four_episodes(train_stored_state=True, **over)
    off, _, keys_off, plan_off = _four_episodes(train_stored_state=False, **over)
    assert plan == plan_off == {"pipelined": (True, True), "four_launch": (True, False), "generic": (False, False)}[form]
    assert "store_hidden" not in keys_off
    if form != "generic":
        assert keys_on == keys_off + ["store_hidden"]
    for e, (ep, ref, (he, hi)) in enumerate(zip(on, off, states)):
        assert "hidden" not in ref and ep["hidden"].shape == (N_ENV, T_EP + 1, 5, 128)
        for k in ref:
            assert th.equal(ep[k], ref[k]), (form, e, k)                      # every other field's bytes as with the key off
        err_e = float((ep["hidden"][..., :64] - he.permute(2, 1, 0, 3)).abs().max())
        err_i = float((ep["hidden"][..., 64:] - hi.permute(2, 1, 0, 3)).abs().max())
        print("%s episode %d: stored state against the learner's whole-episode states: env %.3e, inc %.3e" % (form, e, err_e, err_i))
        assert err_e < 1e-5 and err_i < 1e-5, (form, e)
        assert ep["hidden"][:, T_EP].abs().max() > 0                          # slot T is filed too


# ---- 9. the loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("burn_in,extra", [(0, {}), (2, {}), (2, dict(prioritized_replay=True, td_lambda=0.8))])
def test_loop_starts_every_window_from_the_buffers_stored_state(burn_in, extra, monkeypatch):
    """four iterations of run.train_iteration (two train steps each; the step is captured at the third, every replay checked against
    an eager evaluation by SSD_GRAPH_CHECK): row 0 of every train step was evaluated on the buffer's "hidden" at the recorded (ids, t0)"""
    from homophily_marl_amd.run import train_iteration
    monkeypatch.setenv("SSD_GRAPH_CHECK", "1")
    ctx = _ctx(train_burn_in=burn_in, train_stored_state=True, **extra)
    try:
        buf, learner = ctx.buffer, ctx.learner
        inner, seen = learner.train, []

        def train(sample, t_env, episode):
            inner(sample, t_env, episode)
            ids, t0 = buf.last_window_ids[:BATCH], buf.last_window_t0[:BATCH]
            stored = buf.data.transition_data["hidden"][ids, t0]               # [B, n, 128]
            he0, hi0 = learner.last_first_states
            assert th.equal(he0, stored[..., :64].transpose(0, 1)) and th.equal(hi0, stored[..., 64:].transpose(0, 1)), len(seen)
            assert th.equal(sample["hidden"][:, 0], stored)
            seen.append((learner.sample_out() is not None, t0.cpu().tolist()))
        learner.train = train
        ep = 0
        for _ in range(4):
            ep = train_iteration(ctx, ep)
        th.cuda.synchronize()
        assert len(seen) == 8 and learner._graph is not None and learner._check_n == 6      # the capturing call replays too
        assert any(max(t0) > 0 for _, t0 in seen)                            # windows that start mid-episode
        logs = learner._static_logs
        assert all(np.isfinite(float(logs[k])) for k in ("loss_value_env", "loss_value_inc", "loss_sim"))
        assert all(bool(th.isfinite(p).all()) for p in ctx.mac.parameters())
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


def test_key_false_is_the_loop_without_the_key():
    """train_stored_state absent against False: the stored bytes, the sampled (ids, t0) of every call and the learner's parameters after
    four iterations are equal bit for bit, and no "hidden" field exists"""
    from homophily_marl_amd.run import train_iteration
    runs = []
    for drop, over in ((("train_stored_state",), {}), ((), dict(train_stored_state=False))):
        ctx = _ctx(drop=drop, train_burn_in=2, **over)
        try:
            ids = []
            inner = ctx.learner.train

            def train(sample, t_env, episode, ctx=ctx, ids=ids, inner=inner):
                ids.append((ctx.buffer.last_window_ids.cpu().tolist(), ctx.buffer.last_window_t0.cpu().tolist()))
                inner(sample, t_env, episode)
            ctx.learner.train = train
            ep = 0
            for _ in range(4):
                ep = train_iteration(ctx, ep)
            th.cuda.synchronize()
            assert "store_hidden" not in [k for _, k, _ in ctx.runner.timestep_launches()]
            runs.append((ids, {k: v.cpu().clone() for k, v in ctx.buffer.data.transition_data.items()},
                         [p.detach().cpu().clone() for p in ctx.mac.parameters()], ctx.buffer._sample_calls))
        finally:
            ops.set_strict(False)
            ctx.runner.close_env()
    (ids_a, data_a, par_a, calls_a), (ids_b, data_b, par_b, calls_b) = runs
    assert len(ids_a) == 8 and ids_a == ids_b and calls_a == calls_b
    assert "hidden" not in data_a and set(data_a) == set(data_b)
    for k in data_a:
        assert th.equal(data_a[k], data_b[k]), k
    assert all(th.equal(a, b) for a, b in zip(par_a, par_b)) and len(par_a) > 0
