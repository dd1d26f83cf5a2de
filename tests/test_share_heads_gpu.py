"""GPU suite: heads shared across agents (config key share_heads; DESIGN sections 4.2 and 7).

  6. ssd_tie_agent_grads alone, the flat buffer in the poisoned arena: 2 / 3 / 10 copies, every inner at which the launch takes another
     path, jobs at every residue of 16 bytes, one job and SSD_ADAM_MAX_JOBS jobs with gaps, +-0 / +-inf / NaN -- the buffer bit-equal to
     the numpy restatement (NaN payloads aside), every byte outside the extents untouched;
  7. ssd_agent_spread against numpy float64 on the same f32 inputs; equal copies give exactly 0; two launches give the same bits;
  8. six learner.train calls (eager, capture, replays) at "both" and "inc", and at "both" under Polyak updates, against the REFERENCE's
     recordings (tests/golden/learner_share_heads.npz), the invariant after every call, the logged spreads;
  9. the training loop: the key absent against "none" bit for bit with no tie launch issued, and the loop with the key on.
Host half: tests/test_share_heads_host.py; shared: tests/share_heads_util.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests import share_heads_util as U
from tests import soft_target_util as su
from tests.arena_util import POISON_F32, Arena

pytestmark = pytest.mark.gpu

# below a vector of 4, one vector, around a wave (64), around a workgroup's pass (256), a multiple of 4 a workgroup takes in several
# passes (4096) and its ragged neighbour
INNERS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4096, 4099]
GAPS = [0, 1, 2, 3, 5, 0, 7]                                            # elements between a job's end and the next job's start


def _values(rng, shape):
    g = (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 6, shape)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    hit = rng.random(shape) < 0.05
    g[hit] = special[rng.integers(0, 5, int(hit.sum()))]
    return g


def _layout(copies, inners, first):
    """jobs (offset, copies, inner) laid out with GAPS between them from offset `first`, and the buffer's length (a gap behind the last)"""
    jobs, off = [], first
    for k, inner in enumerate(inners):
        jobs.append((off, copies, inner))
        off += copies * inner + GAPS[k % len(GAPS)]
    return jobs, off + 3


def _run_tie(jobs, total, base_offset, seed):
    """one launch over a flat buffer placed at `base_offset` bytes past a 16-byte boundary; checks the whole buffer"""
    rng = np.random.default_rng(seed)
    flat = np.full(total, POISON_F32, dtype=np.uint32).view(np.float32).copy()           # the gaps: poison that must survive
    want = flat.copy()
    for off, copies, inner in jobs:
        g = _values(rng, (copies, inner))
        flat[off:off + copies * inner] = g.reshape(-1)
        want[off:off + copies * inner] = U.tie_np(g).reshape(-1)
    A = Arena()
    reg = A.place("flat", flat, offset_in_16=base_offset, inout=True)
    host = abi.tie_job_table(jobs)
    dev = th.tensor(list(host), dtype=th.int64, device="cuda")
    lib = abi.load_library()
    abi.check(lib, lib.ssd_tie_agent_grads(reg.ptr, total, host, dev.data_ptr(), len(jobs), None))
    A.check(allow_nan=("flat",))                                             # bands and slack around the buffer bit-identical
    got = reg.array()
    inside = np.zeros(total, bool)
    for off, copies, inner in jobs:
        inside[off:off + copies * inner] = True
        assert U.same_bits(got[off:off + copies * inner], want[off:off + copies * inner]), (off, copies, inner)
    assert (got.view(np.uint32)[~inside] == POISON_F32).all() and (~inside).sum() >= 3           # every byte outside the extents
    return jobs


@pytest.mark.parametrize("copies", [2, 3, 10])
def test_tie_launch_one_job_in_the_arena(copies):
    """one job per launch: every inner, at a job address on every residue of 16 bytes (buffer base x job offset)"""
    seen = set()
    for k, inner in enumerate(INNERS):
        for base in (0, 4, 8, 12) if inner in (4, 64, 4096) else ((4 * k) % 16,):
            first = (k + base // 4) % 4 + (1 if inner == 4096 else 0)
            jobs, total = _layout(copies, [inner], first)
            _run_tie(jobs, total, base, seed=100 * copies + k)
            seen.add((inner % 4 == 0, (base // 4 + first) % 4))
    assert {r for vec, r in seen if vec} == {0, 1, 2, 3} and {r for vec, r in seen if not vec} == {0, 1, 2, 3}


@pytest.mark.parametrize("copies", [2, 3, 10])
def test_tie_launch_with_the_largest_job_table_in_the_arena(copies):
    """SSD_ADAM_MAX_JOBS jobs with gaps of 0 .. 7 elements in one launch: job addresses on every residue, for the vector path too"""
    inners = [INNERS[(5 * k) % len(INNERS)] for k in range(abi.ADAM_MAX_JOBS)]
    jobs, total = _layout(copies, inners, 1)
    assert len(jobs) == abi.ADAM_MAX_JOBS == 64 and set(inners) == set(INNERS)
    base = 8
    res = {(inner % 4 == 0, (base // 4 + off) % 4) for off, _, inner in jobs}
    assert {r for vec, r in res if vec} == {0, 1, 2, 3} and {r for vec, r in res if not vec} == {0, 1, 2, 3}
    _run_tie(jobs, total, base, seed=copies)


def test_tie_launch_mixes_copy_counts_in_one_table():
    jobs, off = [], 2
    for k, inner in enumerate(INNERS):
        copies = (2, 3, 10, 5)[k % 4]
        jobs.append((off, copies, inner))
        off += copies * inner + GAPS[k % len(GAPS)]
    _run_tie(jobs, off + 1, 12, seed=7)


# ---- 7. the spread ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [2, 5, 10])
def test_spread_launch_against_float64(copies):
    rng = np.random.default_rng(copies)
    inners = [1, 3, 64, 255, 256, 257, 4099, 64]
    A = Arena()
    arrays, regs = [], []
    for k, inner in enumerate(inners):
        x = (rng.standard_normal((copies, inner)) * (0.1 if k % 2 else 3.0)).astype(np.float32)
        if k == len(inners) - 1:
            x[:] = x[:1]                                                       # equal copies
        arrays.append(x)
        regs.append(A.place("theta %d" % k, x, offset_in_16=(0, 4, 8, 12)[k % 4]))
    outs = [A.reserve("out %d" % r, (len(inners), 2), dtype=np.float64, align=8) for r in range(2)]
    host = abi.tie_job_table([(r.ptr, copies, inner) for r, inner in zip(regs, inners)])
    dev = th.tensor(list(host), dtype=th.int64, device="cuda")
    lib = abi.load_library()
    for out in outs:
        abi.check(lib, lib.ssd_agent_spread(host, dev.data_ptr(), len(inners), out.ptr, None))
    A.check()
    got = outs[0].array()
    assert got.tobytes() == outs[1].array().tobytes()                        # the same bits run to run
    for k, x in enumerate(arrays):
        want = U.spread_np(x)
        if k == len(inners) - 1:
            assert got[k, 0] == 0.0 and got[k, 1] > 0
        else:
            assert want[0] > 0
        assert np.allclose(got[k], want, rtol=U.SPREAD_RTOL, atol=0), (k, got[k], want)


# ---- 8. the device learner ------------------------------------------------------------------------------------------------------------
def _count(monkeypatch, name):
    lib = abi.load_library()
    inner, calls = getattr(lib, name), []

    def counted(*args):
        calls.append(1)
        return inner(*args)
    monkeypatch.setattr(lib, name, counted, raising=True)
    return calls


def _six_calls(monkeypatch, share, arm, **over):
    th.backends.cuda.matmul.allow_tf32 = False
    zs = U.golden()
    ties = _count(monkeypatch, "ssd_tie_agent_grads")
    batch, mac, learner, seen = U.fixture_learner(share, device="cuda:0", code_obs=True, train_graph=True, learner_log_interval=1, **over)
    assert learner._fused(batch) and learner.use_graph
    stats = []
    learner.logger = SimpleNamespace(log_stat=lambda k, v, t: stats.append((k, v, t)), console_logger=None)
    tags = U.TAGS[share]
    ops.set_strict(True)
    try:
        for k in range(1, 7):
            learner.train(batch, 10 * k, k)
            th.cuda.synchronize()
            assert (learner._graph is not None) == (k >= 3)
            U.assert_invariant(mac, learner, tags, "%s call %d" % (share, k))
            su.assert_call(zs, arm, k, seen[-1], mac, tag="device ")
            err, bar = U.moment_error(zs, arm, k, learner)
            assert err < bar, (arm, k, err, bar)
            # the first call takes the tensor-op tail (the rule as torch adds); the plan and its job table exist from the second on
            assert (learner._opt_plan not in (None, False)) == (k >= 2) and (k < 2 or learner._opt_plan.tie[4] == 18 * len(tags))
            for tag in ("env", "inc"):
                got = [v for key, v, t in stats if key == "head_spread_" + tag and t == 10 * k]
                want = U.head_spread_np(mac.agent, tag)
                assert len(got) == 1
                if tag in tags:
                    assert got[0] == 0.0 == want, (k, tag, got)
                else:
                    assert want > 0 and abs(got[0] - want) <= U.SPREAD_RTOL * want, (k, tag, got[0], want)
        # calls 2 (eager) and 3 (capture) went through the binding; the replays carry the launch inside graph g2
        assert len(ties) == 2
    finally:
        ops.set_strict(False)
    return mac, learner


@pytest.mark.parametrize("share", ["both", "inc"])
def test_six_train_calls_on_the_device_keep_the_copies_tied_and_match_the_reference(monkeypatch, share):
    _six_calls(monkeypatch, share, U.ARMS[share])


def test_six_train_calls_on_the_device_under_polyak_updates(monkeypatch):
    mac, learner = _six_calls(monkeypatch, "both", "bothtau0.25_", target_tau=0.25, target_update_interval=1)
    assert learner._opt_plan.args.n_polyak > 0
    assert not any(th.equal(a, b) for a, b in zip(learner.target_mac.parameters(), mac.parameters()))


# ---- 9. the loop ------------------------------------------------------------------------------------------------------------------------
def _loop_ctx(drop=(), **over):
    from tests.test_stored_state_gpu import _ctx
    return _ctx(drop=drop, batch_size_run=16, buffer_size=32, **over)


def test_key_absent_is_the_loop_at_none_and_issues_no_tie_launch(monkeypatch):
    """share_heads absent against "none": the stored bytes, the sampled ids of every call and every parameter after four iterations are
    equal bit for bit, and the tie's binding is never called"""
    from homophily_marl_amd.run import train_iteration
    ties = _count(monkeypatch, "ssd_tie_agent_grads")
    runs = []
    for drop, over in ((("share_heads",), {}), ((), dict(share_heads="none"))):
        ctx = _loop_ctx(drop=drop, train_burn_in=2, target_update_interval=3, **over)
        try:
            ids, inner = [], ctx.learner.train

            def train(sample, t_env, episode, ctx=ctx, ids=ids, inner=inner):
                ids.append((ctx.buffer.last_window_ids.cpu().tolist(), ctx.buffer.last_window_t0.cpu().tolist()))
                inner(sample, t_env, episode)
            ctx.learner.train = train
            ep = 0
            for _ in range(4):
                ep = train_iteration(ctx, ep)
            th.cuda.synchronize()
            assert ctx.args.share_heads == "none" and ctx.learner._tied == [] and ctx.learner._opt_plan.tie is None
            runs.append((ids, {k: v.cpu().clone() for k, v in ctx.buffer.data.transition_data.items()},
                         [p.detach().cpu().clone() for p in list(ctx.mac.parameters()) + list(ctx.learner.target_mac.parameters())]))
        finally:
            ops.set_strict(False)
            ctx.runner.close_env()
    (ids_a, data_a, par_a), (ids_b, data_b, par_b) = runs
    assert len(ids_a) == 8 and ids_a == ids_b and set(data_a) == set(data_b)
    for k in data_a:
        assert th.equal(data_a[k], data_b[k]), k
    assert all(th.equal(a, b) for a, b in zip(par_a, par_b)) and len(par_a) > 0
    assert not ties


def test_loop_with_tied_heads(monkeypatch):
    """four iterations of the training loop at "both" (rollout kernels, windows, the captured step): the rollout reads the n equal
    copies as it reads any weights; the copies, their Adam state and the target copies stay equal to the bit"""
    from homophily_marl_amd.run import train_iteration
    ties = _count(monkeypatch, "ssd_tie_agent_grads")
    ctx = _loop_ctx(share_heads="both", train_burn_in=2, target_update_interval=3, learner_log_interval=12)
    try:
        stats = []
        inner = ctx.logger.log_stat
        ctx.logger.log_stat = lambda key, value, t: (stats.append((key, value)), inner(key, value, t))[1]
        assert all(U.bits_equal_across_agents(p) for _, p in ctx.mac.agent.tied_parameters()) and len(ctx.learner._tied) == 36
        ep = 0
        for _ in range(4):
            ep = train_iteration(ctx, ep)
        th.cuda.synchronize()
        assert ctx.train_steps == 8 and ctx.learner._graph is not None
        U.assert_invariant(ctx.mac, ctx.learner, U.TAGS["both"], "after the loop")
        assert all(bool(th.isfinite(p).all()) for p in ctx.mac.parameters())
        spreads = [v for k, v in stats if k.startswith("head_spread_")]
        assert len(spreads) >= 2 and all(v == 0.0 for v in spreads)
        assert len(ties) == 2                                                   # steps 2 (eager) and 3 (capture); the replays hold the launch
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()
