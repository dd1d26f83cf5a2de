"""GPU suite of the reward models (config key reward_model; ssd_social_reward, csrc/ssd_social_reward.hip: k_social_reward): the kernel
against the numpy restatement of tests/social_reward_util.py to the bit inside a poisoned arena (dense and padded strides, env counts
that fill no wave, the project's slot count), the accumulator over two rollouts, the fused learner with the key on against the key-off
learner fed the shaped field (eager and captured, whole episodes and windows), and the training loop with the key absent, "individual"
and "inequity_aversion".  Every comparison is bit equality, the logged means included."""
import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests import social_reward_util as U
from tests.arena_util import POISON_F32, Arena

pytestmark = pytest.mark.gpu

MODELS = ("inequity_aversion", "prosocial")
# (N, t_slots, n): one group; three envs of three; N no multiple of the four envs of a wave; two digits of agents over 17 waves; the
# project's slot count (ten chunks of ten slots and nothing left: the chunk loop ends ON a boundary) over 33 waves, the last half empty
SHAPES = [(1, 2, 2), (3, 5, 3), (7, 22, 5), (67, 13, 10), (130, 101, 5)]
PADDED = [(7, 22, 5), (67, 13, 10)]


@pytest.fixture(scope="module")
def references():
    """the restatement of every (model, shape), computed once: (reward, scalars, shaped, accumulator from zero)"""
    out = {}
    for model in MODELS:
        for shape in SHAPES:
            N, T1, n = shape
            r = U.draw(N, T1, n, seed=100 + N)
            p = U.scalars(model, n)
            acc = np.zeros((N, n, 3))
            out[model, shape] = (r, p, U.shaped(model, r, p, acc), acc)
    for v in out.values():
        for a in v[0], v[2], v[3]:
            a.setflags(write=False)
    return out


def _strided(logical, env_stride, slot_stride):
    """(flat f32 array of exactly the extent, bool mask of the logical elements): the gaps hold the arena's NaN poison"""
    N, T1, n = logical.shape
    ext = (N - 1) * env_stride + (T1 - 1) * slot_stride + n
    flat = np.full(ext, POISON_F32, dtype=np.uint32).view(np.float32)
    mask = np.zeros(ext, dtype=bool)
    idx = (np.arange(N)[:, None, None] * env_stride + np.arange(T1)[None, :, None] * slot_stride + np.arange(n)[None, None, :])
    flat[idx] = logical
    mask[idx] = True
    return flat, mask, idx


def _launch(model, r, p, acc_start, strides=None, offset=0):
    N, T1, n = r.shape
    se, ss, de, ds = strides or (T1 * n, n, T1 * n, n)
    src, _, _ = _strided(r, se, ss)
    _, written, idx = _strided(r, de, ds)
    arena = Arena()
    a_src = arena.place("reward", src, offset_in_16=offset)
    a_dst = arena.reserve("shaped", written.shape, written=written, offset_in_16=(offset + 4) % 16)
    a_acc = arena.place("acc", acc_start, align=8, fill=0.0, inout=True) if acc_start is not None else None
    lib = abi.load_library()
    abi.check(lib, lib.ssd_social_reward(ops.REWARD_MODELS[model], a_src.ptr, a_dst.ptr, a_acc.ptr if a_acc else None, N, T1, n, se, ss, de, ds,
                                         float(p[0]), float(p[1]), float(p[2]), th.cuda.current_stream().cuda_stream))
    th.cuda.synchronize()
    arena.check()                    # bands, slack, the input and the gaps of the destination untouched; every logical element written
    return a_dst.array()[idx], (a_acc.array() if a_acc else None)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement_bit_for_bit(references, model, shape):
    r, p, ref, ref_acc = references[model, shape]
    got, acc = _launch(model, r, p, np.zeros(ref_acc.shape), offset=4)
    assert U.bit_equal(got, ref) and (got[:, -1] == 0).all() and (U.bits(got[:, -1]) == 0).all()
    assert U.bit_equal(acc, ref_acc)
    got_plain, none = _launch(model, r, p, None)                                  # acc NULL: the same rewards, nothing else written
    assert none is None and U.bit_equal(got_plain, ref)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", PADDED, ids=lambda s: "x".join(map(str, s)))
def test_kernel_honours_padded_strides(references, model, shape):
    """slot_stride = n + 3 and an env stride with a tail, different for source and destination"""
    r, p, ref, ref_acc = references[model, shape]
    N, T1, n = shape
    strides = (T1 * (n + 3) + 5, n + 3, T1 * (n + 3) + 11, n + 3)
    got, acc = _launch(model, r, p, np.zeros(ref_acc.shape), strides=strides)
    assert U.bit_equal(got, ref) and U.bit_equal(acc, ref_acc)


@pytest.mark.parametrize("model", MODELS)
def test_a_second_call_accumulates(references, model):
    shape = (7, 22, 5)
    r, p, ref, _ = references[model, shape]
    r2 = U.draw(*shape, seed=9)
    want = np.zeros((7, 5, 3))
    U.shaped(model, r, p, want)
    once = want.copy()
    ref2 = U.shaped(model, r2, p, want)
    dev = lambda x: th.from_numpy(np.array(x)).cuda()
    acc, out = th.zeros(7, 5, 3, dtype=th.float64, device="cuda"), th.empty(shape, device="cuda")
    assert ops.social_reward(dev(r), out, model, [float(x) for x in p], acc) is out
    assert U.bit_equal(out.cpu().numpy(), ref) and U.bit_equal(acc.cpu().numpy(), once)
    ops.social_reward(dev(r2), out, model, [float(x) for x in p], acc)
    assert U.bit_equal(out.cpu().numpy(), ref2) and U.bit_equal(acc.cpu().numpy(), want) and not np.array_equal(want, once)


def test_ops_passes_the_strides_of_a_slab_and_refuses_what_does_not_fit(references):
    """the graph runner's storage is a slab of the replay buffer: rows [lo, lo + N) of [size, t_slots, n]"""
    shape = (7, 22, 5)
    r, p, ref, _ = references["inequity_aversion", shape]
    big_r, big_o = th.full((21, 22, 5), float("nan"), device="cuda"), th.full((21, 22, 5), 3.0, device="cuda")
    big_r[7:14] = th.from_numpy(r.copy()).cuda()
    ops.social_reward(big_r[7:14], big_o[7:14], "inequity_aversion", [float(x) for x in p])
    assert U.bit_equal(big_o[7:14].cpu().numpy(), ref) and bool((big_o[:7] == 3.0).all()) and bool((big_o[14:] == 3.0).all())
    with pytest.raises(abi.SsdError, match="distinct buffers"):
        ops.social_reward(big_r[7:14], big_r[7:14], "inequity_aversion", [float(x) for x in p])
    with pytest.raises(ValueError):
        ops.social_reward(big_r[7:14], big_o[7:14].cpu(), "inequity_aversion", [float(x) for x in p])
    with pytest.raises(ValueError):
        ops.social_reward(big_r[7:14].double(), big_o[7:14], "inequity_aversion", [float(x) for x in p])


# ---- the fused learner ---------------------------------------------------------------------------------------------------------------------
def _params(mac):
    return [p.detach().cpu().numpy().copy() for p in mac.parameters()]


@pytest.mark.parametrize("window", [0, 6], ids=["episodes", "window6_burn2"])
@pytest.mark.parametrize("train_graph", [False, True], ids=["eager", "captured"])
def test_fused_learner_with_the_key_on_is_the_key_off_learner_on_the_shaped_field(train_graph, window):
    """the comparison of tests/test_social_reward_host.py on the device: the Cleanup-5 fixture's episodes (paid from the draw family, as
    there), observations as class codes, every operator on the HIP kernels -- five calls, so the captured learners replay their graphs twice.
    As on the host, the comparison departs from "the key-off learner fed a batch whose reward is the shaped field" in one stated way:
    the incentive head's per-receiver features carry r_j in every input set (unroll_shared -> unroll_other), obs_reward False or not, so
    the key-off learner's two controllers are shown the raw rewards (U.key_off_twin patches their unroll_shared, on the reference
    side only; its loss still reads `reward`, the shaped values).  Without that the two runs' network inputs differ."""
    from tests import train_window_util as W
    from tests.learner_util import load_fixture
    th.backends.cuda.matmul.allow_tf32 = False
    z, meta = load_fixture("learner_cleanup5.npz")
    over = dict(obs_reward=False, train_graph=train_graph)
    if window:
        over.update(train_window=window, train_burn_in=2)
    ops.set_strict(True)
    try:
        _, batch_on, mac_on, on = U.build_seeded(z, meta, device="cuda:0", code_obs=True, reward_model="inequity_aversion", **over)
        _, _, mac_off, off = U.build_seeded(z, meta, device="cuda:0", code_obs=True, **over)
        assert all(th.equal(a, b) for a, b in zip(mac_on.parameters(), mac_off.parameters()))
        U.add_field(batch_on)
        if window:
            buf = W.buffer_of(batch_on, size=2 * batch_on.batch_size)
            batch_on = buf.sample_windows(batch_on.batch_size, window, 2)
            assert batch_on.max_seq_length == window + 1 and bool(batch_on["reward_model"].any())
        batch_off = U.key_off_twin(batch_on, off)
        assert on._fused(batch_on) and off._fused(batch_off) and on.use_graph == off.use_graph == train_graph
        for call in range(5):
            on.train(batch_on, 0, 0)
            off.train(batch_off, 0, 0)
            th.cuda.synchronize()
            a, b = _params(mac_on), _params(mac_off)
            assert all(U.bit_equal(x, y) for x, y in zip(a, b)), call
            assert all(np.isfinite(x).all() for x in a)
        assert (on._graph is not None) == (off._graph is not None) == train_graph
        l_on, l_off = (x._static_logs if train_graph else x.cal_loss_and_step(y) for x, y in ((on, batch_on), (off, batch_off)))
        for k in ("loss_value_env", "loss_value_inc", "loss_sim"):
            assert float(l_on[k]) == float(l_off[k]) and np.isfinite(float(l_on[k])), (k, float(l_on[k]), float(l_off[k]))
    finally:
        ops.set_strict(False)


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------------
N_ENV, T_EP, BATCH = 8, 12, 4


def _ctx(drop=(), env="cleanup", **over):
    """8 envs, T = 12, hip_graph, f32 observations written into the replay buffer's own slots.  (Class codes at 8 envs cannot be written
    in place -- 8 x 13 x 5 x 225 code bytes per slab are no multiple of the env kernel's 16-byte rows --, so the test that needs them
    keeps the rollouts in the runner's own storage: replay_in_place False.)"""
    from homophily_marl_amd.run import load_config, setup
    th.manual_seed(0)
    np.random.seed(11)
    env_args = dict(num_agents=5, map="default5", episode_limit=T_EP, seed=3) if env == "cleanup" else dict(
        num_agents=5, map="default10", episode_limit=T_EP, view_size=7, seed=3)
    cfg = load_config(env, overrides=dict(dict(
        runner="hip_graph", batch_size_run=N_ENV, batch_size=BATCH, buffer_size=4 * N_ENV, buffer_cpu_only=False, store_state=False, obs_storage="f32",
        env_args=env_args, use_cuda=True, save_model=False, runner_stats=True,
        runner_log_interval=2 * T_EP, learner_log_interval=10 ** 12, strict_device_ops=True, train_graph=True, train_steps_per_rollout=2), **over))
    for k in drop:
        del cfg[k]
    return setup(cfg)


def _loop(ctx, iterations=3):
    from homophily_marl_amd.run import train_iteration
    ids, inner = [], ctx.learner.train

    def train(sample, t_env, episode):
        ids.append(ctx.buffer._draw_tensors(BATCH).ids.cpu().tolist())
        inner(sample, t_env, episode)
    ctx.learner.train = train
    ep = 0
    for _ in range(iterations):
        ep = train_iteration(ctx, ep)
    th.cuda.synchronize()
    return ids


def test_key_individual_is_the_loop_without_the_key():
    """key absent against "individual": stored bytes, sampled ids and parameters equal bit for bit, no field in the storage.
    (Observations as class codes, as in the sibling key-off tests: the learner's encoder then runs on the project's kernels, whose
    gradients have one summation order, so two runs of one loop can agree to the bit at all.)"""
    runs = []
    for drop, over in ((("reward_model", "ia_alpha", "ia_beta", "ia_decay", "prosocial_weight"), {}), ((), dict(reward_model="individual"))):
        ctx = _ctx(drop=drop, obs_storage="code", replay_in_place=False, **over)
        try:
            ids = _loop(ctx)
            assert ctx.args.reward_model == "individual" and getattr(ctx.runner, "_reward_acc", None) is None
            assert "reward_model" not in ctx.buffer.data.transition_data and "reward_model" not in ctx.buffer.scheme
            assert not [k for k in ctx.logger.stats if k.startswith(("reward_model", "ia_", "prosocial"))]
            runs.append((ids, {k: v.cpu().clone() for k, v in ctx.buffer.data.transition_data.items()},
                         [p.detach().cpu().clone() for p in ctx.mac.parameters()], ctx.buffer._sample_calls))
        finally:
            ops.set_strict(False)
            ctx.runner.close_env()
    (ids_a, data_a, par_a, calls_a), (ids_b, data_b, par_b, calls_b) = runs
    assert len(ids_a) == 6 and ids_a == ids_b and calls_a == calls_b and set(data_a) == set(data_b)
    for k in data_a:
        assert th.equal(data_a[k], data_b[k]), k
    assert all(th.equal(a, b) for a, b in zip(par_a, par_b)) and len(par_a) > 0


def test_loop_files_the_shaped_reward_of_every_training_rollout(monkeypatch):
    """three iterations with "inequity_aversion": the field of every training rollout is the restatement of its stored raw rewards, the raw
    field is what the rollout wrote, a test rollout launches nothing, the accumulator's cells at every log event are the restatement's
    to the bit, and so are the logged means: the runner sums the cells on the host in ascending (env, agent) and divides once
    (U.logged_mean)."""
    launches, inner = [], ops.social_reward

    def recorded(reward, out, model, params, acc=None):
        launches.append((reward.clone(), reward.data_ptr(), out.data_ptr()))
        return inner(reward, out, model, params, acc)
    monkeypatch.setattr(ops, "social_reward", recorded)
    ctx = _ctx(env="harvest", reward_model="inequity_aversion")     # (twelve steps of Cleanup pay nothing: no apple grows before the river is cleaned)
    cells, means = [], ctx.runner.reward_model_means

    def read(reset=True):                                             # the accumulator as every log event finds it, before it is zeroed
        cells.append(ctx.runner._reward_acc.cpu().numpy().copy())
        return means(reset)
    ctx.runner.reward_model_means = read
    try:
        a, buf = ctx.args, ctx.buffer
        n = a.n_agents
        assert a.reward_model_scalars == tuple(float(x) for x in U.scalars("inequity_aversion", n))
        assert buf.scheme["reward_model"]["vshape"] == (n,) and buf.data.transition_data["reward_model"].dtype == th.float32
        _loop(ctx)
        assert len(launches) == 3
        ctx.runner.run(test_mode=True)                                           # a test rollout: no launch
        th.cuda.synchronize()
        assert len(launches) == 3
        raw, field = buf.data.transition_data["reward"].cpu().numpy(), buf.data.transition_data["reward_model"].cpu().numpy()
        p = U.scalars("inequity_aversion", n)
        accs = [np.zeros((N_ENV, n, 3)), np.zeros((N_ENV, n, 3))]                 # the accumulator between the log events (below)
        for k, (seen, src, dst) in enumerate(launches):
            rows = slice(k * N_ENV, (k + 1) * N_ENV)
            assert src == buf.data.transition_data["reward"][rows].data_ptr() and dst == buf.data.transition_data["reward_model"][rows].data_ptr()
            assert U.bit_equal(raw[rows][:, :-1], seen.cpu().numpy()[:, :-1]), k          # the launch left the raw rewards as it found them
            assert U.bit_equal(field[rows], U.shaped("inequity_aversion", raw[rows], p, accs[min(k, 1)])), k
        assert raw[:3 * N_ENV, :-1].any(), "the rollouts earned nothing: the comparison would be 0 == 0"
        # the log events: the first rollout alone (the first event is due at once), then rollouts two and three together
        stats = ctx.logger.stats
        per = float(N_ENV * T_EP * n)
        assert len(cells) == 2 and all(U.bit_equal(got, want) for got, want in zip(cells, accs))
        assert not ctx.runner._reward_acc.any() and ctx.runner._reward_rollouts == 0          # zeroed by the event
        for name, col in (("reward_model_mean", 0), ("ia_envy_mean", 1), ("ia_guilt_mean", 2)):
            got = [v for _, v in stats[name]]
            assert len(got) == 2, (name, stats[name])
            for value, acc, rollouts in zip(got, accs, (1, 2)):
                want = U.logged_mean(acc, col, per * rollouts)
                print("%s: logged %.17g, restatement %.17g" % (name, value, want))
                assert value == want and value != 0, (name, value, want)
        assert "prosocial_others_mean" not in stats
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()
