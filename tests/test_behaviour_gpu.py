"""GPU suite of the behaviour statistics: the export (k_behaviour_partials + k_behaviour_finish) against tests/behaviour_util.reference_stats
for exact equality, in and out of the poisoned arena of tests/arena_util.py, and the runners' use of it (config key behaviour_stats).

Shapes: the smallest at which the kernels can go wrong -- one env / one agent / one step; the golden batch's shape; the largest LEN
(n 10, A 16); 4 G + 1 and 8 G + 3 envs (ragged last workgroups) and W G + 5, more envs than one pass of the grid (G workgroups x W
waves); T = 65 and 129, past one and two passes of a wave's 64 / n time rows.  Slot T of every field holds out-of-range garbage and must not be counted."""
import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops

from . import behaviour_util as bu
from .arena_util import Arena

pytestmark = pytest.mark.gpu

G, W = abi.BEHAVIOUR_MAX_GROUPS, abi.BEHAVIOUR_WAVES
SHAPES = [(1, 1, 2, 9), (1, 1, 1, 9), (3, 12, 5, 9), (5, 3, 10, 16), (4 * G + 1, 2, 3, 8), (8 * G + 3, 1, 2, 9), (W * G + 5, 1, 2, 9), (2, 65, 5, 9), (2, 129, 5, 9)]
IDS = ["N%d_T%d_n%d_A%d" % s for s in SHAPES]
_cache = {}


def _case(shape):
    """(fields, reference vector) of a shape, computed once and shared (never modified)"""
    if shape not in _cache:
        N, T, n, A = shape
        fields = bu.seeded_batch(N, T, n, A, seed=7 * N + T + n)
        _cache[shape] = (fields, bu.reference_stats(*fields, A))
    return _cache[shape]


def _groups(N):
    return min(G, -(-N // W))


def _device_vec(fields, A, calls=1):
    t = [th.from_numpy(x).cuda() for x in fields]
    acc = th.zeros(bu.length(t[2].shape[2], A), dtype=th.float64, device="cuda")
    for _ in range(calls):
        ops.behaviour_stats(t[0], t[1], t[2], t[3], A, acc)
    return acc.cpu().numpy()


@pytest.fixture(autouse=True)
def _strict():
    """a device tensor that would leave the kernels is an error here"""
    was = ops.STRICT
    ops.set_strict(True)
    yield
    ops.set_strict(was)


# ---- the export ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_export_equals_the_reference_exactly(shape):
    fields, ref = _case(shape)
    got = _device_vec(fields, shape[3])
    assert got.dtype == np.float64 and (got == ref).all(), np.flatnonzero(got != ref)[:8]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_export_in_the_arena(shape):
    """every operand between poisoned bands (NaN around the f32 fields, out-of-domain integers around the i64 ones), acc pre-loaded,
    the workspace pre-filled: rows [0, groups) are written in every column, nothing else changes"""
    N, T, n, A = shape
    (actions, inc, reward, clean), ref = _case(shape)
    L = bu.length(n, A)
    acc0 = np.arange(L, dtype=np.float64) * 3.0 - 100.0
    ar = Arena()
    pa = ar.place("actions", actions, align=8, fill=1 << 41)
    pi = ar.place("actions_inc", inc, align=8, fill=9)
    pr, pc = ar.place("reward", reward, offset_in_16=4), ar.place("clean_num", clean, offset_in_16=12)
    written = np.zeros((G, L), dtype=bool)
    written[:_groups(N)] = True
    ws = ar.reserve("workspace", (G, L), dtype=np.int64, align=8, written=written)
    acc = ar.place("acc", acc0, align=8, fill=float("nan"), inout=True)
    a = abi.SsdBehaviourArgs(n_env=N, t_slots=T + 1, n_agents=n, n_actions=A, actions=pa.ptr, actions_inc=pi.ptr, reward=pr.ptr, clean_num=pc.ptr,
                             workspace=ws.ptr, acc=acc.ptr)
    lib = abi.load_library()
    abi.check(lib, lib.ssd_behaviour_stats(a, None))
    ar.check()
    assert (acc.array() == acc0 + ref).all()
    rows = ws.array()[:_groups(N)]
    assert (rows.sum(0) == ref).all() and rows[:, -2].sum() == N          # a row per workgroup, each with its own env count


# ---- accumulation, determinism, capture -------------------------------------------------------------------------------------------------------
def test_two_calls_double_and_repeats_are_bit_identical():
    shape = (4 * G + 1, 2, 3, 8)
    fields, ref = _case(shape)
    assert (_device_vec(fields, 8, calls=2) == 2 * ref).all()
    runs = [_device_vec(fields, 8).tobytes() for _ in range(10)]
    assert len(set(runs)) == 1 and runs[0] == ref.astype(np.float64).tobytes()


def test_the_call_can_be_captured_and_replayed():
    """the runner launches it eagerly; the export's contract (asynchronous on the given stream, no allocation) allows a capture"""
    shape = (3, 12, 5, 9)
    fields, ref = _case(shape)
    t = [th.from_numpy(x).cuda() for x in fields]
    acc = th.zeros(ref.size, dtype=th.float64, device="cuda")
    ws = ops.behaviour_workspace(5, 9, "cuda")
    th.cuda.synchronize()
    g = th.cuda.CUDAGraph()
    with th.cuda.graph(g):
        ops.behaviour_stats(t[0], t[1], t[2], t[3], 9, acc, ws)
    th.cuda.synchronize()
    assert (acc.cpu().numpy() == 0).all()                                 # a capture records, it does not run
    g.replay()
    assert (acc.cpu().numpy() == ref).all()
    g.replay()
    assert (acc.cpu().numpy() == 2 * ref).all()


def test_a_strided_device_field_is_refused_under_strict_device_ops():
    fields, _ = _case((3, 12, 5, 9))
    t = [th.from_numpy(x).cuda() for x in fields]
    with pytest.raises(RuntimeError, match="strict_device_ops"):
        ops.behaviour_stats(t[0], t[1], t[2].double(), t[3], 9, th.zeros(bu.length(5, 9), dtype=th.float64, device="cuda"))


# ---- the runners ------------------------------------------------------------------------------------------------------------------------------
N_ENV, T_EP, SEED = 48, 14, 21
FIELDS = ("actions", "actions_inc", "reward", "clean_num")
SUMMARY_KEYS = ("cleaners_per_env_mean", "role_idle_frac", "role_cleaner_frac", "role_harvester_frac", "role_mixed_frac", "inc_pos_rate",
                "inc_neg_rate", "rollout_incentives_to_cleanup_per", "rollout_incentives_to_harvest_per", "rollout_value_give_mean",
                "rollout_value_receive_mean", "harvest_time_mean", "clean_share_max")
RUNNERS = {"hip_graph": dict(runner="hip_graph"), "hip_graph_pipelined": dict(runner="hip_graph", steps_per_graph=2), "hip_vec": dict(runner="hip_vec")}


def _ctx(**over):
    from homophily_marl_amd.run import load_config, setup
    th.manual_seed(0)
    cfg = load_config("cleanup", overrides=dict(dict(
        batch_size_run=N_ENV, batch_size=8, buffer_size=N_ENV, buffer_cpu_only=False, store_state=False, obs_storage="code",
        env_args=dict(num_agents=5, map="default5", episode_limit=T_EP, seed=SEED), use_cuda=True, save_model=False, runner_stats=False,
        learner_log_interval=10 ** 12, strict_device_ops=True, test_nepisode=N_ENV), **over))
    return setup(cfg)


def _clone(batch):
    return tuple(batch[k].clone() for k in FIELDS)


def _ref(clones, A):
    return sum(bu.reference_stats(*(c.cpu().numpy() for c in ep), A) for ep in clones)


def _flat(blocks):
    return np.concatenate([blocks[k].reshape(-1) for k in bu.ORDER])


@pytest.mark.parametrize("name", list(RUNNERS))
def test_runner_accumulates_exactly_what_it_stored(name):
    """five training episodes (hip_graph: the eager one, the one that captures the rollout graph, the one that captures the opening and
    closing graphs, two that replay everything) and one test episode; the accumulators are per mode"""
    ctx = _ctx(behaviour_stats=True, **RUNNERS[name])
    r, A = ctx.runner, ctx.args.n_actions
    train = []
    for _ in range(5):
        batch = r.run(test_mode=False)
        train.append(_clone(batch))
        ctx.buffer.insert_episode_batch(batch)
    test = [_clone(r.run(test_mode=True))]
    if name.startswith("hip_graph"):
        assert any(x.graph is not None and x.begin_graph is not None and x.finish_graph is not None for x in r._bundles.values())
        assert r.pipe == (name == "hip_graph_pipelined")
    got, got_test = r.behaviour(), r.behaviour(test_mode=True)
    assert set(got) == set(bu.ORDER) and all(v.dtype == np.float64 for v in got.values())
    ref, ref_test = _ref(train, A), _ref(test, A)
    assert (_flat(got) == ref).all() and got["n_episodes"][0] == 5 * N_ENV and got["n_steps"][0] == 5 * N_ENV * T_EP
    assert (_flat(got_test) == ref_test).all() and got_test["n_episodes"][0] == N_ENV
    assert got["action_count"].sum() == 5 * N_ENV * T_EP * 5                  # every stored action is a valid one
    assert (_flat(r.behaviour(reset=True)) == ref).all() and (_flat(r.behaviour()) == 0).all() and (_flat(r.behaviour(test_mode=True)) == ref_test).all()
    ctx.runner.close_env()


def test_runner_logs_every_key_from_the_same_numbers():
    """runner_log_interval small: every episode is logged and zeroes the accumulator, so log entry k is the summary of episode k"""
    ctx = _ctx(behaviour_stats=True, runner="hip_graph", steps_per_graph=2, runner_stats=True, runner_log_interval=1)
    r, A, log = ctx.runner, ctx.args.n_actions, ctx.logger
    eps = []
    for _ in range(3):
        batch = r.run(test_mode=False)
        eps.append(_clone(batch))
        ctx.buffer.insert_episode_batch(batch)
    test = _clone(r.run(test_mode=True))
    for key in SUMMARY_KEYS:
        assert len(log.stats[key]) == 3 and len(log.stats["test_" + key]) == 1, key
        for k, ep in enumerate(eps):
            assert log.stats[key][k][1] == abi.behaviour_summary(_ref([ep], A), 5, A)[key], (key, k)
        assert log.stats["test_" + key][0][1] == abi.behaviour_summary(_ref([test], A), 5, A)[key], key
    assert len(log.stats["return_mean"]) == 3                             # the existing keys are logged alongside
    assert (_flat(r.behaviour()) == 0).all() and (_flat(r.behaviour(test_mode=True)) == 0).all()
    ctx.runner.close_env()


def test_key_on_changes_nothing_else():
    """same configuration and seed, key on against key off: three episodes bit-identical, the same launches per timestep, and nothing
    allocated with the key off"""
    seen = {}
    for on in (False, True):
        ctx = _ctx(behaviour_stats=on, runner="hip_graph", steps_per_graph=2)
        r = ctx.runner
        eps = []
        for _ in range(3):
            batch = r.run(test_mode=False)
            eps.append({k: batch[k].clone() for k in ("actions", "actions_inc", "reward", "obs", "agent_pos")})
            ctx.buffer.insert_episode_batch(batch)
        seen[on] = (eps, [(n, k) for n, k, _ in r.timestep_launches()])
        assert (getattr(r, "_beh_train", None) is not None) == on and getattr(r, "_beh_test", None) is None
        if not on:
            with pytest.raises(RuntimeError):
                r.behaviour()
        ctx.runner.close_env()
    assert seen[False][1] == seen[True][1] and len(seen[True][1]) == 3
    for a, b in zip(seen[False][0], seen[True][0]):
        for k in a:
            assert th.equal(a[k], b[k]), k
