"""CPU suite of prioritised replay (config key prioritized_replay; ssd_priority_sample / ssd_priority_update;
ReplayBuffer.enable_priorities / sample_prioritized): ops' host restatement of the draw against tests/priority_util.py (written from
the header), the proportionality of the draw, the exports' constants as compiled and refusals, the tensor-op learner with per-sample
weights, the buffer's resets on insert, the config refusals, and the key off as today's path."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops, run
from homophily_marl_amd.components.episode_buffer import ReplayBuffer
from tests import priority_util as P
from tests.learner_util import build, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = abi.SSD_ERR_INVALID
SEED = P.SEED


def _host_sample(seed, call, table, population, count, n_starts, beta):
    ids, t0 = th.full((count,), -7, dtype=th.long), th.full((count,), -7, dtype=th.long)
    w, log = th.full((count,), -7.0), th.full((4,), -7.0)
    ops.priority_sample(seed, call, th.as_tensor(table), population, count, n_starts, beta, ids, t0, w, log)
    return ids, t0, w, log


# ---- 1. the restatements agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("population", [1, 2, 63, 64, 65, 1023, 1025, 8192])
def test_host_draws_are_the_header_arithmetic(population):
    for name, table in P.tables(population).items():
        for count in (1, 16, 64, 1024):
            for seed, call, n_starts, beta in ((SEED, 0, 1, 0.4), (2 ** 64 - 1, 2 ** 32 - 1, 76, 1.0)):
                ids, t0, w, log = _host_sample(seed, call, table, population, count, n_starts, beta)
                ref = P.sample(seed, call, table, population, count, n_starts, beta)
                assert ids.tolist() == ref["ids"] and t0.tolist() == ref["t0"], (name, count, call)
                assert 0 <= min(ref["ids"]) and max(ref["ids"]) < population and ref["ids"] == sorted(ref["ids"])
                assert 0 <= min(ref["t0"]) and max(ref["t0"]) < n_starts
                assert np.allclose(w.numpy(), ref["weights"], rtol=1e-6, atol=0) and float(w.max()) == 1.0, (name, count)
                assert np.allclose(log.numpy(), ref["log"], rtol=1e-6, atol=0), (name, count, log, ref["log"])


def test_beta_zero_gives_unit_weights_and_whole_episodes_start_at_zero():
    table = P.tables(65)["random_30pct_zero"]
    ids, t0, w, log = _host_sample(SEED, 3, table, 65, 16, 1, 0.0)
    assert w.tolist() == [1.0] * 16 and t0.tolist() == [0] * 16 and float(log[2]) == 1.0


def test_vectorised_restatement_is_the_scalar_one():
    table = P.tables(64)["random_30pct_zero"]
    got = P.ids_of_calls(SEED, [0, 5, 2 ** 32 - 1], table, 64, 16)
    for row, call in zip(got, (0, 5, 2 ** 32 - 1)):
        assert row.tolist() == P.sample(SEED, call, table, 64, 16, 1, 0.4)["ids"]
    big = np.full(64, P.QMAX, np.int32)                                      # widths above 2^32 never occur at 64 entries; at 2^20 they do
    wide = np.full(1 << 20, P.QMAX, np.int32)
    assert P.ids_of_calls(SEED, [7], wide, 1 << 20, 16)[0].tolist() == P.sample(SEED, 7, wide, 1 << 20, 16, 1, 0.4)["ids"]
    assert P.ids_of_calls(SEED, [7], big, 64, 16)[0].tolist() == P.sample(SEED, 7, big, 64, 16, 1, 0.4)["ids"]


# ---- 2. proportionality ------------------------------------------------------------------------------------------------------------------
def _frequencies_within_five_sigma(table, label):
    """10^5 calls of count 16: every entry's empirical frequency within 5 standard deviations of qeff / total.  The deviation is the
    multinomial one, sqrt(p (1 - p) / draws): stratified sampling only lowers an entry's variance (its count is a sum of independent
    Bernoulli draws, one per stratum, whose success probabilities add up to 16 p), so the bound is the looser of the two."""
    calls, count = 100000, 16
    ids = P.ids_of_calls(SEED, np.arange(calls), table, 64, count)
    draws = calls * count
    freq = np.bincount(ids.ravel(), minlength=64) / draws
    qeff, qmax, total = P.effective(table, 64)
    p = qeff / total
    sd = np.sqrt(p * (1 - p) / draws)
    z = np.abs(freq - p) / sd
    print("%s: largest deviation %.2f sd at entry %d (p %.3e)" % (label, z.max(), int(z.argmax()), p[int(z.argmax())]))
    assert (z <= 5.0).all(), (label, int(z.argmax()), float(z.max()))


def test_draws_are_proportional_to_the_priorities():
    table = np.rint(2.0 ** (24.0 * np.arange(64) / 63.0)).astype(np.int32)            # 1 .. 2^24, geometric
    assert table[0] == 1 and table[-1] == P.QMAX
    _frequencies_within_five_sigma(table, "geometric 1 .. 2^24")


def test_an_all_zero_table_is_drawn_uniformly():
    _frequencies_within_five_sigma(np.zeros(64, np.int32), "all zero")


# ---- 3. exports: constants as compiled, refusals --------------------------------------------------------------------------------------------
def test_exports_are_declared_exported_and_mirrored():
    """declaration, export and argtypes of every name of the table: tests/test_abi_symbols.py"""
    assert {"ssd_priority_sample", "ssd_priority_update"} <= set(abi.HIP_SIGNATURES)
    assert abi.load_library().ssd_abi_version() == abi.ABI_VERSION == 10     # two exports more, no version change


def test_struct_sizes_and_constants_as_compiled(tmp_path):
    """the constants and the two declarations as a C compiler sees them (sizeof / offsetof: tests/test_abi_symbols.py)"""
    c = tmp_path / "p.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssd_hip.h"\nint main(){\n'
                 'printf("%u %u %d %d\\n", SSD_PRIORITY_ONE, SSD_PRIORITY_MAX, SSD_PRIORITY_POP_MAX, SSD_SAMPLE_IDS_MAX);\n'
                 'int (*f)(const ssd_priority_sample_args*, void*) = ssd_priority_sample;\n'
                   'int (*g)(const ssd_priority_update_args*, void*) = ssd_priority_update;\nreturn f == 0 || g == 0;}')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "p.o")])   # the declarations are usable
    c.write_text(re.sub(r"int \(\*f\).*return f == 0 \|\| g == 0;", "return 0;", c.read_text(), flags=re.S))
    exe = tmp_path / "p"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.PRIORITY_ONE, abi.PRIORITY_MAX, abi.PRIORITY_POP_MAX, abi.SAMPLE_IDS_MAX] == [65536, 1 << 24, 1 << 20, 1024]


PTR = 1 << 20                    # a dummy device pointer: non-null, 16-byte aligned, never touched (the checks run before any launch)
NAN = float("nan")


def _sample_args(**over):
    t = abi.SsdPrioritySampleArgs()
    t.seed, t.call, t.population, t.count, t.n_starts, t.beta = 7, 0, 2000, 16, 8, 0.4
    t.table = t.ids = t.t0 = t.weights = t.log = PTR
    for k, v in over.items():
        setattr(t, k, v)
    return t


def _update_args(**over):
    t = abi.SsdPriorityUpdateArgs()
    t.batch, t.t_slots, t.n_agents, t.n_actions, t.table_len, t.alpha, t.eta, t.eps = 16, 101, 5, 9, 4096, 0.6, 0.9, 1e-3
    t.partials = t.ids = t.weights = t.dq_env = t.dq_inc = t.q_new = t.table = PTR
    for k, v in over.items():
        setattr(t, k, v)
    return t


SAMPLE_REFUSALS = [("null %s" % k, {k: None}) for k in ("table", "ids", "t0", "weights", "log")] + [
    ("population 0", dict(population=0)), ("population -1", dict(population=-1)), ("population over SSD_PRIORITY_POP_MAX", dict(population=(1 << 20) + 1)),
    ("count 0", dict(count=0)), ("count -1", dict(count=-1)), ("count over SSD_SAMPLE_IDS_MAX", dict(count=1025)),
    ("n_starts 0", dict(n_starts=0)), ("n_starts -1", dict(n_starts=-1)),
    ("beta below 0", dict(beta=-0.01)), ("beta above 1", dict(beta=1.01)), ("beta NaN", dict(beta=NAN)), ("table at an odd address", dict(table=PTR + 2))]
UPDATE_REFUSALS = [("null %s" % k, {k: None}) for k in ("partials", "ids", "weights", "dq_env", "dq_inc", "q_new", "table")] + [
    ("batch 0", dict(batch=0)), ("batch -1", dict(batch=-1)), ("batch over SSD_SAMPLE_IDS_MAX", dict(batch=1025)),
    ("t_slots 1", dict(t_slots=1)), ("n_agents 0", dict(n_agents=0)), ("n_actions 0", dict(n_actions=0)),
    ("table_len 0", dict(table_len=0)), ("table_len over SSD_PRIORITY_POP_MAX", dict(table_len=(1 << 20) + 1)),
    ("alpha below 0", dict(alpha=-0.5)), ("alpha above 1", dict(alpha=1.5)), ("alpha NaN", dict(alpha=NAN)),
    ("eta below 0", dict(eta=-0.5)), ("eta above 1", dict(eta=1.5)), ("eta NaN", dict(eta=NAN)),
    ("eps 0", dict(eps=0.0)), ("eps negative", dict(eps=-1e-3)), ("eps NaN", dict(eps=NAN)),
    ("rows over SSD_ROWS32_MAX", dict(batch=1024, t_slots=1 << 20, n_agents=16)),
    ("partials off a 16-byte boundary", dict(partials=PTR + 4)), ("dq_env at an odd address", dict(dq_env=PTR + 2))]


@pytest.mark.parametrize("case", SAMPLE_REFUSALS, ids=[c[0].replace(" ", "_") for c in SAMPLE_REFUSALS])
def test_invalid_draw_is_refused_with_a_message(case):
    """only invalid calls are made: nothing here reaches a launch"""
    label, over = case
    lib = abi.load_library()
    rc = lib.ssd_priority_sample(C.byref(_sample_args(**over)), None)
    assert rc == INV and b"ssd_priority_sample" in lib.ssd_last_error(), (label, rc, lib.ssd_last_error())
    with pytest.raises(abi.SsdError):
        abi.check(lib, rc)


@pytest.mark.parametrize("case", UPDATE_REFUSALS, ids=[c[0].replace(" ", "_") for c in UPDATE_REFUSALS])
def test_invalid_update_is_refused_with_a_message(case):
    label, over = case
    lib = abi.load_library()
    rc = lib.ssd_priority_update(C.byref(_update_args(**over)), None)
    assert rc == INV and b"ssd_priority_update" in lib.ssd_last_error(), (label, rc, lib.ssd_last_error())


def test_null_args_are_refused():
    lib = abi.load_library()
    assert lib.ssd_priority_sample(None, None) == INV and b"ssd_priority_sample" in lib.ssd_last_error()
    assert lib.ssd_priority_update(None, None) == INV and b"ssd_priority_update" in lib.ssd_last_error()


def test_ops_refuse_what_the_exports_refuse():
    ids, t0, w, log, table = th.zeros(4, dtype=th.long), th.zeros(4, dtype=th.long), th.zeros(4), th.zeros(4), th.ones(8, dtype=th.int32)
    for pop, count, n_starts, beta in ((0, 4, 1, 0.4), (9, 4, 1, 0.4), (8, 0, 1, 0.4), (8, 4, 0, 0.4), (8, 4, 1, 1.5), (8, 4, 1, NAN)):
        with pytest.raises(ValueError):
            ops.priority_sample(1, 0, table, pop, count, n_starts, beta, ids, t0, w, log)
    with pytest.raises(ValueError):
        ops.priority_sample(1, 0, table, 8, 5, 1, 0.4, ids, t0, w, log)      # outputs shorter than count
    part, dqe, dqi, q = th.zeros(4 * 2 * 3, 16), th.zeros(4, 3, 3, 5), th.zeros(4, 3, 3, 3, 3), th.zeros(4, dtype=th.int32)
    for alpha, eta, eps in ((1.5, 0.9, 1e-3), (0.6, -0.1, 1e-3), (0.6, 0.9, 0.0), (NAN, 0.9, 1e-3)):
        with pytest.raises(ValueError):
            ops.priority_update(part, ids, w, dqe, dqi, q, table, alpha, eta, eps)
    with pytest.raises(ValueError):
        ops.priority_update(part[:-1], ids, w, dqe, dqi, q, table, 0.6, 0.9, 1e-3)


# ---- 4. ops' host restatement of the update --------------------------------------------------------------------------------------------------
def test_host_update_is_the_header_arithmetic():
    rng = np.random.default_rng(5)
    B, T, n, A = 6, 7, 3, 5
    part = np.zeros((B * T * n, 16), np.float32)
    part[:, 0] = rng.random(B * T * n) < 0.7
    part[:, 2], part[:, 3] = rng.random(B * T * n) * part[:, 0], 4 * rng.random(B * T * n) * part[:, 0]
    part[:T * n] = 0                                                         # sample 0 carries no loss row
    ids = [3, 9, 3, 10, -1, 3]                                               # a triple, an id at table_len, a negative one
    table0 = np.arange(10, dtype=np.int32) + 100
    w = rng.random(B).astype(np.float32)
    dqe, dqi = rng.standard_normal((B, T + 1, n, A)).astype(np.float32), rng.standard_normal((B, T + 1, n, n, 3)).astype(np.float32)
    table, te, ti, q = th.as_tensor(table0.copy()), th.as_tensor(dqe.copy()), th.as_tensor(dqi.copy()), th.zeros(B, dtype=th.int32)
    out = ops.priority_update(th.as_tensor(part), th.as_tensor(ids), th.as_tensor(w), te, ti, q, table, 0.6, 0.9, 1e-3)
    exact, want = P.q_new(part, B, 0.6, 0.9, 1e-3)
    assert out is q and q.tolist() == want.tolist() and want[0] == np.rint((1e-3) ** 0.6 * 65536)
    assert np.array_equal(te.numpy(), dqe * w[:, None, None, None]) and np.array_equal(ti.numpy(), dqi * w[:, None, None, None, None])
    assert table.tolist() == P.write_back(table0, ids, want).tolist() and table[3] == max(want[0], want[2], want[5])


# ---- 5. the tensor-op learner with per-sample weights ----------------------------------------------------------------------------------------
def _learner(overrides=None):
    z, meta = load_fixture("learner_cleanup5.npz")
    return build(z, meta, overrides=overrides)


def _step(learner, batch, weights=None):
    """(logs as floats, the flat gradient) of one forward_backward; weights: the batch carries a priority tuple with a host table"""
    batch.priority = batch.priority_log = None
    if weights is not None:
        batch.priority = (th.zeros(8, dtype=th.int32), th.arange(batch.batch_size), th.as_tensor(weights, dtype=th.float32))
    logs = learner.forward_backward(batch)
    return {k: float(v) for k, v in logs.items()}, learner._flat_grad.clone()


@pytest.mark.parametrize("lam", [0.0, 0.8])
def test_unit_weights_reproduce_todays_losses_and_gradients_exactly(lam):
    args, batch, mac, learner = _learner(dict(td_lambda=lam))
    assert not learner._fused(batch)
    logs0, g0 = _step(learner, batch)
    logs1, g1 = _step(learner, batch, weights=[1.0] * 4)
    assert logs0 == logs1 and th.equal(g0, g1) and float(g0.abs().max()) > 0


def test_weighted_gradient_is_the_weighted_sum_of_the_samples_shares():
    """random weights in (0, 1]: the gradient equals sum_e w_e g_e, g_e the gradient with every other weight zeroed, within 1e-6 of
    the gradient's largest element (f32 sums in another order); the logged losses stay the unweighted ones; the restated
    priorities of the step land in the host table."""
    args, batch, mac, learner = _learner()
    logs0, g0 = _step(learner, batch)
    w = np.random.default_rng(11).uniform(0.05, 1.0, 4)
    w[2] = 1.0
    logs, g = _step(learner, batch, weights=w)
    table = batch.priority[0].clone()
    assert logs == logs0
    want = th.zeros_like(g, dtype=th.float64)
    for e in range(4):
        one = np.zeros(4)
        one[e] = 1.0
        want += w[e] * _step(learner, batch, weights=one)[1].double()
    err = float((g.double() - want).abs().max()) / float(want.abs().max())
    print("weighted gradient against the weighted sum: %.3e of the largest element" % err)
    assert err <= 1e-6
    assert float((g - g0).abs().max()) > 1e-3 * float(g0.abs().max())          # the weights do something
    exact, q = P.q_new(learner.last_td_rows.numpy(), 4, 0.6, 0.9, 1e-3)
    assert learner.last_q_new.tolist() == q.tolist() and table[:4].tolist() == q.tolist() and table[4:].tolist() == [0] * 4


# ---- 6. the buffer ---------------------------------------------------------------------------------------------------------------------------
def _buffer(size=8):
    args, batch, mac, learner = _learner()
    derived = {"filled"} | {new for new, _ in batch.preprocess.values()}
    scheme = {k: v for k, v in batch.scheme.items() if k not in derived}
    return ReplayBuffer(scheme, batch.groups, size, batch.max_seq_length, preprocess=batch.preprocess, device="cpu"), batch


def test_no_table_without_the_key_and_inserts_zero_exactly_the_advanced_slots():
    buf, batch = _buffer(10)
    buf.insert_episode_batch(batch)
    assert buf.priority_table is None and buf._draws.weights is None and buf._draws.log is None
    with pytest.raises(ValueError, match="enable_priorities"):
        buf.sample_prioritized(2)
    table = buf.enable_priorities()
    assert table is buf.enable_priorities() and table.dtype == th.int32 and table.tolist() == [0] * 10
    table.copy_(th.arange(10) + 50)
    buf.insert_episode_batch(batch)                                          # slots 4 .. 7, the copying path
    assert table.tolist() == [50, 51, 52, 53, 0, 0, 0, 0, 58, 59] and buf.buffer_index == 8
    table.copy_(th.arange(10) + 50)
    buf.insert_episode_batch(batch)                                          # slots 8, 9, 0, 1: around the ring's end
    assert table.tolist() == [0, 0, 52, 53, 54, 55, 56, 57, 0, 0] and buf.buffer_index == 2
    table.copy_(th.arange(10) + 50)
    view = buf.reserve(3)                                                    # slots 2 .. 4 written in place
    assert table.tolist() == list(range(50, 60))                             # reserving alone resets nothing
    buf.insert_episode_batch(view)
    assert table.tolist() == [50, 51, 0, 0, 0, 55, 56, 57, 58, 59] and buf.buffer_index == 5


def test_host_sample_prioritized_draws_from_the_table_and_carries_the_tuple():
    buf, batch = _buffer(8)
    buf.insert_episode_batch(batch)
    buf.insert_episode_batch(batch)
    table = buf.enable_priorities()
    table.copy_(th.tensor([1, 0, 1 << 24, 5, 0, 70000, 1, 9], dtype=th.int32))
    np.random.seed(3)
    s = buf.sample_prioritized(4, beta=0.7)
    ref = P.sample(buf._sample_seed, 0, table.numpy(), 8, 4, 1, 0.7)
    tab, ids, w = s.priority
    assert tab is table and ids.tolist() == ref["ids"] and np.allclose(w.numpy(), ref["weights"], rtol=1e-6) and buf._sample_calls == 1
    assert np.array_equal(s["reward"].numpy(), buf["reward"].numpy()[ref["ids"]]) and s.max_seq_length == buf.max_seq_length
    s2 = buf.sample_prioritized(4, window=6, burn_in=2, beta=0.7)
    ref2 = P.sample(buf._sample_seed, 1, table.numpy(), 8, 4, buf.max_seq_length - 6, 0.7)
    assert s2.priority[1].data_ptr() == ids.data_ptr() and s2.priority[2].data_ptr() == w.data_ptr()      # persistent tensors
    assert ids.tolist() == ref2["ids"] and buf.last_window_t0.tolist() == ref2["t0"] and s2.max_seq_length == 7 and buf._sample_calls == 2
    assert np.allclose(s2.priority_log.numpy(), ref2["log"], rtol=1e-6)
    with pytest.raises(ValueError):
        buf.sample_prioritized(4, window=buf.max_seq_length)


# ---- 7. the config keys ----------------------------------------------------------------------------------------------------------------------
def _ctx(**keys):
    a = SimpleNamespace(runner="r", batch_size=16, **keys)
    enabled = []
    buf = SimpleNamespace(device="cuda:0", enable_priorities=lambda: enabled.append(1))
    return a, buf, SimpleNamespace(fixed_length_episodes=True), enabled


@pytest.mark.parametrize("keys,match", [
    (dict(per_alpha=1.1), "per_alpha"), (dict(per_alpha=-0.1), "per_alpha"), (dict(per_alpha=NAN), "per_alpha"),
    (dict(per_beta=1.1), "per_beta"), (dict(per_beta=-0.1), "per_beta"), (dict(per_eta=2.0), "per_eta"), (dict(per_eta=NAN), "per_eta"),
    (dict(per_eps=0.0), "per_eps"), (dict(per_eps=-1.0), "per_eps"), (dict(per_eps=NAN), "per_eps"), (dict(per_beta_anneal_steps=-1), "per_beta_anneal_steps"),
    (dict(prioritized_replay=True, _host=True), "device-resident"), (dict(prioritized_replay=True, _ragged=True), "device-resident"),
    (dict(prioritized_replay=True, fused_loss=False), "fused loss"), (dict(prioritized_replay=True, batch_size=1025), "SSD_SAMPLE_IDS_MAX")])
def test_setup_refuses_bad_priority_keys(keys, match):
    keys = dict(keys)
    host, ragged = keys.pop("_host", False), keys.pop("_ragged", False)
    a, buf, runner, enabled = _ctx()
    for k, v in keys.items():
        setattr(a, k, v)
    buf.device = "cpu" if host else buf.device
    runner.fixed_length_episodes = not ragged
    with pytest.raises(ValueError, match=match):
        run._check_prioritized(a, buf, runner)
    assert not enabled


def test_setup_fills_the_defaults_and_enables_the_table_only_with_the_key():
    a, buf, runner, enabled = _ctx()
    assert run._check_prioritized(a, buf, runner) is False and not enabled
    assert (a.prioritized_replay, a.per_alpha, a.per_beta, a.per_beta_anneal_steps, a.per_eta, a.per_eps) == (False, 0.6, 0.4, 0, 0.9, 1e-3)
    a, buf, runner, enabled = _ctx(prioritized_replay=True, per_alpha=0.0, per_beta=1.0, per_eta=0.0)
    assert run._check_prioritized(a, buf, runner) is True and enabled == [1]
    cfg = run.load_config("cleanup")
    assert (cfg["prioritized_replay"], cfg["per_alpha"], cfg["per_beta"], cfg["per_beta_anneal_steps"], cfg["per_eta"], cfg["per_eps"]) == (False, 0.6, 0.4, 0, 0.9, 1e-3)


def test_beta_schedule():
    a = SimpleNamespace(per_beta=0.4, per_beta_anneal_steps=0)
    assert run.per_beta(a, 0) == run.per_beta(a, 10 ** 6) == 0.4
    a.per_beta_anneal_steps = 100
    assert run.per_beta(a, 0) == 0.4 and abs(run.per_beta(a, 50) - 0.7) < 1e-12 and run.per_beta(a, 100) == 1.0 and run.per_beta(a, 10 ** 6) == 1.0


def test_train_iteration_takes_the_prioritised_sampler_only_with_the_key():
    calls = []

    class Buffer:
        def insert_episode_batch(self, b): calls.append("insert")
        def can_sample(self, n): return True
        def sample(self, n, out=None): calls.append(("sample", n)); return SimpleNamespace(device="cpu")
        def sample_windows(self, n, window, burn_in, out=None): calls.append(("sample_windows", n, window, burn_in)); return SimpleNamespace(device="cpu")
        def sample_prioritized(self, n, window=0, burn_in=0, beta=None, out=None):
            calls.append(("sample_prioritized", n, window, burn_in, round(beta, 6), out)); return SimpleNamespace(device="cpu")

    def ctx_of(**keys):
        a = SimpleNamespace(batch_size=16, train_steps_per_rollout=2, device="cpu", schedule_unit="rollouts", batch_size_run=32, **keys)
        runner = SimpleNamespace(run=lambda test_mode: "rollout", fixed_length_episodes=True, t_env=0)
        learner = SimpleNamespace(train=lambda sample, t_env, ep: calls.append("train"), sample_out=lambda: "static")
        return SimpleNamespace(args=a, runner=runner, buffer=Buffer(), learner=learner, train_steps=0)

    for keys in ({}, dict(prioritized_replay=False, per_beta=0.4)):
        del calls[:]
        run.train_iteration(ctx_of(**keys), 0)
        assert calls == ["insert", ("sample", 16), "train", ("sample", 16), "train"], keys
    del calls[:]
    run.train_iteration(ctx_of(prioritized_replay=False, train_window=5, train_burn_in=2), 0)
    assert calls == ["insert", ("sample_windows", 16, 5, 2), "train", ("sample_windows", 16, 5, 2), "train"]
    del calls[:]
    run.train_iteration(ctx_of(prioritized_replay=True, per_beta=0.4, per_beta_anneal_steps=4), 0)
    assert calls == ["insert", ("sample_prioritized", 16, 0, 0, 0.4, "static"), "train", ("sample_prioritized", 16, 0, 0, 0.55, "static"), "train"]
    del calls[:]
    run.train_iteration(ctx_of(prioritized_replay=True, per_beta=0.5, per_beta_anneal_steps=0, train_window=5, train_burn_in=2), 0)
    assert calls == ["insert", ("sample_prioritized", 16, 5, 2, 0.5, "static"), "train", ("sample_prioritized", 16, 5, 2, 0.5, "static"), "train"]
