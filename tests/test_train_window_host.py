"""CPU suite of training on sampled time windows with burn-in (config keys train_window / train_burn_in / train_window_norm;
ssd_sample_windows / ssd_gather_windows; ReplayBuffer.sample_windows / gather_windows): the draw contract against a restatement written
from the header, the host gather against numpy slices, the tensor-op learner on windows against the numbers the reference recorded on
time slices (tests/golden/learner_train_window.npz, tools/gen_train_window_golden.py), the "episode" normaliser, the exports'
declarations as compiled and refusals, the config refusals, and train_window: 0 as today's path."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops, run
from tests import td_lambda_util as U
from tests import train_window_util as W
from tests.test_learner_options import check_step, perturb_target
from tests.test_td_lambda_host import _raw_arrays, within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = abi.SSD_ERR_INVALID
SHAPES = [(7, 3, 1), (7, 7, 2), (40, 16, 8), (8192, 64, 76), (5000, 16, 976)]      # (population, count, n_starts)
SEED = 0x1234567890ABCDEF
CHI2_9999_DF6 = 27.856341          # scipy.stats.chi2.ppf(0.9999, 6): the bar of tests/test_exploration_contract.py (0.9999 quantile, matching df)


# ---- 1. the draw contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("population,count,n_starts", SHAPES)
def test_host_draws_are_the_header_arithmetic(population, count, n_starts):
    for seed, call in ((SEED, 0), (SEED, 5), (3, 2 ** 32 - 1), (2 ** 64 - 1, 77)):
        ids, t0 = ops.sample_windows(seed, call, population, count, n_starts, th.empty(count, dtype=th.long), th.empty(count, dtype=th.long))
        ref_ids, ref_t0 = W.sample_windows(seed, call, population, count, n_starts)
        assert ids.tolist() == ref_ids and t0.tolist() == ref_t0, (seed, call)
        assert th.equal(ids, ops.sample_ids(seed, call, population, count, th.empty(count, dtype=th.long)))       # the episodes sample() draws
        assert len(set(ref_ids)) == count and 0 <= min(ref_ids) and max(ref_ids) < population
        assert 0 <= min(ref_t0) and max(ref_t0) < n_starts
        if n_starts == 1:
            assert ref_t0 == [0] * count


def test_vectorised_restatement_is_the_scalar_one():
    got = W.starts_of_calls(SEED, [0, 5, 2 ** 32 - 1], 16, 976)
    for row, call in zip(got, (0, 5, 2 ** 32 - 1)):
        assert row.tolist() == W.sample_windows(SEED, call, 5000, 16, 976)[1]


def test_starts_are_uniform():
    """10^5 calls of the restatement at n_starts = 7 (16 starts a call): chi-square of the counts against the uniform law, 6 degrees
    of freedom, below the 0.9999 quantile.  Fixed seeds: the statistic is a constant of the contract, printed."""
    for seed in (SEED, 20240607):
        t0 = W.starts_of_calls(seed, np.arange(100000), 16, 7)
        counts = np.bincount(t0.ravel(), minlength=7).astype(np.float64)
        assert counts.size == 7 and counts.sum() == t0.size
        e = t0.size / 7
        chi2 = float(((counts - e) ** 2 / e).sum())
        print("seed %#x: chi2_6 of %d starts %.2f (bar %.2f)" % (seed, t0.size, chi2, CHI2_9999_DF6))
        assert chi2 < CHI2_9999_DF6, (seed, chi2)


# ---- 2. the host gather ------------------------------------------------------------------------------------------------------------------
def _host_buffer():
    """a host buffer of the cleanup fixture's four episodes + four decoys, episode 1 unfilled from slot 9 on, episode 2 from slot 4"""
    from tests.learner_util import build, load_fixture
    z, meta = load_fixture("learner_cleanup5.npz")
    args, batch, mac, learner = build(z, meta)
    buf = W.buffer_of(batch, rows=[4, 1, 6, 3], size=8, norm="episode")
    buf.data.transition_data["filled"][1, 9:] = 0
    buf.data.transition_data["filled"][6, 4:] = 0
    return buf


@pytest.mark.parametrize("window,burn_in,ids,t0", [(6, 2, [4, 1, 6, 3], [0, 3, 6, 2]), (12, 11, [7, 0], [0, 0]), (1, 0, [0, 7, 7, 3, 1], [11, 0, 5, 11, 8]),
                                                   (3, 2, [6, 6, 1], [1, 0, 9])])
def test_host_gather_is_numpy_slices_with_the_filled_rule(window, burn_in, ids, t0):
    buf = _host_buffer()
    before = {k: v.clone() for k, v in buf.data.transition_data.items()}
    win = buf.gather_windows(ids, t0, window, burn_in)
    assert (win.batch_size, win.max_seq_length, win.reward_norm) == (len(ids), window + 1, 13.0)
    for k, v in buf.data.transition_data.items():
        ref = (W.window_filled(v.numpy(), ids, t0, window + 1, burn_in) if k == "filled" else W.window_slices(v.numpy(), ids, t0, window + 1))
        assert np.array_equal(win[k].numpy(), ref) and win[k].dtype == v.dtype, k
        assert th.equal(v, before[k]), k                                     # the source is not written (a window is a copy, not a view)
    f = win["filled"].numpy()[..., 0]
    for e, s in enumerate(t0):
        assert not f[e, :burn_in if s > 0 else 0].any()
    buf.window_norm = "window"
    assert buf.gather_windows(ids, t0, window, burn_in).reward_norm == window + 1.0
    same = buf.gather_windows(th.tensor(ids), np.asarray(t0), window, burn_in, out=win)
    assert same is win


def test_host_gather_and_sample_refuse_what_does_not_fit():
    buf = _host_buffer()
    for window, burn_in in ((0, 0), (13, 0), (6, 6), (6, -1)):
        with pytest.raises(ValueError):
            buf.gather_windows([0], [0], window, burn_in)
    with pytest.raises(IndexError):
        buf.gather_windows([0], [7], 6, 0)
    with pytest.raises(IndexError):
        buf.gather_windows([8], [0], 6, 0)
    with pytest.raises(ValueError):
        buf.sample_windows(4, 13, 0)


def test_host_sample_windows_draws_with_numpy():
    """host buffers: ids by np.random.choice as sample() draws them, starts by np.random.randint; one call counted"""
    buf = _host_buffer()
    np.random.seed(5)
    win = buf.sample_windows(4, 6, 2)
    np.random.seed(5)
    ids, t0 = np.random.choice(8, 4, replace=False), np.random.randint(0, 7, 4)
    assert buf.last_window_ids.tolist() == ids.tolist() and buf.last_window_t0.tolist() == t0.tolist() and buf._sample_calls == 1
    assert np.array_equal(win["reward"].numpy(), W.window_slices(buf["reward"].numpy(), ids, t0, 7))
    np.random.seed(5)
    sample = buf.sample(4)                                                   # the same episodes without windows
    assert np.array_equal(sample["reward"].numpy(), buf["reward"].numpy()[ids])
    buf.episodes_in_buffer = 4
    buf.sample_windows(4, 12, 0)
    assert buf.last_window_ids.tolist() == [0, 1, 2, 3] and buf.last_window_t0.tolist() == [0] * 4 and buf._sample_calls == 2


# ---- 3. the reference pin ----------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_stated_cases():
    z, meta = W.load_golden()
    assert meta["norm"] == "window" and "sin(0.37" in meta["target_perturbation"]
    got = {(c["base"], c["window"], c["burn_in"], tuple(c["t0"]), tuple(c["k_e"]), c["overrides"].get("sim_horizon"),
            c["overrides"]["double_q"], c["overrides"]["consider_others_inc"]) for c in meta["cases"]}
    want = {(b, L, K, t0, ke, h, dq, oth) for b in ("learner_cleanup5.npz", "learner_harvest5.npz")
            for L, K, t0, ke, h in ((6, 2, (0, 3, 6, 2), (0, 2, 2, 2), None), (3, 1, (9, 0, 5, 9), (1, 0, 1, 1), None),
                                    (11, 3, (1, 0, 1, 0), (3, 0, 3, 0), None), (6, 2, (0, 3, 6, 2), (0, 2, 2, 2), 3))
            for dq, oth in ((True, False), (False, True))}
    assert got == want and len(meta["cases"]) == 16
    assert all(z[k].dtype != object for k in z.files) and not any("/w_" in k or "batch" in k for k in z.files)
    assert os.path.getsize(os.path.join(W.GOLDEN, "learner_train_window.npz")) < 300 * 1024


@pytest.mark.parametrize("name", W.CASES)
def test_tensor_op_learner_on_windows_matches_the_reference_on_slices(name):
    """Two optimisation steps of the tensor-op learner on windows that ReplayBuffer.gather_windows built from the fixture's episodes
    (held among decoy rows), norm "window": every logged value and the parameter checksums within the project's 1e-5."""
    rec, c = W.golden_case(name)
    args, batch, mac, learner = W.build_case(c)
    assert args.sim_horizon == c["overrides"].get("sim_horizon", args.sim_horizon) and args.double_q == c["overrides"]["double_q"]
    rows = [4, 1, 6, 3]
    buf = W.buffer_of(batch, rows=rows, size=8, norm="window")
    win = buf.gather_windows(rows, c["t0"], c["window"], c["burn_in"])
    assert win.reward_norm == c["window"] + 1.0 and not learner._fused(win)
    f = win["filled"][..., 0]
    assert [int((f[e] == 0).sum()) for e in range(4)] == c["k_e"]
    perturb_target(learner)
    for step in range(2):
        logs = learner.cal_loss_and_step(win)
        for k in ("loss_value_env", "loss_value_inc", "loss_sim"):
            print(name, step, k, "%.3e" % abs(float(logs[k]) - float(rec["step%d_%s" % (step, k)])))
        check_step(logs, mac, rec, step)


def test_fixture_pins_the_window_the_burn_in_and_the_norm():
    """each of the three, changed alone, misses the recorded losses by far more than the tolerance"""
    name = "cleanup5_L6_K2_dq1_oth0"
    rec, c = W.golden_case(name)
    for label, t0, burn_in, norm in (("t0", [1, 3, 6, 2], 2, "window"), ("burn-in", c["t0"], 0, "window"), ("norm", c["t0"], 2, "episode")):
        args, batch, mac, learner = W.build_case(c)
        win = W.buffer_of(batch, norm=norm).gather_windows(range(4), t0, c["window"], burn_in)
        perturb_target(learner)
        logs = learner.cal_loss_and_step(win)
        miss = max(abs(float(logs[k]) - float(rec["step0_" + k])) for k in ("loss_value_env", "loss_value_inc", "loss_sim"))
        assert miss > 1e-3, (label, miss)


# ---- 4. norm "episode" -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in W.CASES if n.startswith("cleanup5_L6_K2_d") or n.startswith("harvest5_L3_K1_d")])
@pytest.mark.parametrize("lam", [0.0, 0.8])
def test_episode_norm_divides_the_rewards_by_the_episode_length(name, lam):
    """norm "episode" on the golden's windows: the learner's two value losses (and at td_lambda 0.8 its lambda-returns) equal the
    numpy rows of tests/td_lambda_util.host_rows with seq_len = 13 -- the episode's slot count, not the window's."""
    rec, c = W.golden_case(name)
    args, batch, mac, learner = W.build_case(c, overrides=dict(td_lambda=lam))
    win = W.buffer_of(batch, norm="episode").gather_windows(range(4), c["t0"], c["window"], c["burn_in"])
    assert win.reward_norm == 13.0 and win.max_seq_length == c["window"] + 1
    perturb_target(learner)
    with th.no_grad():
        arr = _raw_arrays(win, learner.unroll_pair(win))
    logs = learner.cal_loss_and_step(win)
    rows = lambda seq_len: U.host_rows(arr["q_env"], arr["q_inc"], arr["tq_env"], arr["tq_inc"], arr["avail"], arr["actions"], arr["actions_inc"],
                                       arr["reward"], arr["terminated"], arr["filled"], args.double_q, args.consider_others_inc, args.reward_scale,
                                       args.incentive_ratio, args.incentive_cost, float(args.incentive), seq_len)
    p, q = rows(13.0), rows(float(win.max_seq_length))
    assert np.abs(p["r_env"] - q["r_env"]).max() > 1e-3                      # the two norms differ on these windows
    for i, (h, gamma) in enumerate((("env", args.gamma_env), ("inc", args.gamma_inc))):
        G = U.serial_returns(p["r_" + h], p["term"], p["mask"], p["live"], p["v_" + h], gamma, lam)
        if lam > 0:
            assert within(learner.last_lambda_returns[i].numpy(), G, 1e-5), (h, float(np.abs(learner.last_lambda_returns[i].numpy() - G).max()))
        loss = (((p["chosen_" + h] - G) * p["mask"][..., None]) ** 2).sum() / (p["mask"].sum() * G.shape[-1])
        assert abs(float(logs["loss_value_" + h]) - loss) <= 1e-5 * max(1.0, abs(loss)), (h, float(logs["loss_value_" + h]), loss)


def test_td_loss_args_carry_the_normaliser():
    """ops._td_loss_args hands the batch's reward_norm to the loss kernel as seq_len (CPU tensors: the struct only); a batch without
    the attribute keeps its slot count."""
    rec, c = W.golden_case("cleanup5_L6_K2_dq1_oth0")
    args, batch, mac, learner = W.build_case(c)
    a = SimpleNamespace(**vars(args))
    assert ops._td_loss_args(batch, a, args.n_actions, th.zeros(1, 16))[0].seq_len == 13.0 and ops.reward_norm(batch) == 13.0
    for norm, want in (("episode", 13.0), ("window", 7.0)):
        win = W.buffer_of(batch, norm=norm).gather_windows(range(4), c["t0"], 6, 2)
        t, keep = ops._td_loss_args(win, a, args.n_actions, th.zeros(1, 16))
        assert (t.seq_len, t.t_slots, t.batch) == (want, 7, 4)


# ---- 5. exports: declarations as compiled, refusals; config refusals -----------------------------------------------------------------------------
def test_exports_are_declared_exported_and_mirrored():
    """declaration, export and argtypes of every name of the table: tests/test_abi_symbols.py"""
    assert {"ssd_sample_windows", "ssd_gather_windows"} <= set(abi.HIP_SIGNATURES)
    assert abi.load_library().ssd_abi_version() == abi.ABI_VERSION == 10     # two exports more, no version change


def test_struct_size_and_declarations_as_compiled(tmp_path):
    c = tmp_path / "w.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssd_hip.h"\n'
                 'int main(){printf("%zu %zu %zu %zu %d %d\\n", sizeof(ssd_window_field), offsetof(ssd_window_field, dst), offsetof(ssd_window_field, slot_bytes),'
                 'offsetof(ssd_window_field, filled), SSD_COPY_BLOCKS_MAX, SSD_SAMPLE_IDS_MAX);'
                 'int (*f)(uint64_t, uint32_t, int32_t, int32_t, int32_t, int64_t*, int64_t*, void*) = ssd_sample_windows;'
                 'int (*g)(const ssd_window_field*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, int32_t, void*) = ssd_gather_windows;'
                 'return f == 0 || g == 0;}')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "w.o")])   # the declarations are usable
    c.write_text(re.sub(r"int \(\*f\).*return f == 0 \|\| g == 0;", "return 0;", c.read_text(), flags=re.S))
    exe = tmp_path / "w"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 8, 16, 24, abi.COPY_BLOCKS_MAX, abi.SAMPLE_IDS_MAX] == [32, 8, 16, 24, 32, 1024]      # the layout itself, as literals


P = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched (the checks run before any launch)
_keep = []


def _fields(*specs):
    """specs: (src, dst, slot_bytes, filled)"""
    tab = (abi.SsdWindowField * max(1, len(specs)))()
    for e, (src, dst, sb, fl) in zip(tab, specs):
        e.src, e.dst, e.slot_bytes, e.filled = src, dst, sb, fl
    _keep.append(tab)
    return tab


def _gather(fields=None, count=2, ids=P, t0=P, n_ids=4, src_slots=13, win_slots=7, burn_in=2):
    fields = _fields((P, P, 1125, 0), (P, P, 8, 1)) if fields is None else fields
    return (fields, count, ids, t0, n_ids, src_slots, win_slots, burn_in, None)


GATHER_REFUSALS = [
    ("null fields", _gather(fields=False)), ("null ids", _gather(ids=None)), ("null t0", _gather(t0=None)),
    ("count 0", _gather(count=0)), ("count -1", _gather(count=-1)), ("count over SSD_COPY_BLOCKS_MAX", _gather(fields=_fields(*[(P, P, 4, 0)] * 33), count=33)),
    ("n_ids 0", _gather(n_ids=0)), ("n_ids 65536", _gather(n_ids=65536)), ("n_ids -1", _gather(n_ids=-1)),
    ("win_slots 1", _gather(win_slots=1, burn_in=0)), ("win_slots 0", _gather(win_slots=0, burn_in=0)), ("win_slots over src_slots", _gather(win_slots=14)),
    ("burn_in -1", _gather(burn_in=-1)), ("burn_in win_slots - 1", _gather(burn_in=6)), ("burn_in at win_slots 2", _gather(win_slots=2, burn_in=1)),
    ("slot_bytes 0", _gather(fields=_fields((P, P, 0, 0)), count=1)), ("slot_bytes -8", _gather(fields=_fields((P, P, -8, 0)), count=1)),
    ("null src", _gather(fields=_fields((None, P, 4, 0)), count=1)), ("null dst", _gather(fields=_fields((P, P, 4, 0), (P, None, 4, 0)))),
    ("two filled fields", _gather(fields=_fields((P, P, 8, 1), (P, P, 8, 1)))), ("filled of 4-byte slots", _gather(fields=_fields((P, P, 4, 1)), count=1)),
    ("filled at an odd source", _gather(fields=_fields((P + 4, P, 8, 1)), count=1)), ("filled at an odd destination", _gather(fields=_fields((P, P + 1, 8, 1)), count=1)),
    ("destination over 64 GiB", _gather(fields=_fields((P, P, 1 << 22, 0)), count=1, n_ids=65535, src_slots=1024, win_slots=1024)),
]
SAMPLE_REFUSALS = [("null ids", (7, 0, 2000, 16, 8, None, P, None)), ("null t0", (7, 0, 2000, 16, 8, P, None, None)),
                   ("count 0", (7, 0, 2000, 0, 8, P, P, None)), ("count -1", (7, 0, 2000, -1, 8, P, P, None)),
                   ("count over SSD_SAMPLE_IDS_MAX", (7, 0, 2000, 1025, 8, P, P, None)), ("population under count", (7, 0, 15, 16, 8, P, P, None)),
                   ("n_starts 0", (7, 0, 2000, 16, 0, P, P, None)), ("n_starts -1", (7, 0, 2000, 16, -1, P, P, None))]


@pytest.mark.parametrize("case", GATHER_REFUSALS, ids=[c[0].replace(" ", "_") for c in GATHER_REFUSALS])
def test_invalid_gather_is_refused_with_a_message(case):
    """only invalid calls are made: nothing here reaches a launch"""
    label, args = case
    lib = abi.load_library()
    rc = lib.ssd_gather_windows(*[None if a is False else a for a in args])
    assert rc == INV, (label, rc, lib.ssd_last_error())
    assert b"ssd_gather_windows" in lib.ssd_last_error(), label
    with pytest.raises(abi.SsdError):
        abi.check(lib, rc)


@pytest.mark.parametrize("case", SAMPLE_REFUSALS, ids=[c[0].replace(" ", "_") for c in SAMPLE_REFUSALS])
def test_invalid_draw_is_refused_with_a_message(case):
    label, args = case
    lib = abi.load_library()
    rc = lib.ssd_sample_windows(*args)
    assert rc == INV and b"ssd_sample_windows" in lib.ssd_last_error(), (label, rc, lib.ssd_last_error())


def test_ops_gather_windows_declines_host_tensors_and_misfits():
    src, dst = th.zeros(8, 13, 5), th.zeros(4, 7, 5)
    ids = t0 = th.zeros(4, dtype=th.long)
    assert not ops.gather_windows([(src, dst)], ids, t0, 13, 7, 2, None)     # host tensors: the caller indexes
    assert not ops.gather_windows([], ids, t0, 13, 7, 2, None)


@pytest.mark.parametrize("keys,match", [
    (dict(train_window=13), "train_window"), (dict(train_window=-1), "train_window"), (dict(train_window=6, train_burn_in=6), "train_burn_in"),
    (dict(train_window=6, train_burn_in=-1), "train_burn_in"), (dict(train_burn_in=1), "train_burn_in"),
    (dict(train_window=6, train_window_norm="slots"), "train_window_norm"), (dict(train_window_norm=None), "train_window_norm"),
    (dict(train_window=6, _ragged=True), "fills every slot")])
def test_setup_refuses_bad_window_keys(keys, match):
    keys = dict(keys)
    runner = SimpleNamespace(fixed_length_episodes=not keys.pop("_ragged", False))
    with pytest.raises(ValueError, match=match):
        run._check_train_window(SimpleNamespace(runner="r", **keys), 12, runner)


def test_setup_accepts_the_range_and_fills_the_defaults():
    runner = SimpleNamespace(fixed_length_episodes=True)
    a = SimpleNamespace(runner="r")
    assert run._check_train_window(a, 12, runner) == "episode" and (a.train_window, a.train_burn_in, a.train_window_norm) == (0, 0, "episode")
    for L, K in ((1, 0), (12, 11), (12, 0), (5, 2)):
        a = SimpleNamespace(runner="r", train_window=L, train_burn_in=K, train_window_norm="window")
        assert run._check_train_window(a, 12, runner) == "window"
    ragged = SimpleNamespace(fixed_length_episodes=False)
    assert run._check_train_window(SimpleNamespace(runner="r", train_window=0), 12, ragged) == "episode"      # whole episodes: any runner


# ---- 6. train_window: 0 ------------------------------------------------------------------------------------------------------------------
def test_defaults_load_and_window_zero_takes_todays_path():
    cfg = run.load_config("cleanup")
    assert (cfg["train_window"], cfg["train_burn_in"], cfg["train_window_norm"]) == (0, 0, "episode")
    calls = []

    class Buffer:
        def insert_episode_batch(self, b): calls.append("insert")
        def can_sample(self, n): return True
        def sample(self, n, out=None): calls.append(("sample", n, out)); return SimpleNamespace(device="cpu")
        def sample_windows(self, n, window, burn_in, out=None): calls.append(("sample_windows", n, window, burn_in, out)); return SimpleNamespace(device="cpu")

    def ctx_of(**keys):
        a = SimpleNamespace(batch_size=16, train_steps_per_rollout=2, device="cpu", schedule_unit="rollouts", batch_size_run=32, **keys)
        runner = SimpleNamespace(run=lambda test_mode: "rollout", fixed_length_episodes=True, t_env=0)
        learner = SimpleNamespace(train=lambda sample, t_env, ep: calls.append("train"), sample_out=lambda: "static")
        return SimpleNamespace(args=a, runner=runner, buffer=Buffer(), learner=learner, train_steps=0)

    for keys in ({}, dict(train_window=0, train_burn_in=0)):
        del calls[:]
        assert run.train_iteration(ctx_of(**keys), 0) == 32
        assert calls == ["insert", ("sample", 16, "static"), "train", ("sample", 16, "static"), "train"], keys
    del calls[:]
    run.train_iteration(ctx_of(train_window=5, train_burn_in=2), 0)
    assert calls == ["insert", ("sample_windows", 16, 5, 2, "static"), "train", ("sample_windows", 16, 5, 2, "static"), "train"]
