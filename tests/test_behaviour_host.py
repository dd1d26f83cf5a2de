"""CPU suite of the behaviour statistics (ssd_behaviour_stats / ops.behaviour_stats / abi.behaviour_layout / abi.behaviour_summary).

The independent statement is tests/behaviour_util.reference_stats (numpy int64, written from the table in include/ssd_hip.h); every
comparison of counters is for exact equality.  The golden batches pin the four rollout_* keys to the values the reference learner
recorded for the same batch (f32 there: bar 1e-6 absolute, |value| <= 3, more than 2 f32 ulps).

The export's refusal table lives here too (tests/test_learner_abi_refusals.py names this file for it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops

from . import behaviour_util as bu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INV = abi.SSD_ERR_INVALID
F = 1 << 20                      # a dummy device pointer: non-null, never touched (every case is refused before any launch)

SHAPES = [(1, 1, 2, 9), (3, 12, 5, 9), (7, 5, 10, 8), (2, 3, 1, 9)]


def _ops_vec(fields, A, calls=1, trailing=False):
    actions, inc, reward, clean = (th.from_numpy(np.ascontiguousarray(x)) for x in fields)
    if trailing:                 # the storage's trailing singleton dims
        actions, inc = actions.unsqueeze(-1), inc.unsqueeze(-1)
    acc = th.zeros(bu.length(reward.shape[2], A), dtype=th.float64)
    for _ in range(calls):
        assert ops.behaviour_stats(actions, inc, reward, clean, A, acc) is acc
    return acc.numpy()


# ---- pinned to the reference learner's logs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["learner_cleanup5", "learner_cleanup5_w4", "learner_harvest5"])
def test_rollout_keys_reproduce_the_reference_learner_logs(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    fields = (z["batch_actions"], z["batch_actions_inc"], z["batch_reward"], z["batch_clean_num"])
    n, A = z["batch_reward"].shape[2], z["batch_avail_actions"].shape[-1]
    assert z["batch_reward"].shape[:2] == (4, 13) and n == 5
    ref = bu.reference_stats(*fields, A)
    got = _ops_vec(tuple(np.asarray(f) for f in fields), A)
    assert (got == ref).all()
    for vec in (ref, got):
        s = abi.behaviour_summary(vec, n, A)
        for key in ("incentives_to_cleanup_per", "incentives_to_harvest_per", "value_give_mean", "value_receive_mean"):
            want, have = float(z["step0_" + key]), s["rollout_" + key]
            print(name, key, want, have, abs(want - have))
            assert abs(want - have) <= 1e-6, (name, key, want, have)


def test_the_recorded_reference_values_are_the_expected_ones():
    """the reference learner's values as decimals, so that a changed fixture cannot move the pin silently"""
    table = {"learner_cleanup5": (-0.5714285, None, 2.6875, 0.1041667), "learner_cleanup5_w4": (-0.9999999, None, 2.7166667, -0.025),
             "learner_harvest5": (None, 0.125, 2.5625, -0.0208333)}
    for name, want in table.items():
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        for key, w in zip(("incentives_to_cleanup_per", "incentives_to_harvest_per", "value_give_mean", "value_receive_mean"), want):
            if w is None:       # no such term in this env: zero over (0 + 1e-6)
                assert float(z["step0_" + key]) == 0.0
            else:
                assert abs(float(z["step0_" + key]) - w) <= 1e-6


def test_both_coupling_terms_on_one_synthetic_batch():
    """the Cleanup fixtures have no reward and the Harvest fixture no cleaning: here both sums are non-zero at once"""
    fields = bu.seeded_batch(5, 9, 4, 9, seed=12, hostile=False)        # (a seed at which neither total happens to cancel to 0)
    ref, got = bu.reference_stats(*fields, 9), _ops_vec(fields, 9)
    assert (got == ref).all()
    b = abi.behaviour_blocks(got, 4, 9)
    assert b["recv_on_clean"].sum() != 0 and b["recv_on_reward"].sum() != 0 and b["clean_steps"].sum() > 0 and b["reward_sum"].sum() != 0
    # the learner's two expressions on the same numbers, in f64
    actions, inc, reward, clean = fields
    off = 1 - np.eye(4, dtype=np.int64)
    m = inc[:, :-1] * off
    rv = (m == 1).sum(2) - (m == 2).sum(2)
    cl, r = (clean[:, :-1] > 0).astype(np.float64), reward[:, :-1].astype(np.float64)
    s = abi.behaviour_summary(got, 4, 9)
    assert abs(s["rollout_incentives_to_cleanup_per"] - (cl * rv).sum() / (cl.sum() + 1e-6)) < 1e-12
    assert abs(s["rollout_incentives_to_harvest_per"] - (r * rv).sum() / (r.sum() + 1e-6)) < 1e-12
    assert abs(s["rollout_value_give_mean"] - (m != 0).sum(3).mean()) < 1e-12 and abs(s["rollout_value_receive_mean"] - rv.mean()) < 1e-12


# ---- the tensor-op statement against the independent one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["N%d_T%d_n%d_A%d" % s for s in SHAPES])
def test_host_statement_equals_the_reference_exactly(shape):
    N, T, n, A = shape
    fields = bu.seeded_batch(N, T, n, A, seed=100 + N)
    ref = bu.reference_stats(*fields, A)
    assert (_ops_vec(fields, A) == ref).all()
    assert (_ops_vec(fields, A, trailing=True) == ref).all()
    assert (_ops_vec(fields, A, calls=2) == 2 * ref).all()              # two calls on one accumulator
    b = abi.behaviour_blocks(ref, n, A)
    assert b["n_episodes"][0] == N and b["n_steps"][0] == N * T and b["role_count"].sum() == N * n and b["cleaners_hist"].sum() == N
    assert all(b["inc_count"][i, i].sum() == 0 for i in range(n))       # the stored diagonal is non-zero
    if n == 1:
        assert b["inc_count"].sum() == 0 and b["recv_on_clean"].sum() == 0 and b["recv_on_reward"].sum() == 0
    else:
        assert b["action_count"].sum() < N * T * n and b["inc_count"].sum() < N * T * n * (n - 1)      # -1 / A / 3 were ignored


def test_roles_and_the_cleaners_histogram_by_hand():
    """n 2, T 3, four envs: (idle, cleaner), (harvester, mixed), (cleaner, cleaner), (cleaner by 2 > 1, harvester)"""
    N, T, n, A = 4, 3, 2, 9
    clean, reward = np.zeros((N, T + 1, n), np.float32), np.zeros((N, T + 1, n), np.float32)
    clean[0, :2, 1], reward[0, 2, 1] = 3, 1                             # env 0: agent 1 cleans twice, harvests once
    reward[1, 0, 0] = 1; clean[1, 1, 1] = 1; reward[1, 2, 1] = 2        # env 1: agent 0 harvester, agent 1 one of each
    clean[2, 0, :] = 1                                                  # env 2: two cleaners
    clean[3, :2, 0], reward[3, 2, 0] = 1, 1; reward[3, 1, 1] = 1       # env 3: agent 0 cleaner (2 > 1), agent 1 harvester
    reward[0, 0, 0] = -1                                                # a fire cost is not a harvest
    fields = (np.zeros((N, T + 1, n), np.int64), np.zeros((N, T + 1, n, n), np.int64), reward, clean)
    want_roles = np.array([[1, 2, 1, 0], [0, 2, 1, 1]])                  # agent x (idle, cleaner, harvester, mixed)
    for vec in (bu.reference_stats(*fields, A), _ops_vec(fields, A)):
        b = abi.behaviour_blocks(vec, n, A)
        assert (b["role_count"] == want_roles).all()
        assert b["cleaners_hist"].tolist() == [1, 2, 1]                  # a tie between 0 and 2 cleaners
        assert b["harvest_time"].tolist() == [0 + 2, 2 + 2 + 1] and b["reward_sum"].tolist() == [1, 4]
    s = abi.behaviour_summary(vec, n, A)
    assert s["cleaners_per_env_mean"] == 1.0 and s["role_cleaner_frac"] == 0.5 and s["role_idle_frac"] == 0.125


def test_device_ops_are_strict_about_the_tensor_op_branch():
    """a CPU accumulator is fine; what is refused outright are sizes the export refuses"""
    with pytest.raises(ValueError):
        ops.behaviour_stats(th.zeros(1, 1, 2, dtype=th.long), th.zeros(1, 1, 2, 2, dtype=th.long), th.zeros(1, 1, 2), th.zeros(1, 1, 2), 9,
                            th.zeros(bu.length(2, 9), dtype=th.float64))


# ---- layout, macros -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,A", [(1, 1), (2, 9), (5, 9), (10, 16)])
def test_layout_tiles_the_vector(n, A):
    lay = abi.behaviour_layout(n, A)
    assert tuple(lay) == bu.ORDER
    pos = 0
    for name, (off, shape) in lay.items():
        assert off == pos, name
        pos += int(np.prod(shape))
    assert pos == abi.behaviour_len(n, A) == bu.length(n, A)


def test_len_macro_and_struct_size_as_compiled(tmp_path):
    """the macros as a C compiler sees them (sizeof / offsetof of every struct: tests/test_abi_symbols.py)"""
    c = tmp_path / "b.c"
    c.write_text('#include <stdio.h>\n#include "ssd_hip.h"\nint main(){printf("%d %d %d %d %d %d\\n", SSD_BEHAVIOUR_LEN(1, 1),'
                 'SSD_BEHAVIOUR_LEN(2, 9), SSD_BEHAVIOUR_LEN(5, 9), SSD_BEHAVIOUR_LEN(SSD_MAX_AGENTS, 16), SSD_BEHAVIOUR_MAX_GROUPS, SSD_BEHAVIOUR_WAVES);'
                 'int (*f)(const ssd_behaviour_args*, void*) = ssd_behaviour_stats; return f == 0;}')
    exe = tmp_path / "b"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "b.o")])   # the declaration is usable
    c.write_text(c.read_text().replace("int (*f)(const ssd_behaviour_args*, void*) = ssd_behaviour_stats; return f == 0;", "return 0;"))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.behaviour_len(n, A) for n, A in ((1, 1), (2, 9), (5, 9), (abi.MAX_AGENTS, 16))] + [abi.BEHAVIOUR_MAX_GROUPS, abi.BEHAVIOUR_WAVES]
    assert abi.behaviour_len(abi.MAX_AGENTS, 16) == 583


def test_export_is_declared_exported_and_mirrored():
    """declaration, export and argtypes of every name of the table: tests/test_abi_symbols.py"""
    assert "ssd_behaviour_stats" in abi.HIP_SIGNATURES
    assert abi.load_library().ssd_abi_version() == abi.ABI_VERSION == 10


# ---- refusals (only invalid calls are made: nothing here reaches a launch) ---------------------------------------------------------------------
_keep = []


def _args(**kw):
    a = abi.SsdBehaviourArgs(n_env=4, t_slots=13, n_agents=5, n_actions=9, actions=F, actions_inc=F, reward=F, clean_num=F, workspace=F, acc=F)
    for k, v in kw.items():
        setattr(a, k, v)
    _keep.append(a)
    return C.byref(a)


REFUSALS = [("null args", None)] + [("%s = %r" % (k, v), dict([(k, v)])) for k, v in (
    ("actions", None), ("actions_inc", None), ("reward", None), ("clean_num", None), ("workspace", None), ("acc", None),
    ("n_env", 0), ("n_env", -1), ("t_slots", 1), ("t_slots", 0), ("n_agents", 0), ("n_agents", abi.MAX_AGENTS + 1), ("n_actions", 0), ("n_actions", 17))] + [
    ("t_slots * n^2 = INT32_MAX + 53 (32-bit index inside an env's block)", dict(t_slots=(2 ** 31 - 1) // 100 + 1, n_agents=10)),
    ("t_slots = INT32_MAX, n 2", dict(t_slots=2 ** 31 - 1, n_agents=2))]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0].replace(" ", "_") for c in REFUSALS])
def test_invalid_call_is_refused_with_a_message(case):
    label, change = case
    lib = abi.load_library()
    rc = lib.ssd_behaviour_stats(None if change is None else _args(**change), None)
    assert rc == INV, (label, rc, lib.ssd_last_error())
    assert b"ssd_behaviour_stats" in lib.ssd_last_error(), label
    with pytest.raises(abi.SsdError):
        abi.check(lib, rc)


# ---- the summary --------------------------------------------------------------------------------------------------------------------------
def test_behaviour_summary_on_a_hand_written_vector():
    n, A = 2, 2
    blocks = dict(reward_sum=[6, 2], clean_sum=[3, 9], clean_steps=[2, 3], harvest_steps=[4, 1], harvest_time=[10, 5],
                  action_count=[[7, 3], [4, 6]], inc_count=[[[0, 0, 0], [6, 3, 1]], [[5, 1, 4], [0, 0, 0]]],
                  recv_on_clean=[-2, 1], recv_on_reward=[3, 1], role_count=[[0, 1, 1, 0], [1, 0, 0, 1]], cleaners_hist=[1, 1, 0],
                  n_episodes=[2], n_steps=[10])
    vec = np.zeros(abi.behaviour_len(n, A))
    for name, (off, shape) in abi.behaviour_layout(n, A).items():
        vec[off:off + int(np.prod(shape))] = np.asarray(blocks[name], np.float64).reshape(-1)
    s = abi.behaviour_summary(vec, n, A)
    want = {"cleaners_per_env_mean": 0.5, "role_idle_frac": 0.25, "role_cleaner_frac": 0.25, "role_harvester_frac": 0.25, "role_mixed_frac": 0.25,
            "inc_pos_rate": 4 / 20, "inc_neg_rate": 5 / 20, "rollout_incentives_to_cleanup_per": -1 / (5 + 1e-6),
            "rollout_incentives_to_harvest_per": 4 / (8 + 1e-6), "rollout_value_give_mean": 9 / 20, "rollout_value_receive_mean": -1 / 20,
            "harvest_time_mean": 3.0, "clean_share_max": 0.75}
    assert set(s) == set(want)
    for k, w in want.items():
        assert abs(s[k] - w) < 1e-12, (k, s[k], w)
    empty = abi.behaviour_summary(np.zeros(abi.behaviour_len(n, A)), n, A)      # nothing accumulated: every key is finite
    assert all(np.isfinite(v) for v in empty.values()) and empty["harvest_time_mean"] == 0.0 and empty["clean_share_max"] == 0.0
    one = abi.behaviour_summary(np.zeros(abi.behaviour_len(1, 3)), 1, 3)        # a single agent has no pairs
    assert one["inc_pos_rate"] == 0.0
