"""CPU suite of the reward models (config key reward_model: "inequity_aversion" / "prosocial"; ssd_social_reward, include/ssd_hip_reward.h;
ops.social_reward): the two hand cases, the host statement of ops against the numpy restatement of tests/social_reward_util.py to the
bit, the power of the inputs to tell a wrong summation order, the export's header / table / refusals (dummy pointers, ONLY invalid calls:
nothing is launched), the config refusals and the scheme, the tensor-op learner with the key on against the key-off learner fed the
shaped field, and the window gather of the stored field."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, run
from tests import social_reward_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("inequity_aversion", "prosocial")
SHAPES = [(1, 2, 2), (7, 22, 5), (5, 13, 10)]


def _ops_host(model, reward, p, acc=None):
    from homophily_marl_amd import ops
    out = th.full(reward.shape, float("nan"))
    ops.social_reward(th.from_numpy(reward.copy()), out, model, [float(x) for x in p], None if acc is None else acc)
    return out.numpy()


# ---- 1. hand cases -------------------------------------------------------------------------------------------------------------------------
def test_inequity_aversion_hand_case():
    r = np.array([[[1, 0], [0, 0], [9, 9]]], dtype=np.float32)                       # slot 2: the bootstrap slot, never read
    p = U.scalars("inequity_aversion", 2, alpha=4.0, beta=0.25, decay=0.5)
    assert [float(x) for x in p] == [4.0, 0.25, 0.5]
    want = np.array([[[0.75, -4.0], [-0.125, -2.0], [0.0, 0.0]]], dtype=np.float32)
    assert U.bit_equal(U.shaped("inequity_aversion", r, p), want)
    assert U.bit_equal(_ops_host("inequity_aversion", r, p), want)


def test_prosocial_hand_case():
    r = np.array([[[1, 0, 2], [9, 9, 9]]], dtype=np.float32)
    p = U.scalars("prosocial", 3, rho=0.5)
    assert [float(x) for x in p] == [0.5, 0.25, 0.0]
    want = np.array([[[1.0, 0.75, 1.25], [0.0, 0.0, 0.0]]], dtype=np.float32)
    assert U.bit_equal(U.shaped("prosocial", r, p), want)
    assert U.bit_equal(_ops_host("prosocial", r, p), want)


# ---- 2. the host statement of ops == the restatement, to the bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_statement_equals_the_restatement_bit_for_bit(model, shape):
    from homophily_marl_amd import ops
    N, T1, n = shape
    r = U.draw(N, T1, n, seed=11 + n)
    p = U.scalars(model, n)
    assert [float(x) for x in p] == list(ops.social_reward_scalars(model, n))
    start = np.random.default_rng(3).standard_normal((N, n, 3))                      # the accumulator is added to, not overwritten
    ref_acc, acc = start.copy(), th.from_numpy(start.copy())
    ref = U.shaped(model, r, p, ref_acc)
    got = _ops_host(model, r, p, acc)
    assert U.bit_equal(got, ref) and (got[:, -1] == 0).all()
    assert U.bit_equal(acc.numpy(), ref_acc)
    assert not np.array_equal(ref_acc, start)
    if model == "prosocial":
        assert (ref_acc[..., 2] == start[..., 2]).all()
    # views of a wider storage: the strides are honoured, nothing between the logical elements is written
    wide_r, wide_o = th.full((N, T1 + 2, n + 3), float("nan")), th.full((N, T1 + 2, n + 3), 5.0)
    wide_r[:, :T1, :n] = th.from_numpy(r)
    ops.social_reward(wide_r[:, :T1, :n], wide_o[:, :T1, :n], model, [float(x) for x in p])
    assert U.bit_equal(wide_o[:, :T1, :n].contiguous().numpy(), ref)
    wide_o[:, :T1, :n] = 5.0
    assert (wide_o == 5.0).all()


def test_ops_refuses_unfit_operands():
    from homophily_marl_amd import ops
    r, p = th.zeros(2, 3, 4), [1.0, 1.0, 0.5]
    for bad_r, bad_o, model, acc in ((r.double(), r.clone(), "prosocial", None), (r, th.zeros(2, 3, 5), "prosocial", None), (r, r, "prosocial", None),
                                     (r, r.clone(), "svo", None), (r[:, :, :1], r.clone()[:, :, :1], "prosocial", None),
                                     (r, r.clone(), "prosocial", th.zeros(2, 4, 3)), (r.transpose(1, 2), r.clone().transpose(1, 2), "prosocial", None)):
        with pytest.raises(ValueError):
            ops.social_reward(bad_r, bad_o, model, p, acc)


# ---- 3. the inputs can catch a wrong summation order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 22, 5), (5, 13, 10)], ids=lambda s: "x".join(map(str, s)))
def test_the_draw_family_tells_descending_sums_from_ascending(shape):
    """(n <= 3 has at most two partners: the two orders are the same sum, nothing to assert there)"""
    N, T1, n = shape
    r = U.draw(N, T1, n, seed=11 + n)
    p = U.scalars("inequity_aversion", n)
    up, down = U.shaped("inequity_aversion", r, p), U.shaped("inequity_aversion", r, p, descending=True)
    differ = float((U.bits(up[:, :-1]) != U.bits(down[:, :-1])).mean())
    print("n = %d: %.1f %% of the entries differ between ascending and descending j" % (n, 100 * differ))
    assert differ > 0.02


# ---- 4. the export: header, table, library ------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssd_hip_reward.h")).read(), flags=re.S)


def test_header_table_and_library_name_the_same_export():
    names = set(abi.REWARD_SIGNATURES)
    assert sorted(set(re.findall(r"\b(ssd_[a-z_0-9]+)\s*\(", _header()))) == sorted(names) == ["ssd_social_reward"]
    assert not names & set(abi.HIP_SIGNATURES) and not names & set(abi.TRAIN_SIGNATURES)
    defines = dict(re.findall(r"#define (SSD_REWARD_[A-Z]+) (\d+)", _header()))
    assert defines == {"SSD_REWARD_IA": "1", "SSD_REWARD_PROSOCIAL": "2"} and (abi.REWARD_IA, abi.REWARD_PROSOCIAL) == (1, 2)
    raw, bound = ctypes.CDLL(abi.HIP_LIB_PATH), abi.load_library()
    for name, (res, argtypes) in abi.REWARD_SIGNATURES.items():
        assert hasattr(raw, name), name
        assert getattr(bound, name).argtypes == argtypes and getattr(bound, name).restype is res, name
    assert len(abi.REWARD_SIGNATURES["ssd_social_reward"][1]) == len(BASE) == 15
    assert bound.ssd_abi_version() == abi.ABI_VERSION == 10


def test_the_header_compiles_as_c(tmp_path):
    import subprocess
    c = tmp_path / "t.c"
    c.write_text('#include "ssd_hip_reward.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])


# ---- 5. refusals (dummy pointers; every row is refused before any launch) -----------------------------------------------------------------------------
F = 1 << 20                      # dummy device pointers: non-null, aligned, never touched
G = 1 << 24
NAN, INF = float("nan"), float("inf")
# model, reward, shaped, acc, n_env, t_slots, n_agents, src_env_stride, src_slot_stride, dst_env_stride, dst_slot_stride, p0, p1, p2, stream
BASE = [1, F, G, None, 8, 13, 5, 65, 5, 65, 5, 1.25, 0.0125, 0.96525, None]
ROWS = [("null reward", {1: None}), ("null shaped", {2: None}), ("shaped == reward", {2: F}),
        ("shaped overlaps the end of reward", {2: F + 4 * (7 * 65 + 12 * 5 + 4)}), ("reward overlaps the end of shaped", {1: G + 4 * (7 * 65 + 12 * 5 + 4)}),
        ("model 0", {0: 0}), ("model 3", {0: 3}), ("n_env 0", {4: 0}), ("t_slots 1", {5: 1}), ("n_agents 1", {6: 1, 8: 5, 10: 5}),
        ("n_agents 11", {6: 11, 8: 11, 10: 11, 7: 200, 9: 200}), ("src slot stride below n_agents", {8: 4}), ("dst slot stride below n_agents", {10: 4}),
        ("src env stride below t_slots * slot_stride", {7: 64}), ("dst env stride below t_slots * slot_stride", {9: 64}),
        ("p0 negative", {11: -1.0}), ("p0 NaN", {11: NAN}), ("p0 infinite", {11: INF}), ("p1 negative", {12: -0.5}), ("p1 NaN", {12: NAN}),
        ("p1 infinite", {12: INF}), ("decay 1", {13: 1.0}), ("decay negative", {13: -0.1}), ("decay NaN", {13: NAN}),
        ("src extent past 2^31 - 1", {4: 1 << 20, 7: 1 << 12}), ("dst extent past 2^31 - 1", {4: 1 << 20, 9: 1 << 12}),
        ("reward not 4-byte aligned", {1: F + 2}), ("shaped not 4-byte aligned", {2: G + 1}), ("acc not 4-byte aligned", {3: (1 << 26) + 2}), ("acc (f64) at 4 bytes, not 8", {3: (1 << 26) + 4}),
        ("prosocial: p0 negative", {0: 2, 11: -1.0}), ("prosocial: null shaped", {0: 2, 2: None})]


def _call(change):
    lib = abi.load_library()
    args = list(BASE)
    for k, v in change.items():
        args[k] = v
    return lib, lib.ssd_social_reward(*args)


@pytest.mark.parametrize("label,change", ROWS, ids=[r[0].replace(" ", "_") for r in ROWS])
def test_invalid_call_is_refused_with_a_message(label, change):
    lib, rc = _call(change)
    assert rc == abi.SSD_ERR_INVALID, (label, rc, lib.ssd_last_error())
    assert lib.ssd_last_error() and b"ssd_social_reward" in lib.ssd_last_error(), label
    with pytest.raises(abi.SsdError):
        abi.check(lib, rc)


def test_the_base_row_differs_from_a_valid_call_only_by_the_row():
    """every change above moves ONE property of an otherwise valid argument list: the extents of the base fit (7 * 65 + 12 * 5 + 5 elements),
    the buffers are 15 MiB apart, and the touching layout -- shaped right behind reward's last element -- is no overlap.  (The valid
    call itself is made by the GPU suite: it would launch.)"""
    ext = 7 * 65 + 12 * 5 + 5
    assert G - F > 4 * ext and BASE[7] >= BASE[5] * BASE[8] and 2 <= BASE[6] <= abi.MAX_AGENTS


# ---- 6. setup -----------------------------------------------------------------------------------------------------------------------------------------
CFG = dict(runner="hip_graph", ind_reward=True, n_agents=5, per_initial_priority="max")


@pytest.mark.parametrize("keys,match", [
    (dict(reward_model="svo"), "reward_model must be"), (dict(reward_model=["inequity_aversion"]), "reward_model must be"),
    (dict(reward_model={"model": "prosocial"}), "reward_model must be"), (dict(reward_model=True), "reward_model must be"), (dict(reward_model="ia"), "reward_model must be"),
    (dict(reward_model="prosocial", n_agents=1), "reward_model.*n_agents"), (dict(reward_model="inequity_aversion", ind_reward=False), "reward_model.*ind_reward"),
    (dict(reward_model="prosocial", runner="episode"), "reward_model.*vectorised runner"),
    (dict(reward_model="inequity_aversion", per_initial_priority="rollout"), "reward_model.*per_initial_priority"),
    (dict(reward_model="inequity_aversion", ia_alpha=-1.0), "reward_model.*ia_alpha"), (dict(reward_model="inequity_aversion", ia_alpha=float("inf")), "reward_model.*ia_alpha"),
    (dict(reward_model="inequity_aversion", ia_beta=-0.5), "reward_model.*ia_beta"), (dict(reward_model="inequity_aversion", ia_beta=float("nan")), "reward_model.*ia_beta"),
    (dict(reward_model="inequity_aversion", ia_decay=1.0), "reward_model.*ia_decay"), (dict(reward_model="inequity_aversion", ia_decay=-0.1), "reward_model.*ia_decay"),
    (dict(reward_model="inequity_aversion", ia_decay="0.9"), "reward_model.*ia_decay"),
    (dict(reward_model="prosocial", prosocial_weight=1.5), "reward_model.*prosocial_weight"), (dict(reward_model="prosocial", prosocial_weight=-0.1), "reward_model.*prosocial_weight")])
def test_setup_refuses(keys, match):
    with pytest.raises(ValueError, match=match):
        run._check_reward_model(SimpleNamespace(**dict(CFG, **keys)))


def test_setup_accepts_and_the_scheme_follows_the_key():
    cfg = run.load_config("cleanup")
    assert (cfg["reward_model"], cfg["ia_alpha"], cfg["ia_beta"], cfg["ia_decay"], cfg["prosocial_weight"]) == ("individual", 5.0, 0.05, 0.96525, 0.5)
    src = inspect.getsource(run.setup)
    assert src.index("_check_reward_model(args)") < src.index("build_scheme(args, env_info)")          # the scheme sees the validated key
    info = dict(state_shape=10, obs_shape=20, n_actions=9)
    base = dict(CFG, name="homophily", obs_storage="f32", store_state=True, n_actions=9)
    for drop, keys in ((True, {}), (False, dict(reward_model="individual")), (False, dict(reward_model=None))):
        a = SimpleNamespace(**dict(base, **keys))
        assert run._check_reward_model(a) is None and a.reward_model == "individual"
        if drop:
            del a.reward_model
        assert "reward_model" not in run.build_scheme(a, info)[0]
    for model, vec in (("inequity_aversion", (1.25, float(np.float32(0.05) / np.float32(4)), float(np.float32(0.96525)))), ("prosocial", (0.5, 0.125, 0.0))):
        for runner in ("hip_vec", "hip_graph"):
            a = SimpleNamespace(**dict(base, reward_model=model, runner=runner, ia_alpha=5.0, ia_beta=0.05, ia_decay=0.96525, prosocial_weight=0.5))
            assert run._check_reward_model(a) == vec == a.reward_model_scalars
            scheme = run.build_scheme(a, info)[0]
            assert scheme["reward_model"] == {"vshape": (5,), "dtype": th.float32} and scheme["reward"] == {"vshape": (5,)}
            assert "group" not in scheme["reward_model"]
    # a model's own keys alone are validated: the other model's may hold anything
    run._check_reward_model(SimpleNamespace(**dict(CFG, reward_model="prosocial", ia_alpha=-1.0)))
    run._check_reward_model(SimpleNamespace(**dict(CFG, reward_model="inequity_aversion", prosocial_weight=7)))


# ---- 7. the tensor-op learner ------------------------------------------------------------------------------------------------------------------------
def _state(mac):
    return {k: v.detach().clone() for k, v in mac.agent.state_dict().items()}


@pytest.mark.parametrize("model", MODELS)
def test_host_learner_with_the_key_on_is_the_key_off_learner_on_the_shaped_field(model):
    """obs_reward: False (the fixture's weights are shaped for the shipped input set: both learners start from one seeded initialisation)"""
    from tests.learner_util import load_fixture
    z, meta = load_fixture("learner_cleanup5.npz")
    over = dict(obs_reward=False)
    build = lambda z, meta, overrides: U.build_seeded(z, meta, **overrides)
    _, batch_on, mac_on, on = build(z, meta, overrides=dict(over, reward_model=model))
    _, _, mac_off, off = build(z, meta, overrides=over)
    assert all(th.equal(a, b) for a, b in zip(mac_on.parameters(), mac_off.parameters()))
    U.add_field(batch_on, model)
    batch_off = U.key_off_twin(batch_on, off)
    assert th.equal(batch_off["reward"], batch_on["reward_model"]) and not th.equal(batch_off["reward"], batch_on["reward"])
    for step in range(2):
        logs_on, logs_off = on.cal_loss_and_step(batch_on), off.cal_loss_and_step(batch_off)
        for k in ("loss_value_env", "loss_value_inc", "loss_sim"):
            assert float(logs_on[k]) == float(logs_off[k]) and np.isfinite(float(logs_on[k])), (step, k, float(logs_on[k]), float(logs_off[k]))
        a, b = _state(mac_on), _state(mac_off)
        assert all(U.bit_equal(a[k].numpy(), b[k].numpy()) for k in a), step
    # the comparison can fail: the key-on learner on a batch whose field holds the RAW rewards steps elsewhere
    _, batch_raw, mac_raw, raw = build(z, meta, overrides=dict(over, reward_model=model))
    U.add_field(batch_raw, model)
    batch_raw.data.transition_data["reward_model"] = batch_raw["reward"].clone()
    for step in range(2):
        raw.cal_loss_and_step(batch_raw)
    a, b = _state(mac_on), _state(mac_raw)
    assert not all(U.bit_equal(a[k].numpy(), b[k].numpy()) for k in a)


def test_the_shaping_does_not_reach_the_observations():
    """obs_reward: True -- the built inputs of the key-on batch (per step and time-batched) are those of the raw-reward batch"""
    from tests.learner_util import build, load_fixture
    z, meta = load_fixture("learner_cleanup5.npz")
    _, batch_on, mac_on, _ = build(z, meta, overrides=dict(obs_reward=True, reward_model="inequity_aversion"))
    _, batch, mac, _ = build(z, meta, overrides=dict(obs_reward=True))
    U.add_field(batch_on)
    batch.data.transition_data["reward"].copy_(batch_on["reward"])                    # the raw-reward batch: what the env paid, no field
    assert "reward_model" not in batch.data.transition_data and batch["reward"][:, :-1].any()
    with th.no_grad():
        for t in (0, 3, batch.max_seq_length - 1):
            assert th.equal(mac_on._build_inputs(batch_on, t), mac._build_inputs(batch, t))
        sh_on, sh = mac_on.unroll_shared(batch_on), mac.unroll_shared(batch)
        assert th.equal(mac_on.unroll_inputs(batch_on, sh_on), mac.unroll_inputs(batch, sh)) and th.equal(sh_on["other"], sh["other"])
        # ... and the comparison can fail: a batch whose `reward` is the shaped field builds other inputs
        twisted = U.key_off_twin(batch_on, SimpleNamespace(mac=SimpleNamespace(unroll_shared=None), target_mac=SimpleNamespace(unroll_shared=None)))
        assert not th.equal(mac._build_inputs(twisted, 3), mac._build_inputs(batch, 3))


# ---- 8. the window gather ------------------------------------------------------------------------------------------------------------------------------
def test_window_gather_returns_the_slot_slices_of_the_stored_field():
    from tests import train_window_util as W
    from tests.learner_util import build, load_fixture
    z, meta = load_fixture("learner_cleanup5.npz")
    _, batch, _, _ = build(z, meta)
    U.add_field(batch)
    buf = W.buffer_of(batch, size=2 * batch.batch_size)
    stored = buf.data.transition_data["reward_model"].numpy().copy()
    assert np.array_equal(stored[:batch.batch_size], batch["reward_model"].numpy())
    T = batch.max_seq_length - 1
    ids, t0 = [0, batch.batch_size - 1, 1, batch.batch_size + 1], [0, T - 6, 3, 1]
    win = buf.gather_windows(ids, t0, 6, 2)
    assert win["reward_model"].dtype == th.float32 and win["reward_model"].shape == (4, 7, stored.shape[-1])
    assert np.array_equal(win["reward_model"].numpy(), W.window_slices(stored, ids, t0, 7))
    assert np.array_equal(win["reward"].numpy(), W.window_slices(buf.data.transition_data["reward"].numpy(), ids, t0, 7))


# ---- 9. the logged means ---------------------------------------------------------------------------------------------------------------------------------
def test_logged_means_are_sums_in_a_stated_order():
    """HipVecRunner.reward_model_means on a stand-in that holds an accumulator whose cells span 30 binary orders: each mean is the
    running sum over ascending (env, agent) divided once by the count, to the bit; the accumulator is zeroed by the read"""
    from homophily_marl_amd.runners.hip_vec_runner import HipVecRunner
    rng = np.random.default_rng(4)
    acc = rng.standard_normal((67, 5, 3)) * np.exp2(rng.integers(-15, 15, size=(67, 5, 3)))
    for model, names in (("inequity_aversion", ("reward_model_mean", "ia_envy_mean", "ia_guilt_mean")), ("prosocial", ("reward_model_mean", "prosocial_others_mean"))):
        me = SimpleNamespace(_reward_acc=th.from_numpy(acc.copy()), _reward_rollouts=3, batch_size=67, episode_limit=12,
                             args=SimpleNamespace(n_agents=5, reward_model=model))
        got = HipVecRunner.reward_model_means(me)
        assert tuple(got) == names
        for col, name in enumerate(names):
            assert got[name] == U.logged_mean(acc, col, 3 * 67 * 12 * 5), name
        assert not me._reward_acc.any() and me._reward_rollouts == 0 and HipVecRunner.reward_model_means(me) == {}
    assert any(U.logged_mean(acc, c, 1.0) != float(acc[..., c].sum()) for c in range(3))          # (numpy's pairwise sum is another order)


def test_one_predicate_says_whether_a_model_is_named():
    """runner, scheme and learner agree: absent, None and "individual" are off"""
    from homophily_marl_amd import ops
    from homophily_marl_amd.runners.hip_vec_runner import HipVecRunner
    info = dict(state_shape=10, obs_shape=20, n_actions=9)
    base = dict(CFG, name="homophily", obs_storage="f32", store_state=True, n_actions=9)
    for keys, on in (({}, False), (dict(reward_model=None), False), (dict(reward_model="individual"), False), (dict(reward_model="prosocial"), True),
                     (dict(reward_model="inequity_aversion"), True)):
        a = SimpleNamespace(**dict(base, **keys))
        assert HipVecRunner._reward_model_on(SimpleNamespace(args=a)) is on
        assert (ops.reward_field(a) == "reward_model") is on and ("reward_model" in run.build_scheme(a, info)[0]) is on
