"""CPU suite: Polyak target updates (config key target_tau) -- the tensor-op learner against the REFERENCE's own train()
with its _update_targets replaced by the rule (tests/golden/learner_soft_target.npz, tools/gen_soft_target_golden.py), the key's
off state, the refusals, the logged gap.  Device half: tests/test_soft_target_gpu.py; shared: tests/soft_target_util.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from tests import motion_util as mu
from tests import soft_target_util as su

INV = abi.SSD_ERR_INVALID
F = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched


def test_fixture_holds_results_only_and_its_arms_are_apart():
    zs, meta = su.load_fixture("learner_soft_target.npz")
    assert meta["batch"] == "learner_cleanup5.npz" and meta["overrides"] == dict(target_update_interval=1)
    assert not [k for k in zs.files if k.startswith("batch_") or k.startswith("w_")]
    assert int(zs["n_calls"]) == 6 and zs["taus"].tolist() == [0.25, 0.05, 1.0]
    for k in range(1, 7):                                                     # tau = 1 is the reference's hard sync at interval 1
        for key in mu.LOG_KEYS:
            assert float(zs["tau1_call%d_%s" % (k, key)]) == float(zs["hard_call%d_%s" % (k, key)])
        assert np.array_equal(zs["tau1_call%d_param_sq" % k], zs["hard_call%d_param_sq" % k])
    for name in ("power_tau0.25_vs_never", "power_tau0.25_vs_hard", "power_tau0.05_vs_never", "power_tau0.05_vs_tau0.25"):
        print(name, ["%.1f" % v for v in zs[name]])
        assert zs[name][0] == 0 and zs[name][1:].min() >= su.POWER_BARS


@pytest.mark.parametrize("tau", [0.25, 0.05, 1.0])
def test_six_train_calls_under_polyak_updates_match_the_reference(tau):
    """every call at the golden's bars; from call 2 on the never-updated and the hard-sync recordings are missed by more than 10 bars
    (tau = 1 IS the hard sync at interval 1: there the never-updated arm alone); the target net's caches follow in place; the
    reference's hard sync is never called (target_update_interval 1 would call it after every step)"""
    zs, arm = su.golden(), su.TAU_ARMS[tau]
    batch, mac, learner, seen = su.host_learner(target_tau=tau, target_update_interval=1)
    assert [str(x) for x in zs["param_names"]] == list(mac.agent.state_dict().keys())
    hard = []
    learner._update_targets = lambda: hard.append(1)
    tgt, ptrs = learner.target_mac.agent, None
    for k in range(1, 7):
        learner.train(batch, 0, k)
        assert len(seen) == k and learner.last_target_update_episode == 0
        su.assert_call(zs, arm, k, seen[-1], mac)
        if k == 1:
            ptrs = [t.data_ptr() for t in mu.cache_tensors(tgt)]
        mu.assert_caches_follow(tgt, tgt, ptrs, "after call %d" % k)
        if tau == 1.0:
            mu.assert_caches_follow(tgt, mac.agent, ptrs, "tau 1, call %d" % k)
            assert all(th.equal(a, b) for a, b in zip(tgt.parameters(), mac.agent.parameters()))
        if k >= 2:
            others = ("never_",) + (("hard_",) if tau != 1.0 else ())
            miss = {o: su.power(zs, arm, o, k, seen[-1], mac) for o in others}
            print("tau %g call %d: distance from the other arms in bars %s" % (tau, k, {o: "%.1f" % v for o, v in miss.items()}))
            assert min(miss.values()) > su.POWER_BARS, (k, miss)
    assert not hard


def test_target_follows_the_restated_recursion_bit_for_bit_on_the_host():
    batch, mac, learner, _ = su.host_learner(target_tau=0.25)
    want = su.params_np(learner.target_mac.agent)
    for k in range(1, 4):
        learner.train(batch, 0, k)
        live = su.params_np(mac.agent)
        want = {name: su.polyak_np(want[name], live[name], 0.25) for name in want}
        got = su.params_np(learner.target_mac.agent)
        assert all(got[name].tobytes() == want[name].tobytes() for name in want), k


def test_key_zero_is_the_learner_without_the_key():
    """target_tau 0 against the key absent: parameters, both optimisers' state and the target net bit-identical after six calls, and
    the hard syncs still happen (interval 2: three of them)"""
    runs = []
    for absent in (True, False):
        batch, mac, learner, _ = su.host_learner(target_tau=0, target_update_interval=2)
        if absent:
            a2 = SimpleNamespace(**vars(learner.args))
            del a2.target_tau
            learner = type(learner)(mac, batch.scheme, learner.logger, a2)
            assert not hasattr(learner.args, "target_tau")
        assert learner.target_tau == 0.0
        syncs, inner = [], learner._update_targets
        learner._update_targets = lambda syncs=syncs, inner=inner: (syncs.append(1), inner())
        for k in range(1, 7):
            learner.train(batch, 0, k)
        assert len(syncs) == 3 and learner._gap_partials is None and learner._polyak is None
        state = [st[key].clone() for opt in (learner.optimiser_inc, learner.optimiser_env) for p in opt.param_groups[0]["params"]
                 for st in (opt.state[p],) for key in ("step", "exp_avg", "exp_avg_sq")]
        runs.append(([p.detach().clone() for p in mac.parameters()], [p.detach().clone() for p in learner.target_mac.parameters()], state))
    for a, b in zip(*runs):
        assert len(a) == len(b) > 0 and all(th.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf"), -float("inf"), "fast", True])
def test_setup_refuses_a_tau_outside_the_unit_interval(bad):
    from homophily_marl_amd.run import load_config, setup
    cfg = load_config("cleanup", overrides=dict(target_tau=bad, use_cuda=False, env_args=dict(num_agents=5, map="default5", episode_limit=12)))
    with pytest.raises(ValueError, match="target_tau"):
        setup(cfg)


def test_learner_refuses_a_tau_outside_the_unit_interval():
    batch, mac, learner, _ = su.host_learner()
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "fast"):
        with pytest.raises(ValueError, match="target_tau"):
            type(learner)(mac, batch.scheme, learner.logger, SimpleNamespace(**dict(vars(learner.args), target_tau=bad)))


def test_setup_accepts_the_ends_of_the_interval_and_the_key_absent():
    from homophily_marl_amd.run import _check_target_tau
    assert _check_target_tau(SimpleNamespace()) == 0.0 and _check_target_tau(SimpleNamespace(target_tau=None)) == 0.0
    for v in (0, 0.0, 1, 1.0, 0.05, 2.0 ** -30):
        a = SimpleNamespace(target_tau=v)
        assert _check_target_tau(a) == float(v) and a.target_tau == float(v)


def test_the_console_says_once_that_the_interval_is_ignored():
    lines = []
    _, _, learner, _ = su.host_learner()
    logger = SimpleNamespace(log_stat=lambda *a, **k: None, console_logger=SimpleNamespace(info=lines.append))
    batch = su.host_learner()[0]
    on = type(learner)(learner.mac, batch.scheme, logger, SimpleNamespace(**dict(vars(learner.args), target_tau=0.05)))
    assert len(lines) == 1 and "target_update_interval" in lines[0] and "ignored" in lines[0]
    for k in range(1, 3):
        on.train(batch, 0, k)
    assert len(lines) == 1                                                    # ("Updated target network" never appears)
    type(learner)(learner.mac, batch.scheme, logger, SimpleNamespace(**dict(vars(learner.args), target_tau=0.0)))
    assert len(lines) == 1


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------
def _args(**over):
    """valid arguments of ssd_clip_adam_step with one Polyak job (dummy pointers; never called as they are)"""
    kw = dict(flat_grad=F, total=10, jobs=F, n_jobs=1, partials=F, lr_inc=1e-3, lr_env=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip=1.0,
              polyak_jobs=F, n_polyak=1, target_tau=0.5, polyak_partials=F)
    kw.update(over)
    return abi.SsdClipAdamArgs(**kw)


@pytest.mark.parametrize("label,over,text", [
    ("n_polyak < 0", dict(n_polyak=-1), b"n_polyak"), ("n_polyak = limit + 1", dict(n_polyak=abi.POLYAK_MAX_JOBS + 1), b"n_polyak"),
    ("jobs NULL", dict(polyak_jobs=None), b"polyak_jobs"), ("tau < 0", dict(target_tau=-0.25), b"target_tau"),
    ("tau > 1", dict(target_tau=1.0 + 2.0 ** -23), b"target_tau"), ("tau NaN", dict(target_tau=float("nan")), b"target_tau"),
    ("tau inf", dict(target_tau=float("inf")), b"target_tau"), ("tau 0 with jobs", dict(target_tau=0.0), b"target_tau 0"),
    ("tau outside without jobs", dict(n_polyak=0, polyak_jobs=None, target_tau=2.0), b"target_tau"),
    ("the Adam checks still come first", dict(clip=0.0), b"clip")], ids=lambda v: v if isinstance(v, str) else "")
def test_entry_point_refuses_before_any_launch(label, over, text):
    lib = abi.load_library()
    assert lib.ssd_clip_adam_step(C.byref(_args(**over)), None) == INV, label
    msg = lib.ssd_last_error()
    assert b"ssd_clip_adam_step" in msg and text in msg, (label, msg)


def test_job_table_builder_checks_what_the_entry_point_cannot():
    ok = (F, F + 4, 7, 3, 9)
    assert C.sizeof(abi.polyak_job_table([ok])) == C.sizeof(abi.SsdPolyakJob) == 32 and abi.POLYAK_MAX_JOBS == 128
    t = abi.polyak_job_table([ok] * abi.POLYAK_MAX_JOBS)
    assert (t[127].src, t[127].dst, t[127].rows, t[127].cols, t[127].dst_row_stride) == ok
    for bad in ([], [ok] * (abi.POLYAK_MAX_JOBS + 1), [(F, F, 0, 3, 3)], [(F, F, 7, 0, 3)], [(F, F, 7, 3, 2)], [(0, F, 7, 3, 3)], [(F, None, 7, 3, 3)],
                [(F + 2, F, 7, 3, 3)], [(F, F + 1, 7, 3, 3)], [(F, F, 1 << 16, 1 << 15, 1 << 15)]):
        with pytest.raises(ValueError, match="Polyak job"):
            abi.polyak_job_table(bad)


# ---- the logged gap ----------------------------------------------------------------------------------------------------------------------
def test_target_gap_rel_is_logged_at_the_float64_value():
    batch, mac, learner, _ = su.host_learner(target_tau=0.05, learner_log_interval=1)
    stats = []
    learner.logger = SimpleNamespace(log_stat=lambda k, v, t: stats.append((k, v, t)), console_logger=None)
    for k in range(1, 4):
        learner.train(batch, 10 * k, k)
        want = su.gap_rel64(su.params_np(mac.agent), su.params_np(learner.target_mac.agent))
        got = [v for key, v, t in stats if key == "target_gap_rel" and t == 10 * k]
        print("call %d: target_gap_rel %.9e, float64 %.9e" % (k, got[0], want))
        assert len(got) == 1 and want > 0 and abs(got[0] - want) <= 1e-6 * want
    _, _, off, _ = su.host_learner(learner_log_interval=1)
    off.logger = SimpleNamespace(log_stat=lambda k, v, t: stats.append(("off " + k, v, t)), console_logger=None)
    off.train(batch, 10, 1)
    assert "off loss_value_env" in [s[0] for s in stats] and "off target_gap_rel" not in [s[0] for s in stats]


def test_launch_partials_restatement_adds_up():
    """the numpy restatement of the launch's partial sums (used by the device test) against plain float64 sums"""
    rng = np.random.default_rng(5)
    live, new = rng.standard_normal(70001).astype(np.float32), rng.standard_normal(70001).astype(np.float32)
    whole = rng.random(70001) < 0.6
    p = su.launch_partials(live, new, whole, abi.POLYAK_WORKGROUPS)
    assert p.shape == (256, 2) and p.dtype == np.float32 and (p[-1] == 0).all()            # P = 512: 137 workgroups hold elements
    want = [(((live - new).astype(np.float64)) ** 2)[whole].sum(), (live.astype(np.float64) ** 2)[whole].sum()]
    assert np.allclose(p.astype(np.float64).sum(0), want, rtol=1e-6)
