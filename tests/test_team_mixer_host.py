"""CPU suite: the VDN mixer of the env head (config key mixer: "vdn"; DESIGN sections 4.2 and 7) -- the refusals of run.setup and the
key's off values against the learner without the key; the tensor-op learner against a float64 statement of PyMARL's QLearner under its
VDNMixer; the linearity that ties the rule to the pinned per-agent seeds; the export's header / table / refusals (dummy pointers, ONLY
invalid calls: nothing is launched); the kernel ledger's counts.  Device half: tests/test_team_mixer_gpu.py; shared:
tests/team_mixer_util.py."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops, run
from homophily_marl_amd.learners import homophily_learner as HL
from tests import kernel_cases as kc
from tests import td_lambda_util as TU
from tests import team_mixer_util as U
from tests.test_td_lambda_gpu import random_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = abi.SSD_ERR_INVALID
F = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched
LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")
SHAPES = {2: (3, 9, 2), 5: (3, 9, 5)}                                   # (B, T, n) of the learner tests: three episodes, two end early


# ---- 1. config and refusals --------------------------------------------------------------------------------------------------------------
def _cfg(**over):
    return run.load_config("cleanup", overrides=dict(dict(use_cuda=False, env_args=dict(num_agents=5, map="default5", episode_limit=12)), **over))


@pytest.mark.parametrize("bad", ["qmix", "VDN", "vdn ", True, 1, 0, ("vdn",)])
def test_setup_refuses_an_unknown_mixer(bad):
    with pytest.raises(ValueError, match=r'mixer must be null \(or "none"\) or "vdn"'):
        run.setup(_cfg(mixer=bad))
    with pytest.raises(ValueError, match="mixer must be"):
        run._check_mixer(SimpleNamespace(mixer=bad, n_agents=5))
    with pytest.raises(ValueError, match="mixer must be"):
        U.learner_on(random_arrays(*SHAPES[2]), mixer=bad)                # the learner reads the key once, in __init__


def test_setup_refuses_one_agent_and_a_team_reward():
    with pytest.raises(ValueError, match=r"mixer 'vdn' needs n_agents >= 2"):
        run._check_mixer(SimpleNamespace(mixer="vdn", n_agents=1))
    with pytest.raises(ValueError, match=r"mixer 'vdn' needs ind_reward: True .*n times"):
        run.setup(_cfg(mixer="vdn", ind_reward=False))
    with pytest.raises(ValueError, match="ind_reward"):
        run._check_mixer(SimpleNamespace(mixer="vdn", n_agents=5, ind_reward=False))
    import inspect
    src = inspect.getsource(run.setup)                                        # setup asks again once n_agents is known, before the controller
    assert src.index("args.n_agents, args.n_actions = ") < src.rindex("_check_mixer(args)") < src.index("mac_REGISTRY[args.mac]")
    assert src.index("_check_mixer(args)") < src.index("r_REGISTRY[args.runner]")


def test_setup_allows_every_other_key_and_writes_the_value_back():
    for raw in (None, "", "none"):
        a = SimpleNamespace(mixer=raw, n_agents=1, ind_reward=False)          # off: nothing is asked of the other keys
        assert run._check_mixer(a) is None and a.mixer is None
    a = SimpleNamespace(n_agents=1)
    assert run._check_mixer(a) is None and a.mixer is None                    # the key absent
    a = SimpleNamespace(mixer="vdn", n_agents=2, ind_reward=True, reward_model="prosocial", td_lambda=0.5, train_window=4, share_heads="both",
                        target_tau=0.1, prioritized_replay=True, per_initial_priority="rollout")
    assert run._check_mixer(a) == "vdn" == a.mixer
    assert run.load_config("cleanup")["mixer"] is None and ops.MIXERS == ("vdn",)


def _two_steps(arr, **over):
    args, batch, mac, learner = U.learner_on(arr, **over)
    logs = []
    for _ in range(2):
        out = learner.cal_loss_and_step(batch)
        logs.append([float(out[k]) for k in LOG_KEYS])
    return learner, logs, [p.detach().clone() for p in mac.parameters()]


def test_the_off_values_are_the_learner_without_the_key():
    """mixer null, "" and "none" against the key absent (the parent ignored it): two CPU train steps, every logged value and every
    parameter equal to the bit; "vdn" moves the env loss and the parameters"""
    arr = random_arrays(3, 6, 2)
    runs = {}
    for name, over in (("absent", None), ("null", dict(mixer=None)), ("empty", dict(mixer="")), ("none", dict(mixer="none")), ("vdn", dict(mixer="vdn"))):
        if over is None:
            args, batch, mac, learner = U.learner_on(arr)
            del args.mixer                                                     # (the learner was built with the config's empty key ...)
            th.manual_seed(5)
            from tests.learner_util import le_REGISTRY
            learner = le_REGISTRY[args.learner](mac, batch.scheme, learner.logger, args)    # ... and again without the attribute
            assert learner.mixer is None
            logs = []
            for _ in range(2):
                out = learner.cal_loss_and_step(batch)
                logs.append([float(out[k]) for k in LOG_KEYS])
            runs[name] = (logs, [p.detach().clone() for p in mac.parameters()])
        else:
            learner, logs, params = _two_steps(arr, **over)
            assert learner.mixer == (over["mixer"] if over["mixer"] == "vdn" else None)
            runs[name] = (logs, params)
    for name in ("null", "empty", "none"):
        assert runs[name][0] == runs["absent"][0], name
        assert all(th.equal(a, b) for a, b in zip(runs[name][1], runs["absent"][1])) and len(runs[name][1]) > 0, name
    k = LOG_KEYS.index("loss_value_env")
    assert runs["vdn"][0][0][k] != runs["absent"][0][0][k]
    assert [v for i, v in enumerate(runs["vdn"][0][0]) if i != k] == [v for i, v in enumerate(runs["absent"][0][0]) if i != k]   # nothing else is logged differently
    assert not all(th.equal(a, b) for a, b in zip(runs["vdn"][1], runs["absent"][1]))


# ---- 2. the tensor-op learner against the independent statement ---------------------------------------------------------------------------
def vdn_loss_f64(arr, cfg, lam):
    """PyMARL's QLearner under VDNMixer in float64 torch: the chosen values and the selected target values summed over the agents (what
    VDNMixer.forward does to both), the team reward sum_i rewards_for_env,i, ONE mask entry per (b, t), loss = (masked_td^2).sum() /
    mask.sum(), differentiated by autograd.  With td_lambda the target is the forward-view recursion on the team's quantities.
    Returns (loss, d loss / d q_env [B, T + 1, n, A]).  cfg: the scalars of ssd_td_loss_args (gamma as the f32 the code is handed)."""
    p = TU.host_rows(arr["q_env"], arr["q_inc"], arr["tq_env"], arr["tq_inc"], arr["avail"], arr["actions"], arr["actions_inc"], arr["reward"],
                     arr["terminated"], arr["filled"], cfg["double_q"], 0, cfg["reward_scale"], cfg["incentive_ratio"], cfg["incentive_cost"],
                     cfg["incentive"], cfg["seq_len"])
    r, term, mask = (th.tensor(p[k]) for k in ("r_env", "term", "mask"))
    r = r.sum(2)                                                                           # the team reward [B, T]
    q = th.tensor(arr["q_env"], dtype=th.float64, requires_grad=True)
    tq = th.tensor(arr["tq_env"], dtype=th.float64)
    ok = th.as_tensor(arr["avail"]) != 0
    acts = th.as_tensor(arr["actions"])[..., None]
    chosen = th.gather(q[:, :-1], 3, acts[:, :-1]).squeeze(3).sum(2)                       # mixer(chosen_action_qvals)
    tqm = tq.masked_fill(~ok, TU.NEG)[:, 1:]
    if cfg["double_q"]:
        best = q.detach().masked_fill(~ok, TU.NEG)[:, 1:].argmax(3, keepdim=True)
        tmax = th.gather(tqm, 3, best).squeeze(3)
    else:
        tmax = tqm.max(3)[0]
    tmax = tmax.sum(2)                                                                     # target_mixer(target_max_qvals)
    gamma, T = cfg["gamma_env"], r.shape[1]
    if lam == 0:
        target = r + gamma * (1 - term) * tmax
    else:
        g = tmax[:, T - 1] * (1 - term.sum(1))
        rows = [None] * T
        for t in range(T - 1, -1, -1):
            g = lam * gamma * g + mask[:, t] * (r[:, t] + (1 - lam) * gamma * tmax[:, t] * (1 - term[:, t]))
            rows[t] = g
        target = th.stack(rows, 1)
    masked = (chosen - target.detach()) * mask
    loss = (masked ** 2).sum() / mask.sum()
    loss.backward()
    return float(loss.detach()), q.grad.numpy()


def f64_bounds(arr, cfg, lam, dens, loss_off, dq_off):
    """The bar of the comparison with vdn_loss_f64, from the mixer-OFF path's own distance to float64 on the same arrays (tests/
    td_lambda_util.host_loss: the per-agent statement the loss kernel is held to): n times that gap, for the loss and for the largest
    gradient element.  The gaps are carried as RELATIVE numbers -- |loss - f64| / f64 and max |dq - f64| / max |f64| -- because the
    team's values are not of the per-agent values' size (the team error is a sum of n errors and its seed carries the factor n: a team
    loss of 3.18 stands against a per-agent loss of 1.1 on the same arrays); n times the ABSOLUTE gap lies below half an f32 ulp of
    the team's own values (1.95e-7 against a spacing of 2.4e-7 at 3.18) and no f32 code could meet it.  A measured gap can fall under
    the rounding step of the f32 value itself by luck (the loss is ONE number; the per-agent gradient's largest element came out
    2.9e-8 from float64 at n = 2, td_lambda 0.5); half an ulp (2^-24 relative) is the least any f32 result can promise, so each gap
    enters at no less.  Returns the two relative bars (to be scaled by the float64 team loss and by the largest float64 team gradient
    element) and the two measured relative gaps."""
    n = arr["q_env"].shape[2]
    ref = TU.host_loss(arr, dict(cfg, consider_others_inc=0), lam, dens)
    loss64 = float(ref["sq_env"].sum() / dens[0])
    gap_loss = abs(loss_off - loss64) / loss64
    gap_dq = float(np.abs(dq_off - ref["dq_env"]).max() / np.abs(ref["dq_env"]).max())
    return n * max(gap_loss, 2.0 ** -24), n * max(gap_dq, 2.0 ** -24), (gap_loss, gap_dq)


_ops_runs = {}


def _ops_run(n, double_q, lam, others, mixer):
    """one forward_backward of the tensor-op learner on the recipe's Q-values (made once per case, shared, never written)"""
    key = (n, double_q, lam, others, mixer)
    if key not in _ops_runs:
        arr = random_arrays(*SHAPES[n])
        args, batch, mac, learner = U.learner_on(arr, double_q=bool(double_q), td_lambda=lam, consider_others_inc=bool(others), mixer=mixer)
        cfg = U.learner_cfg(args, batch)
        cfg["gamma_env"] = float(np.float32(cfg["gamma_env"]))           # a python float times an f32 tensor: the f32 of the float
        loss, dq, dens = U.with_fixed_q(learner, batch, arr)
        dq.setflags(write=False)
        _ops_runs[key] = (arr, cfg, loss, dq, [float(d) for d in dens])
    return _ops_runs[key]


@pytest.mark.parametrize("others", [0, 1])
@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("double_q", [1, 0])
@pytest.mark.parametrize("n", [2, 5])
def test_tensor_op_learner_is_the_float64_vdn_statement(n, double_q, lam, others):
    """loss_value_env and d loss / d q_env of the CPU learner under mixer: "vdn" against vdn_loss_f64.  The bar is f64_bounds: on these
    arrays the mixer-off tensor-op loss sits 1.3e-8 .. 1.1e-7 (relative) from its float64 statement and its largest gradient element
    2.9e-8 .. 9.2e-8; the mixer is allowed n times that, each gap counted at 2^-24 = 6.0e-8 at least (as measured here: the team loss at
    1.9e-8 .. 1.5e-7 from float64, 0.07 .. 0.8 of its bar; the gradient at 3.5e-8 .. 9.6e-8, 0.2 .. 0.7 of its bar).
    consider_others_inc is an option of the inc head: the env part must not move by a bit."""
    arr, cfg, loss_off, dq_off, dens = _ops_run(n, double_q, lam, others, None)
    _, _, loss, dq, dens_on = _ops_run(n, double_q, lam, others, "vdn")
    assert dens_on == dens and dens[0] == float(U.mask_f32(arr).sum() * n)
    bar_loss, bar_dq, gaps = f64_bounds(arr, cfg, lam, dens, loss_off, dq_off)
    want_loss, want_dq = vdn_loss_f64(arr, cfg, lam)
    e_loss, e_dq = abs(loss - want_loss) / want_loss, float(np.abs(dq - want_dq).max() / np.abs(want_dq).max())
    print("n %d dq %d lam %g oth %d: mixer-off relative gaps %.2e / %.2e; team loss %.6f off by %.2e (bar %.2e), gradient max %.3e off by %.2e (bar %.2e)"
          % (n, double_q, lam, others, gaps[0], gaps[1], want_loss, e_loss, bar_loss, np.abs(want_dq).max(), e_dq, bar_dq))
    assert np.abs(want_dq).max() > 0 and want_loss > 0
    assert e_loss <= bar_loss and e_dq <= bar_dq
    if others:
        _, _, loss0, dq0, _ = _ops_run(n, double_q, lam, 0, "vdn")
        assert loss == loss0 and np.array_equal(dq, dq0)


# ---- 3. linearity against the pinned path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("n", [2, 5])
def test_every_seed_is_n_times_the_ascending_sum_of_the_mixer_off_seeds(n, lam):
    """seed_vdn[b, t, i, a_i] against n (((s_0 + s_1) + s_2) + ...), s_k = the mixer-off seed dq_env[b, t, k, a_k] of the same (b, t).
    mask is 0 or 1 and the factor 2 is exact, so an s_k is 2 td_k mask / den0 with one rounding (the division); its sum takes n - 1 adds,
    the team's td another n - 1, then one division and the factor n: at most 2 (n - 1) + 3 roundings of 2^-24 each, relative to
    n sum_k |s_k|.  The bar is (2 (n - 1) + 3) 2^-24 n sum_k |s_k|."""
    arr, _, _, dq_off, _ = _ops_run(n, 1, lam, 0, None)
    _, _, _, dq_on, _ = _ops_run(n, 1, lam, 0, "vdn")
    T = arr["q_env"].shape[1] - 1
    idx = arr["actions"][:, :T, :, None]
    s = np.take_along_axis(dq_off[:, :T], idx, -1)[..., 0]                                 # [B, T, n]
    total = s[..., 0].copy()
    for k in range(1, n):
        total = total + s[..., k]
    want = np.float32(n) * total
    got = np.take_along_axis(dq_on[:, :T], idx, -1)[..., 0]
    bar = (2 * (n - 1) + 3) * 2.0 ** -24 * n * np.abs(s).astype(np.float64).sum(-1)
    err = np.abs(got.astype(np.float64) - want[..., None])
    print("n %d lam %g: worst seed at %.2f of its bar" % (n, lam, float((err / np.maximum(bar[..., None], 1e-300)).max())))
    assert (err <= bar[..., None]).all() and np.abs(want).max() > 0
    assert (got == got[..., :1]).all()                                                     # the n rows of a (b, t): the same bits
    rest = dq_on.copy()
    np.put_along_axis(rest[:, :T], idx, 0.0, -1)
    assert not rest.any()                                                                   # the other A - 1 entries and slot T: zeros


def test_team_td_adds_in_ascending_order():
    """2^24 + 1 + 1 in f32 is 2^24 from the left and 2^24 + 2 from the right"""
    td = th.tensor([[[2.0 ** 24, 1.0, 1.0]]])
    assert HL.team_td(td).reshape(-1).tolist() == [2.0 ** 24] * 3
    assert HL.team_td(td.flip(-1)).reshape(-1).tolist() == [2.0 ** 24 + 2] * 3
    dq, col2 = U.rule_f32(td.numpy(), np.ones((1, 1), np.float32), np.zeros((1, 2, 3), np.int64), 1.0, 2)
    assert dq[0, 0, :, 0].tolist() == [2.0 * 2.0 ** 24 * 3] * 3 and U.rule_f32(td.numpy(), np.ones((1, 1), np.float32), np.zeros((1, 2, 3), np.int64), 1.0, 2,
                                                                                 reverse=True)[0][0, 0, 0, 0] == 2.0 * (2.0 ** 24 + 2) * 3


@pytest.mark.parametrize("shape", [(3, 43, 3), (2, 7, 10)])
def test_the_recipes_arrays_tell_the_order_of_the_agent_sum(shape):
    """the power check of the device test, decided here without a device: on the recipe's arrays (its seed is the shape's) the one-step
    rule with the agents added in descending order differs from the stated order in at least one row"""
    from tests.test_td_lambda_gpu import CFG
    arr = random_arrays(*shape)
    for double_q in (1, 0):
        td = U.one_step_td_f32(arr, dict(CFG, double_q=double_q, seq_len=float(shape[1] + 1)))
        fwd = U.rule_f32(td, U.mask_f32(arr), arr["actions"], 7.0, 9)
        rev = U.rule_f32(td, U.mask_f32(arr), arr["actions"], 7.0, 9, reverse=True)
        assert (fwd[1] != rev[1]).any() and (fwd[0] != rev[0]).any()


# ---- 4. header, exports and entry refusals -------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssd_hip_mix.h")).read(), flags=re.S)


def test_header_table_and_library_name_the_same_export():
    names = set(abi.MIX_SIGNATURES)
    assert sorted(set(re.findall(r"\b(ssd_[a-z_0-9]+)\s*\(", _header()))) == sorted(names) == ["ssd_team_td"]
    assert not names & (set(abi.HIP_SIGNATURES) | set(abi.TRAIN_SIGNATURES) | set(abi.REWARD_SIGNATURES) | set(abi.TIE_SIGNATURES))
    raw, bound = C.CDLL(abi.HIP_LIB_PATH), abi.load_library()
    for name, (res, argtypes) in abi.MIX_SIGNATURES.items():
        assert hasattr(raw, name), name
        assert getattr(bound, name).argtypes == argtypes and getattr(bound, name).restype is res, name
    assert bound.ssd_abi_version() == abi.ABI_VERSION == 10                    # no member more, the same version


def test_the_header_compiles_as_c(tmp_path):
    import subprocess
    c = tmp_path / "t.c"
    c.write_text('#include "ssd_hip_mix.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])


POINTERS = ("q_env", "tq_env", "actions", "actions_inc", "avail", "reward", "terminated", "filled", "dens", "dq_env", "partials")


def _args(**over):
    a = abi.SsdTdLossArgs(batch=3, t_slots=7, n_agents=5, n_actions=9, sim_horizon=3, double_q=1, gamma_env=0.99, gamma_inc=0.99, reward_scale=1.0,
                          incentive_ratio=1.0, incentive_cost=0.5, incentive=2.0, seq_len=7.0, sim_threshold=0.1, sim_loss_weight=0.1, td_lambda=0.0)
    for k, name in enumerate(POINTERS + ("q_inc", "tq_inc", "clean_num", "dq_inc")):
        setattr(a, name, F + 4096 * k)
    for k, v in over.items():
        setattr(a, k, v)
    return a


ROWS = ([("n_agents 1", dict(n_agents=1), b"n_agents"), ("n_agents 11", dict(n_agents=abi.MAX_AGENTS + 1), b"n_agents"), ("n_agents 0", dict(n_agents=0), b"n_agents"),
         ("rows over SSD_ROWS32_MAX", dict(batch=1 << 12, t_slots=1 << 18, n_agents=10), b"SSD_ROWS32_MAX"),
         ("rows at the limit + 1", dict(batch=(2 ** 31 - 1 - 256) // 4 + 1, t_slots=2, n_agents=2), b"SSD_ROWS32_MAX"),
         ("batch 0", dict(batch=0), b"batch"), ("t_slots 1", dict(t_slots=1), b"t_slots"), ("n_actions 0", dict(n_actions=0), b"n_actions"),
         ("td_lambda -0.1", dict(td_lambda=-0.1), b"td_lambda"), ("td_lambda 1.5", dict(td_lambda=1.5), b"td_lambda"),
         ("td_lambda NaN", dict(td_lambda=float("nan")), b"td_lambda"),
         ("seq_len 0", dict(seq_len=0.0), b"seq_len"), ("reward_scale 0", dict(reward_scale=0.0), b"reward_scale")]
        + [("null %s" % p, {p: None}, b"null") for p in POINTERS]
        + [("%s at 2 bytes" % p, {p: F + 4096 * k + 2}, b"4-byte") for k, p in enumerate(POINTERS) if p != "terminated"]
        + [("%s at 1 byte" % p, {p: F + 4096 * k + 1}, b"4-byte") for k, p in enumerate(POINTERS) if p in ("dq_env", "partials")])


@pytest.mark.parametrize("label,over,text", ROWS, ids=[r[0] for r in ROWS])
def test_entry_point_refuses_before_any_launch(label, over, text):
    lib = abi.load_library()
    rc = lib.ssd_team_td(C.byref(_args(**over)), None)
    msg = lib.ssd_last_error()
    assert rc == INV and b"ssd_team_td" in msg and text in msg, (label, rc, msg)


def test_entry_point_refuses_null_args():
    lib = abi.load_library()
    assert lib.ssd_team_td(None, None) == INV and b"ssd_team_td" in lib.ssd_last_error()


# ---- 5. the ledger is still closed --------------------------------------------------------------------------------------------------------
def test_the_five_ledger_sources_hold_the_kernels_they_held():
    counts = {"ssd_env.hip": 30, "ssd_learner.hip": 30, "ssd_bmm.hip": 16, "ssd_gru_seq.hip": 12, "ssd_policy.hip": 10}
    assert set(kc.SOURCES) == set(counts)
    for src, want in counts.items():
        assert len(kc.compiled(src)) == want, (src, sorted(kc.compiled(src)))
    assert sum(counts.values()) == 98
    assert not any("team_td" in k for src in kc.SOURCES for k in kc.compiled(src))          # the new kernel lives in its own source
