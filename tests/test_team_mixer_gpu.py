"""GPU suite: the VDN mixer of the env head (config key mixer: "vdn"; include/ssd_hip_mix.h; DESIGN sections 4.2 and 7).

  1. ssd_team_td alone, behind ssd_td_sim_loss mode 1 on the same operands in the poisoned arena: dq_env at every element and column 2
     of the partials against the f32 numpy restatement of the rule (tests/team_mixer_util.py) bit for bit; everything else the loss
     launch wrote, and every input, untouched; the n rows of a (b, t) identical; the restatement with the agents added in descending
     order must miss;
  2. the restatement's own one-step td_i, squared under the mask, is the mixer-off launch's column 2 to the bit;
  3. the device learner under the key against the tensor-op learner, eager and captured; the priorities written under prioritised
     replay; the launches counted;
  4. the launch against the float64 statement of PyMARL's VDN loss (tests/test_team_mixer_host.py).
Host half: tests/test_team_mixer_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests import priority_util as P
from tests import team_mixer_util as U
from tests.arena_util import Arena
from tests.test_td_lambda_gpu import CFG, LOG_KEYS, _dens, random_arrays

pytestmark = pytest.mark.gpu

f32 = np.float32
bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
# one loss row in front of the bootstrap slot; 129 (b, t) pairs (past eight 16-pair workgroups, one past a 128-thread block); the
# largest team; rows past 256, where the lambda kernel changes chunk
SHAPES = [(2, 1, 2), (3, 43, 3), (2, 7, 10), (1, 260, 2)]
CASES = [(s, lam, dq) for s in SHAPES for lam in (0.0, 0.5) for dq in (1, 0)]
_runs = {}


def both_launches(shape, lam, double_q):
    """ssd_td_sim_loss mode 1, then ssd_team_td on the same struct, every operand in the arena (operands at odd 4-byte offsets);
    Arena.check() after each: bands, slack and inputs untouched, the written sets kept, no NaN.  Returns the arrays, the scalars and
    the outputs after the first and after the second launch; made once per case and shared."""
    key = (shape, lam, double_q)
    if key in _runs:
        return _runs[key]
    arr = random_arrays(*shape)
    B, T1, n, A = arr["q_env"].shape
    T = T1 - 1
    dens = _dens(arr)
    ar = Arena()
    a = abi.SsdTdLossArgs(batch=B, t_slots=T1, n_agents=n, n_actions=A, double_q=double_q, consider_others_inc=0, seq_len=float(T1), td_lambda=lam, **CFG)
    Pl = ar.place
    regs = dict(q_env=Pl("q_env", arr["q_env"], offset_in_16=4), q_inc=Pl("q_inc", arr["q_inc"], offset_in_16=8), tq_env=Pl("tq_env", arr["tq_env"], offset_in_16=12),
                tq_inc=Pl("tq_inc", arr["tq_inc"], offset_in_16=4), actions=Pl("actions", arr["actions"], align=8, fill=A),
                actions_inc=Pl("actions_inc", arr["actions_inc"], align=8, fill=3), avail=Pl("avail", arr["avail"], offset_in_16=12, fill=0),
                reward=Pl("reward", arr["reward"], offset_in_16=8), clean_num=Pl("clean_num", arr["clean_num"], offset_in_16=12),
                terminated=Pl("terminated", arr["terminated"], align=1, fill=1), filled=Pl("filled", arr["filled"], align=8, fill=0),
                dens=Pl("dens", f32(dens), offset_in_16=4))
    wp = np.zeros((B * T * n, abi.TD_LOSS_PARTIALS), dtype=bool)
    wp[:, :15 if lam > 0 else 13] = True
    regs["partials"] = ar.reserve("partials", wp.shape, offset_in_16=8, written=wp)
    regs["dq_env"] = ar.reserve("dq_env", arr["q_env"].shape, offset_in_16=12, written=True)
    regs["dq_inc"] = ar.reserve("dq_inc", arr["q_inc"].shape, offset_in_16=4, written=True)
    for k, r in regs.items():
        setattr(a, k, r.ptr)
    lib = abi.load_library()
    outs = []
    for call in (lambda: lib.ssd_td_sim_loss(C.byref(a), 1, None), lambda: lib.ssd_team_td(C.byref(a), None)):
        abi.check(lib, call())
        ar.check()
        outs.append(dict(partials=regs["partials"].array().reshape(B, T, n, abi.TD_LOSS_PARTIALS).copy(), dq_env=regs["dq_env"].array().copy(),
                         dq_inc=regs["dq_inc"].array().copy()))
    cfg = dict(CFG, double_q=double_q, consider_others_inc=0, seq_len=float(T1))
    _runs[key] = (arr, cfg, dens, outs[0], outs[1])
    return _runs[key]


def _agents_td(arr, cfg, lam, loss_out):
    """the rule's td_i: the one-step restatement, or columns 5 and 13 of the rows the loss launch wrote"""
    if lam > 0:
        return loss_out["partials"][..., 5] - loss_out["partials"][..., 13]
    return U.one_step_td_f32(arr, cfg)


# ---- 1. the launch alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lam,double_q", CASES, ids=["%dx%dx%d-lam%g-dq%d" % (s + (l, d)) for s, l, d in CASES])
def test_team_launch_in_the_arena(shape, lam, double_q):
    arr, cfg, dens, loss_out, out = both_launches(shape, lam, double_q)
    B, T, n = shape
    A = arr["q_env"].shape[-1]
    td = _agents_td(arr, cfg, lam, loss_out)
    assert td.dtype == f32
    mask = U.mask_f32(arr)
    want_dq, want_c2 = U.rule_f32(td, mask, arr["actions"], f32(dens[0]), A)
    # dq_env at every element, zeros included, and column 2
    assert np.array_equal(bits(out["dq_env"]), bits(want_dq)), int((bits(out["dq_env"]) != bits(want_dq)).sum())
    assert np.array_equal(bits(out["partials"][..., 2]), bits(want_c2))
    assert np.abs(want_dq).max() > 0 and not out["dq_env"][:, T].any()
    # every other column, and dq_inc, as the loss launch wrote them (column 15 keeps the arena's pre-fill: Arena.check)
    keep = [c for c in range(abi.TD_LOSS_PARTIALS) if c != 2]
    assert np.array_equal(bits(out["partials"][..., keep]), bits(loss_out["partials"][..., keep]))
    assert np.array_equal(bits(out["dq_inc"]), bits(loss_out["dq_inc"]))
    # the n rows of a (b, t): identical
    seeds = np.take_along_axis(out["dq_env"][:, :T], arr["actions"][:, :T, :, None], -1)[..., 0]
    assert (bits(seeds) == bits(seeds)[..., :1]).all() and (bits(out["partials"][..., 2]) == bits(out["partials"][..., 2])[..., :1]).all()
    # something moved: the team's numbers are not the agents'
    assert not np.array_equal(out["partials"][..., 2], loss_out["partials"][..., 2])
    # power: the agents added in descending order are told apart (n >= 3; at n = 2 the two orders are one)
    rev_dq, rev_c2 = U.rule_f32(td, mask, arr["actions"], f32(dens[0]), A, reverse=True)
    if n >= 3:
        assert (bits(out["dq_env"]) != bits(rev_dq)).any() and (bits(out["partials"][..., 2]) != bits(rev_c2)).any()
    else:
        assert np.array_equal(bits(rev_dq), bits(want_dq))


# ---- 2. the restated expressions are the loss kernel's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,double_q", [(s, d) for s in SHAPES for d in (1, 0)], ids=["%dx%dx%d-dq%d" % (s + (d,)) for s in SHAPES for d in (1, 0)])
def test_restated_one_step_td_is_the_loss_kernels(shape, double_q):
    arr, cfg, dens, loss_out, _ = both_launches(shape, 0.0, double_q)
    td = U.one_step_td_f32(arr, cfg)
    m = U.mask_f32(arr)[..., None]
    assert np.array_equal(bits((td * m) * (td * m)), bits(loss_out["partials"][..., 2]))
    chosen = np.take_along_axis(arr["q_env"][:, :shape[1]], arr["actions"][:, :shape[1], :, None], -1)[..., 0]
    assert np.array_equal(bits(chosen), bits(loss_out["partials"][..., 5]))


# ---- 3. the device learner ----------------------------------------------------------------------------------------------------------------
def _record(monkeypatch, names):
    lib = abi.load_library()
    calls = []
    for name in names:
        def counted(*args, _inner=getattr(lib, name), _name=name):
            calls.append(_name)
            return _inner(*args)
        monkeypatch.setattr(lib, name, counted, raising=True)
    return calls


@pytest.mark.parametrize("train_graph", [False, True])
@pytest.mark.parametrize("n,lam", [(2, 0.0), (5, 0.5)])
def test_device_learner_matches_the_tensor_op_learner(n, lam, train_graph, monkeypatch):
    """batch 3, T = 6, two optimisation steps under mixer: "vdn": the device learner (strict_device_ops) against the tensor-op learner
    on CPU tensors -- every logged value and the per-parameter checksums within 1e-5, the bar of tests/test_td_lambda_gpu.py for the
    same comparison; eagerly and as the captured step (checked against an eager evaluation at every replay).  ssd_team_td is called
    once per train step that goes through the binding; the replays carry it inside the graph."""
    from tests.learner_util import param_checksums
    from tests.test_learner_options import perturb_target
    th.backends.cuda.matmul.allow_tf32 = False
    monkeypatch.setenv("SSD_GRAPH_CHECK", "1")
    arr = random_arrays(3, 6, n)
    over = dict(td_lambda=lam, mixer="vdn")
    want = []
    args, batch, mac, learner = U.learner_on(arr, **over)
    perturb_target(learner)
    for step in range(2):
        logs = learner.cal_loss_and_step(batch)
        want.append(({k: float(logs[k]) for k in LOG_KEYS}, param_checksums(mac)))
    # the key changes what is trained: the same two steps without it end elsewhere
    _, batch0, mac0, plain = U.learner_on(arr, td_lambda=lam)
    perturb_target(plain)
    assert abs(float(plain.cal_loss_and_step(batch0)["loss_value_env"]) - want[0][0]["loss_value_env"]) > 1e-3
    calls = _record(monkeypatch, ["ssd_team_td"])
    args, batch, mac, learner = U.learner_on(arr, device="cuda:0", code_obs=True, train_graph=train_graph, **over)
    ops.set_strict(True)
    try:
        assert learner._fused(batch) and learner.use_graph == train_graph and learner.mixer == "vdn"
        if train_graph:
            sd0 = {k: v.clone() for k, v in mac.agent.state_dict().items()}
            for _ in range(3):
                learner.train(batch, 0, 0)
            assert learner._graph is not None and len(calls) == 3 + 1                # three steps, and SSD_GRAPH_CHECK's eager evaluation
            mac.agent.load_state_dict(sd0)
            learner.target_mac.load_state(mac)
            for opt in (learner.optimiser_env, learner.optimiser_inc):
                for st in opt.state.values():
                    st["step"].zero_(); st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
            del calls[:]
        perturb_target(learner)
        for step in range(2):
            if train_graph:
                learner.train(batch, 0, 0)
                logs = learner._static_logs
            else:
                logs = learner.cal_loss_and_step(batch)
            ref_logs, (sums, sqs, heads) = want[step]
            for k in LOG_KEYS:
                assert abs(float(logs[k]) - ref_logs[k]) < 1e-5, (step, k, float(logs[k]), ref_logs[k])
            got = param_checksums(mac)
            assert np.abs(got[2] - heads).max() < 1e-5, step
            assert (np.abs(got[0] - sums) <= 1e-5 * np.maximum(1.0, np.abs(sums))).all(), step
            assert (np.abs(got[1] - sqs) <= 1e-5 * np.maximum(1.0, np.abs(sqs))).all(), step
        # eager: one call per step; captured: the replays issue none through the binding (only the check's eager evaluation does)
        assert len(calls) == 2
    finally:
        ops.set_strict(False)


@pytest.mark.parametrize("n,lam", [(5, 0.0), (2, 0.5)])
def test_priorities_are_formed_from_the_teams_rows_and_the_launches_are_counted(n, lam, monkeypatch):
    """prioritised replay on: q_new as ssd_priority_update forms it from the rows behind ssd_team_td, against priority_update's rule in
    float64 (tests/priority_util.q_new, bar within_q) over the tensor-op learner's rows under the key, whose column 2 is the team's;
    the table written accordingly; the per-agent rows would have given other priorities.  One ssd_team_td per train step, between the
    loss launch and ssd_priority_update; none with the key off."""
    from tests.test_learner_options import perturb_target
    th.backends.cuda.matmul.allow_tf32 = False
    arr = random_arrays(3, 6, n)
    calls = _record(monkeypatch, ["ssd_td_sim_loss", "ssd_team_td", "ssd_priority_update"])
    made = {}
    for name, over in (("fused", dict(mixer="vdn")), ("plain", dict(mixer="vdn", fused_loss=False)), ("off", dict()), ("off_plain", dict(fused_loss=False))):
        args, batch, mac, learner = U.learner_on(arr, device="cuda:0", td_lambda=lam, **over)
        perturb_target(learner)
        table = th.zeros(8, dtype=th.int32, device="cuda")
        ids, w = th.tensor([5, 1, 5], device="cuda"), th.tensor([1.0, 0.5, 0.25], device="cuda")
        batch.priority = (table, ids, w)
        del calls[:]
        for _ in range(2):
            learner.forward_backward(batch)
        th.cuda.synchronize()
        made[name] = (learner, table.cpu().tolist(), list(calls))
        del batch.priority
    # (the denominators are a mode-0 ssd_td_sim_loss of their own: two loss calls per step)
    assert made["fused"][2] == ["ssd_td_sim_loss", "ssd_td_sim_loss", "ssd_team_td", "ssd_priority_update"] * 2, made["fused"][2]
    assert made["off"][2] == ["ssd_td_sim_loss", "ssd_td_sim_loss", "ssd_priority_update"] * 2, made["off"][2]
    assert "ssd_team_td" not in made["plain"][2] + made["off_plain"][2]
    q = made["fused"][0].last_q_new.cpu().numpy().astype(np.int64)
    rows = made["plain"][0].last_td_rows.cpu().numpy()
    team = rows[:, 2].reshape(3, 6, n)
    assert (team == team[..., :1]).all() and rows[:, 2].max() > 0
    exact, _ = P.q_new(rows, 3, *made["fused"][0].per)
    assert P.within_q(q, exact), (q, exact)
    assert made["fused"][1] == P.write_back(np.zeros(8, np.int64), [5, 1, 5], q).tolist()
    exact_off, _ = P.q_new(made["off_plain"][0].last_td_rows.cpu().numpy(), 3, *made["fused"][0].per)
    assert not P.within_q(q, exact_off), (q, exact_off)


# ---- 4. the float64 statement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("double_q", [1, 0])
def test_team_launch_against_the_float64_vdn_statement(double_q, lam):
    """(3, 43, 3): the launch's column 2 summed over the rows and divided by dens[0] (the logged loss_value_env) and its seeds against
    tests/test_team_mixer_host.vdn_loss_f64, at the bar stated there (f64_bounds: n times the mixer-off launch's own relative distance
    to its float64 statement on the same arrays, each gap counted at 2^-24 at least)."""
    from tests.test_team_mixer_host import f64_bounds, vdn_loss_f64
    arr, cfg, dens, loss_out, out = both_launches((3, 43, 3), lam, double_q)
    cfg = dict(cfg, gamma_env=float(f32(cfg["gamma_env"])), gamma_inc=float(f32(cfg["gamma_inc"])), sim_threshold=float(f32(cfg["sim_threshold"])),
               sim_loss_weight=float(f32(cfg["sim_loss_weight"])))
    dens = [float(f32(d)) for d in dens]
    loss_of = lambda o: float(o["partials"][..., 2].astype(np.float64).sum() / dens[0])
    bar_loss, bar_dq, gaps = f64_bounds(arr, cfg, lam, dens, loss_of(loss_out), loss_out["dq_env"])
    want_loss, want_dq = vdn_loss_f64(arr, cfg, lam)
    e_loss, e_dq = abs(loss_of(out) - want_loss) / want_loss, float(np.abs(out["dq_env"] - want_dq).max() / np.abs(want_dq).max())
    print("dq %d lam %g: mixer-off relative gaps %.2e / %.2e; team loss %.6f off by %.2e (bar %.2e), gradient max %.3e off by %.2e (bar %.2e)"
          % (double_q, lam, gaps[0], gaps[1], want_loss, e_loss, bar_loss, np.abs(want_dq).max(), e_dq, bar_dq))
    assert e_loss <= bar_loss and e_dq <= bar_dq
