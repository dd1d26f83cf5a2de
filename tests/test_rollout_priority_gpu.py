"""GPU suite of prioritised replay's initial priorities (config key per_initial_priority: "rollout"; ssd_rollout_priority):
  1. the kernel, driven slot by slot over given arrays, against the numpy float64 restatement (tests/rollout_priority_util.py) on
     inputs whose TD errors are exact in f32 -- only the sqrt / sum / pow chain rounds: the bar is priority_util.within_q;
  2. the same on general floats, the bar widened by the propagated rounding of the TD subtraction (derived in the test);
  3. every operand in the poisoned arena of tests/arena_util.py: only carry, acc and (at slot T) q_init change;
  4. the rollout in each timestep form: the launch list, the inserted table slots, q_init against the restatement on Q-values
     recomputed from the stored episode by the learner's whole-episode forward, a second rollout, a train step's write-back;
  5. the key absent against "max": the loop bit for bit, and no q_out buffer on the runner.

Masks (the learner's _td_mask): row 0 of an episode always carries loss where it is filled, so an env that terminates AT slot 0 keeps
row 0 alone (with live = 0); an env with no filled slot has no loss row and gets p = eps."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests import priority_util as P
from tests import rollout_priority_util as U
from tests.arena_util import Arena

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 1), (3, 5, 9), (67, 10, 16), (64, 3, 9)]             # (N, n, A): one env; ragged; over four workgroups, n and A at their limits; whole waves
T = 7
FIELDS = ("actions", "actions_inc", "reward", "terminated", "filled")


def _layout(q, layout):
    """q [N, n, ...] of one slot as the heads leave it: agent-major [n, N, ...] or env-major"""
    return np.ascontiguousarray(np.swapaxes(q, 0, 1)) if layout == "agent_major" else np.ascontiguousarray(q)


def _strides(N, n, A, layout):
    return (N * A, A, N * n * 3, n * 3) if layout == "agent_major" else (A, n * A, n * 3, n * n * 3)


def _drive(ep, N, n, A, layout, c, alpha, eta, eps, avail_bits, filled=True):
    """the T + 1 launches of an episode over device copies of the arrays: q_init [N] as int64"""
    lib = abi.load_library()
    dev = {k: th.as_tensor(ep[k]).cuda() for k in FIELDS}
    q_env, q_inc = th.zeros(_layout(ep["q_env"][:, 0], layout).shape, device="cuda"), th.zeros(_layout(ep["q_inc"][:, 0], layout).shape, device="cuda")
    t_index = th.zeros(1, dtype=th.long, device="cuda")
    carry, acc = th.full((N, n, 2), float("nan"), device="cuda"), th.full((N, n, 3), float("nan"), device="cuda")
    q_init = th.zeros(N, dtype=th.int32, device="cuda")
    a = abi.SsdRolloutPriorityArgs()
    a.t_index, a.n_env, a.n_agents, a.n_actions, a.t_slots, a.avail_bits = t_index.data_ptr(), N, n, A, T + 1, avail_bits
    a.q_env, a.q_inc, a.carry, a.acc, a.q_init = q_env.data_ptr(), q_inc.data_ptr(), carry.data_ptr(), acc.data_ptr(), q_init.data_ptr()
    a.q_env_agent_stride, a.q_env_env_stride, a.q_inc_agent_stride, a.q_inc_env_stride = _strides(N, n, A, layout)
    for k in FIELDS:
        setattr(a, k, dev[k].data_ptr() if (k != "filled" or filled) else None)
    for k, v in dict(c, alpha=alpha, eta=eta, eps=eps).items():
        setattr(a, k, v)
    st = th.cuda.current_stream().cuda_stream
    for t in range(T + 1):
        q_env.copy_(th.as_tensor(_layout(ep["q_env"][:, t], layout)))
        q_inc.copy_(th.as_tensor(_layout(ep["q_inc"][:, t], layout)))
        t_index.fill_(t)
        assert lib.ssd_rollout_priority(C.byref(a), st) == 0, lib.ssd_last_error()
    th.cuda.synchronize()
    return q_init.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _reference(ep, c, alpha, eta, eps, avail_bits, filled=True):
    return U.initial_priority(ep["q_env"], ep["q_inc"], ep["actions"], ep["actions_inc"], ep["reward"], ep["terminated"],
                              ep["filled"] if filled else None, avail_bits, c, alpha, eta, eps)


def _exact_case(N, n, A):
    ep = U.episodes(N, T, n, A, seed=100 * N + 10 * n + A, exact=True)
    if A > 1:
        ep["q_env"][..., 0] = 2.0                                         # the largest Q-value of every row: excluded by avail_bits below
    ep["filled"][N - 1] = 0                                               # an env without a loss row: p = eps (with `filled` given)
    return ep


# ---- 1. exact TD inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["agent_major", "env_major"])
@pytest.mark.parametrize("N,n,A", SHAPES)
def test_kernel_is_the_restatement_on_exact_td_inputs(N, n, A, layout):
    ep = _exact_case(N, n, A)
    c = dict(U.DYADIC)
    assert c["seq_len"] == T + 1
    eps = 2.0 ** -10
    full, partial = (1 << A) - 1, ((1 << A) - 2) if A > 1 else 1
    for filled, bits in ((True, partial), (False, full)):
        for alpha in (0.0, 0.6, 1.0):
            for eta in (0.0, 0.9, 1.0):
                got = _drive(ep, N, n, A, layout, c, alpha, eta, eps, bits, filled)
                ref = _reference(ep, c, alpha, eta, eps, bits, filled)
                err = np.abs(got - ref.exact)
                print("N %d n %d A %d %s filled %s alpha %.1f eta %.1f: q in [%d, %d], largest |got - exact| %.3f (bar 1 + exact 2^-20)"
                      % (N, n, A, layout, filled, alpha, eta, got.min(), got.max(), err.max()))
                assert P.within_q(got, ref.exact), (filled, alpha, eta, got, ref.exact)
                if filled:                                                   # no loss row: p = eps exactly
                    assert got[N - 1] == int(np.rint(np.clip(eps ** alpha * P.ONE, 1, P.QMAX))), (alpha, got[N - 1])
    # the cases mean something: rows after a termination add nothing, the excluded action would have changed the value
    ref = _reference(ep, c, 1.0, 0.9, eps, partial, True)
    if N > 1:
        term = ep["terminated"]
        b = int(np.argmax(term[1:].any(axis=1))) + 1 if term[1:].any() else None
        if b is not None and b != N - 1:
            t_end = int(np.argmax(term[b]))
            assert not ref.mask[b, t_end + 1:].any() and ref.mask[b, :t_end + 1].all()
        if N > 1:
            assert ref.mask[0, 0].all() and not ref.mask[0, 1:].any()       # terminated at slot 0: row 0 alone
    if A > 1:
        other = _reference(ep, c, 1.0, 0.9, eps, full, True)
        assert (other.q != ref.q).any()


# ---- 2. general floats ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["agent_major", "env_major"])
@pytest.mark.parametrize("N,n,A", [(3, 5, 9), (67, 10, 16)])
def test_kernel_on_general_floats_within_the_propagated_rounding(N, n, A, layout):
    """The config's constants (gamma 0.95 / 0.995, incentive_cost 0.1) and normal random Q-values: the TD subtraction rounds too.
    Derivation of the bar.  td_h = chosen_h - (r_h + gamma_h live V_h) is evaluated in f32 from f32 inputs; its roundings (the reward
    arithmetic, the product, the sum, the difference) are each relative 2^-24 of a term bounded by M_h = |chosen_h| + |r_h| +
    gamma_h |V_h|, four of them at most: |td_h(f32) - td_h| <= 2^-22 M_h.  d = sqrt(td_env^2 + td_inc^2) is 1-Lipschitz in each error, so
    |d(f32 tds) - d| <= delta = 2^-22 (max_rows M_env + max_rows M_inc); p = eta max d + (1 - eta) mean d + eps has weights that sum to 1:
    |p' - p| <= delta.  q = ONE p^alpha has the slope ONE alpha p^(alpha - 1), which falls with p (alpha <= 1): on [p - delta, p + delta] it
    is at most its value at max(p - delta, eps) (p >= eps always).  The remaining chain (sqrt, sums, pow) is priority_util.within_q's:
        |got - exact| <= 1 + exact 2^-20 + ONE alpha max(p - delta, eps)^(alpha - 1) delta."""
    from homophily_marl_amd.run import load_config
    cfg = load_config("cleanup")
    assert (cfg["gamma_env"], cfg["gamma_inc"], cfg["incentive_cost"]) == (0.95, 0.995, 0.1)
    c = ops.td_constants(SimpleNamespace(**cfg), T + 1)
    ep = U.episodes(N, T, n, A, seed=7 * N + n, exact=False)
    bits = (1 << A) - 1 - 4
    for alpha, eta, eps in ((0.6, 0.9, 1e-3), (1.0, 0.0, 1e-3), (0.3, 1.0, 1e-6)):
        got = _drive(ep, N, n, A, layout, c, alpha, eta, eps, bits)
        ref = _reference(ep, c, alpha, eta, eps, bits)
        delta = 2.0 ** -22 * (ref.bound[0].reshape(N, -1).max(axis=1) + ref.bound[1].reshape(N, -1).max(axis=1))
        slope = P.ONE * alpha * np.maximum(ref.p - delta, eps) ** (alpha - 1.0)
        bar = 1.0 + ref.exact * 2.0 ** -20 + slope * delta
        err = np.abs(got - ref.exact)
        print("N %d n %d A %d %s alpha %.1f eta %.1f: p in [%.4f, %.4f], delta <= %.3e, largest |got - exact| %.3f at a bar of %.3f"
              % (N, n, A, layout, alpha, eta, ref.p.min(), ref.p.max(), delta.max(), err.max(), bar[np.argmax(err)]))
        assert (err <= bar).all(), (alpha, eta, err.max())


# ---- 3. bounds --------------------------------------------------------------------------------------------------------------------------
def _arena_case(ep, N, n, A, layout, t, c, rng):
    ar = Arena()
    reg = dict(t_index=ar.place("t_index", np.array([t], np.int64), align=8, fill=0))
    tq = min(max(t, 0), T)
    reg["q_env"] = ar.place("q_env", _layout(ep["q_env"][:, tq], layout))
    reg["q_inc"] = ar.place("q_inc", _layout(ep["q_inc"][:, tq], layout), offset_in_16=4)
    reg["actions"] = ar.place("actions", ep["actions"], align=8, fill=0)
    reg["actions_inc"] = ar.place("actions_inc", ep["actions_inc"], align=8, fill=0)
    reg["reward"] = ar.place("reward", ep["reward"], offset_in_16=12)
    reg["terminated"] = ar.place("terminated", ep["terminated"], align=1, fill=0)
    reg["filled"] = ar.place("filled", ep["filled"], align=8, fill=1)
    carry0, acc0 = rng.uniform(-1, 1, (N, n, 2)).astype(np.float32), rng.uniform(0, 1, (N, n, 3)).astype(np.float32)
    reg["carry"] = ar.place("carry", carry0, offset_in_16=8, inout=True)
    reg["acc"] = ar.place("acc", acc0, offset_in_16=4, inout=True)
    reg["q_init"] = ar.reserve("q_init", (N,), np.uint32, written=(t == T))
    a = abi.SsdRolloutPriorityArgs()
    for k, r in reg.items():
        setattr(a, k, r.ptr)
    a.n_env, a.n_agents, a.n_actions, a.t_slots, a.avail_bits = N, n, A, T + 1, (1 << A) - 1
    a.q_env_agent_stride, a.q_env_env_stride, a.q_inc_agent_stride, a.q_inc_env_stride = _strides(N, n, A, layout)
    for k, v in dict(c, alpha=0.6, eta=0.9, eps=1e-3).items():
        setattr(a, k, v)
    return ar, a, reg, carry0, acc0


@pytest.mark.parametrize("layout", ["agent_major", "env_major"])
@pytest.mark.parametrize("N,n,A", SHAPES[:3])
def test_launch_stays_inside_its_operands_and_writes_only_its_state(N, n, A, layout):
    lib = abi.load_library()
    st = th.cuda.current_stream().cuda_stream
    ep = U.episodes(N, T, n, A, seed=N + n + A, exact=True)
    c = dict(U.DYADIC)
    rng = np.random.default_rng(N)
    off = 1 - np.eye(n, dtype=np.int64)
    for t in (0, 3, T, -1, T + 1):
        ar, a, reg, carry0, acc0 = _arena_case(ep, N, n, A, layout, t, c, rng)
        assert lib.ssd_rollout_priority(C.byref(a), st) == 0, lib.ssd_last_error()
        ar.check()                                                           # bands, slack and inputs bit-identical; q_init written iff t == T
        carry, acc = reg["carry"].array(), reg["acc"].array()
        if not 0 <= t <= T:
            assert carry.tobytes() == carry0.tobytes() and acc.tobytes() == acc0.tobytes(), t
            continue
        assert not np.isnan(carry).any() and not np.isnan(acc).any(), t      # no poison reached the state
        if t < T:                                                            # carry: this slot's Q at the actions filed in slot t (f32, j rising)
            chosen_env = np.take_along_axis(ep["q_env"][:, t], ep["actions"][:, t, :, None], axis=2)[..., 0]
            taken = np.take_along_axis(ep["q_inc"][:, t], ep["actions_inc"][:, t, :, :, None], axis=3)[..., 0]
            chosen_inc = np.zeros((N, n), np.float32)
            for j in range(n):
                chosen_inc = (chosen_inc + taken[:, :, j] * off[:, j].astype(np.float32)).astype(np.float32)
            assert carry[..., 0].tobytes() == chosen_env.astype(np.float32).tobytes() and carry[..., 1].tobytes() == chosen_inc.tobytes(), t
        else:
            assert carry.tobytes() == carry0.tobytes()
        if t == 0:
            assert not acc.any()
        else:
            mask = ep["filled"][:, t - 1] * (1 - ep["terminated"][:, t - 2] if t > 1 else 1)
            assert np.array_equal(acc[..., 2], acc0[..., 2] + mask[:, None].astype(np.float32))
            assert (acc[..., 0] >= acc0[..., 0]).all() and (acc[..., 1] >= acc0[..., 1]).all()
            assert np.array_equal(acc[mask == 0], acc0[mask == 0])            # a row without loss adds nothing
        if t == T:                                                           # q_init is the aggregate of the state the launch left
            a64 = acc.astype(np.float64)
            p = 0.9 * a64[..., 0].max(axis=1) + 0.1 * a64[..., 1].sum(axis=1) / np.maximum(1.0, a64[..., 2].sum(axis=1)) + 1e-3
            assert P.within_q(reg["q_init"].array().astype(np.int64), np.clip(p ** 0.6 * P.ONE, 1.0, P.QMAX))


def test_refusals_launch_nothing():
    lib = abi.load_library()
    st = th.cuda.current_stream().cuda_stream
    ep = U.episodes(3, T, 5, 9, seed=1, exact=True)
    for field, value in (("q_env", 0), ("carry", 0), ("n_agents", 11), ("n_actions", 17), ("avail_bits", 0), ("eps", 0.0), ("alpha", 2.0),
                         ("q_inc_env_stride", -15), ("acc", "+2"), ("actions", "+4"), ("t_slots", 1)):
        ar, a, reg, carry0, acc0 = _arena_case(ep, 3, 5, 9, "agent_major", T, dict(U.DYADIC), np.random.default_rng(0))
        reg["q_init"].written = False
        setattr(a, field, getattr(a, field) + int(value) if isinstance(value, str) else value)
        assert lib.ssd_rollout_priority(C.byref(a), st) == abi.SSD_ERR_INVALID, field
        assert b"ssd_rollout_priority" in lib.ssd_last_error(), field
        ar.check()
        assert reg["carry"].array().tobytes() == carry0.tobytes() and reg["acc"].array().tobytes() == acc0.tobytes(), field


@pytest.mark.parametrize("agent_major", [True, False])
def test_operator_reads_the_layout_it_is_told_at_as_many_envs_as_agents(agent_major):
    """N == n: [n, N, ...] and [N, n, ...] are the same shape, so the operator takes the layout from its caller; read the other way
    round the priorities would differ"""
    N = n = 5
    A = 9
    ep = U.episodes(N, T, n, A, seed=55, exact=True, terminate=False)
    layout = "agent_major" if agent_major else "env_major"
    store = {k: th.as_tensor(ep[k]).cuda() for k in ("actions", "actions_inc", "reward", "terminated", "filled")}
    store.update({k: store[k].unsqueeze(-1) for k in ("actions", "actions_inc", "terminated", "filled")})      # the scheme's trailing 1
    q_env, q_inc = th.zeros(N, n, A, device="cuda"), th.zeros(N, n, n, 3, device="cuda")
    t_index = th.zeros(1, dtype=th.long, device="cuda")
    args, keep = ops.rollout_priority_args(t_index, q_env, q_inc, agent_major, 0x1FF, store, dict(U.DYADIC), 0.6, 0.9, 2.0 ** -10)
    assert (args.q_env_agent_stride, args.q_env_env_stride, args.q_inc_agent_stride, args.q_inc_env_stride) == _strides(N, n, A, layout)
    for t in range(T + 1):
        q_env.copy_(th.as_tensor(_layout(ep["q_env"][:, t], layout)))
        q_inc.copy_(th.as_tensor(_layout(ep["q_inc"][:, t], layout)))
        t_index.fill_(t)
        ops.rollout_priority(args, q_env.device)
    th.cuda.synchronize()
    got = keep["q_init"].cpu().numpy().astype(np.int64)
    ref = _reference(ep, dict(U.DYADIC), 0.6, 0.9, 2.0 ** -10, 0x1FF)
    swapped = dict(ep, q_env=np.ascontiguousarray(ep["q_env"].transpose(2, 1, 0, 3)), q_inc=np.ascontiguousarray(ep["q_inc"].transpose(2, 1, 0, 3, 4)))
    wrong = _reference(swapped, dict(U.DYADIC), 0.6, 0.9, 2.0 ** -10, 0x1FF)
    assert P.within_q(got, ref.exact), (got, ref.exact)
    assert (np.abs(wrong.exact - ref.exact) > 1.0 + ref.exact * 2.0 ** -20).all()      # the other reading would not have passed
    with pytest.raises(ValueError, match="rollout_priority: q_env"):
        ops.rollout_priority_args(t_index, th.zeros(N, n + 1, A, device="cuda"), q_inc, agent_major, 0x1FF, store, dict(U.DYADIC), 0.6, 0.9, 1e-3)


# ---- 4. the rollout ---------------------------------------------------------------------------------------------------------------------
N_ENV, T_EP, BATCH = 8, 6, 4
TOL_Q = 1e-5                 # tests/test_policy_mfma.py: the rollout heads' Q-values against the f32 controller


def _ctx(drop=(), n_env=N_ENV, t_ep=T_EP, obs_storage="f32", **over):
    """(f32 observation storage at 8 envs: 8 episodes of 7 slots of u8 class codes are not a multiple of 16 bytes, and the env kernel
    writes 16-byte rows into the replay buffer's own slots)"""
    from homophily_marl_amd.run import load_config, setup
    th.manual_seed(0)
    np.random.seed(11)
    cfg = load_config("cleanup", overrides=dict(dict(
        runner="hip_graph", batch_size_run=n_env, batch_size=BATCH, buffer_size=2 * n_env, buffer_cpu_only=False, store_state=False, obs_storage=obs_storage,
        env_args=dict(num_agents=5, map="default5", episode_limit=t_ep, seed=3), use_cuda=True, save_model=False, runner_stats=False,
        learner_log_interval=10 ** 12, strict_device_ops=True, train_graph=True, train_steps_per_rollout=2, prioritized_replay=True), **over))
    for k in drop:
        del cfg[k]
    return setup(cfg)


def _launch_keys(**over):
    ctx = _ctx(**over)
    try:
        ctx.runner.run(test_mode=False)
        th.cuda.synchronize()
        return [k for _, k, _ in ctx.runner.timestep_launches()], (ctx.runner.fast is not None, ctx.runner.pipe), ctx.runner.q_env
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


GATHERED = dict(obs_others_last_action=True, fused_others_last_action=True)
# form -> (config keys, (FastPolicy kernels, pipelined)).  store_step: a store-step launch files the slot, not the heads.  generic_square:
# as many envs as agents, where the shapes of the Q buffers do not tell their layout.  gathered: the heads that gather fc1's rows.
FORMS = {"pipelined": ({}, (True, True)), "four_launch": (dict(pipeline_encode=False), (True, False)),
         "generic": (dict(fast_policy=False), (False, False)), "store_step": (dict(fold_store=False), (True, False)),
         "generic_square": (dict(fast_policy=False, n_env=5), (False, False)), "gathered": (GATHERED, (True, False)),
         "gathered_pipelined": (dict(GATHERED, pipeline_gathered=True), (True, True))}


@pytest.mark.parametrize("form", list(FORMS))
def test_rollout_files_the_priority_of_its_own_td_errors(form, monkeypatch):
    """four rollouts with frozen weights (eager, rollout-graph capture, edge-graph capture, pure replays), then one train step.
    The band of q_init.  The rollout's Q-values are within TOL_Q = 1e-5 of the learner's whole-episode forward on the stored episode
    (the project's bar for the heads).  td_env holds one chosen value and gamma_env times one bootstrap value, td_inc n - 1 of each:
    |td_env - ref| <= (1 + gamma_env) TOL_Q and |td_inc - ref| <= (n - 1)(1 + gamma_inc) TOL_Q; d is 1-Lipschitz in each and the max and
    the mean are 1-Lipschitz, so |p - p_ref| <= delta = (1 + gamma_env + (n - 1)(1 + gamma_inc)) TOL_Q, and q(p) = ONE p^alpha is monotone:
    q_init lies in [q(p_ref - delta) - 1, q(p_ref + delta) + 1] (1: the kernel's own f32 chain and rounding at these magnitudes)."""
    over, want_plan = FORMS[form]
    keys_off, plan_off, q_off = _launch_keys(**over)
    assert q_off is None
    launches, inner = [], ops.rollout_priority
    monkeypatch.setattr(ops, "rollout_priority", lambda args, device: (launches.append(1), inner(args, device))[1])
    ctx = _ctx(per_initial_priority="rollout", **over)
    try:
        runner, buf, a = ctx.runner, ctx.buffer, ctx.args
        n, N = a.n_agents, a.batch_size_run
        assert (N == n) == (form == "generic_square")
        c = ops.td_constants(a, T_EP + 1)
        delta = (1 + c["gamma_env"] + (n - 1) * (1 + c["gamma_inc"])) * TOL_Q
        table = buf.priority_table
        assert runner.initial_priorities() is None                            # before any rollout
        for e in range(4):
            before = table.cpu().numpy().astype(np.int64)
            lo = buf.buffer_index
            batch = runner.run(test_mode=False)
            q_init = runner.initial_priorities()
            assert q_init.dtype == th.int32 and tuple(q_init.shape) == (N,)
            if e == 0:                                                         # the eager rollout: one launch per slot, slot T included
                assert len(launches) == T_EP + 1, (form, len(launches))
            with th.no_grad():
                q_env, q_inc = ctx.mac.unroll(batch)                          # the learner's forward under the acting weights
            buf.insert_episode_batch(batch, priorities=q_init)
            th.cuda.synchronize()
            got, after = q_init.cpu().numpy().astype(np.int64), table.cpu().numpy().astype(np.int64)
            want = before.copy()
            want[lo:lo + N] = got
            assert np.array_equal(after, want) and (got > 0).all(), (form, e)  # the rollout's slots and nothing else; none is 0
            st = {k: batch[k].cpu().numpy() for k in ("actions", "actions_inc", "reward", "terminated", "filled", "avail_actions")}
            bits = sum(1 << k for k, v in enumerate(st["avail_actions"][0, 0, 0].tolist()) if v)
            ref = U.initial_priority(q_env.cpu().numpy(), q_inc.cpu().numpy(), st["actions"][..., 0], st["actions_inc"][..., 0], st["reward"],
                                     st["terminated"][..., 0], st["filled"][..., 0], bits, c, a.per_alpha, a.per_eta, a.per_eps)
            q_lo, q_hi = U.fixed(ref.p - delta, a.per_alpha) - 1, U.fixed(ref.p + delta, a.per_alpha) + 1
            print("%s rollout %d: q_init %s against the restatement %s (p in [%.4f, %.4f], band half-width %.1f)"
                  % (form, e, got.tolist(), ref.q.tolist(), ref.p.min(), ref.p.max(), ((q_hi - q_lo) / 2).max()))
            assert ((q_lo <= got) & (got <= q_hi)).all(), (form, e, got, q_lo, q_hi)
            assert len(set(got.tolist())) > 1                                  # not a constant
        keys_on = [k for _, k, _ in runner.timestep_launches()]
        plan = (runner.fast is not None, runner.pipe)
        assert plan == plan_off == want_plan, (form, plan, plan_off)
        # (timestep_launches lists the fused, head-filed timestep only: elsewhere the launch count above and the band show the launch)
        assert (keys_off == []) == (form in ("generic", "generic_square", "store_step")), (form, keys_off)
        if keys_off:
            assert "rollout_priority" not in keys_off and keys_on == keys_off + ["rollout_priority"]
        # a test episode takes the same launches on its own storage: the table and the training storage's priorities are untouched
        kept = runner._bundle.priority_state["q_init"].clone()
        bundle = runner._bundle
        runner.run(test_mode=True)
        th.cuda.synchronize()
        assert runner.initial_priorities() is None and th.equal(bundle.priority_state["q_init"], kept)
        assert np.array_equal(table.cpu().numpy().astype(np.int64), after)
        # a train step replaces the drawn episodes' entries (ssd_priority_update)
        sample = buf.sample_prioritized(BATCH, 0, 0, beta=a.per_beta, out=ctx.learner.sample_out() if hasattr(ctx.learner, "sample_out") else None)
        ids = sample.priority[1].cpu().tolist()
        ctx.learner.train(sample, runner.t_env, 0)
        th.cuda.synchronize()
        q_new = ctx.learner.last_q_new.cpu().numpy().astype(np.int64)
        assert np.array_equal(table.cpu().numpy().astype(np.int64), P.write_back(after, ids, q_new))
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


# ---- 5. the key off --------------------------------------------------------------------------------------------------------------------
def test_key_max_is_the_loop_without_the_key():
    """per_initial_priority absent against "max": the stored bytes, the sampled ids of every call, the priority table and the learner's
    parameters after four iterations are equal bit for bit, and the runner holds no q_out buffer"""
    from homophily_marl_amd.run import train_iteration
    runs = []
    for drop, over in ((("per_initial_priority",), {}), ((), dict(per_initial_priority="max"))):
        ctx = _ctx(drop=drop, n_env=32, t_ep=12, obs_storage="code", **over)      # (shape and storage of the sibling key-off tests)
        try:
            ids = []
            inner = ctx.learner.train

            def train(sample, t_env, episode, ids=ids, inner=inner):
                ids.append(sample.priority[1].cpu().tolist())
                inner(sample, t_env, episode)
            ctx.learner.train = train
            ep = 0
            for _ in range(4):
                ep = train_iteration(ctx, ep)
            th.cuda.synchronize()
            assert ctx.args.per_initial_priority == "max" and ctx.runner.q_env is None and ctx.runner.q_inc is None
            assert ctx.runner.initial_priorities() is None
            assert "rollout_priority" not in [k for _, k, _ in ctx.runner.timestep_launches()]
            runs.append((ids, {k: v.cpu().clone() for k, v in ctx.buffer.data.transition_data.items()}, ctx.buffer.priority_table.cpu().clone(),
                         [p.detach().cpu().clone() for p in ctx.mac.parameters()], ctx.buffer._sample_calls))
        finally:
            ops.set_strict(False)
            ctx.runner.close_env()
    (ids_a, data_a, tab_a, par_a, calls_a), (ids_b, data_b, tab_b, par_b, calls_b) = runs
    assert len(ids_a) == 8 and ids_a == ids_b and calls_a == calls_b and th.equal(tab_a, tab_b) and bool((tab_a != 0).any())
    assert set(data_a) == set(data_b)
    for k in data_a:
        assert th.equal(data_a[k], data_b[k]), k
    assert all(th.equal(a, b) for a, b in zip(par_a, par_b)) and len(par_a) > 0
