"""GPU suite: TD(lambda) targets in the fused loss kernel (k_td_lambda_loss behind ssd_td_sim_loss with td_lambda > 0) -- in the poisoned
arena against the float64 statement of tests/td_lambda_util.py, at a lambda too small to be seen against the one-step kernel, the
device learner against the tensor-op learner (eager and captured), and the reference's recorded returns through the kernel."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from tests import td_lambda_util as U
from tests.arena_util import Arena

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -100
LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")
f32 = lambda x: np.asarray(x, dtype=np.float32)
CFG = dict(gamma_env=0.99, gamma_inc=0.99, reward_scale=1.0, incentive_ratio=1.0, incentive_cost=0.5, incentive=2.0, sim_threshold=0.1,
           sim_loss_weight=0.1, sim_horizon=3)
_arrays = {}


def random_arrays(B, T, n):
    """the arrays of tests/test_learner_kernel_bounds.py::test_td_sim_loss_in_the_arena: early termination and unfilled tails, rewards
    of both signs, random availability; made once per shape and shared (never written)."""
    if (B, T, n) not in _arrays:
        rng = np.random.default_rng(1000 * B + 10 * T + n)
        T1, A = T + 1, 9
        arr = dict(q_env=f32(rng.standard_normal((B, T1, n, A))), tq_env=f32(rng.standard_normal((B, T1, n, A))),
                   q_inc=f32(rng.standard_normal((B, T1, n, n, 3))), tq_inc=f32(rng.standard_normal((B, T1, n, n, 3))))
        arr["avail"] = (rng.random((B, T1, n, A)) < 0.7).astype(np.int32); arr["avail"][..., 4] = 1
        arr["actions"] = rng.integers(0, A, (B, T1, n)).astype(np.int64)
        arr["actions_inc"] = (rng.integers(0, 3, (B, T1, n, n)) * (1 - np.eye(n, dtype=np.int64))).astype(np.int64)
        arr["reward"] = f32(rng.integers(-1, 3, (B, T1, n)) * (rng.random((B, T1, n)) < 0.3))
        arr["clean_num"] = f32(rng.integers(0, 3, (B, T1, n)) * (rng.random((B, T1, n)) < 0.3))
        term = np.zeros((B, T1), dtype=np.uint8)
        for b in range(B):
            if b != 1 and (B > 1 or T == 1):                             # episode 1, and a lone long episode, run to the end: G_T keeps
                term[b, max(0, T - 1 - (b % 3) * 2)] = 1                 # the bootstrap value
        arr["terminated"] = term
        arr["filled"] = np.ones((B, T1), dtype=np.int64)
        arr["filled"][:, 1:] = 1 - np.minimum(1, np.cumsum(term, 1)[:, :-1])
        for v in arr.values():
            v.setflags(write=False)
        _arrays[(B, T, n)] = arr
    return _arrays[(B, T, n)]


def launch_in_arena(arr, double_q, others, lam, dens):
    """mode 1 with every operand in the arena; returns (partials [B, T, n, 16], dq_env, dq_inc) after Arena.check()."""
    B, T1, n, A = arr["q_env"].shape
    T = T1 - 1
    ar = Arena()
    a = abi.SsdTdLossArgs(batch=B, t_slots=T1, n_agents=n, n_actions=A, double_q=double_q, consider_others_inc=others, seq_len=float(T1),
                          td_lambda=lam, **CFG)
    P = ar.place
    regs = dict(q_env=P("q_env", arr["q_env"], offset_in_16=4), q_inc=P("q_inc", arr["q_inc"], offset_in_16=8), tq_env=P("tq_env", arr["tq_env"], offset_in_16=12),
                tq_inc=P("tq_inc", arr["tq_inc"], offset_in_16=4), actions=P("actions", arr["actions"], align=8, fill=A),
                actions_inc=P("actions_inc", arr["actions_inc"], align=8, fill=3), avail=P("avail", arr["avail"], fill=0),
                reward=P("reward", arr["reward"], offset_in_16=8), clean_num=P("clean_num", arr["clean_num"], offset_in_16=12),
                terminated=P("terminated", arr["terminated"], align=1, fill=1), filled=P("filled", arr["filled"], align=8, fill=0),
                dens=P("dens", f32(dens), offset_in_16=4))
    wp = np.zeros((B * T * n, abi.TD_LOSS_PARTIALS), dtype=bool)
    wp[:, :15 if lam > 0 else 13] = True                                 # 13 / 14: the rows' lambda-returns; 15 is never written
    regs["partials"] = ar.reserve("partials", wp.shape, offset_in_16=8, written=wp)
    regs["dq_env"] = ar.reserve("dq_env", arr["q_env"].shape, offset_in_16=12, written=True)
    regs["dq_inc"] = ar.reserve("dq_inc", arr["q_inc"].shape, offset_in_16=4, written=True)
    for k, r in regs.items():
        setattr(a, k, r.ptr)
    lib = abi.load_library()
    abi.check(lib, lib.ssd_td_sim_loss(C.byref(a), 1, None))
    ar.check()                                                           # bands, inputs untouched, written sets, no NaN
    return regs["partials"].array().reshape(B, T, n, abi.TD_LOSS_PARTIALS), regs["dq_env"].array(), regs["dq_inc"].array()


def _dens(arr):
    T = arr["q_env"].shape[1] - 1
    p_mask = arr["filled"][:, :T].astype(np.float64)
    p_mask[:, 1:] *= 1 - arr["terminated"][:, :T - 1]
    return [max(1.0, float(p_mask.sum() * arr["q_env"].shape[2])), 3.0]


SHAPES = [(1, 1, 2), (3, 9, 2), (2, 63, 3), (2, 64, 3), (3, 65, 5), (2, 255, 2), (1, 256, 3), (2, 257, 5), (1, 513, 2), (5, 23, 10)]
ARENA_CASES = [(s, dq, oth) for s in SHAPES[:3] for dq, oth in ((1, 0), (0, 0), (1, 1), (0, 1))] + [(s, 1, 0) for s in SHAPES[3:]] + [((2, 257, 5), 0, 1)]


@pytest.mark.parametrize("lam", [0.5, 1.0])
@pytest.mark.parametrize("shape,double_q,others", ARENA_CASES, ids=["%dx%dx%d-dq%d-oth%d" % (s + (d, o)) for s, d, o in ARENA_CASES])
def test_lambda_kernel_in_the_arena(shape, double_q, others, lam):
    """Bands and inputs untouched, every dq element written, partial columns 0 .. 14 written and 15 kept; the lambda-returns (columns
    13 / 14) and the squared errors within 1e-5 max(1, |ref|), the gradient within 2e-6 max(1, max |g|) of the float64 statement
    (tests/test_hip_learner_path.py:245,254), whose gamma is the f32 value the kernel is handed."""
    arr = random_arrays(*shape)
    dens = _dens(arr)
    part, dq_env, dq_inc = launch_in_arena(arr, double_q, others, lam, dens)
    cfg = dict(CFG, double_q=double_q, consider_others_inc=others, seq_len=float(shape[1] + 1),
               gamma_env=float(np.float32(CFG["gamma_env"])), gamma_inc=float(np.float32(CFG["gamma_inc"])),
               sim_threshold=float(np.float32(CFG["sim_threshold"])), sim_loss_weight=float(np.float32(CFG["sim_loss_weight"])))
    ref = U.host_loss(arr, cfg, lam, dens)
    for col, key in ((13, "G_env"), (14, "G_inc"), (2, "sq_env"), (3, "sq_inc")):
        err = np.abs(part[..., col] - ref[key])
        print(key, "max err %.3e, max |ref| %.3e" % (err.max(), np.abs(ref[key]).max()))
        assert (err <= 1e-5 * np.maximum(1.0, np.abs(ref[key]))).all(), (key, float(err.max()))
    T = shape[1]
    assert not dq_env[:, T].any() and not dq_inc[:, T].any()                                  # the bootstrap slot: zeros
    for got, key in ((dq_env, "dq_env"), (dq_inc, "dq_inc")):
        err, top = float(np.abs(got - ref[key]).max()), float(np.abs(ref[key]).max())
        print(key, "max err %.3e, max |g| %.3e" % (err, top))
        assert top > 0 and err < 2e-6 * max(1.0, top), (key, err, top)


@pytest.mark.parametrize("shape", [(3, 65, 5), (2, 257, 5)])
def test_a_lambda_too_small_to_see_is_the_one_step_kernel(shape):
    """td_lambda = 2^-100 (lambda gamma squared underflows: a row sees b_t and 7e-31 of the row behind) against td_lambda = 0, the
    one-step kernel, on the same arrays: dq_env, dq_inc and the partial columns 0 .. 12 come out equal element for element on the
    MI355X (the rows' expressions are the one-step kernel's and the library is built without contraction), so that is what is
    asserted -- stricter than the 1e-6 relative the option's specification asks for."""
    arr = random_arrays(*shape)
    dens = _dens(arr)
    p0, e0, i0 = launch_in_arena(arr, 1, 0, 0.0, dens)
    p1, e1, i1 = launch_in_arena(arr, 1, 0, TINY, dens)
    for name, x, y in (("dq_env", e0, e1), ("dq_inc", i0, i1), ("partials[:, :13]", p0[..., :13], p1[..., :13])):
        assert np.array_equal(x, y), (name, float(np.abs(x.astype(np.float64) - y).max()))
    mask = p1[..., 0]
    if (mask == 0).any():
        assert np.abs(p1[..., 13][mask == 0]).max() < 1e-20              # an unfilled row's return is only what leaks from behind it


def _device_partials(batch, args, learner):
    """one mode-1 launch on the device learner's own Q-values: (partials [B, T, n, 16], dens)"""
    from homophily_marl_amd import ops
    with th.no_grad():
        q_env, q_inc, tq_env, tq_inc = (x.contiguous() for x in learner.unroll_pair(batch))
    dens = learner.denominators(batch).contiguous().float()
    B, T, n = batch.batch_size, batch.max_seq_length - 1, args.n_agents
    partials = th.zeros(B * T * n, abi.TD_LOSS_PARTIALS, device=q_env.device)
    dq_env, dq_inc = th.empty_like(q_env), th.empty_like(q_inc)
    t, keep = ops._td_loss_args(batch, args, args.n_actions, partials)
    t.q_env, t.q_inc, t.tq_env, t.tq_inc = q_env.data_ptr(), q_inc.data_ptr(), tq_env.data_ptr(), tq_inc.data_ptr()
    t.dens, t.dq_env, t.dq_inc = dens.data_ptr(), dq_env.data_ptr(), dq_inc.data_ptr()
    lib = abi.load_library()
    abi.check(lib, lib.ssd_td_sim_loss(C.byref(t), 1, th.cuda.current_stream().cuda_stream))
    th.cuda.synchronize()
    return partials.reshape(B, T, n, -1).cpu().numpy(), dens.cpu().numpy()


Z, META = U.load_golden()


@pytest.mark.parametrize("name", [c["name"] for c in META["b_cases"]])
def test_kernel_reproduces_the_reference_returns(name):
    """Group (B) of the fixture through the kernel: the device learner's Q-values under the case's flags, the rows' lambda-returns
    (partial columns 13 / 14) and both value losses against what the reference's build_td_lambda_targets recorded, at 1e-5."""
    from tests.learner_util import build, load_fixture
    from tests.test_learner_options import perturb_target
    th.backends.cuda.matmul.allow_tf32 = False
    c = next(c for c in META["b_cases"] if c["name"] == name)
    z, meta = load_fixture(c["base"])
    for li, lam in enumerate(META["b_lambdas"]):
        args, batch, mac, learner = build(z, meta, device="cuda:0", overrides=dict(c["overrides"], td_lambda=lam))
        assert learner._fused(batch)
        perturb_target(learner)
        part, dens = _device_partials(batch, args, learner)
        for col, h in ((13, "env"), (14, "inc")):
            ref = Z["B/%s/l%d/ret_%s" % (name, li, h)]
            err = np.abs(part[..., col] - ref)
            assert (err <= 1e-5 * np.maximum(1.0, np.abs(ref))).all(), (lam, h, float(err.max()))
            loss, ref_loss = part[..., col - 11].astype(np.float64).sum() / dens[0], float(Z["B/%s/l%d/loss_value_%s" % (name, li, h)])
            assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (lam, h, loss, ref_loss)


@pytest.mark.parametrize("train_graph", [False, True])
@pytest.mark.parametrize("base", ["learner_cleanup5.npz", "learner_harvest5.npz"])
def test_device_learner_matches_the_tensor_op_learner(base, train_graph, monkeypatch):
    """td_lambda = 0.8, two optimisation steps: the device learner (every operator on the HIP kernels: strict_device_ops) against the
    tensor-op learner on CPU tensors -- every logged value and the per-parameter checksums within 1e-5; eagerly and as the captured
    step (checked against an eager evaluation at every replay, six replays in all)."""
    from homophily_marl_amd import ops
    from tests.learner_util import build, load_fixture, param_checksums
    from tests.test_learner_options import perturb_target
    th.backends.cuda.matmul.allow_tf32 = False
    monkeypatch.setenv("SSD_GRAPH_CHECK", "1")
    z, meta = load_fixture(base)
    want = []
    args, batch, mac, learner = build(z, meta, overrides=dict(td_lambda=0.8))
    perturb_target(learner)
    for step in range(2):
        logs = learner.cal_loss_and_step(batch)
        want.append(({k: float(logs[k]) for k in LOG_KEYS}, param_checksums(mac)))
    args, batch, mac, learner = build(z, meta, device="cuda:0", overrides=dict(td_lambda=0.8, train_graph=train_graph), code_obs=True)
    ops.set_strict(True)
    try:
        assert learner._fused(batch) and learner.use_graph == train_graph
        if train_graph:
            # past the capture (third call) on a scratch copy of the weights, then rewind weights, target net and optimiser state
            sd0 = {k: v.clone() for k, v in mac.agent.state_dict().items()}
            for _ in range(3):
                learner.train(batch, 0, 0)
            assert learner._graph is not None
            mac.agent.load_state_dict(sd0)
            learner.target_mac.load_state(mac)
            for opt in (learner.optimiser_env, learner.optimiser_inc):
                for st in opt.state.values():
                    st["step"].zero_(); st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
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
        if train_graph:
            for _ in range(3):                                           # replays 4 .. 6, each checked against eager by SSD_GRAPH_CHECK
                learner.train(batch, 0, 0)
            assert learner._graph is not None and learner._check_n == 6
            assert all(bool(th.isfinite(p).all()) for p in mac.parameters())
    finally:
        ops.set_strict(False)
