"""CPU suite of prioritised replay's initial priorities (config key per_initial_priority: "rollout"; ssd_rollout_priority): the
export's declaration as compiled, every refusal of the export, the setup refusals of the key, the
insert with priorities (wrap-around split, None = zeroing) on a host buffer, the operator's refusals, and the numpy restatement
(tests/rollout_priority_util.py) pinned to the CPU tensor-op learner independently of the kernel."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops, run
from homophily_marl_amd.components.episode_buffer import ReplayBuffer
from tests import rollout_priority_util as U
from tests.learner_util import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ssd_rollout_priority"


# ---- 1. the export ------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_exported_and_mirrored():
    """declaration, export and argtypes of every name of the table: tests/test_abi_symbols.py"""
    assert NAME in abi.HIP_SIGNATURES
    assert abi.load_library().ssd_abi_version() == abi.ABI_VERSION            # one export more, no version change


def test_struct_size_and_declaration_as_compiled(tmp_path):
    """the declaration is usable from C (sizeof / offsetof: tests/test_abi_symbols.py)"""
    c = tmp_path / "s.c"
    c.write_text('#include "ssd_hip.h"\nint main(){\nint (*f)(const ssd_rollout_priority_args*, void*) = ssd_rollout_priority;\nreturn f == 0;}')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "s.o")])


P = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched (the checks run before any launch)
POINTERS = ("t_index", "q_env", "q_inc", "actions", "actions_inc", "reward", "terminated", "filled", "carry", "acc", "q_init")


def _args(**over):
    a = abi.SsdRolloutPriorityArgs()
    for k in POINTERS:
        setattr(a, k, P)
    a.n_env, a.n_agents, a.n_actions, a.t_slots, a.avail_bits = 3, 5, 9, 8, 0x1FF
    a.q_env_agent_stride, a.q_env_env_stride, a.q_inc_agent_stride, a.q_inc_env_stride = 27, 9, 45, 15
    for k, v in dict(U.DYADIC, alpha=0.6, eta=0.9, eps=1e-3).items():
        setattr(a, k, v)
    for k, v in over.items():
        setattr(a, k, v)
    return a


NAN = float("nan")
REFUSALS = ([{k: None} for k in POINTERS if k != "filled"]
            + [dict(n_env=0), dict(n_env=-1), dict(t_slots=1), dict(t_slots=0), dict(n_agents=1), dict(n_agents=11), dict(n_actions=0), dict(n_actions=17),
               dict(avail_bits=0), dict(avail_bits=0xFFFFFE00), dict(n_actions=1, avail_bits=2),
               dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=NAN), dict(eta=-0.1), dict(eta=1.01), dict(eta=NAN),
               dict(eps=0.0), dict(eps=-1.0), dict(eps=NAN), dict(seq_len=0.0), dict(seq_len=-8.0), dict(seq_len=NAN),
               dict(reward_scale=0.0), dict(reward_scale=-1.0), dict(reward_scale=NAN),
               dict(q_env_agent_stride=-27), dict(q_env_env_stride=-9), dict(q_inc_agent_stride=-45), dict(q_inc_env_stride=-1)]
            + [{k: P + 2} for k in ("q_env", "q_inc", "reward", "carry", "acc", "q_init")]
            + [{k: P + 4} for k in ("t_index", "actions", "actions_inc", "filled")])


def test_invalid_launches_are_refused_with_a_message_that_names_the_function():
    lib = abi.load_library()
    INV = abi.SSD_ERR_INVALID
    assert lib.ssd_rollout_priority(None, None) == INV and NAME.encode() in lib.ssd_last_error()
    for kw in REFUSALS:
        lib.ssd_priority_sample(None, None)                                   # another name in ssd_last_error before every case
        assert lib.ssd_rollout_priority(C.byref(_args(**kw)), None) == INV, kw
        assert NAME.encode() in lib.ssd_last_error(), (kw, lib.ssd_last_error())


def test_operator_refuses_tensors_that_do_not_qualify_and_names_them():
    N, T1, n, A = 3, 5, 4, 9
    st = dict(reward=th.zeros(N, T1, n), actions=th.zeros(N, T1, n, 1, dtype=th.long), actions_inc=th.zeros(N, T1, n, n, 1, dtype=th.long),
              terminated=th.zeros(N, T1, 1, dtype=th.uint8), filled=th.ones(N, T1, 1, dtype=th.long))
    with pytest.raises(ValueError, match=r"rollout_priority: reward \(3, 5, 4\)"):       # host tensors: no launch
        ops.rollout_priority_args(th.zeros(1, dtype=th.long), th.zeros(n, N, A), th.zeros(n, N, n, 3), True, 0x1FF, st, U.DYADIC, 0.6, 0.9, 1e-3)
    with pytest.raises(ValueError, match="copy_blocks"):
        ops.copy_blocks([(th.zeros(4, dtype=th.int32), th.zeros(4, dtype=th.int32))])
    with pytest.raises(ValueError, match="copy_blocks"):
        ops.copy_blocks([])
    # the constants come from one helper: what the loss launch is given is what the rollout is given
    a = SimpleNamespace(gamma_env=0.95, gamma_inc=0.995, reward_scale=2.0, incentive_ratio=1.0, incentive_cost=0.1, incentive=3)
    c = ops.td_constants(a, 101)
    assert set(c) == set(U.CONSTANTS) and c["seq_len"] == 101.0 and c["incentive"] == 3.0 and all(isinstance(v, float) for v in c.values())
    assert ops.window_reward_norm("episode", 101, 20) == 101.0 and ops.window_reward_norm("window", 101, 20) == 21.0
    assert ops.window_reward_norm("window", 101, 0) == 101.0


# ---- 2. setup ----------------------------------------------------------------------------------------------------------------------------
class _Buffer:
    def __init__(self, device):
        self.device, self.enabled = device, 0

    def enable_priorities(self):
        self.enabled += 1


BASE = dict(runner="hip_graph", prioritized_replay=True, per_initial_priority="rollout", batch_size=16, fused_loss=True)
RUNNER = SimpleNamespace(fixed_length_episodes=True)


@pytest.mark.parametrize("keys,device,match", [(dict(prioritized_replay=False), "cuda:0", "needs prioritized_replay"),
                                               (dict(runner="hip_vec"), "cuda:0", "needs runner hip_graph"),
                                               (dict(runner="episode"), "cuda:0", "needs runner hip_graph"),
                                               ({}, "cpu", "device-resident replay buffer"),
                                               (dict(per_initial_priority="td"), "cuda:0", 'must be "max" or "rollout"'),
                                               (dict(per_initial_priority=None), "cuda:0", 'must be "max" or "rollout"'),
                                               (dict(per_initial_priority=True), "cuda:0", 'must be "max" or "rollout"')])
def test_setup_refuses_the_key_where_it_cannot_work(keys, device, match):
    buf = _Buffer(device)
    with pytest.raises(ValueError, match="per_initial_priority.*" + match):
        run._check_prioritized(SimpleNamespace(**dict(BASE, **keys)), buf, RUNNER)
    assert buf.enabled == 0


def test_key_defaults_to_max_and_is_written_back():
    assert run.load_config("cleanup")["per_initial_priority"] == "max"
    a = SimpleNamespace(runner="hip_vec", batch_size=16)
    assert run._check_prioritized(a, _Buffer("cpu"), RUNNER) is False and a.per_initial_priority == "max"
    a = SimpleNamespace(**BASE)
    buf = _Buffer("cuda:0")
    assert run._check_prioritized(a, buf, RUNNER) is True and a.per_initial_priority == "rollout" and buf.enabled == 1
    a = SimpleNamespace(**dict(BASE, per_initial_priority="max", runner="hip_vec"))          # "max" asks nothing of the runner
    assert run._check_prioritized(a, _Buffer("cuda:0"), RUNNER) is True


# ---- 3. insert with priorities ---------------------------------------------------------------------------------------------------------
def _buffer(size):
    scheme = {"reward": {"vshape": (2,)}, "terminated": {"vshape": (1,), "dtype": th.uint8}}
    buf = ReplayBuffer(scheme, {}, size, 3, device="cpu")
    buf.enable_priorities()
    return buf, scheme


def _episodes(scheme, n, first):
    from homophily_marl_amd.components.episode_buffer import EpisodeBatch
    b = EpisodeBatch(scheme, {}, n, 3, device="cpu")
    b.update({"reward": th.arange(first, first + n, dtype=th.float32).reshape(n, 1, 1).expand(n, 3, 2)})
    return b


def test_insert_with_priorities_splits_them_on_wrap_around_and_none_zeroes():
    buf, scheme = _buffer(5)
    buf.priority_table.fill_(7)
    buf.insert_episode_batch(_episodes(scheme, 3, 10), priorities=th.tensor([11, 12, 13], dtype=th.int32))
    assert buf.priority_table.tolist() == [11, 12, 13, 7, 7] and buf.buffer_index == 3
    calls = []
    write = buf._write_priorities
    buf._write_priorities = lambda start, pr: (calls.append((start, pr.tolist())), write(start, pr))
    buf.insert_episode_batch(_episodes(scheme, 4, 20), priorities=th.tensor([21, 22, 23, 24], dtype=th.int32))        # wraps after two
    assert calls == [(3, [21, 22]), (0, [23, 24])]                                 # one write per contiguous run of slots
    assert buf.priority_table.tolist() == [23, 24, 13, 21, 22] and buf.buffer_index == 2 and buf.episodes_in_buffer == 5
    assert buf["reward"][:, 0, 0].tolist() == [22.0, 23.0, 12.0, 20.0, 21.0]       # the priorities travel with their episodes
    buf.insert_episode_batch(_episodes(scheme, 2, 30))                             # None: today's zeroing
    assert buf.priority_table.tolist() == [23, 24, 0, 0, 22]
    buf.insert_episode_batch(_episodes(scheme, 2, 40), priorities=None)
    assert buf.priority_table.tolist() == [0, 24, 0, 0, 0]
    for bad in (th.tensor([1, 2, 3], dtype=th.int32), th.tensor([1, 2], dtype=th.int64), th.tensor([[1, 2]], dtype=th.int32)):
        with pytest.raises(ValueError, match="insert_episode_batch: priorities"):
            buf.insert_episode_batch(_episodes(scheme, 2, 50), priorities=bad)
    plain = ReplayBuffer(scheme, {}, 4, 3, device="cpu")
    with pytest.raises(ValueError, match="enable_priorities"):
        plain.insert_episode_batch(_episodes(scheme, 2, 0), priorities=th.tensor([1, 2], dtype=th.int32))


# ---- 4. the restatement against the CPU tensor-op learner -----------------------------------------------------------------------------
class _Fixture(dict):
    files = property(lambda self: list(self))


def test_restatement_agrees_with_the_cpu_learner_rows():
    """4 random episodes, n = 3, T = 6, q = tq: the tensor-op learner (homophily_learner.py, the reference path) evaluated in float64 on
    given Q-values.  Its per-row errors are read off its own loss: with sim_loss_weight 0 and dens = (1, 0) the loss is
    sum (td_env mask)^2 + sum (td_inc mask)^2, so dL/dq_env[t, i, a_t] = 2 td_env mask^2 and dL/dq_inc[t, i, j, a_inc_ij] = 2 td_inc mask^2 for
    every j != i; the mask is the learner's _td_mask.  Rewards are integers and the constants dyadic, so the learner's f32 reward
    arithmetic is exact and everything else runs in float64: p must agree within 1e-12 relative."""
    B, T, n, A, V = 4, 6, 3, 9, 7
    ep = U.episodes(B, T, n, A, seed=11, exact=False)
    ep["filled"][:] = 1                                                       # (the fixture builder marks every slot filled)
    rng = np.random.default_rng(5)
    ep["reward"] = rng.integers(-1, 4, (B, T + 1, n)).astype(np.float32)
    z = _Fixture(batch_obs=np.zeros((B, T + 1, n, 3, V, V), np.uint8), batch_actions=ep["actions"][..., None], batch_actions_inc=ep["actions_inc"][..., None],
                 batch_reward=ep["reward"], batch_terminated=ep["terminated"][..., None], batch_clean_num=np.zeros((B, T + 1, n), np.float32),
                 batch_apple_den=np.zeros((B, T + 1, n), np.float32), batch_agent_pos=np.zeros((B, T + 1, n, 2), np.float32),
                 batch_agent_orientation=np.zeros((B, T + 1, n, 2), np.float32), batch_avail_actions=np.ones((B, T + 1, n, A), np.int32),
                 batch_filled=np.ones((B, T + 1, 1), np.int64))
    z["batch_avail_actions"][..., 7:] = 0                                     # two actions are not available
    meta = dict(env="cleanup", env_args=dict(num_agents=n, episode_limit=T, view_size=3, map="default3"))
    c = dict(U.DYADIC)
    over = dict(gamma_env=c["gamma_env"], gamma_inc=c["gamma_inc"], reward_scale=c["reward_scale"], incentive_ratio=c["incentive_ratio"],
                incentive_cost=c["incentive_cost"], incentive=c["incentive"], sim_loss_weight=0.0, consider_others_inc=False, td_lambda=0.0,
                fused_loss=False)
    args, batch, mac, learner = build(z, meta, overrides=over)
    batch.reward_norm = c["seq_len"]
    for double_q in (True, False):
        args.double_q = double_q
        q_env = th.tensor(ep["q_env"], dtype=th.float64, requires_grad=True)
        q_inc = th.tensor(ep["q_inc"], dtype=th.float64, requires_grad=True)
        learner.unroll_pair = lambda b: (q_env, q_inc, q_env.detach(), q_inc.detach())
        learner._backward = lambda loss, seeds=None: loss.backward()
        learner._forward_backward_ops(batch, th.tensor([1.0, 0.0], dtype=th.float64))
        mask = learner._td_mask(batch).double().numpy()
        ge = th.gather(q_env.grad[:, :-1], -1, batch["actions"][:, :-1]).squeeze(-1).numpy()                  # 2 td_env mask^2
        gi = th.gather(q_inc.grad[:, :-1], -1, batch["actions_inc"][:, :-1]).squeeze(-1).numpy()              # [B, T, i, j]
        td_env_m, td_inc_m = ge / 2, gi[:, :, np.arange(n), (np.arange(n) + 1) % n] / 2                       # (any j != i carries td_inc)
        assert not q_env.grad[:, -1].any() and (mask.max() == 1.0) and (mask.min() == 0.0)
        ref = U.initial_priority(filled=ep["filled"], avail_bits=0x7F, c=c, alpha=0.6, eta=0.9, eps=1e-3,
                                 **{k: ep[k] for k in ("q_env", "q_inc", "actions", "actions_inc", "reward", "terminated")})
        assert np.array_equal(ref.mask, mask)
        p, _, q = U.aggregate(td_env_m, td_inc_m, mask, 0.6, 0.9, 1e-3)           # the errors already carry the mask (0 / 1)
        rel = np.abs(p - ref.p) / ref.p
        print("double_q %s: p %s, largest relative difference %.3e" % (double_q, np.round(ref.p, 4), rel.max()))
        assert rel.max() < 1e-12 and np.array_equal(q, ref.q)
        assert ref.p.min() > 1e-2                                                 # the errors are not trivially zero
