"""Shared by tests/test_weights_in_motion_host.py / _gpu.py: the derived copies of the weights while training moves them.

  * controller64: a float64 stepwise controller over a stored episode, teacher-forced with the stored actions -- the reference every
    rollout of the GPU tests is held to, with the weights that rollout was played with.  The loop is written here (not the library's
    unroll): the learner's time-batched path assembles its inputs in f32.
  * the reference trajectory across target syncs (tests/golden/learner_target_sync.npz, oracle/gen_target_sync_golden.py): bars and
    the comparison of one train call.
  * the target net's caches against fresh concatenations of the live parameters.
"""
import copy
from types import SimpleNamespace

import numpy as np
import torch as th
import torch.nn.functional as F

from tests.learner_util import param_checksums

LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")
LOSS_TOL, HEAD_TOL, SQ_TOL = 1e-5, 2e-5, 1e-5        # tests/test_learner_parity.py: the two-step bars
SENS_FACTOR = 8                                       # this package's summation order on top of the reference's input-rounding sensitivity
STATE_TOL = 1e-5                                      # tests/test_stored_state_gpu.py: stored state against the unroll
TOL_Q = 1e-5                                          # tests/test_policy_instantiations.py / DESIGN section 2 "Bars"
EXCLUDED_CAP = 0.01                                   # share of rows within 4 TOL_Q of a tie (tests/test_policy_instantiations.py:241)
# The same cap for a whole greedy rollout.  Its rows are not independent: every env is reset to the same state and plays the same
# greedy actions, so the envs stay copies of each other until the env's own draws reach an agent's window, and ONE near-tie of one
# agent at one slot takes all N envs at once -- 1 / ((T + 1) n) = 1 / 65 = 1.54 % of the rows at 13 slots x 5 agents, above 1 % by
# itself.  With gaps between the top two of the order 1e-2 a cell lies within 4 TOL_Q of a tie with probability ~1e-3: one such cell in
# 65 happens in ~6 % of the runs, four in none.  Cap: three cells = 4.6 % -> 5 %.  Measured on the device: 0.0154 (pipelined: slot 6,
# agent 4, all 32 envs) and 0.0000 (four_launch) for the env head, 0.0000 for the incentive head.
ROLLOUT_EXCLUDED_CAP = 0.05


# ---- float64 controller ------------------------------------------------------------------------------------------------------------
def agent64(mac):
    """a float64 deep copy of the controller's network on the host (tests/test_policy_instantiations.py:226)"""
    return copy.deepcopy(mac.agent).double().cpu()


def host_controller(mac, scheme):
    """a controller of the same configuration on the host, for its input assembly only (its own network is never evaluated);
    the global generator is left where it was"""
    args = SimpleNamespace(**dict(vars(mac.args), device="cpu", use_cuda=False))
    with th.random.fork_rng(devices=[]):
        return type(mac)(scheme, {"agents": mac.n_agents}, args)


def episode_fields(data):
    """the fields of a stored episode batch the controller and the learner's unroll read, on the host"""
    keys = ("obs", "actions", "actions_inc", "reward", "clean_num", "apple_den", "agent_pos", "agent_orientation")
    return {k: data[k].detach().cpu().clone() for k in keys}


def controller64(host_mac, net, ep):
    """q_env [B, T, n, A], q_inc [B, T, n, n, 3], h_env / h_inc [B, T, n, H] of the float64 network `net` over the stored episode `ep`
    (episode_fields) from zero state: per slot the encoder and forward_env / forward_inc in float64 on inputs assembled by
    host_mac.assemble_inputs from the STORED previous actions / reward / incentive actions (the tail columns are one-hots, signs and
    f32 positions: taken as the controller builds them), the inc head on the stored env action and the stored pose / reward / clean /
    density of the slot (homophily_agent.py:194-201)."""
    a = host_mac.args
    obs = ep["obs"]
    if obs.dtype == th.uint8:
        obs = host_mac.expand_codes(obs)
    B, T, n = obs.shape[:3]
    A, H, F0 = a.n_actions, a.rnn_hidden_dim, a.obs_dim_net
    acts, inc = ep["actions"].squeeze(-1), ep["actions_inc"].squeeze(-1)
    h_env = th.zeros(B, n, 1, H, dtype=th.float64)
    h_inc = th.zeros(B, n, 1, H, dtype=th.float64)
    out = ([], [], [], [])
    with th.no_grad():
        for t in range(T):
            feat = net.conv_to_fc(obs[:, t].reshape(B * n, 3, a.obs_dims[0], a.obs_dims[1]).double())
            blank = th.zeros(B * n, F0)
            if t == 0:
                rows = host_mac.assemble_inputs(blank, None, None, None, ep["agent_pos"][:, 0], True)
            else:
                rows = host_mac.assemble_inputs(blank, acts[:, t - 1], ep["reward"][:, t - 1], inc[:, t - 1], ep["agent_pos"][:, t], False)
            assert rows.shape == (B * n, host_mac.input_shape) and not rows[:, :F0].any()
            x = th.cat([feat, rows[:, F0:].double()], dim=1)
            q_env, h_env, _ = net.forward_env(x, h_env)
            q_inc, h_inc, _ = net.forward_inc(x, h_inc, F.one_hot(acts[:, t], A), ep["agent_pos"][:, t].double() / host_mac.pos_scale,
                                              ep["agent_orientation"][:, t].double(), ep["reward"][:, t].double().unsqueeze(-1),
                                              ep["clean_num"][:, t].double().unsqueeze(-1), ep["apple_den"][:, t].double().unsqueeze(-1))
            for dst, v in zip(out, (q_env.reshape(B, n, A), q_inc.reshape(B, n, n, -1), h_env.squeeze(2), h_inc.squeeze(2))):
                dst.append(v.clone())
    return tuple(th.stack(v, dim=1) for v in out)


def state_error(hidden, h_env, h_inc):
    """max |stored state - float64 state| over every slot: hidden [B, T, n, 2H] as the rollout files it (env head first)"""
    H = h_env.shape[-1]
    hidden = hidden.detach().cpu().double()
    return max(float((hidden[..., :H] - h_env).abs().max()), float((hidden[..., H:] - h_inc).abs().max()))


def greedy_rows(q_env, q_inc, avail):
    """(greedy env actions, rows whose top two available values are more than 4 TOL_Q apart, greedy incentive actions, the same for
    them, the off-diagonal mask) of float64 Q-values; avail [A] (one mask for every row, as the env has it)"""
    masked = q_env.masked_fill(avail.reshape(-1).cpu() == 0, -float("inf"))
    top = masked.topk(2, dim=-1).values
    t2 = q_inc.topk(2, dim=-1).values
    n = q_inc.shape[-2]
    off = ~th.eye(n, dtype=th.bool).expand(q_inc.shape[:-1])
    return masked.argmax(-1), (top[..., 0] - top[..., 1]) > 4 * TOL_Q, q_inc.argmax(-1), (t2[..., 0] - t2[..., 1]) > 4 * TOL_Q, off


def excluded_share(clear, clear_i, off):
    """share of (env rows, off-diagonal incentive rows) left out of the greedy comparison"""
    return 1.0 - float(clear.float().mean()), 1.0 - float(clear_i[off].float().mean())


# ---- the trajectory across target syncs -------------------------------------------------------------------------------------------
def bars(z, k):
    """the bars of train call k (1-based): max(the two-step bar, 8 x the sensitivity the fixture recorded for that call), per log key
    and for param_head / param_sq (relative)"""
    logs = {key: max(LOSS_TOL, SENS_FACTOR * float(z["sens%d_%s" % (k, key)])) for key in LOG_KEYS}
    return logs, max(HEAD_TOL, SENS_FACTOR * float(z["sens%d_param_head" % k])), max(SQ_TOL, SENS_FACTOR * float(z["sens%d_param_sq_rel" % k]))


def call_errors(z, k, logs, mac):
    """|this call's logs and parameter checksums - the reference's| in units of their bars: {name: (error, bar)}"""
    log_bars, head_bar, sq_bar = bars(z, k)
    out = {key: (abs(float(logs[key]) - float(z["call%d_%s" % (k, key)])), log_bars[key]) for key in LOG_KEYS}
    _, sqs, heads = param_checksums(mac)
    ref_sq = z["call%d_param_sq" % k]
    out["param_head"] = (float(np.abs(heads - z["call%d_param_head" % k]).max()), head_bar)
    out["param_sq"] = (float(np.abs(sqs - ref_sq).max() / np.abs(ref_sq).max()), sq_bar)
    return out


def worst(errors):
    """(name, error / bar) of the entry furthest along its bar"""
    name = max(errors, key=lambda key: errors[key][0] / errors[key][1])
    return name, errors[name][0] / errors[name][1]


def suppress_sync(learner):
    """the learner with its target sync replaced by a no-op (the power arm): the schedule still counts, nothing is copied"""
    learner._update_targets = lambda: None
    return learner


# ---- the target net's caches -------------------------------------------------------------------------------------------------------
def cache_tensors(agent):
    """the target net's derived buffers in a fixed order: the eight GRU images, the four merged dueling layers"""
    assert agent._gru_cache is not None and agent._fc2_cache is not None
    return [t for h in ("env", "inc") for t in agent._gru_cache[h]] + list(agent._fc2_cache)


def fresh_concatenations(agent):
    """what the caches must hold: th.cat of the net's parameters as they are now (no cache, no cat_groups launch)"""
    w, b = agent._w, agent._b
    with th.no_grad():
        fc2 = [th.cat([w("fc2_env_w"), w("fc2_env_v_w")], dim=2), th.cat([b("fc2_env_b"), b("fc2_env_v_b")], dim=2),
               th.cat([w("fc2_inc_w"), w("fc2_inc_v_w")], dim=2), th.cat([b("fc2_inc_b"), b("fc2_inc_v_b")], dim=2)]
        return [t for h in ("env", "inc") for t in agent._gru_weights_cat(h)] + fc2


def assert_caches_follow(target_agent, live_agent, ptrs, where):
    """the target net's caches equal the concatenations of the LIVE net's parameters bit for bit, at the addresses `ptrs`"""
    got, want = cache_tensors(target_agent), fresh_concatenations(live_agent)
    assert [t.data_ptr() for t in got] == ptrs, where
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and th.equal(x, y), (where, i)
