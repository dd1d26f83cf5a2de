"""GPU suite of obs_others_last_action on the fused rollout heads (k_head GEN = 2: fc1 row gather; config key
fused_others_last_action).  Bars: TOL_Q = 1e-5 (DESIGN section 2 "Bars") for precision 2; for precision 1 the bf16 variant's bars of
test_policy_mfma.py::test_bf16_variant_is_close_to_fp32_and_labelled (1e-6 < max |dq| < 5e-2 against the f32-equivalent heads).
The argument refusals run without a device and live in test_others_last_action_host.py."""
import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

from homophily_marl_amd import abi

pytestmark = pytest.mark.gpu
TOL_Q = 1e-5

OTHERS = dict(obs_others_last_action=True, fused_others_last_action=True)
FLAG_SETS = {
    "shipped_others": dict(OTHERS),
    "all_seven": dict(OTHERS, obs_distance=True),
    "no_act_no_id": dict(OTHERS, obs_last_action=False, obs_agent_id=False),
}
SHAPES = [("cleanup", 5, 203, "shipped_others"), ("cleanup", 5, 203, "all_seven"), ("cleanup", 5, 203, "no_act_no_id"),
          ("harvest", 5, 64, "shipped_others"), ("harvest", 5, 64, "all_seven"), ("cleanup", 10, 64, "shipped_others"),
          ("cleanup", 10, 4112, "shipped_others")]


def _ctx(kind, n, N, seed=3, **over):
    from homophily_marl_amd.run import load_config, setup
    cfg = load_config(kind, overrides=dict(dict(runner="hip_vec", batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False,
                                                store_state=False,
                                                env_args=dict(num_agents=n, map="default10" if (kind == "harvest" or n == 10) else "default5",
                                                              episode_limit=20, seed=seed, view_size=7),
                                                use_cuda=True, save_model=False, runner_stats=False), **over))
    return setup(cfg)


def _dense_columns(mac):
    """columns of the controller's input row that are NOT the others' last-action block (what `inputs` holds, compacted)"""
    a, n, A = mac.args, mac.n_agents, mac.args.n_actions
    off = 32 + A * bool(a.obs_last_action) + n * bool(a.obs_agent_id) + bool(a.obs_reward) + bool(a.obs_inc_reward)
    return th.tensor([c for c in range(mac.input_shape) if not off <= c < off + n * A], device="cuda")


@pytest.mark.parametrize("kind,n,N,flags", SHAPES)
def test_gather_heads_match_the_torch_controller(kind, n, N, flags):
    """Both heads against assemble_inputs -> forward_env / forward_inc, previous actions drawn from [-1, A) (-1: the row that adds
    nothing).  N = 203: ragged last tile; Harvest: A = 8; Cleanup-10 without distance: dense 55 + 9 = 64, the limit; N = 4112 at
    n = 10: the looped instantiations (asserted through the head plan).  Precision 1 against the f32-equivalent heads, and not equal
    to them."""
    from homophily_marl_amd.fast_policy import FastPolicy
    th.manual_seed(2)
    ctx = _ctx(kind, n, N, **FLAG_SETS[flags])
    mac, env = ctx.mac, ctx.runner.env
    A = mac.args.n_actions
    assert mac.input_flags is None and mac.rollout_input_flags & 64 and FastPolicy.supports(mac)
    if N == 4112:
        wg, waves, walks = abi.policy_head_plan(N, n, 2)          # the gathered heads' own plan: 7 compute waves
        assert waves == 7 and walks > 1 and wg * waves * walks >= (N + 15) // 16
    env.reset_batch()
    g = th.Generator(device="cuda").manual_seed(0)
    ok_actions = th.nonzero(env.avail_actions_batch[0, 0]).squeeze(-1).to(th.int32)
    for _ in range(5):
        env.step_batch(ok_actions[th.randint(0, ok_actions.numel(), (N, n), generator=g, device="cuda")].contiguous(), observe=False)
    o = env.observe_batch(out=env.native.obs_buffers(abi.OBS_F32, want_code=True))
    obs, pos, orient, codes = o["obs"].clone(), o["pos"].clone(), o["orient"].clone(), o["code"].clone()
    prev_a = th.randint(-1, A, (N, n), generator=g, device="cuda")
    prev_r = th.randint(-1, 2, (N, n), generator=g, device="cuda").float()
    prev_i = th.randint(0, 3, (N, n, n), generator=g, device="cuda")
    h0e = th.randn(N, n, 1, 64, generator=g, device="cuda") * 0.3
    h0i = th.randn(N, n, 1, 64, generator=g, device="cuda") * 0.3
    reward = th.randint(-1, 2, (N, n), generator=g, device="cuda").float()
    clean = th.randint(0, 3, (N, n), generator=g, device="cuda").float()
    den = th.rand(N, n, generator=g, device="cuda")
    eps, step = th.zeros((), device="cuda"), th.zeros(1, dtype=th.long, device="cuda")
    avail = env.avail_actions_batch[0, 0]
    with th.no_grad():
        inputs = mac.assemble_inputs(mac.encode_obs(obs), prev_a, prev_r, prev_i, pos, False)
        assert inputs.shape[1] == mac.input_shape
        q_env, h_env, _ = mac.agent.forward_env(inputs, h0e)
        act = q_env.masked_fill(avail.view(1, 1, -1) == 0, -float("inf")).argmax(-1)
        q_inc, h_inc, _ = mac.agent.forward_inc(inputs, h0i, F.one_hot(act, A), pos / mac.pos_scale, orient, reward.unsqueeze(-1),
                                                clean.unsqueeze(-1), den.unsqueeze(-1))
    res = {}
    for prec in (2, 1):
        fp = FastPolicy(mac, N, avail, seed=7, precision=prec)
        assert fp.fused and fp.fused_enc and fp.others and not fp.inc_encode
        qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
        fp.h_env.copy_(h0e.squeeze(2).transpose(0, 1)); fp.h_inc.copy_(h0i.squeeze(2).transpose(0, 1))
        fp.act_env(obs, prev_a, prev_r, prev_i, pos, eps, step, codes=codes, q_out=qe)
        fp.act_inc(act, pos, orient, reward, clean, den, eps, step, q_out=qi)
        th.cuda.synchronize()
        res[prec] = (qe.transpose(0, 1), fp.h_env.transpose(0, 1).clone(), qi.transpose(0, 1), fp.h_inc.transpose(0, 1).clone(), fp)
    qe, he, qi, hi, fp = res[2]
    dense = _dense_columns(mac)
    rows = fp.inputs.transpose(0, 1).reshape(N * n, -1)
    assert (rows[:, :dense.numel()] - inputs[:, dense]).abs().max() < 2e-6 and (rows[:, dense.numel():] == 0).all()
    d = [(qe - q_env).abs().max().item(), (he - h_env.squeeze(2)).abs().max().item(), (qi - q_inc).abs().max().item(),
         (hi - h_inc.squeeze(2)).abs().max().item()]
    print("%s n=%d N=%d %s: max |diff| vs torch f32: q_env %.2e h_env %.2e q_inc %.2e h_inc %.2e" % ((kind, n, N, flags) + tuple(d)))
    assert max(d) < TOL_Q, d
    b_env = (res[1][0] - qe).abs().max().item(); b_inc = (res[1][2] - qi).abs().max().item()
    print("bf16 vs f32-equivalent: q_env %.3e q_inc %.3e" % (b_env, b_inc))
    assert 1e-6 < b_env < 5e-2 and 1e-6 < b_inc < 5e-2
    assert b_env > TOL_Q or b_inc > TOL_Q                                       # the variant really ran
    env.close()


def test_two_consecutive_timesteps_hand_the_previous_actions_over():
    """env head -> inc head -> env head -> inc head at N = 4096, n = 5 (160 workgroups of 5 agents in one launch), the second step's
    previous actions being the first step's picks, carried ONLY by the record pair (parity 0, then 1).  This is the case a raced or
    stale previous-action read shows in: the env head of agent i reads agent g's record byte while agent g's workgroup, in the same
    launch, writes its new pick (to the other buffer), and the inc head of a step must still see the actions of the step before."""
    from homophily_marl_amd.fast_policy import FastPolicy
    th.manual_seed(4)
    n, N = 5, 4096
    ctx = _ctx("cleanup", n, N, **OTHERS)
    mac, env = ctx.mac, ctx.runner.env
    A = mac.args.n_actions
    env.reset_batch()
    g = th.Generator(device="cuda").manual_seed(1)
    o = env.observe_batch(out=env.native.obs_buffers(abi.OBS_F32, want_code=True))
    obs, pos, orient, codes = o["obs"].clone(), o["pos"].clone(), o["orient"].clone(), o["code"].clone()
    avail = env.avail_actions_batch[0, 0]
    fp = FastPolicy(mac, N, avail, seed=7)
    eps, step = th.zeros((), device="cuda"), th.zeros(1, dtype=th.long, device="cuda")
    qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
    prev_a = th.randint(-1, A, (N, n), generator=g, device="cuda")
    prev_r = th.randint(-1, 2, (N, n), generator=g, device="cuda").float()
    prev_i = th.randint(0, 3, (N, n, n), generator=g, device="cuda")
    z = th.zeros(N, n, device="cuda")
    h_env = th.zeros(N, n, 1, 64, device="cuda"); h_inc = th.zeros(N, n, 1, 64, device="cuda")
    fp.reset()
    fp.set_prev_actions(prev_a, 0)
    own = prev_a.clone()                                                        # the head's own last-action block (prev_actions argument)
    with th.no_grad():
        feat = mac.encode_obs(obs)
        for t in range(2):
            inputs = mac.assemble_inputs(feat, prev_a, prev_r, prev_i, pos, False)
            q_env, h_env, _ = mac.agent.forward_env(inputs, h_env)
            fp.encode(None, codes=codes)
            picks = fp.head_env(own, prev_r, prev_i, pos, eps, step, q_out=qe, par=t).clone()
            de = (qe.transpose(0, 1) - q_env).abs().max().item()
            q_inc, h_inc, _ = mac.agent.forward_inc(inputs, h_inc, F.one_hot(picks, A), pos / mac.pos_scale, orient, z.unsqueeze(-1),
                                                    z.unsqueeze(-1), z.unsqueeze(-1))
            fp.act_inc(picks, pos, orient, z, z, z, eps, step, q_out=qi, par=t)
            di = (qi.transpose(0, 1) - q_inc).abs().max().item()
            print("step %d: q_env %.2e q_inc %.2e" % (t, de, di))
            assert de < TOL_Q and di < TOL_Q, (t, de, di)
            assert (fp.prev_rec[(t & 1) ^ 1, :, :n].view(th.int8).long() == picks).all()
            assert (fp.prev_rec[t & 1, :, :n].view(th.int8).long() == prev_a).all()          # the buffer that was read is untouched
            prev_a = own = picks
    env.close()


def test_gather_heads_reproduce_the_reference_q_values():
    """tests/golden/rollout_others_cleanup5.npz holds the REFERENCE controller's q_env / q_inc with obs_others_last_action: True
    (tools/gen_rollout_others_golden.py).  FastPolicy, driven step by step over the same batch, reproduces them within 1e-5 with the
    reference's greedy action wherever the top-2 gap exceeds 1e-6."""
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_others_last_action_host import load_others_fixture
    z, meta, args, batch, mac = load_others_fixture(device="cuda:0")
    B, n, A = batch.batch_size, args.n_agents, args.n_actions
    avail = batch["avail_actions"][0, 0, 0].to(th.uint8)
    fp = FastPolicy(mac, B, avail, seed=1)
    assert fp.fused and fp.fused_enc and fp.others
    q_env_ref, q_inc_ref = th.as_tensor(z["q_env"]).cuda(), th.as_tensor(z["q_inc"]).cuda()
    eps, step = th.zeros((), device="cuda"), th.zeros(1, dtype=th.long, device="cuda")
    qe, qi = th.zeros(n, B, A, device="cuda"), th.zeros(n, B, n, 3, device="cuda")
    acts, rew, ainc = batch["actions"].squeeze(-1), batch["reward"], batch["actions_inc"].squeeze(-1)
    worst_e = worst_i = 0.0
    n_clear = 0
    for t in range(meta["steps"]):
        prev_a = acts[:, t - 1].contiguous() if t else th.full((B, n), -1, dtype=th.long, device="cuda")
        prev_r = rew[:, t - 1].contiguous() if t else th.zeros(B, n, device="cuda")
        prev_i = ainc[:, t - 1].contiguous() if t else th.zeros(B, n, n, dtype=th.long, device="cuda")
        pos, orient = batch["agent_pos"][:, t].contiguous(), batch["agent_orientation"][:, t].contiguous()
        a_env = fp.act_env(batch["obs"][:, t].contiguous(), prev_a, prev_r, prev_i, pos, eps, step, q_out=qe)
        worst_e = max(worst_e, (qe.transpose(0, 1) - q_env_ref[:, t]).abs().max().item())
        masked = q_env_ref[:, t].masked_fill(batch["avail_actions"][:, t] == 0, -float("inf"))
        top2 = masked.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-6
        assert (a_env == masked.argmax(-1))[clear].all(), t
        n_clear += int(clear.sum())
        fp.act_inc(acts[:, t].contiguous(), pos, orient, rew[:, t].contiguous(), batch["clean_num"][:, t].contiguous(),
                   batch["apple_den"][:, t].contiguous(), eps, step, q_out=qi)
        worst_i = max(worst_i, (qi.transpose(0, 1) - q_inc_ref[:, t]).abs().max().item())
    print("max |q - reference| over %d steps: env %.2e inc %.2e; %d clear greedy rows" % (meta["steps"], worst_e, worst_i, n_clear))
    assert worst_e < TOL_Q and worst_i < TOL_Q
    assert n_clear > 0.9 * B * meta["steps"] * n


def _runner_cfg(key, N=48, T=12):
    from homophily_marl_amd.run import load_config
    return load_config("cleanup", overrides=dict(
        runner="hip_graph", batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False, store_state=False, use_cuda=True,
        save_model=False, runner_stats=False, learner_log_interval=10 ** 12, strict_device_ops=True, obs_others_last_action=True,
        fused_others_last_action=key, env_args=dict(num_agents=5, map="default5", episode_limit=T, seed=3)))


def test_graph_runner_takes_the_fused_heads_with_the_key_on():
    """Three greedy episodes (eager, captured, replayed) under strict_device_ops: every stored env action is the argmax of
    mac.unroll(batch) wherever the top two are more than 1e-4 apart (at most 10 % of the cases may be ties), and a train step runs."""
    from homophily_marl_amd.run import setup, train_iteration
    th.manual_seed(0)
    ctx = setup(_runner_cfg(True))
    runner, mac = ctx.runner, ctx.mac
    for ep in range(3):
        batch = runner.run(test_mode=True)
        assert runner.fast is not None and runner.fast.fused and runner.fast.others and not runner.pipe
        with th.no_grad():
            q_env, _ = mac.unroll(batch)
        T = runner.episode_limit
        q = q_env[:, :T].masked_fill(runner.env.avail_actions_batch[0, 0].view(1, 1, 1, -1) == 0, -float("inf"))
        top2 = q.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-4
        stored = batch["actions"][:, :T].squeeze(-1)
        tie_share = 1.0 - clear.float().mean().item()
        assert tie_share <= 0.10, "episode %d: %.4f of the (env, t, agent) cases left out as ties" % (ep, tie_share)
        assert (stored == q.argmax(-1))[clear].all(), "episode %d (tie share %.4f)" % (ep, tie_share)
    assert runner._graph is not None
    train_iteration(ctx, 0)
    th.cuda.synchronize()
    assert runner.env.native.poll_error() == 0
    runner.close_env()


def test_graph_runner_keeps_the_generic_timestep_with_the_key_off():
    from homophily_marl_amd.run import setup
    ctx = setup(_runner_cfg(False))
    ctx.runner.run(test_mode=True)
    assert ctx.runner.fast is None
    ctx.runner.close_env()
