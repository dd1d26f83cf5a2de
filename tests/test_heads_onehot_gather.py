"""GPU suite of the gathered one-hot layout on the fused rollout heads (k_head GEN = 3: every one-hot block of the input row as fc1
rows; config key fused_onehot_gather).  Bars: TOL_Q = 1e-5 (DESIGN section 2 "Bars") for precision 2; for precision 1 the bf16
variant's bars of test_policy_mfma.py::test_bf16_variant_is_close_to_fp32_and_labelled (1e-6 < max |dq| < 5e-2 against the
f32-equivalent heads).  The argument refusals and the supports() table run without a device: test_onehot_gather_host.py."""
import pytest
import torch as th
import torch.nn.functional as F

from homophily_marl_amd import abi

pytestmark = pytest.mark.gpu
TOL_Q = 1e-5
GATHER = abi.INPUT_GATHER_ONEHOT

KEY = dict(fused_onehot_gather=True)
FLAG_SETS = {
    "shipped": dict(KEY),
    "shipped_distance": dict(KEY, obs_distance=True),
    "all_seven": dict(KEY, obs_distance=True, obs_others_last_action=True),
}
#          map / env                 n   N     flags
SHAPES = [("cleanup", "default10", 6, 203, "shipped_distance"),      # 57 + 9 columns: the first width that does not fit; ragged last tile
          ("cleanup", "default10", 10, 64, "shipped_distance"),      # 65 / 74
          ("cleanup", "default10", 10, 64, "all_seven"),             # combined with bit 64
          ("harvest", "default10", 10, 64, "all_seven"),             # A = 8
          ("cleanup", "default10", 10, 4112, "all_seven"),           # the looped instantiations
          ("cleanup", "default5", 5, 203, "shipped")]                # fits densely too: compared with the dense fused heads as well


def _ctx(kind, map_, n, N, seed=3, runner="hip_vec", T=20, **over):
    from homophily_marl_amd.run import load_config, setup
    cfg = load_config(kind, overrides=dict(dict(runner=runner, batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False,
                                                store_state=False,
                                                env_args=dict(num_agents=n, map=map_, episode_limit=T, seed=seed, view_size=7),
                                                use_cuda=True, save_model=False, runner_stats=False), **over))
    return setup(cfg)


def _dense_columns(mac):
    """columns of the controller's input row that belong to no one-hot block (what `inputs` holds, compacted)"""
    a, n, A = mac.args, mac.n_agents, mac.args.n_actions
    cols, c = list(range(32)), 32
    for on, width, dense in ((a.obs_last_action, A, False), (a.obs_agent_id, n, False), (a.obs_reward, 1, True), (a.obs_inc_reward, 1, True),
                             (getattr(a, "obs_others_last_action", False), n * A, False), (getattr(a, "obs_distance", False), n, True),
                             (a.obs_agent_pos, 2, True)):
        if on:
            cols += list(range(c, c + width)) if dense else []
            c += width
    assert c == mac.input_shape
    return th.tensor(cols, device="cuda")


def _run_heads(mac, N, avail, prec, h0e, h0i, obs, codes, prev, pos, orient, act, reward, clean, den):
    from homophily_marl_amd.fast_policy import FastPolicy
    n, A = mac.n_agents, mac.args.n_actions
    eps, step = th.zeros((), device="cuda"), th.zeros(1, dtype=th.long, device="cuda")
    fp = FastPolicy(mac, N, avail, seed=7, precision=prec)
    qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
    fp.h_env.copy_(h0e.squeeze(2).transpose(0, 1)); fp.h_inc.copy_(h0i.squeeze(2).transpose(0, 1))
    fp.act_env(obs, prev[0], prev[1], prev[2], pos, eps, step, codes=codes, q_out=qe)
    fp.act_inc(act, pos, orient, reward, clean, den, eps, step, q_out=qi)
    th.cuda.synchronize()
    return qe.transpose(0, 1), fp.h_env.transpose(0, 1).clone(), qi.transpose(0, 1), fp.h_inc.transpose(0, 1).clone(), fp


@pytest.mark.parametrize("kind,map_,n,N,flags", SHAPES)
def test_onehot_gather_heads_match_the_torch_controller(kind, map_, n, N, flags):
    """Both heads against assemble_inputs -> forward_env / forward_inc, previous actions drawn from [-1, A) (-1: the row that adds
    nothing).  Precision 1 against the f32-equivalent heads, and not equal to them."""
    from homophily_marl_amd.fast_policy import FastPolicy
    th.manual_seed(2)
    ctx = _ctx(kind, map_, n, N, **FLAG_SETS[flags])
    mac, env = ctx.mac, ctx.runner.env
    A = mac.args.n_actions
    others = flags == "all_seven"
    assert mac.rollout_input_flags & GATHER and bool(mac.rollout_input_flags & 64) == others and FastPolicy.supports(mac)
    if (kind, n) == ("cleanup", 6):
        assert mac.input_shape == 57
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
    avail = env.avail_actions_batch[0, 0]
    with th.no_grad():
        inputs = mac.assemble_inputs(mac.encode_obs(obs), prev_a, prev_r, prev_i, pos, False)
        assert inputs.shape[1] == mac.input_shape
        q_env, h_env, _ = mac.agent.forward_env(inputs, h0e)
        act = q_env.masked_fill(avail.view(1, 1, -1) == 0, -float("inf")).argmax(-1)
        q_inc, h_inc, _ = mac.agent.forward_inc(inputs, h0i, F.one_hot(act, A), pos / mac.pos_scale, orient, reward.unsqueeze(-1),
                                                clean.unsqueeze(-1), den.unsqueeze(-1))
    common = (h0e, h0i, obs, codes, (prev_a, prev_r, prev_i), pos, orient, act, reward, clean, den)
    res = {prec: _run_heads(mac, N, avail, prec, *common) for prec in (2, 1)}
    qe, he, qi, hi, fp = res[2]
    assert fp.fused and fp.fused_enc and fp.gather and fp.others == others and not fp.inc_encode
    dense = _dense_columns(mac)
    assert dense.numel() == fp.inp_dense <= 46
    rows = fp.inputs.transpose(0, 1).reshape(N * n, -1)
    assert (rows[:, :dense.numel()] - inputs[:, dense]).abs().max() < 2e-6 and (rows[:, dense.numel():] == 0).all()
    d = [(qe - q_env).abs().max().item(), (he - h_env.squeeze(2)).abs().max().item(), (qi - q_inc).abs().max().item(),
         (hi - h_inc.squeeze(2)).abs().max().item()]
    print("%s n=%d N=%d %s: max |diff| vs torch f32: q_env %.2e h_env %.2e q_inc %.2e h_inc %.2e" % ((kind, n, N, flags) + tuple(d)))
    assert max(d) < TOL_Q, d
    b_env = (res[1][0] - qe).abs().max().item(); b_inc = (res[1][2] - qi).abs().max().item()
    print("bf16 vs f32-equivalent: q_env %.3e q_inc %.3e" % (b_env, b_inc))
    assert 1e-6 < b_env < 5e-2 and 1e-6 < b_inc < 5e-2
    assert not th.equal(res[1][0], qe) and not th.equal(res[1][2], qi)          # the variant really ran
    if flags == "shipped":      # the same controller through the dense fused heads (the layout it takes with the key off)
        mac.rollout_input_flags = mac.input_flags
        dq = _run_heads(mac, N, avail, 2, *common)
        assert dq[4].fused and not dq[4].gather and dq[4].prev_rec is None
        dd = [(x - y).abs().max().item() for x, y in zip(dq[:4], (qe, he, qi, hi))]
        print("gathered vs dense fused heads: q_env %.2e h_env %.2e q_inc %.2e h_inc %.2e" % tuple(dd))
        assert max(dd) < TOL_Q, dd
    env.close()


def test_two_consecutive_timesteps_carry_the_previous_actions_on_the_device():
    """env head -> inc head -> env head -> inc head at N = 4096, n = 6 with obs_distance (the width that does not fit densely), the
    second step's previous actions being the first step's picks, carried ONLY by the record pair (parity 0, then 1): the prev_actions
    argument holds -1 throughout.  A raced or stale previous-action read shows here: the inc head of a step must still see the actions
    of the step before, while the env head has already written its picks to the other buffer."""
    from homophily_marl_amd.fast_policy import FastPolicy
    th.manual_seed(4)
    n, N = 6, 4096
    ctx = _ctx("cleanup", "default10", n, N, **FLAG_SETS["shipped_distance"])
    mac, env = ctx.mac, ctx.runner.env
    A = mac.args.n_actions
    env.reset_batch()
    g = th.Generator(device="cuda").manual_seed(1)
    o = env.observe_batch(out=env.native.obs_buffers(abi.OBS_F32, want_code=True))
    obs, pos, orient, codes = o["obs"].clone(), o["pos"].clone(), o["orient"].clone(), o["code"].clone()
    avail = env.avail_actions_batch[0, 0]
    fp = FastPolicy(mac, N, avail, seed=7)
    assert fp.gather and not fp.others
    eps, step = th.zeros((), device="cuda"), th.zeros(1, dtype=th.long, device="cuda")
    qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
    prev_a = th.randint(-1, A, (N, n), generator=g, device="cuda")
    prev_r = th.randint(-1, 2, (N, n), generator=g, device="cuda").float()
    prev_i = th.randint(0, 3, (N, n, n), generator=g, device="cuda")
    z = th.zeros(N, n, device="cuda")
    none = th.full((N, n), -1, dtype=th.long, device="cuda")
    h_env = th.zeros(N, n, 1, 64, device="cuda"); h_inc = th.zeros(N, n, 1, 64, device="cuda")
    fp.reset()
    fp.set_prev_actions(prev_a, 0)
    with th.no_grad():
        feat = mac.encode_obs(obs)
        for t in range(2):
            inputs = mac.assemble_inputs(feat, prev_a, prev_r, prev_i, pos, False)
            q_env, h_env, _ = mac.agent.forward_env(inputs, h_env)
            fp.encode(None, codes=codes)
            picks = fp.head_env(none, prev_r, prev_i, pos, eps, step, q_out=qe, par=t).clone()
            de = (qe.transpose(0, 1) - q_env).abs().max().item()
            q_inc, h_inc, _ = mac.agent.forward_inc(inputs, h_inc, F.one_hot(picks, A), pos / mac.pos_scale, orient, z.unsqueeze(-1),
                                                    z.unsqueeze(-1), z.unsqueeze(-1))
            fp.act_inc(picks, pos, orient, z, z, z, eps, step, q_out=qi, par=t)
            di = (qi.transpose(0, 1) - q_inc).abs().max().item()
            print("step %d: q_env %.2e q_inc %.2e" % (t, de, di))
            assert de < TOL_Q and di < TOL_Q, (t, de, di)
            assert (fp.prev_rec[(t & 1) ^ 1, :, :n].view(th.int8).long() == picks).all()
            assert (fp.prev_rec[t & 1, :, :n].view(th.int8).long() == prev_a).all()          # the buffer that was read is untouched
            prev_a = picks
    env.close()


def test_onehot_gather_heads_reproduce_the_reference_q_values():
    """tests/golden/rollout_wide_cleanup10.npz holds the REFERENCE controller's q_env / q_inc with all seven flags at Cleanup-10
    (tools/gen_rollout_wide_golden.py).  FastPolicy, driven step by step over the same batch, reproduces them within 1e-5 with the
    reference's greedy action wherever the top-2 gap exceeds 1e-6."""
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_onehot_gather_host import load_wide_fixture
    z, meta, args, batch, mac = load_wide_fixture(device="cuda:0")
    B, n, A = batch.batch_size, args.n_agents, args.n_actions
    avail = batch["avail_actions"][0, 0, 0].to(th.uint8)
    fp = FastPolicy(mac, B, avail, seed=1)
    assert fp.fused and fp.fused_enc and fp.gather and fp.others
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


def _runner_ctx(graph, N=64, T=20):
    th.manual_seed(0)
    return _ctx("cleanup", "default10", 10, N, runner="hip_graph", T=T, learner_log_interval=10 ** 12,
                obs_distance=True, fused_onehot_gather=True, rollout_graph=graph)


def _episode_copy(batch):
    return {k: v.clone() for k, v in batch.data.transition_data.items()}


def test_graph_runner_takes_the_fused_heads_at_cleanup10_with_distance():
    """hip_graph at Cleanup-10 with obs_distance (65 / 74 columns: the generic timestep without the key).  Three exploring episodes
    (eager, captured, replayed) store bit-equal batches with graphs on and off; then a greedy episode's stored env actions are the torch
    controller's greedy actions recomputed from the stored batch wherever its top two are more than 1e-6 apart."""
    runs = {}
    for graph in (True, False):
        ctx = _runner_ctx(graph)
        runner = ctx.runner
        eps = []
        for ep in range(3):
            eps.append(_episode_copy(runner.run(test_mode=False)))
            assert runner.fast is not None and runner.fast.fused and runner.fast.gather and not runner.pipe
        assert (runner._graph is not None) == graph
        runs[graph] = eps
        if graph:
            mac = ctx.mac
            batch = runner.run(test_mode=True)
            T, B, n = runner.episode_limit, batch.batch_size, mac.n_agents
            avail = runner.env.avail_actions_batch[0, 0].view(1, 1, -1)
            stored = batch["actions"][:, :T].squeeze(-1)
            mac.init_hidden(B)
            n_clear = 0
            with th.no_grad():
                for t in range(T):
                    q = mac.forward(batch, t)[0].reshape(B, n, -1).masked_fill(avail == 0, -float("inf"))
                    top2 = q.topk(2, dim=-1).values
                    clear = (top2[..., 0] - top2[..., 1]) > 1e-6
                    assert (stored[:, t] == q.argmax(-1))[clear].all(), t
                    n_clear += int(clear.sum())
            assert n_clear > 0.9 * B * T * n
            assert runner.env.native.poll_error() == 0
        runner.close_env()
    for ep, (a, b) in enumerate(zip(runs[True], runs[False])):
        assert a.keys() == b.keys()
        for k in a:
            assert th.equal(a[k], b[k]), (ep, k)
