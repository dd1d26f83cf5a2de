"""Training driver: the reference's run_sequential loop (src/run.py:81-244) re-stated around the same four registries.
One learner.train per runner.run (run.py:184-210).  `load_config` reproduces the yaml layering default <- env <- alg
of src/main.py:57-63,78-90 (with yaml.safe_load); sacred / tensorboard plumbing is out of scope.
"""
import os
from types import SimpleNamespace

import torch as th
import yaml

from .components.episode_buffer import ReplayBuffer
from .components.transforms import OneHot
from .controllers import REGISTRY as mac_REGISTRY
from .learners import REGISTRY as le_REGISTRY
from .runners import REGISTRY as r_REGISTRY
from .utils.logging import Logger

_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config")


def _merge(d, u):
    for k, v in u.items():
        d[k] = _merge(d.get(k, {}), v) if isinstance(v, dict) else v
    return d


def load_config(env_config="cleanup", alg_config="homophily", overrides=None):
    cfg = {}
    for name in ("default", env_config, alg_config):
        with open(os.path.join(_CFG, name + ".yaml")) as f:
            _merge(cfg, yaml.safe_load(f))
    _merge(cfg, overrides or {})
    return cfg


def build_scheme(args, env_info):
    """Scheme / groups / preprocess of run.py:97-119."""
    scheme = {
        "state": {"vshape": env_info["state_shape"]},
        "obs": {"vshape": env_info["obs_shape"], "group": "agents"},
        "actions": {"vshape": (1,), "group": "agents", "dtype": th.long},
        "avail_actions": {"vshape": (env_info["n_actions"],), "group": "agents", "dtype": th.int},
        "reward": {"vshape": (1,) if not args.ind_reward else (args.n_agents,)},
        "terminated": {"vshape": (1,), "dtype": th.uint8},
        "clean_num": {"vshape": (args.n_agents,)},
        "apple_den": {"vshape": (args.n_agents,)},
        "agent_pos": {"vshape": (args.n_agents, 2)},
        "agent_orientation": {"vshape": (args.n_agents, 2)},
    }
    if getattr(args, "obs_storage", "f32") == "code":      # compact storage: one u8 class code per window cell (include/ssd_hip.h)
        # (the env rejects the code format under extra_args.obs_color: "full")
        scheme["obs"] = {"vshape": tuple(env_info["obs_dims"]), "group": "agents", "dtype": th.uint8}
    if not getattr(args, "store_state", True):
        del scheme["state"]        # nothing downstream reads it; 22 MB/step at 4096 envs
    if "homophily" in args.name:
        scheme["actions_inc"] = {"vshape": (args.n_agents, 1), "group": "agents", "dtype": th.long}
    if getattr(args, "train_stored_state", False):
        # the rollout's recurrent state AFTER the controller consumed the slot, [h_env | h_inc] per agent (ssd_store_hidden)
        scheme["hidden"] = {"vshape": (2 * args.rnn_hidden_dim,), "group": "agents", "dtype": th.float32}
    from . import ops
    if ops.reward_field(args) != "reward":
        # the rollout's rewards shaped by the reward model (ssd_social_reward, one launch per training rollout): what the loss reads
        scheme["reward_model"] = {"vshape": (args.n_agents,), "dtype": th.float32}
    groups = {"agents": args.n_agents}
    preprocess = {"actions": ("actions_onehot", [OneHot(out_dim=args.n_actions)])}
    return scheme, groups, preprocess


def _check_train_window(args, episode_limit, runner):
    """The config keys of training on sampled time windows (absent = 0 / 0 / "episode": whole episodes), validated; returns the norm.
    train_window L in 1 .. episode_limit: a train step sees batch_size windows of L transitions (L + 1 slots); train_burn_in K in
    0 .. L - 1: the first K rows of a window that does not start at slot 0 carry no loss; train_window_norm: the length the rewards
    are divided by, "episode" (episode_limit + 1) or "window" (L + 1)."""
    L = args.train_window = int(getattr(args, "train_window", 0) or 0)
    K = args.train_burn_in = int(getattr(args, "train_burn_in", 0) or 0)
    norm = args.train_window_norm = getattr(args, "train_window_norm", "episode")
    if norm not in ("episode", "window"):
        raise ValueError('train_window_norm must be "episode" or "window", got %r' % (norm,))
    if L < 0 or L > episode_limit:
        raise ValueError("train_window %d outside 0 .. episode_limit = %d" % (L, episode_limit))
    if K < 0 or (K >= L and (L > 0 or K > 0)):
        raise ValueError("train_burn_in %d outside 0 .. train_window - 1 = %d" % (K, L - 1))
    if L > 0 and not getattr(runner, "fixed_length_episodes", False):
        raise ValueError("train_window > 0 needs a runner that fills every slot of an episode (the vectorised runners); runner %r does not" % (args.runner,))
    return norm


def _check_stored_state(args):
    """train_stored_state (absent = off), validated: sampled windows start their recurrence from the state the rollout stored for
    their first slot (R2D2's stored state) instead of zeros.  The episode scheme gains the field "hidden"; slot t holds the state
    AFTER the controller consumed slot t, so a window's row 0 is loaded, not computed, and carries loss.  train_burn_in stays legal
    (the stored state is as stale as the episode is old; burn-in refreshes it) and 0 is a sensible value."""
    on = args.train_stored_state = bool(getattr(args, "train_stored_state", False))
    if not on:
        return False
    if int(getattr(args, "train_window", 0) or 0) <= 0:
        raise ValueError("train_stored_state needs train_window > 0: whole episodes start at slot 0, where the state is zero anyway")
    if args.runner != "hip_graph":
        raise ValueError("train_stored_state needs runner hip_graph (the runner that files the recurrent state with the episode); runner %r does not" % (args.runner,))
    if args.buffer_cpu_only or not args.use_cuda:
        raise ValueError("train_stored_state needs a device-resident replay buffer (buffer_cpu_only: False, use_cuda: True): "
                         "the state is filed by a device launch and read in place by the learner's recurrence")
    if int(args.rnn_hidden_dim) != 64:
        raise ValueError("train_stored_state needs rnn_hidden_dim 64 (the snapshot and the sequence kernels are instantiated for it), got %r" % (args.rnn_hidden_dim,))
    return True


def _check_prioritized(args, buffer, runner):
    """The config keys of prioritised replay (absent = off), validated and written back with their defaults; returns whether it is on.
    prioritized_replay: proportional draws from a device-side priority table, importance weights on the gradient seeds, new
    priorities written in the train step (ssd_priority_sample / ssd_priority_update).  per_alpha: the priority exponent; per_beta:
    the importance-weight exponent at the first train step, annealed linearly to 1 over per_beta_anneal_steps train steps (0:
    constant); per_eta: the weight of a sample's largest TD error against its mean; per_eps: added to the aggregate error.
    per_initial_priority: what a new episode enters the table with -- "max" (default): 0, drawn at the table's current maximum until a
    train step has seen it; "rollout": the priority of its own one-step TD errors under the acting network, formed by the rollout
    (ssd_rollout_priority; always the plain one-step form, also under td_lambda / consider_others_inc -- a starting estimate the first
    train step on the episode overwrites).
    per_unit: what a table entry stands for -- "episode" (default): one priority per stored episode, a window's start drawn uniformly
    inside it; "window" (needs prioritized_replay and train_window L > 0): one priority per training window on a stride grid.  An
    episode of T transitions has S = ceil((T - L) / s) + 1 windows, window k starting at min(k s, T - L) (the last one clamped onto the
    episode's tail), s = per_window_stride, 0 = (L + 1) // 2 (R2D2's half overlap; written back resolved).  The table holds
    buffer_size * S entries, the draw is over entries -- several windows of one episode can sit in one train step, and the priority a
    train step measures on a window is spent on that window -- and with per_initial_priority "rollout" every window enters with the
    priority of its own loss rows.  Refused: s outside 1 .. L (gaps), ceil(L / s) over 8 (the windows one row feeds), S over
    PRIORITY_SEGMENTS_MAX, buffer_size * S over PRIORITY_POP_MAX."""
    on = args.prioritized_replay = bool(getattr(args, "prioritized_replay", False))
    alpha = args.per_alpha = float(getattr(args, "per_alpha", 0.6))
    beta = args.per_beta = float(getattr(args, "per_beta", 0.4))
    eta = args.per_eta = float(getattr(args, "per_eta", 0.9))
    eps = args.per_eps = float(getattr(args, "per_eps", 1e-3))
    steps = args.per_beta_anneal_steps = int(getattr(args, "per_beta_anneal_steps", 0) or 0)
    initial = args.per_initial_priority = getattr(args, "per_initial_priority", "max")
    if initial not in ("max", "rollout"):
        raise ValueError('per_initial_priority must be "max" or "rollout", got %r' % (initial,))
    for name, v in (("per_alpha", alpha), ("per_beta", beta), ("per_eta", eta)):
        if not 0.0 <= v <= 1.0:                        # (NaN fails both comparisons)
            raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
    if not eps > 0.0:
        raise ValueError("per_eps must be positive, got %r" % (eps,))
    if steps < 0:
        raise ValueError("per_beta_anneal_steps must not be negative, got %r" % (steps,))
    if initial == "rollout":
        if not on:
            raise ValueError('per_initial_priority "rollout" needs prioritized_replay: True (there is no priority table without it)')
        if args.runner != "hip_graph":
            raise ValueError('per_initial_priority "rollout" needs runner hip_graph (the runner that forms the priorities during the rollout); '
                             "runner %r does not" % (args.runner,))
        if th.device(buffer.device).type != "cuda":
            raise ValueError('per_initial_priority "rollout" needs a device-resident replay buffer (buffer_cpu_only: False, use_cuda: True): '
                             "the priorities are written into the table by a device launch; buffer on %s" % (buffer.device,))
    from . import abi, ops
    unit = args.per_unit = getattr(args, "per_unit", "episode")
    stride = args.per_window_stride = int(getattr(args, "per_window_stride", 0) or 0)
    if unit not in ("episode", "window"):
        raise ValueError('per_unit must be "episode" or "window", got %r' % (unit,))
    segments = 1
    if unit == "window":
        L = int(getattr(args, "train_window", 0) or 0)
        if not on:
            raise ValueError('per_unit "window" needs prioritized_replay: True (there is no priority table without it)')
        if L <= 0:
            raise ValueError('per_unit "window" needs train_window > 0: whole episodes have no windows to prioritise')
        stride = args.per_window_stride = stride or (L + 1) // 2
        if not 1 <= stride <= L:
            raise ValueError("per_window_stride %d outside 1 .. train_window = %d (a larger stride leaves rows no window trains on)" % (stride, L))
        if -(-L // stride) > 8:
            raise ValueError("per_window_stride %d: ceil(train_window / per_window_stride) = %d over 8 windows per row" % (stride, -(-L // stride)))
        segments = ops.window_grid(buffer.max_seq_length - 1, L, stride)[0]
        if segments > abi.PRIORITY_SEGMENTS_MAX:
            raise ValueError("per_window_stride %d: %d windows per episode over SSD_PRIORITY_SEGMENTS_MAX = %d" % (stride, segments, abi.PRIORITY_SEGMENTS_MAX))
        if buffer.buffer_size * segments > abi.PRIORITY_POP_MAX:
            raise ValueError("per_unit \"window\": buffer_size %d * %d windows per episode (per_window_stride %d) over SSD_PRIORITY_POP_MAX = %d"
                             % (buffer.buffer_size, segments, stride, abi.PRIORITY_POP_MAX))
    if not on:
        return False
    if not getattr(runner, "fixed_length_episodes", False) or th.device(buffer.device).type != "cuda":
        raise ValueError("prioritized_replay needs a device-resident replay buffer filled by a vectorised runner (buffer_cpu_only: False); "
                         "runner %r, buffer on %s" % (args.runner, buffer.device))
    if not getattr(args, "fused_loss", True):
        raise ValueError("prioritized_replay needs the fused loss (fused_loss: True): the priorities come from its per-row partials")
    if args.batch_size > abi.SAMPLE_IDS_MAX:
        raise ValueError("prioritized_replay: batch_size %d over SSD_SAMPLE_IDS_MAX = %d" % (args.batch_size, abi.SAMPLE_IDS_MAX))
    if unit == "window":
        buffer.enable_priorities(segments=segments, stride=stride, window=int(args.train_window))
    else:
        buffer.enable_priorities()
    return True


def _check_epsilon_ladder(args, fused_heads=True):
    """epsilon_ladder_alpha (absent = 0 = off: every env explores at the scheduled epsilon), validated and written back.  alpha > 0:
    env g of the job's G envs (batch_size_run x ranks, g = env_id_base + local env) explores at epsilon(t) ** (1 + alpha g / (G - 1)) --
    the Ape-X / R2D2 actor ladder: env 0 at the scheduled rate, env G - 1 at epsilon ** (1 + alpha).  The rates are rows of a device
    table the fused rollout heads read (ssd_policy_head.epsilon_rows), so the key needs runner hip_graph on the fused heads
    (`fused_heads`: what the runner planned; the generic torch timestep and the per-layer heads keep the scalar).  Runs without a
    device; returns alpha."""
    raw = getattr(args, "epsilon_ladder_alpha", 0.0)
    alpha = float(0.0 if raw is None else raw)
    if not alpha >= 0.0 or alpha == float("inf"):       # (NaN fails the comparison)
        raise ValueError("epsilon_ladder_alpha must be a finite number >= 0, got %r" % (raw,))
    args.epsilon_ladder_alpha = alpha
    if alpha > 0.0:
        if args.runner != "hip_graph":
            raise ValueError("epsilon_ladder_alpha > 0 needs runner hip_graph (the runner whose heads read a rate per env); runner %r does not" % (args.runner,))
        if not fused_heads:
            raise ValueError("epsilon_ladder_alpha > 0 needs the fused rollout heads (fast_policy and fused_policy on a layout they take): "
                             "the generic timestep and the per-layer heads explore at the scalar epsilon")
    return alpha


def _check_reward_model(args):
    """reward_model (absent = "individual" = off: the env's own rewards, no field, no launch), validated and written back.
    "inequity_aversion" (ia_alpha, ia_beta, ia_decay; Hughes et al. 2018) or "prosocial" (prosocial_weight): after every TRAINING
    rollout the runner shapes the stored rewards into the storage field "reward_model" (ops.social_reward, one eager launch over the
    finished rollout: inequity aversion carries a recurrence from slot 0, which a sampled window cannot form), and the loss reads that
    field.  Observations, statistics, returns and replays keep the env's rewards.  Needs args.n_agents; runs without a device; returns
    the three scalars of the launch, or None when off."""
    from . import ops
    model = getattr(args, "reward_model", "individual")
    args.reward_model = model = "individual" if model is None else model
    if model == "individual":
        return None
    if not isinstance(model, str) or model not in ops.REWARD_MODELS:
        raise ValueError('reward_model must be "individual", "inequity_aversion" or "prosocial", got %r' % (model,))
    if not getattr(args, "ind_reward", True):
        raise ValueError("reward_model %r needs ind_reward: True (a model compares the agents' own rewards; a team reward has nothing to compare)" % (model,))
    if args.runner not in ("hip_vec", "hip_graph"):
        raise ValueError("reward_model %r needs a vectorised runner (hip_vec or hip_graph: the runners that shape a finished rollout on the "
                         "device); runner %r does not" % (model, args.runner))
    if getattr(args, "per_initial_priority", "max") == "rollout":
        raise ValueError('reward_model %r with per_initial_priority "rollout": those priorities are formed during the rollout from the '
                         "env's rewards and would not be the errors the train step measures" % (model,))
    keys = {k: getattr(args, k) for k in ("ia_alpha", "ia_beta", "ia_decay", "prosocial_weight") if hasattr(args, k)}
    try:
        args.reward_model_scalars = ops.social_reward_scalars(model, args.n_agents, **keys)
    except ValueError as e:
        raise ValueError("reward_model %r: %s" % (model, e)) from None
    return args.reward_model_scalars


def _check_share_heads(args):
    """share_heads (absent = "none" = off: every agent keeps its own heads, no launch, the same bits), validated and written back.
    "env", "inc" or "both": the per-agent copies of that head group start equal (agent 0's initialisation) and the learner ties their
    gradients in front of the first clip (homophily_learner.tie_agent_grads; on the device ssd_tie_agent_grads inside the captured
    optimiser graph), which keeps them equal to the bit.  setup calls it twice: before the runner exists (the value) and once
    args.n_agents is known (one agent has nothing to share).  Runs without a device; returns the tied groups."""
    from .modules.agents.homophily_agent import share_heads_tags
    tags = share_heads_tags(getattr(args, "share_heads", "none"))
    args.share_heads = "none" if getattr(args, "share_heads", None) is None else args.share_heads
    if tags and getattr(args, "n_agents", None) is not None and args.n_agents < 2:
        raise ValueError("share_heads %r needs n_agents >= 2 (one agent has nothing to share with)" % (args.share_heads,))
    return tags


def _check_mixer(args):
    """mixer (PyMARL's key; absent, None, "" or "none" = off: independent learners, no launch, no tensor, the same bits), validated and
    written back as None or the name.  "vdn": the env head trains on the team's TD error, the sum over the agents of a (b, t)
    (homophily_learner.team_td; on the device ssd_team_td directly behind the loss launch); acting, the inc head and every other key
    are as without it -- reward_model, td_lambda, train_window, share_heads, target_tau and prioritized_replay compose, and under
    per_initial_priority "rollout" the starting priorities stay the per-agent one-step form the first train step overwrites.  setup
    calls it twice: before the runner exists (the value, ind_reward) and once args.n_agents is known.  Runs without a device."""
    from . import ops
    args.mixer = mixer = ops.team_mixer(args)
    if mixer is None:
        return None
    if not getattr(args, "ind_reward", True):
        raise ValueError("mixer %r needs ind_reward: True (the mixer sums the agents' own rewards into the team's; under ind_reward: False "
                         "every agent is already paid the team reward and the sum would pay it n times)" % (mixer,))
    if getattr(args, "n_agents", None) is not None and args.n_agents < 2:
        raise ValueError("mixer %r needs n_agents >= 2 (one agent is its own team)" % (mixer,))
    return mixer


def _check_target_tau(args):
    """target_tau (absent = 0 = off: the reference's hard sync every target_update_interval), validated and written back.  A value in
    (0, 1]: after every learner.train call the target net becomes (1 - tau) target + tau live on the device, inside the optimiser tail
    (HomophilyLearner.clip_and_step), and target_update_interval is ignored.  Runs without a device; returns tau."""
    from .learners.homophily_learner import validate_target_tau
    args.target_tau = validate_target_tau(getattr(args, "target_tau", 0.0))
    return args.target_tau


def per_beta(args, train_steps):
    """the importance-weight exponent of train step number train_steps (0-based): per_beta, annealed linearly to 1 over
    per_beta_anneal_steps train steps (0: constant)"""
    steps = getattr(args, "per_beta_anneal_steps", 0)
    if steps <= 0:
        return args.per_beta
    return args.per_beta + (1.0 - args.per_beta) * min(1.0, train_steps / steps)


def setup(config, logger=None):
    """Build runner / buffer / mac / learner exactly in the order of run.py:84-135."""
    args = SimpleNamespace(**config)
    if args.use_cuda and not th.cuda.is_available():
        args.use_cuda = False
    args.device = ("cuda:%d" % getattr(args, "device_index", 0)) if args.use_cuda else "cpu"
    # Units of the two schedules that the reference counts in env steps / episodes of its ONE env (epsilon_anneal_time,
    # target_update_interval).  "env_steps": the reference's literal arithmetic (default at batch_size_run == 1).  "rollouts"
    # (default for vectorised rollouts): one rollout of all envs advances the epsilon clock by episode_limit and the target-sync
    # counter counts learner.train calls -- the same number of rollouts / optimisation steps per anneal and per sync as the reference.
    if getattr(args, "schedule_unit", None) not in ("env_steps", "rollouts"):
        args.schedule_unit = "env_steps" if args.batch_size_run == 1 else "rollouts"
    args.train_steps_per_rollout = max(1, int(getattr(args, "train_steps_per_rollout", 1) or 1))
    if getattr(args, "strict_device_ops", False):
        from . import ops
        ops.set_strict(True)
    logger = logger or Logger()
    _check_stored_state(args)
    _check_target_tau(args)
    _check_share_heads(args)
    _check_mixer(args)
    runner =r_REGISTRY[args.runner](args=args, logger=logger)
    env_info = runner.get_env_info()
    args.n_agents, args.n_actions = env_info["n_agents"], env_info["n_actions"]
    args.state_shape, args.obs_shape = env_info["state_shape"], env_info["obs_shape"]
    if args.rgb_input:
        args.state_dims, args.obs_dims = env_info["state_dims"], env_info["obs_dims"]
    _check_reward_model(args)
    _check_share_heads(args)
    _check_mixer(args)
    scheme, groups, preprocess = build_scheme(args, env_info)
    buffer = ReplayBuffer(scheme, groups, args.buffer_size, env_info["episode_limit"] + 1, preprocess=preprocess,
                          device="cpu" if args.buffer_cpu_only else args.device)
    buffer.window_norm = _check_train_window(args, env_info["episode_limit"], runner)
    _check_prioritized(args, buffer, runner)
    mac = mac_REGISTRY[args.mac](buffer.scheme, groups, args)
    runner.setup(scheme=scheme, groups=groups, preprocess=preprocess, mac=mac)
    _check_epsilon_ladder(args, fused_heads=runner.plans_fused_heads() if hasattr(runner, "plans_fused_heads") else False)
    learner = le_REGISTRY[args.learner](mac, buffer.scheme, logger, args)
    if args.use_cuda:
        learner.cuda()
    if args.schedule_unit == "rollouts":       # the log intervals run on the schedule clock too (see HomophilyLearner.log_clock)
        learner.log_clock = lambda: runner.sched_t
    if getattr(args, "replay_in_place", True) and hasattr(runner, "set_replay_buffer"):
        runner.set_replay_buffer(buffer)        # hip_graph: rollouts land in the replay buffer's own slots when the sizes allow
    return SimpleNamespace(args=args, logger=logger, runner=runner, buffer=buffer, mac=mac, learner=learner, train_steps=0)


def settle_gc():
    """Call once the loop's long-lived objects exist (networks, buffers, captured graphs): collect what setup left behind and move
    every surviving object into the permanent generation (gc.freeze).  A full collection of CPython's cyclic GC walks every tracked
    object -- with the tensors, modules and ctypes tables of this loop that is a 40-70 ms host pause, and at 8 train steps per
    rollout one of them lands every few dozen iterations; the host runs only ~5 iterations ahead of the GPU, so the device ran dry
    (bench trace, round 4: one train step of 55 ms on the device timeline).  Frozen objects are not walked again; the loop's own
    short-lived garbage stays cheap to collect."""
    import gc
    gc.collect()
    gc.freeze()


def train_iteration(ctx, episode):
    """One pass of the while-loop body of run.py:181-210: rollout, insert, sample, train (train_steps_per_rollout times; the
    reference's cadence is one).  The learner's episode counter (target sync every target_update_interval, homophily_learner.py:255-257)
    is the env-episode count under schedule_unit "env_steps" and the number of learner.train calls under "rollouts"."""
    a = ctx.args
    window = getattr(a, "train_window", 0)
    marks = getattr(ctx, "_trace_marks", None)          # diagnostic (bench SSD_BENCH_TRACE): device events between the phases

    def mark(tag):
        if marks is not None:
            e = th.cuda.Event(enable_timing=True); e.record(); marks.append((tag, e))
    mark("start")
    batch = ctx.runner.run(test_mode=False)
    mark("rollout")
    initial = getattr(ctx.runner, "initial_priorities", None)
    priorities = initial() if initial is not None else None
    if priorities is None:
        ctx.buffer.insert_episode_batch(batch)
    else:                                   # per_initial_priority "rollout": the episodes enter the table with the rollout's own priorities
        ctx.buffer.insert_episode_batch(batch, priorities=priorities)
    if ctx.buffer.can_sample(a.batch_size):
        for _ in range(a.train_steps_per_rollout):
            out = ctx.learner.sample_out() if hasattr(ctx.learner, "sample_out") else None
            if getattr(a, "prioritized_replay", False):     # whole episodes or windows, drawn in proportion to the priority table
                sample = ctx.buffer.sample_prioritized(a.batch_size, window, a.train_burn_in if window else 0, beta=per_beta(a, ctx.train_steps), out=out)
            elif window > 0:               # windows of a runner that fills every slot (setup checked): nothing to trim
                sample = ctx.buffer.sample_windows(a.batch_size, window, a.train_burn_in, out=out)
            else:
                sample = ctx.buffer.sample(a.batch_size, out=out)
            # run.py:188-189 trims the sample to its longest episode; the vectorised runners always write episode_limit + 1 slots
            # (`filled` is all ones), so the trim is the identity there and the device -> host read of max_t_filled() is skipped
            if not window and not getattr(ctx.runner, "fixed_length_episodes", False):
                sample = sample[:, :sample.max_t_filled()]
            if str(sample.device) != str(a.device):
                sample.to(a.device)
            ctx.learner.train(sample, ctx.runner.t_env, ctx.train_steps if a.schedule_unit == "rollouts" else episode)
            ctx.train_steps += 1
            mark("train")
    return episode + a.batch_size_run


def run_sequential(config, logger=None):
    ctx = setup(config, logger)
    a, runner, learner, log = ctx.args, ctx.runner, ctx.learner, ctx.logger
    if a.checkpoint_path:
        steps = [int(d) for d in os.listdir(a.checkpoint_path) if d.isdigit() and os.path.isdir(os.path.join(a.checkpoint_path, d))]
        pick = max(steps) if a.load_step == 0 else min(steps, key=lambda x: abs(x - a.load_step))     # run.py:137-164
        learner.load_models(os.path.join(a.checkpoint_path, str(pick)))
        runner.t_env = pick
        if a.evaluate or getattr(a, "save_replay", False):                  # run.py:166-170
            for _ in range(a.test_nepisode):
                runner.run(test_mode=True)
            if getattr(a, "save_replay", False):                            # run.py:76-77 (evaluate_sequential)
                ctx.replay_dir = runner.save_replay()
            runner.close_env()
            return ctx
    episode, last_test_T, last_log_T, saved_at = 0, -a.test_interval - 1, 0, 0
    settled = 0
    while runner.t_env <= a.t_max:
        episode = train_iteration(ctx, episode)
        if settled < 2 and ctx.train_steps >= (4, 64)[settled]:      # after the graphs are captured, and once more when everything is warm
            settle_gc()
            settled += 1
        if (runner.t_env - last_test_T) / a.test_interval >= 1.0:
            last_test_T = runner.t_env
            for _ in range(max(1, a.test_nepisode // runner.batch_size)):
                runner.run(test_mode=True)
        if a.save_model and (runner.t_env - saved_at >= a.save_model_interval or saved_at == 0):
            saved_at = runner.t_env
            path = os.path.join(a.local_results_path, "models", getattr(a, "unique_token", a.name), str(runner.t_env))
            os.makedirs(path, exist_ok=True)
            learner.save_models(path)                                        # agent.th, opt_env.th, opt_inc.th
        if runner.t_env - last_log_T >= a.log_interval:
            log.log_stat("episode", episode, runner.t_env)
            log.print_recent_stats()
            last_log_T = runner.t_env
    runner.close_env()
    return ctx
