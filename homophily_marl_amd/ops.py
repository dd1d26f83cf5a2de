"""The operator layer: every torch-facing operator of the learner, the controller and the replay buffer over the C ABI of
libssd_hip.so (include/ssd_hip.h) -- loss and incentive transfer, agent inputs, affine layers, dueling heads, encoder, recurrence,
replay draws and gathers, priorities, fills and statistics -- with the autograd Functions that give the kernels their backward.

Guard rules, the same for every operator:
  * device tensors go through the library (load_library() raises if it is missing: no silent fallback on a GPU box);
  * every launch is guarded over device, dtype and the sizes its arguments are derived from.  A call its kernel is not instantiated
    for takes the operator's tensor-op statement -- the same arithmetic in torch expressions -- after _leaving_kernels, or raises a
    ValueError naming the argument (_unfit) where no statement can take it either;
  * host tensors -- the CPU test-suite and the gloo rehearsal of the data-parallel path, where no HIP device exists -- always take the
    tensor-op statement; a GPU run never does;
  * a Function records the learner precision (LEARNER_PRECISION, _precision) at forward and runs its backward launches under it.

Strict mode (config key strict_device_ops, SSD_STRICT_DEVICE_OPS=1, set_strict): _leaving_kernels raises for a device tensor, so a
tensor-op branch on a GPU run is a failure, not a fallback.  bench.py, smoke() and the GPU suite run under it.
"""
import ctypes as C

import torch as th

from . import abi


def _stream(t):
    return th.cuda.current_stream(t.device).cuda_stream


# strict_device_ops: raise where a DEVICE tensor would leave the HIP kernels for a tensor-op statement (shapes / dtypes an operator's
# kernel is not instantiated for).  bench.py, smoke() and the GPU suite switch it on (config key `strict_device_ops`, or
# SSD_STRICT_DEVICE_OPS=1): a silent torch branch on a GPU run is a failure there, not a fallback.
import os as _os
STRICT = _os.environ.get("SSD_STRICT_DEVICE_OPS") == "1"


def numeric_status():
    """Sticky numeric-status bits of the current device, cleared on read (ssd_numeric_status; abi.ERRBIT_F16_RANGE: a scaled value of
    a two-term f16 split product left f16's range in a pack kernel, a rollout head or the learner's recurrence).  Synchronises."""
    lib = abi.load_library()
    bits = C.c_int32(0)
    abi.check(lib, lib.ssd_numeric_status(C.byref(bits)))
    return bits.value


def reserve_bmm_scratch(stream):
    """The per-(device, stream) scratch of the row-chunked affine backward (ssd_bias_bmm_bwd) for a stream that is about to capture
    the train step: nothing can be allocated inside a capture."""
    lib = abi.load_library()
    abi.check(lib, lib.ssd_bmm_reserve_scratch(stream.cuda_stream))


def unroll_other(actions, pos, orient, reward, clean_num, apple_den, pos_scale, n_actions):
    """(other [T * B, n, A + 7], act_tm [n, T * B, A]) of a sampled batch on the device in ONE launch (ssd_unroll_other): the
    incentive head's per-receiver features [one-hot(a_j), pos_j / scale, orient_j, r_j, clean_j, apple_den_j] (homophily_agent.py:194-201)
    and the one-hot actions agent-major.  actions i64 [B, T, n], pos / orient [B, T, n, 2], reward / clean_num / apple_den [B, T, n]."""
    if actions.dtype != th.int64 or actions.dim() != 3:       # the kernel reads 8-byte indices [B, T, n]
        raise _unfit("unroll_other", "actions", actions, "int64 [B, T, n] expected")
    B, T, n = actions.shape[:3]
    for name, t, shape in (("pos", pos, (B, T, n, 2)), ("orient", orient, (B, T, n, 2)), ("reward", reward, (B, T, n)),
                           ("clean_num", clean_num, (B, T, n)), ("apple_den", apple_den, (B, T, n))):
        if t.shape != shape or t.device != actions.device:
            raise _unfit("unroll_other", name, t, "%s on the device of actions expected" % (shape,))
    lib = abi.load_library()
    c = lambda x: x.contiguous()
    actions, pos, orient, reward, clean_num, apple_den = c(actions), c(pos.float()), c(orient.float()), c(reward.float()), c(clean_num.float()), c(apple_den.float())
    other = th.empty(T * B, n, n_actions + 7, dtype=th.float32, device=actions.device)
    act_tm = th.empty(n, T * B, n_actions, dtype=th.float32, device=actions.device)
    abi.check(lib, lib.ssd_unroll_other(actions.data_ptr(), pos.data_ptr(), orient.data_ptr(), reward.data_ptr(), clean_num.data_ptr(), apple_den.data_ptr(),
                                        float(pos_scale), B, T, n, n_actions, other.data_ptr(), act_tm.data_ptr(), _stream(other)))
    return other, act_tm


LEARNER_PRECISION = 2


def set_learner_precision(precision):
    """Arithmetic of the learner's matrix products (ssd_set_learner_precision): 2 = f32 (default), 1 = the labelled bf16 variant (single
    bf16 MFMA products in the per-agent affine layers, the recurrence and the encoder; f32 accumulation / parameters / optimiser / loss).
    CPU tensors are unaffected (the tensor-op statements are f32)."""
    global LEARNER_PRECISION
    precision = int(precision)
    if precision != LEARNER_PRECISION or precision != 2:
        lib = abi.load_library()
        abi.check(lib, lib.ssd_set_learner_precision(precision))
    LEARNER_PRECISION = precision


class _precision:
    """The learner precision for the launches of a block, what was set before restored on the way out.  Every Function whose launches
    select on it (the affine layers, the dueling head, the encoder, the recurrence) records LEARNER_PRECISION in ctx at forward and runs
    its backward launches under it: the precision belongs to the call, whatever the process-wide switch reads by the time the gradients
    are asked for.  No launch, no library call when nothing changes."""

    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        self.found = LEARNER_PRECISION
        if self.precision != self.found:
            set_learner_precision(self.precision)

    def __exit__(self, *exc):
        if self.precision != self.found:
            set_learner_precision(self.found)


def _f32_on(t, *others):
    """every tensor f32 on t's device (the kernels read raw f32 pointers of one device)"""
    return all(o.dtype == th.float32 and o.device == t.device for o in (t,) + others)


def _unfit(op, arg, t, why):
    """an argument neither the kernels nor the tensor-op statement can take: the error names it"""
    return ValueError("ops.%s: %s %s: %s" % (op, arg, "%s %s on %s" % (tuple(t.shape), t.dtype, t.device), why))


def set_strict(on=True):
    global STRICT
    STRICT = bool(on)


class capture:
    """th.cuda.graph(graph, **kw) with Python's cyclic collector kept out of the capture.  torch.cuda.graph no longer collects before
    it begins to capture (torch >= 2.9: only under torch.compiler.config.force_cudagraph_gc), so a dead reference cycle that owns
    device resources -- an earlier learner with its captured graphs and their memory pool, an env handle -- could be finalised by a
    collection that happens to start between two captured launches; what its finalisers call (hipFree, hipGraphExecDestroy, a
    synchronisation) is illegal on a capturing thread, invalidates the capture and ends the process in abort().  Here the cycles
    are collected before the capture begins, where their finalisers are legal, and none is collected until it has ended."""

    def __init__(self, graph, **kw):
        self.ctx = th.cuda.graph(graph, **kw)

    def __enter__(self):
        import gc
        gc.collect()
        self.gc_was_on = gc.isenabled()
        gc.disable()
        try:
            return self.ctx.__enter__()
        except BaseException:
            if self.gc_was_on:
                gc.enable()
            raise

    def __exit__(self, *exc):
        import gc
        try:
            return self.ctx.__exit__(*exc)
        finally:
            if self.gc_was_on:
                gc.enable()


def _leaving_kernels(op, t, why):
    """called on every branch that evaluates an operator with tensor ops: fine for host tensors, an error for device tensors under
    strict_device_ops."""
    if STRICT and t is not None and t.is_cuda:
        raise RuntimeError("strict_device_ops: ops.%s would take the tensor-op branch for a device tensor (%s)" % (op, why))


def build_inputs_tail(out, offset, last_actions, last_reward, last_actions_inc, pos, pos_scale, n_actions, t0, flags=None, seq_len=0):
    """Fill out[:, offset : offset + A + n + 4] with the non-visual agent-input features of
    HomophilyMAC._build_inputs (controllers/homophily_controller.py:137-184):
    onehot(last action) | onehot(agent id) | sign(last reward) | sign(#recv+ - #recv-) | pos / ||(H, W)||.
    out: f32 [B * n, stride]; last_actions i64 [B, n]; last_reward f32 [B, n]; last_actions_inc i64 [B, n, n];
    pos f32 [B, n, 2].  t0: the t == 0 branch (the three history terms are zero, their tensors may be None).
    flags (device tensors only): abi.INPUT_* bits of any other flag set -- the blocks present, in the reference's order, incl.
    everybody's last action (obs_others_last_action) and 1 - distances (obs_distance); out must be that wide.
    seq_len = T > 0 (device tensors only): B counts [episodes, T] rows and the history tensors hold every step's OWN values -- the
    kernel reads the previous timestep's row itself (no shifted copies)."""
    B, n = pos.shape[0], pos.shape[1]
    A = n_actions
    if out.is_cuda:
        for name, t, dtype in (("last_actions", last_actions, th.int64), ("last_actions_inc", last_actions_inc, th.int64),      # read as 8-byte indices
                               ("last_reward", last_reward, th.float32), ("pos", pos, th.float32)):
            if t is not None and (t.dtype != dtype or t.device != out.device):
                raise _unfit("build_inputs_tail", name, t, "%s on the device of out expected" % dtype)
        lib = abi.load_library()
        cont = lambda x: None if x is None else x.contiguous()
        la, lr, li, p = cont(last_actions), cont(last_reward), cont(last_actions_inc), pos.contiguous()
        assert out.is_contiguous() and out.dtype == th.float32
        ptr = lambda x: None if x is None else x.data_ptr()
        word = (1 if t0 else 0) | (int(seq_len) << 8)
        if flags is not None:       # any _build_inputs flag set (abi.INPUT_* bits), blocks in the reference's order
            abi.check(lib, lib.ssd_build_inputs_flags(B, n, A, word, abi.INPUT_EXPLICIT | int(flags), ptr(la), ptr(lr), ptr(li),
                                                      p.data_ptr(), float(pos_scale), out.data_ptr(), out.shape[1], offset, _stream(out)))
            return out
        abi.check(lib, lib.ssd_build_inputs(B, n, A, word, ptr(la), ptr(lr), ptr(li), p.data_ptr(), float(pos_scale),
                                            out.data_ptr(), out.shape[1], offset, _stream(out)))
        return out
    assert flags is None and not seq_len, "CPU tensors: only the shipped flag set has a tensor-op statement here (HomophilyMAC.assemble_inputs has all)"
    o = out.view(B, n, -1)
    if t0:
        o[..., offset:offset + A] = 0
        o[..., offset + A + n] = 0
        o[..., offset + A + n + 1] = 0
    else:
        valid = (last_actions >= 0).unsqueeze(-1)                        # index -1 = "no previous action": all-zero one-hot
        o[..., offset:offset + A] = th.nn.functional.one_hot(last_actions.clamp(min=0), A).to(o.dtype) * valid
        o[..., offset + A + n] = th.sign(last_reward)
        m = last_actions_inc * (1 - th.eye(n, dtype=last_actions_inc.dtype, device=o.device))
        recv = (m == 1).sum(dim=1) - (m == 2).sum(dim=1)                 # giver dim summed -> per receiver
        o[..., offset + A + n + 1] = th.sign(recv.to(o.dtype))
    o[..., offset + A:offset + A + n] = th.eye(n, dtype=o.dtype, device=o.device)
    o[..., offset + A + n + 2:offset + A + n + 4] = pos / pos_scale
    return out


def incentive_transfer(actions_inc, rewards, effect_ratio, cost_ratio, incentive, seq_len):
    """Incentive reward transfer (learners/homophily_learner.py:94-115).
    actions_inc i64 [B, T, n, n] (giver dim 2, receiver dim 3), rewards f32 [B, T-1, n].
    Returns give [B,T-1,n], recv_pos / recv_neg / recv_zero [B,T,n], rewards_for_env, rewards_for_inc [B,T-1,n] (f32)."""
    B, T, n = actions_inc.shape[0], actions_inc.shape[1], actions_inc.shape[2]
    dev = actions_inc.device
    if actions_inc.is_cuda:
        if actions_inc.dtype != th.int64 or actions_inc.dim() != 4 or actions_inc.shape[3] != n:       # the kernel reads 8-byte indices [B, T, n, n]
            raise _unfit("incentive_transfer", "actions_inc", actions_inc, "int64 [B, T, n, n] expected")
        if rewards.shape != (B, T - 1, n) or rewards.device != dev:
            raise _unfit("incentive_transfer", "rewards", rewards, "%s on the device of actions_inc expected" % ((B, T - 1, n),))
        lib = abi.load_library()
        a = actions_inc.contiguous()
        r = rewards.contiguous().float()
        mk = lambda t: th.empty(B, t, n, dtype=th.float32, device=dev)
        give, rp, rn, rz, re, ri = mk(T - 1), mk(T), mk(T), mk(T), mk(T - 1), mk(T - 1)
        abi.check(lib, lib.ssd_incentive_transfer(B, T, n, a.data_ptr(), r.data_ptr(), float(effect_ratio), float(cost_ratio),
                                                  float(incentive), float(seq_len), give.data_ptr(), rp.data_ptr(), rn.data_ptr(),
                                                  rz.data_ptr(), re.data_ptr(), ri.data_ptr(), _stream(a)))
        return give, rp, rn, rz, re, ri
    mask = (1 - th.eye(n, dtype=actions_inc.dtype, device=dev)).view(1, 1, n, n)
    m = actions_inc * mask
    give = (m[:, :-1] != 0).sum(dim=3).float()
    rp = (m == 1).sum(dim=2).float()
    rn = (m == 2).sum(dim=2).float()
    rz = (n - 1) - rp - rn
    rv = rp[:, :-1] - rn[:, :-1]
    re = (rewards + rv * effect_ratio * incentive) / seq_len
    ri = (rewards - give * cost_ratio * incentive) / seq_len
    return give, rp, rn, rz, re, ri


def reward_norm(batch):
    """The length the rewards are divided by (homophily_learner.py:112-115, `/ batch.max_seq_length`): the attribute a window batch
    carries (ReplayBuffer.gather_windows; config key train_window_norm), else the batch's own slot count."""
    return float(batch.reward_norm or batch.max_seq_length)


def window_reward_norm(norm, slots, window):
    """The length a batch's rewards are divided by under train_window_norm `norm`: the episode's slot count ("episode", or whole
    episodes), else window + 1 -- one statement for the buffer's window batches and the rollout's initial priorities."""
    return float(slots if norm == "episode" or not window else window + 1)


def td_constants(a, seq_len):
    """The scalars of the TD targets by the names the argument blocks carry them under, from the config `a` and the reward norm: what
    the loss launch (_td_loss_args) and the rollout's initial priorities (rollout_priority_args) both take, so the two cannot drift."""
    return dict(gamma_env=float(a.gamma_env), gamma_inc=float(a.gamma_inc), reward_scale=float(a.reward_scale),
                incentive_ratio=float(a.incentive_ratio), incentive_cost=float(a.incentive_cost), incentive=float(a.incentive),
                seq_len=float(seq_len))


def _td_loss_args(batch, a, n_actions, partials):
    """ssd_td_loss_args over the batch's tensors (contiguous copies where a view is not); returns (args, keep-alive list)."""
    c = lambda x: x.contiguous()
    B, T1, n = batch.batch_size, batch.max_seq_length, batch["reward"].shape[-1]
    keep = dict(actions=c(batch["actions"].squeeze(-1)), actions_inc=c(batch["actions_inc"].squeeze(-1)), avail=c(batch["avail_actions"]),
                reward=c(batch[reward_field(a)].float()), clean_num=c(batch["clean_num"].float()),
                terminated=c(batch["terminated"].squeeze(-1)), filled=c(batch["filled"].squeeze(-1)))
    assert keep["avail"].dtype == th.int32 and keep["terminated"].dtype == th.uint8 and keep["filled"].dtype == th.int64
    t = abi.SsdTdLossArgs()
    t.batch, t.t_slots, t.n_agents, t.n_actions, t.sim_horizon, t.double_q = B, T1, n, n_actions, int(a.sim_horizon), int(bool(a.double_q))
    for k, v in td_constants(a, reward_norm(batch)).items():
        setattr(t, k, v)
    t.sim_threshold, t.sim_loss_weight = float(a.sim_threshold), float(a.sim_loss_weight)
    t.consider_others_inc = int(bool(a.consider_others_inc))
    t.td_lambda = float(getattr(a, "td_lambda", 0.0) or 0.0)
    for k, v in keep.items():
        setattr(t, k, v.data_ptr())
    t.partials = partials.data_ptr()
    return t, keep


def loss_denominators(batch, a, n_actions):
    """[mask.sum(), sim_loss_mask.sum()] of this batch (homophily_learner.py:62-64,184-206,214) from ONE launch of ssd_td_sim_loss
    (mode 0) instead of ~30 tensor ops; device tensors only."""
    lib = abi.load_library()
    B, T, n = batch.batch_size, batch.max_seq_length - 1, batch["reward"].shape[-1]
    partials = th.empty(B * T * n, abi.TD_LOSS_PARTIALS, dtype=th.float32, device=batch["reward"].device)   # mode 0 writes columns 0, 1 of every row
    t, keep = _td_loss_args(batch, a, n_actions, partials)
    abi.check(lib, lib.ssd_td_sim_loss(C.byref(t), 0, _stream(partials)))
    return column_sums(partials)[:2]


MIXERS = ("vdn",)


def team_mixer(a):
    """The mixer of the env head under the config `a`: None (key absent, None, "" or "none": independent learners, no launch), or
    "vdn".  Anything else raises ValueError.  One predicate for run.setup, the learner and the loss launch."""
    raw = getattr(a, "mixer", None)
    if raw is None or (isinstance(raw, str) and raw in ("", "none")):
        return None
    if not isinstance(raw, str) or raw not in MIXERS:
        raise ValueError('mixer must be null (or "none") or "vdn", got %r' % (raw,))
    return raw


def td_sim_loss_grads(q_env, q_inc, tq_env, tq_inc, dens, batch, a, with_partials=False, mixer=None):
    """(dL/dq_env, dL/dq_inc, column sums of the per-row partials) of the loss
        (sum (td_env mask)^2 + sum (td_inc mask)^2) / dens[0] + sim_loss_weight * sum_sim / (1 + dens[1])
    from one launch (csrc/ssd_learner.hip: k_td_sim_loss / k_td_lambda_loss), WITHOUT an autograd node: the learner seeds the backward pass of the two Q tensors with the gradients directly (th.autograd.grad(..., grad_outputs=...)) --
    the loss scalar is a logged quantity only (_FusedLogs forms it when it is read), so the six scalar launches that assembled it and
    the two multiplications by d loss / d loss = 1 of the autograd form are gone.  Columns 13..15 of the partials are never read
    (13 / 14 are written only with td_lambda > 0: the rows' lambda-returns).  with_partials: the per-row partials as a fourth result
    (prioritised replay forms the samples' new priorities from columns 0, 2, 3: priority_update).  mixer (team_mixer(a); None: no
    second launch, nothing changes): "vdn" issues ssd_team_td directly behind the loss launch -- dq_env's seeds and column 2 become the
    team's (the sum over the agents of a (b, t)), every other output stays the loss launch's."""
    lib = abi.load_library()
    B, T, n = batch.batch_size, batch.max_seq_length - 1, q_env.shape[2]
    q_env, q_inc, tq_env, tq_inc = q_env.detach().contiguous(), q_inc.detach().contiguous(), tq_env.contiguous(), tq_inc.contiguous()
    partials = th.empty(B * T * n, abi.TD_LOSS_PARTIALS, dtype=th.float32, device=q_env.device)
    dq_env, dq_inc = th.empty_like(q_env), th.empty_like(q_inc)
    t, keep = _td_loss_args(batch, a, q_env.shape[-1], partials)
    t.q_env, t.q_inc, t.tq_env, t.tq_inc = q_env.data_ptr(), q_inc.data_ptr(), tq_env.data_ptr(), tq_inc.data_ptr()
    dens = dens.contiguous().float()
    t.dens, t.dq_env, t.dq_inc = dens.data_ptr(), dq_env.data_ptr(), dq_inc.data_ptr()
    abi.check(lib, lib.ssd_td_sim_loss(C.byref(t), 1, _stream(q_env)))
    if mixer is not None:
        if mixer not in MIXERS:
            raise ValueError("td_sim_loss_grads: mixer must be None or one of %r, got %r" % (MIXERS, mixer))
        # VDN: the team's TD error from the rows the loss launch just wrote, over the env head's seeds and column 2 (include/ssd_hip_mix.h),
        # in front of the column sums and of priority_update, which then read the team's numbers
        abi.check(lib, lib.ssd_team_td(C.byref(t), _stream(q_env)))
    if with_partials:
        return dq_env, dq_inc, column_sums(partials), partials
    return dq_env, dq_inc, column_sums(partials)


def fill_blocks(entries):
    """entries: (tensor, 32-bit pattern) pairs -> ONE ssd_fill_blocks launch for device tensors (contiguous, element size 4 or 8: an i64
    -1 is the pattern 0xFFFFFFFF twice); host tensors are filled one by one."""
    dev = [(t, v) for t, v in entries if t.is_cuda]
    for t, v in entries:
        if not t.is_cuda:
            t.fill_(-1 if v == 0xFFFFFFFF else 0)
            assert v in (0, 0xFFFFFFFF)
    if not dev:
        return
    lib = abi.load_library()
    for i in range(0, len(dev), abi.FILL_BLOCKS_MAX):
        part = dev[i:i + abi.FILL_BLOCKS_MAX]
        tab = (abi.SsdBlockFill * len(part))()
        for e, (t, v) in zip(tab, part):
            assert t.is_contiguous() and (t.numel() * t.element_size()) % 4 == 0
            e.dst, e.bytes, e.value = t.data_ptr(), t.numel() * t.element_size(), v
        abi.check(lib, lib.ssd_fill_blocks(tab, len(part), _stream(part[0][0])))


def runner_stats(collective_return, equality, episode_return, acc):
    """acc f64 [4] += [sum collective_return, sum equality, sum episode_return, sum episode_return^2] (EpisodeRunner's statistics of one
    rollout, episode_runner.py:121-152): one launch on the device."""
    if acc.is_cuda and all(t.is_cuda and t.dtype == th.float32 and t.is_contiguous() for t in (collective_return, equality, episode_return)):
        lib = abi.load_library()
        abi.check(lib, lib.ssd_runner_stats(collective_return.data_ptr(), equality.data_ptr(), episode_return.data_ptr(), collective_return.numel(),
                                            episode_return.numel(), acc.data_ptr(), _stream(acc)))
        return acc
    _leaving_kernels("runner_stats", acc, "dtype / layout")
    r = episode_return.to(th.float64)
    acc += th.stack([collective_return.sum(dtype=th.float64), equality.sum(dtype=th.float64), r.sum(), (r * r).sum()])
    return acc


def behaviour_workspace(n_agents, n_actions, device):
    """the int64 workspace of ssd_behaviour_stats: one row per workgroup"""
    return th.empty(abi.BEHAVIOUR_MAX_GROUPS, abi.behaviour_len(n_agents, n_actions), dtype=th.int64, device=device)


def behaviour_stats(actions, actions_inc, reward, clean_num, n_actions, acc, workspace=None):
    """acc f64 [abi.behaviour_len(n, A)] += the per-agent behaviour statistics of one rollout (ssd_behaviour_stats; blocks:
    abi.behaviour_layout): two launches on the device, integer accumulation.  The fields are those of an episode storage over T + 1
    slots -- actions i64 [N, T+1, n(, 1)], actions_inc i64 [N, T+1, n, n(, 1)], reward / clean_num f32 [N, T+1, n]; slot T is not read.
    workspace (device tensors): behaviour_workspace(n, A), allocated here when None."""
    if actions.dim() == 4:
        actions = actions.squeeze(-1)
    if actions_inc.dim() == 5:
        actions_inc = actions_inc.squeeze(-1)
    N, T1, n = actions.shape
    A = int(n_actions)
    assert actions_inc.shape == (N, T1, n, n) and reward.shape == (N, T1, n) and clean_num.shape == (N, T1, n)
    assert acc.dtype == th.float64 and acc.shape == (abi.behaviour_len(n, A),)
    fields = ((actions, th.int64), (actions_inc, th.int64), (reward, th.float32), (clean_num, th.float32))
    if acc.is_cuda and acc.is_contiguous() and all(t.is_cuda and t.dtype == d and t.is_contiguous() for t, d in fields):
        lib = abi.load_library()
        if workspace is None:
            workspace = behaviour_workspace(n, A, acc.device)
        assert workspace.is_cuda and workspace.dtype == th.int64 and workspace.is_contiguous() and workspace.numel() >= abi.BEHAVIOUR_MAX_GROUPS * acc.numel()
        a = abi.SsdBehaviourArgs(n_env=N, t_slots=T1, n_agents=n, n_actions=A, actions=actions.data_ptr(), actions_inc=actions_inc.data_ptr(),
                                 reward=reward.data_ptr(), clean_num=clean_num.data_ptr(), workspace=workspace.data_ptr(), acc=acc.data_ptr())
        abi.check(lib, lib.ssd_behaviour_stats(C.byref(a), _stream(acc)))
        return acc
    _leaving_kernels("behaviour_stats", acc, "dtype / layout")
    if N < 1 or T1 < 2 or not 1 <= n <= abi.MAX_AGENTS or not 1 <= A <= 16:
        raise ValueError("behaviour_stats: n_env >= 1, t_slots >= 2, n_agents 1..%d, n_actions 1..16" % abi.MAX_AGENTS)
    T, dev = T1 - 1, acc.device
    i64 = lambda x: x.to(th.int64)
    rnd = lambda x: i64(th.round(th.nan_to_num(x[:, :T].float(), nan=0.0).clamp(-16777216.0, 16777216.0)))
    act, r, c = i64(actions[:, :T]), rnd(reward), rnd(clean_num)
    inc = i64(actions_inc[:, :T])
    off = ~th.eye(n, dtype=th.bool, device=dev).view(1, 1, n, n)
    is_c = [((inc == k) & off) for k in range(3)]                       # [N, T, giver, receiver]
    rv = i64(is_c[1].sum(2)) - i64(is_c[2].sum(2))                      # per receiver
    cl, hv = i64(c > 0), i64(r > 0)
    t_idx = th.arange(T, dtype=th.int64, device=dev).view(1, T, 1)
    C_ep, H_ep = cl.sum(1), hv.sum(1)                                   # [N, n]
    role = th.where((C_ep == 0) & (H_ep == 0), 0, th.where(C_ep > H_ep, 1, th.where(H_ep > C_ep, 2, 3)))
    cleaners = (role == 1).sum(1)
    parts = [r.sum((0, 1)), c.sum((0, 1)), cl.sum((0, 1)), hv.sum((0, 1)), (hv * t_idx).sum((0, 1)),
             th.stack([i64(act == k).sum((0, 1)) for k in range(A)], dim=-1).reshape(-1),
             th.stack([i64(m).sum((0, 1)) for m in is_c], dim=-1).reshape(-1),
             (cl * rv).sum((0, 1)), (r * rv).sum((0, 1)),
             th.stack([i64(role == k).sum(0) for k in range(4)], dim=-1).reshape(-1),
             th.stack([i64(cleaners == k).sum() for k in range(n + 1)]),
             th.tensor([N, N * T], dtype=th.int64, device=dev)]
    acc += th.cat([i64(p).reshape(-1) for p in parts]).to(th.float64)
    return acc


REWARD_MODELS = {"inequity_aversion": abi.REWARD_IA, "prosocial": abi.REWARD_PROSOCIAL}


def reward_field(a):
    """The storage field the loss reads its reward from under the config `a`: "reward", or "reward_model" (the rollout's rewards shaped
    by social_reward) when the key reward_model names a model.  Observations, statistics and returns always read "reward"."""
    model = getattr(a, "reward_model", "individual")
    return "reward" if model is None or model == "individual" else "reward_model"


def social_reward_scalars(model, n_agents, ia_alpha=5.0, ia_beta=0.05, ia_decay=0.96525, prosocial_weight=0.5):
    """(p0, p1, p2) of ssd_social_reward as Python floats that hold f32 values: the keys rounded to f32, then one f32 operation each --
    inequity_aversion (alpha / (n - 1), beta / (n - 1), decay), prosocial (1 - rho, rho / (n - 1), 0).  Raises ValueError for a model,
    a team size or a key outside the ranges of include/ssd_hip_reward.h."""
    import numpy as np
    if not isinstance(model, str) or model not in REWARD_MODELS:
        raise ValueError('reward_model must be "individual", "inequity_aversion" or "prosocial", got %r' % (model,))
    if not 2 <= int(n_agents) <= abi.MAX_AGENTS:
        raise ValueError("reward_model %r needs n_agents 2 .. %d (a model compares an agent with the others), got %r" % (model, abi.MAX_AGENTS, n_agents))
    f, others = np.float32, np.float32(int(n_agents) - 1)
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if model == "inequity_aversion":
        for name, v in (("ia_alpha", ia_alpha), ("ia_beta", ia_beta)):
            if not num(v) or not 0.0 <= v < float("inf"):
                raise ValueError("%s must be a finite number >= 0, got %r" % (name, v))
        if not num(ia_decay) or not 0.0 <= ia_decay < 1.0 or not float(f(ia_decay)) < 1.0:
            raise ValueError("ia_decay must lie in [0, 1), got %r" % (ia_decay,))
        return float(f(ia_alpha) / others), float(f(ia_beta) / others), float(f(ia_decay))
    if not num(prosocial_weight) or not 0.0 <= prosocial_weight <= 1.0:
        raise ValueError("prosocial_weight must lie in [0, 1], got %r" % (prosocial_weight,))
    return float(f(1.0) - f(prosocial_weight)), float(f(prosocial_weight) / others), 0.0


def social_reward(reward, out, model, params, acc=None):
    """out = the rewards of a finished rollout shaped by a reward model (include/ssd_hip_reward.h, ssd_social_reward: the contract of
    the arithmetic and its order).  reward, out f32 [N, t_slots, n] with unit stride over the agents (views of a larger storage are
    fine: the env and slot strides are passed on), distinct memory; slot t_slots - 1 of out becomes 0.  model "inequity_aversion" or
    "prosocial"; params the three scalars of social_reward_scalars.  acc (optional) f64 [N, n, 3] contiguous: += the column sums over
    the slots.  Device tensors: one launch.  Host tensors: the same rule in f32 tensor operations in the stated order, equal to the bit."""
    if not isinstance(model, str) or model not in REWARD_MODELS:
        raise ValueError('ops.social_reward: model must be "inequity_aversion" or "prosocial", got %r' % (model,))
    if reward.dim() != 3 or reward.dtype != th.float32 or reward.stride(2) != 1:
        raise _unfit("social_reward", "reward", reward, "f32 [N, t_slots, n] with unit stride over the agents expected")
    N, T1, n = reward.shape
    if out.shape != reward.shape or out.dtype != th.float32 or out.device != reward.device or out.stride(2) != 1:
        raise _unfit("social_reward", "out", out, "f32 %s with unit stride over the agents on the device of reward expected" % ((N, T1, n),))
    if acc is not None and (acc.shape != (N, n, 3) or acc.dtype != th.float64 or acc.device != reward.device or not acc.is_contiguous()):
        raise _unfit("social_reward", "acc", acc, "contiguous f64 %s on the device of reward expected" % ((N, n, 3),))
    if N < 1 or T1 < 2 or not 2 <= n <= abi.MAX_AGENTS:
        raise _unfit("social_reward", "reward", reward, "n_env >= 1, t_slots >= 2, n_agents 2 .. %d" % abi.MAX_AGENTS)
    p0, p1, p2 = (float(p) for p in params)
    if reward.is_cuda:
        lib = abi.load_library()
        abi.check(lib, lib.ssd_social_reward(REWARD_MODELS[model], reward.data_ptr(), out.data_ptr(), acc.data_ptr() if acc is not None else None, N, T1, n,
                                             reward.stride(0), reward.stride(1), out.stride(0), out.stride(1), p0, p1, p2, _stream(reward)))
        return out
    if reward.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
        raise _unfit("social_reward", "out", out, "must not share memory with reward")
    s = lambda v: th.tensor(v, dtype=th.float32)
    p0, p1, p2 = s(p0), s(p1), s(p2)
    agents = th.arange(n).view(1, n)
    e = th.zeros(N, n)
    zero = th.zeros(())
    for t in range(T1 - 1):
        r = reward[:, t]
        first, third = th.zeros(N, n), th.zeros(N, n)
        if model == "inequity_aversion":
            e = p2 * e + r
            for j in range(n):
                ej = e[:, j:j + 1]
                first = th.where(agents == j, first, first + th.maximum(ej - e, zero))
                third = th.where(agents == j, third, third + th.maximum(e - ej, zero))
            second, third = p0 * first, p1 * third
            u = (r - second) - third
        else:
            for j in range(n):
                first = th.where(agents == j, first, first + r[:, j:j + 1])
            second = p1 * first
            u = p0 * r + second
        out[:, t] = u
        if acc is not None:
            acc += th.stack([u, second, third], dim=-1).to(th.float64)
    out[:, T1 - 1] = 0.0
    return out


def column_sums(x):
    """x [R, C] -> [C] or x [G, R, C] -> [G, C]: row sums by the HIP kernel k_column_sums (one launch, deterministic, no
    cross-workgroup hand-off).  ATen's multi-block reduction kernels keep block-arrival semaphores that a memset node clears; inside a
    captured hipGraph they were observed to return ANOTHER reduction's partial sums on MI355X / ROCm 7.2 once other work ran
    between two replays (diverging / NaN training runs) -- so nothing inside the captured train step reduces over rows with them."""
    if x.dim() < 2:
        raise _unfit("column_sums", "x", x, "[R, C] or [G, R, C] expected")
    if not (x.is_cuda and x.dtype == th.float32 and x.dim() <= 3):      # the kernel reads f32 [G, R, C]
        _leaving_kernels("column_sums", x, "dtype %s / rank %d" % (x.dtype, x.dim()))
        return x.sum(-2)
    lib = abi.load_library()
    x = x.contiguous()
    G = 1 if x.dim() == 2 else x.shape[0]
    R, Cc = x.shape[-2], x.shape[-1]
    out = th.empty((Cc,) if x.dim() == 2 else (G, Cc), dtype=th.float32, device=x.device)
    chunks = -(-R // abi.COLSUM_CHUNK)
    ws = th.empty(G, chunks, Cc, dtype=th.float32, device=x.device) if chunks > 1 else None
    abi.check(lib, lib.ssd_column_sums(x.data_ptr(), out.data_ptr(), G, R, Cc, None if ws is None else ws.data_ptr(), _stream(x)))
    return out


def _copy_blocks(entries, like):
    """entries: (src_ptr, dst_ptr, rows, cols, src_stride, dst_stride) -> ONE ssd_copy_blocks launch."""
    lib = abi.load_library()
    tab = (abi.SsdBlockCopy * len(entries))()
    for e, (src, dst, rows, cols, ss, ds) in zip(tab, entries):
        e.src, e.dst, e.rows, e.cols, e.src_stride, e.dst_stride = src, dst, rows, cols, ss, ds
    abi.check(lib, lib.ssd_copy_blocks(tab, len(entries), _stream(like)))


class _DuelingQ(th.autograd.Function):
    """q = v + a - mean_k a (homophily_agent.py:168-170, 203-207) from the layers' time-major rows straight into the batch layout
    [B, T, n, inner, K], one launch forward and one backward (ssd_dueling_q_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, a, v, B, T, inner):
        lib = abi.load_library()
        a, v = a.contiguous(), v.contiguous()
        n, K = a.shape[0], a.shape[-1]
        q = th.empty(B, T, n, inner, K, dtype=th.float32, device=a.device)
        abi.check(lib, lib.ssd_dueling_q_fwd(a.data_ptr(), v.data_ptr(), q.data_ptr(), n, T, B, inner, K, _stream(a)))
        ctx.dims = (n, T, B, inner, K)
        return q

    @staticmethod
    def backward(ctx, dq):
        lib = abi.load_library()
        n, T, B, inner, K = ctx.dims
        dq = dq.contiguous()
        da = th.empty(n, T * B * inner, K, dtype=th.float32, device=dq.device)
        dv = th.empty(n, T * B * inner, 1, dtype=th.float32, device=dq.device)
        abi.check(lib, lib.ssd_dueling_q_bwd(dq.data_ptr(), da.data_ptr(), dv.data_ptr(), n, T, B, inner, K, _stream(dq)))
        return da, dv, None, None, None


def dueling_q(a, v, B, T, inner):
    """a [n, T * B * inner, K] (rows (t * B + b) * inner + j), v [n, T * B * inner, 1] -> q = v + a - mean_k a as [B, T, n, K]
    (inner = 1) or [B, T, n, inner, K]."""
    n, K = a.shape[0], a.shape[-1]
    if a.dim() != 3 or a.shape[1] != T * B * inner:
        raise _unfit("dueling_q", "a", a, "[n, T * B * inner = %d, K] expected" % (T * B * inner))
    if v.shape != (n, T * B * inner, 1) or v.device != a.device:
        raise _unfit("dueling_q", "v", v, "%s on the device of a expected" % ((n, T * B * inner, 1),))
    if a.is_cuda and _f32_on(a, v) and K <= 16:
        q = _DuelingQ.apply(a, v, B, T, inner)
    else:
        _leaving_kernels("dueling_q", a, "K = %d > 16 or dtypes %s, %s" % (K, a.dtype, v.dtype))
        q = (v + a - a.mean(dim=-1, keepdim=True)).reshape(n, T, B, inner, K).permute(2, 1, 0, 3, 4)
    return q.reshape(B, T, n, K) if inner == 1 else q


class _DuelingHead(th.autograd.Function):
    """One dueling head of the learner's time-batched evaluation as TWO launches forward (the layer, the dueling combination) and three
    backward: w [n, in, K + 1] holds the advantage layer (columns 0..K-1) and the value layer (column K) side by side, b [n, 1, K + 1].
    other None (env head): rows = h [n, T * B, in].  other [T * B, inner, E] (incentive head): the layer input of row (tb, j) is
    [h[i, tb] | other[tb, j]] -- read from the two tensors where they are (ssd_bias_bmm2_fwd), never concatenated; backward, the
    gradient of h comes from the row-group sums the dueling backward emits (ssd_dueling_head_bwd gs -> ssd_bias_bmm_bwd_x)."""

    @staticmethod
    def forward(ctx, h, other, w, b, B, T, inner):
        lib = abi.load_library()
        h, w, b = h.contiguous(), w.contiguous(), b.contiguous()
        n, TB, H = h.shape
        K = w.shape[2] - 1
        st = _stream(h)
        y = th.empty(n, TB * inner, K + 1, dtype=th.float32, device=h.device)
        if other is None:
            assert inner == 1 and w.shape[1] == H
            abi.check(lib, lib.ssd_bias_bmm_fwd(h.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), n, TB, H, K + 1, st))
        else:
            other = other.contiguous()
            E = other.shape[-1]
            assert other.shape[0] == TB and other.shape[1] == inner and w.shape[1] == H + E
            abi.check(lib, lib.ssd_bias_bmm2_fwd(h.data_ptr(), other.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), n, TB * inner, H, E, K + 1,
                                                 inner, 1, st))
        q = th.empty((B, T, n, inner, K), dtype=th.float32, device=h.device)
        abi.check(lib, lib.ssd_dueling_head_fwd(y.data_ptr(), q.data_ptr(), n, T, B, inner, K, st))
        ctx.save_for_backward(h, w, *(() if other is None else (other,)))
        ctx.dims = (B, T, inner, K)
        ctx.precision = LEARNER_PRECISION
        return q

    @staticmethod
    def backward(ctx, dq):
        with _precision(ctx.precision):
            return _DuelingHead._backward(ctx, dq)

    @staticmethod
    def _backward(ctx, dq):
        lib = abi.load_library()
        h, w = ctx.saved_tensors[:2]
        other = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        B, T, inner, K = ctx.dims
        n, TB, H = h.shape
        st = _stream(h)
        dq = dq.contiguous()
        need = ctx.needs_input_grad
        dy = th.empty(n, TB * inner, K + 1, dtype=th.float32, device=h.device)
        two = other is not None
        gs = th.empty(n, TB, K + 1, dtype=th.float32, device=h.device) if (two and need[0]) else None
        abi.check(lib, lib.ssd_dueling_head_bwd(dq.data_ptr(), dy.data_ptr(), None if gs is None else gs.data_ptr(), n, T, B, inner, K, st))
        dw = th.empty_like(w) if need[2] else None
        db = th.empty(n, 1, K + 1, dtype=th.float32, device=h.device) if need[3] else None
        ptr = lambda t: None if t is None else t.data_ptr()
        dh = None
        if not two:
            dh = th.empty_like(h) if need[0] else None
            abi.check(lib, lib.ssd_bias_bmm_bwd(dy.data_ptr(), h.data_ptr(), w.data_ptr(), ptr(dh), ptr(dw), ptr(db), None, n, TB, H, K + 1, st))
        else:
            E = other.shape[-1]
            if dw is not None or db is not None:
                abi.check(lib, lib.ssd_bias_bmm2_bwd_w(dy.data_ptr(), h.data_ptr(), other.data_ptr(), ptr(dw), ptr(db), n, TB * inner, H, E, K + 1, inner, 1, st))
            if need[0]:
                dh = th.empty_like(h)
                abi.check(lib, lib.ssd_bias_bmm_bwd_x(gs.data_ptr(), w.data_ptr(), dh.data_ptr(), n, TB, H, K + 1, (H + E) * (K + 1), st))
        assert not need[1]       # no kernel emits dL/d other: dueling_head sends such a request to the tensor-op statement
        return dh, None, dw, db, None, None, None


def _dueling_head_fit(h, other, w, b, B, T, inner):
    """dueling_head's argument checks (ValueError naming the argument); True when the kernels take the call"""
    if h.dim() != 3 or h.shape[1] != T * B:
        raise _unfit("dueling_head", "h", h, "[n, T * B = %d, H] expected" % (T * B))
    n, TB, H = h.shape
    if other is not None and (other.dim() != 3 or tuple(other.shape[:2]) != (TB, inner) or other.device != h.device):
        raise _unfit("dueling_head", "other", other, "[T * B = %d, inner = %d, E] on the device of h expected" % (TB, inner))
    E = 0 if other is None else other.shape[-1]
    if w.dim() != 3 or tuple(w.shape[:2]) != (n, H + E) or w.shape[2] < 2 or w.device != h.device:
        raise _unfit("dueling_head", "w", w, "[n = %d, H (+ E) = %d, K + 1] on the device of h expected" % (n, H + E))
    K = w.shape[2] - 1
    if b.device != h.device:
        raise _unfit("dueling_head", "b", b, "the device of h expected")
    # the kernels: f32 throughout, b one row per weight set, the gradient of `other` not among those they emit
    return (h.is_cuda and _f32_on(h, w, b) and K <= 15 and H % 16 == 0 and b.shape == (n, 1, K + 1) and (other is not None or inner == 1)
            and (other is None or (other.dtype == th.float32 and E >= 1 and not (other.requires_grad and th.is_grad_enabled()))))


def dueling_head(h, other, w, b, B, T, inner):
    """q [B, T, n, K] (inner = 1, other None) or [B, T, n, inner, K] of one dueling head: h [n, T * B, H] the recurrence states (rows
    t * B + b), other [T * B, inner, E] or None, w [n, H (+ E), K + 1] = [advantage layer | value layer], b [n, 1, K + 1]."""
    fit = _dueling_head_fit(h, other, w, b, B, T, inner)
    n, TB, K = h.shape[0], h.shape[1], w.shape[2] - 1
    if fit:
        q = _DuelingHead.apply(h, other, w, b, B, T, inner)
    else:
        _leaving_kernels("dueling_head", h, "layout / dtypes / a bias that is not [n, 1, K + 1] / other requires a gradient")
        x = h if other is None else th.cat([h.unsqueeze(2).expand(n, TB, inner, h.shape[-1]), other.unsqueeze(0).expand(n, TB, inner, other.shape[-1])],
                                          dim=-1).reshape(n, TB * inner, -1)
        y = _baddbmm(b, x, w)
        a, v = y[..., :K], y[..., K:]
        q = (v + a - a.mean(dim=-1, keepdim=True)).reshape(n, T, B, inner, K).permute(2, 1, 0, 3, 4)
    return q.reshape(B, T, n, K) if inner == 1 else q


class _DuelingHeadPair(th.autograd.Function):
    """_DuelingHead of a live net (h, w, b: gradients as _DuelingHead) and of a second, frozen net (h_t, w_t, b_t: no gradient) on the same
    `other`, the layer of both as ONE launch and the dueling combination of both as one (ssd_bias_bmm_pair_fwd, ssd_dueling_head_pair_fwd):
    (q, q_t), each what _DuelingHead returns for its net alone, bit for bit.  Backward: _DuelingHead's, on the live operands."""

    @staticmethod
    def forward(ctx, h, other, w, b, B, T, inner, h_t, w_t, b_t):
        lib = abi.load_library()
        h, w, b, h_t, w_t, b_t = (t.contiguous() for t in (h, w, b, h_t, w_t, b_t))
        n, TB, H = h.shape
        n_t = h_t.shape[0]
        K = w.shape[2] - 1
        st = _stream(h)
        y = th.empty(n, TB * inner, K + 1, dtype=th.float32, device=h.device)
        y_t = th.empty(n_t, TB * inner, K + 1, dtype=th.float32, device=h.device)
        if other is None:
            assert inner == 1 and w.shape[1] == H
            abi.check(lib, lib.ssd_bias_bmm_pair_fwd(h.data_ptr(), None, w.data_ptr(), b.data_ptr(), y.data_ptr(), n, h_t.data_ptr(), None, w_t.data_ptr(),
                                                     b_t.data_ptr(), y_t.data_ptr(), n_t, TB, H, 0, K + 1, 1, 0, 0, st))
        else:
            other = other.contiguous()
            E = other.shape[-1]
            assert other.shape[0] == TB and other.shape[1] == inner and w.shape[1] == H + E
            abi.check(lib, lib.ssd_bias_bmm_pair_fwd(h.data_ptr(), other.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), n, h_t.data_ptr(), other.data_ptr(),
                                                     w_t.data_ptr(), b_t.data_ptr(), y_t.data_ptr(), n_t, TB * inner, H, E, K + 1, inner, 1, 0, st))
        q = th.empty((B, T, n, inner, K), dtype=th.float32, device=h.device)
        q_t = th.empty((B, T, n_t, inner, K), dtype=th.float32, device=h.device)
        abi.check(lib, lib.ssd_dueling_head_pair_fwd(y.data_ptr(), q.data_ptr(), n, y_t.data_ptr(), q_t.data_ptr(), n_t, T, B, inner, K, st))
        ctx.save_for_backward(h, w, *(() if other is None else (other,)))
        ctx.dims = (B, T, inner, K)
        ctx.precision = LEARNER_PRECISION
        ctx.mark_non_differentiable(q_t)
        ctx.set_materialize_grads(False)         # (no zero-filled gradient for q_t: a launch per backward otherwise)
        return q, q_t

    @staticmethod
    def backward(ctx, dq, dq_t):
        if dq is None:
            return (None,) * 10
        with _precision(ctx.precision):
            return _DuelingHead._backward(ctx, dq) + (None, None, None)


def dueling_head_pair(h, other, w, b, h_t, w_t, b_t, B, T, inner):
    """(dueling_head(h, other, w, b, ...), dueling_head(h_t, other, w_t, b_t, ...) without a gradient): a live net and a frozen copy
    (the learner's target network) on the same batch.  On the device both go out together: one launch for the layer of both, one for
    the dueling combination of both; anywhere else, or when the second net asks for a gradient, the two calls one after the other."""
    fit = _dueling_head_fit(h, other, w, b, B, T, inner)
    frozen = not (th.is_grad_enabled() and (h_t.requires_grad or w_t.requires_grad or b_t.requires_grad))
    if (fit and frozen and _dueling_head_fit(h_t, other, w_t, b_t, B, T, inner) and h_t.device == h.device
            and tuple(h_t.shape[1:]) == tuple(h.shape[1:]) and tuple(w_t.shape[1:]) == tuple(w.shape[1:])):
        q, q_t = _DuelingHeadPair.apply(h, other, w, b, B, T, inner, h_t, w_t, b_t)
        K = w.shape[2] - 1
        return (q.reshape(B, T, h.shape[0], K), q_t.reshape(B, T, h_t.shape[0], K)) if inner == 1 else (q, q_t)
    q = dueling_head(h, other, w, b, B, T, inner)
    with th.no_grad() if frozen else th.enable_grad():
        q_t = dueling_head(h_t, other, w_t, b_t, B, T, inner)
    return q, q_t


def _mix32p(x):
    x &= 0xFFFFFFFF
    x ^= x >> 17; x = (x * 0xed5ad4bb) & 0xFFFFFFFF; x ^= x >> 11; x = (x * 0xac4c1b51) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x31848bab) & 0xFFFFFFFF; x ^= x >> 14
    return x


def _sample_draw(seed, call, i):
    s0, s1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    x = _mix32p(s0 ^ ((call * 0x9E3779B9) & 0xFFFFFFFF))
    return _mix32p(x ^ ((s1 + i * 0x85EBCA6B) & 0xFFFFFFFF))


def sample_ids(seed, call, population, count, out):
    """out[0 .. count) (int64) = `count` distinct indices drawn uniformly from [0, population): the replay buffer's
    np.random.choice(population, count, replace=False) (episode_buffer.py:240-244) as a counter generator keyed by (seed, call).
    Device tensor: one launch (ssd_sample_ids), nothing crosses the host boundary.  Host tensor: the same arithmetic restated
    (Floyd's subset sampling, then Fisher-Yates over the picks), so both give the same ids."""
    assert out.dtype == th.long and out.numel() >= count and 1 <= count <= population
    if out.is_cuda:
        lib = abi.load_library()
        abi.check(lib, lib.ssd_sample_ids(seed & (2 ** 64 - 1), call & 0xFFFFFFFF, population, count, out.data_ptr(), _stream(out)))
        return out
    ids = []
    for i in range(count):
        j = population - count + i
        t = (_sample_draw(seed, call & 0xFFFFFFFF, i) * (j + 1)) >> 32
        ids.append(j if t in ids else t)
    for i in range(count - 1, 0, -1):
        k = (_sample_draw(seed, call & 0xFFFFFFFF, count + i) * (i + 1)) >> 32
        ids[i], ids[k] = ids[k], ids[i]
    out[:count] = th.tensor(ids, dtype=th.long)
    return out


def gather_rows(pairs, ids):
    """dst[e] = src[ids[e]] along axis 0 for every (src, dst) pair of contiguous device tensors, as ONE launch (ssd_gather_rows).
    ids: int64 device tensor.  Returns False (nothing done) when a pair does not qualify -- the caller indexes field by field."""
    if not pairs or len(pairs) > abi.COPY_BLOCKS_MAX or not ids.is_cuda or ids.dtype != th.long:
        return False
    n = ids.numel()
    if n < 1 or n > 65535:                      # the launch's grid-z limit: the caller indexes field by field
        return False
    for src, dst in pairs:
        if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype
                and dst.shape[0] == n and dst.shape[1:] == src.shape[1:] and src[0].numel() > 0):
            return False
    lib = abi.load_library()
    tab = (abi.SsdRowGather * len(pairs))()
    for e, (src, dst) in zip(tab, pairs):
        e.src, e.dst, e.row_bytes = src.data_ptr(), dst.data_ptr(), src[0].numel() * src.element_size()
    abi.check(lib, lib.ssd_gather_rows(tab, len(pairs), ids.contiguous().data_ptr(), n, _stream(ids)))
    return True


def sample_windows(seed, call, population, count, n_starts, ids_out, t0_out):
    """ids_out[0 .. count) as sample_ids gives them for the same (seed, call, population, count), and t0_out[e] uniform on
    [0, n_starts) from the draws the ids do not use: t0[e] = floor(draw(2 count + e) n_starts / 2^32) (include/ssd_hip.h:
    ssd_sample_windows).  Device tensors: ONE launch.  Host tensors: the same arithmetic restated.  Returns (ids_out, t0_out)."""
    assert ids_out.dtype == th.long and t0_out.dtype == th.long and ids_out.numel() >= count and t0_out.numel() >= count
    assert 1 <= count <= population and n_starts >= 1 and ids_out.is_cuda == t0_out.is_cuda
    if ids_out.is_cuda:
        assert ids_out.is_contiguous() and t0_out.is_contiguous()
        lib = abi.load_library()
        abi.check(lib, lib.ssd_sample_windows(seed & (2 ** 64 - 1), call & 0xFFFFFFFF, population, count, n_starts, ids_out.data_ptr(),
                                              t0_out.data_ptr(), _stream(ids_out)))
        return ids_out, t0_out
    sample_ids(seed, call, population, count, ids_out)
    t0_out[:count] = th.tensor([(_sample_draw(seed, call & 0xFFFFFFFF, 2 * count + e) * n_starts) >> 32 for e in range(count)], dtype=th.long)
    return ids_out, t0_out


def gather_windows(pairs, ids, t0, src_slots, win_slots, burn_in, filled_index):
    """dst[e] = src[ids[e], t0[e] : t0[e] + win_slots] for every (src, dst) pair of contiguous device tensors [rows, src_slots, ...] ->
    [len(ids), win_slots, ...], as ONE launch (ssd_gather_windows); pair number filled_index (None: no such pair) is the int64
    `filled` mask and is written with the burn-in rule dst[e, r] = src[..] * (r >= K_e), K_e = burn_in if t0[e] > 0 else 0.
    ids, t0: int64 device tensors; the caller guarantees ids within the rows and t0 + win_slots <= src_slots.
    Returns False (nothing done) when a pair does not qualify -- the caller indexes field by field."""
    if not pairs or len(pairs) > abi.COPY_BLOCKS_MAX or not (ids.is_cuda and t0.is_cuda) or ids.dtype != th.long or t0.dtype != th.long:
        return False
    n = ids.numel()
    if n < 1 or n > 65535 or t0.numel() != n or not 2 <= win_slots <= src_slots or not 0 <= burn_in <= win_slots - 2:
        return False
    for k, (src, dst) in enumerate(pairs):
        if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype and src.dim() >= 2
                and src.shape[1] == src_slots and tuple(dst.shape[:2]) == (n, win_slots) and dst.shape[2:] == src.shape[2:] and src[0, 0].numel() > 0):
            return False
        if k == filled_index and not (src.dtype == th.long and src[0, 0].numel() == 1):
            return False
    lib = abi.load_library()
    tab = (abi.SsdWindowField * len(pairs))()
    for k, (e, (src, dst)) in enumerate(zip(tab, pairs)):
        e.src, e.dst, e.slot_bytes, e.filled = src.data_ptr(), dst.data_ptr(), src[0, 0].numel() * src.element_size(), int(k == filled_index)
    abi.check(lib, lib.ssd_gather_windows(tab, len(pairs), ids.contiguous().data_ptr(), t0.contiguous().data_ptr(), n, src_slots, win_slots,
                                          burn_in, _stream(ids)))
    return True


def store_hidden_args(t_index, h_env, h_inc, dst):
    """The argument block of ssd_store_hidden (include/ssd_hip.h) for a rollout's static tensors: the recurrent states h_env / h_inc,
    agent-major [n, N, 64] (FastPolicy) or [N, n, 1, 64] (the generic timestep), filed as dst[:, *t_index] of the episode field
    "hidden" f32 [N, t_slots, n, 128] = [h_env | h_inc] -- the state AFTER the controller consumed slot t.  t_index: int64 device scalar.
    The block holds raw addresses: the caller keeps the tensors alive (the runner's per-storage bundle)."""
    if dst.dim() != 4 or dst.shape[3] != 128 or dst.dtype != th.float32 or not dst.is_cuda or not dst.is_contiguous():
        raise _unfit("store_hidden", "dst", dst, "contiguous f32 [N, t_slots, n, 128] on the device expected")
    N, slots, n = dst.shape[:3]
    if t_index.dtype != th.long or t_index.numel() != 1 or t_index.device != dst.device:
        raise _unfit("store_hidden", "t_index", t_index, "one int64 on the device of dst expected")
    a = abi.SsdStoreHiddenArgs()
    for name, h in (("h_env", h_env), ("h_inc", h_inc)):
        if h.dtype != th.float32 or h.device != dst.device or h.shape[-1] != 64 or h.stride(-1) != 1:
            raise _unfit("store_hidden", name, h, "f32 [n, N, 64] or [N, n, 1, 64] on the device of dst expected")
        if h.dim() == 3 and tuple(h.shape[:2]) == (n, N):
            strides = (h.stride(0), h.stride(1))
        elif h.dim() == 4 and tuple(h.shape[:3]) == (N, n, 1):
            strides = (h.stride(1), h.stride(0))
        else:
            raise _unfit("store_hidden", name, h, "f32 [n = %d, N = %d, 64] or [N, n, 1, 64] expected" % (n, N))
        if name == "h_inc" and strides != (a.src_agent_stride, a.src_env_stride):
            raise _unfit("store_hidden", name, h, "the layout of h_env expected")
        a.src_agent_stride, a.src_env_stride = strides
    a.t_index, a.n_env, a.n_agents, a.t_slots = t_index.data_ptr(), N, n, slots
    a.h_env, a.h_inc, a.dst = h_env.data_ptr(), h_inc.data_ptr(), dst.data_ptr()
    return a


def store_hidden(args, device):
    """one ssd_store_hidden launch of the block store_hidden_args built, on the current stream of `device`"""
    lib = abi.load_library()
    abi.check(lib, lib.ssd_store_hidden(C.byref(args), th.cuda.current_stream(device).cuda_stream))


def rollout_priority_args(t_index, q_env, q_inc, agent_major, avail_bits, store, constants, alpha, eta, eps, windows=None):
    """The argument block of ssd_rollout_priority (include/ssd_hip.h) for a rollout's static tensors, and the state it owns.
    q_env / q_inc: the heads' Q-values of the current slot; agent_major says which layout they have -- True: f32 [n, N, A] /
    [n, N, n, 3] (FastPolicy's q_out), False: env-major [N, n, A] / [N, n, n, 3] (the generic timestep).  The caller states the layout:
    with N == n the shapes cannot tell.  store: the transition data of the episode storage being written (actions,
    actions_inc, reward [N, T + 1, n], terminated, filled); constants: td_constants(...); t_index: int64 device scalar.
    Returns (args, keep): keep holds carry f32 [N, n, 2], acc f32 [N, n, 3] and q_init int32 [N] plus every tensor the block points
    to -- the block holds raw addresses, the caller keeps `keep` alive (the runner's per-storage bundle).
    windows = (S, L, s, K): a priority per training window of the grid window_grid(T, L, s) under burn-in K (k_rollout_priority_seq):
    acc is f32 [N, n, S, 3] and q_init int32 [N, S]."""
    reward = store["reward"]
    if reward.dim() != 3 or reward.dtype != th.float32 or not reward.is_cuda or not reward.is_contiguous():
        raise _unfit("rollout_priority", "reward", reward, "contiguous f32 [N, t_slots, n] on the device expected (ind_reward)")
    N, slots, n = reward.shape
    dev = reward.device
    if t_index.dtype != th.long or t_index.numel() != 1 or t_index.device != dev:
        raise _unfit("rollout_priority", "t_index", t_index, "one int64 on the device of the storage expected")
    fields = (("actions", th.long, N * slots * n), ("actions_inc", th.long, N * slots * n * n), ("terminated", th.uint8, N * slots),
              ("filled", th.long, N * slots))
    for name, dtype, count in fields:
        f = store[name]
        if f.dtype != dtype or f.device != dev or not f.is_contiguous() or f.numel() != count or f.shape[:2] != (N, slots):
            raise _unfit("rollout_priority", name, f, "contiguous %s of %d elements [N = %d, t_slots = %d, ...] on the device of reward expected" % (dtype, count, N, slots))
    a = abi.SsdRolloutPriorityArgs()
    for name, q, inner in (("q_env", q_env, None), ("q_inc", q_inc, (n, 3))):
        if q.dtype != th.float32 or q.device != dev or q.stride(-1) != 1:
            raise _unfit("rollout_priority", name, q, "f32 agent-major [n, N, ...] or env-major [N, n, ...] on the device of the storage expected")
        tail = tuple(q.shape[2:])
        if (inner is None and len(tail) != 1) or (inner is not None and (tail != inner or not q[0, 0].is_contiguous())):
            raise _unfit("rollout_priority", name, q, "rows [A] (q_env) or contiguous [n, 3] (q_inc) per (env, agent) expected")
        if tuple(q.shape[:2]) != ((n, N) if agent_major else (N, n)):
            raise _unfit("rollout_priority", name, q, "%s expected" % ("agent-major [n = %d, N = %d, ...]" % (n, N) if agent_major else
                                                                      "env-major [N = %d, n = %d, ...]" % (N, n)))
        strides = (q.stride(0), q.stride(1)) if agent_major else (q.stride(1), q.stride(0))       # (agent, env), elements
        if name == "q_env":
            a.q_env_agent_stride, a.q_env_env_stride = strides
        else:
            a.q_inc_agent_stride, a.q_inc_env_stride = strides
    A = q_env.shape[2]
    if windows is not None:
        S, L, stride, K = (int(v) for v in windows)
        if not 1 <= L <= slots - 1 or (S, stride) != window_grid(slots - 1, L, stride or -1)[:2] or S > abi.PRIORITY_SEGMENTS_MAX or -(-L // stride) > 8 or not 0 <= K < L:
            raise ValueError("ops.rollout_priority_args: windows %r is not (S, L, s, K) of a grid over %d transitions with S <= PRIORITY_SEGMENTS_MAX, "
                             "ceil(L / s) <= 8 and 0 <= K < L" % (tuple(windows), slots - 1))
        a.n_segments, a.win_len, a.seg_stride, a.burn_in = S, L, stride, K
    acc_shape, q_shape = ((N, n, 3), (N,)) if windows is None else ((N, n, S, 3), (N, S))
    keep = dict(t_index=t_index, q_env=q_env, q_inc=q_inc, carry=th.zeros(N, n, 2, device=dev), acc=th.zeros(acc_shape, device=dev),
                q_init=th.zeros(q_shape, dtype=th.int32, device=dev), **{name: store[name] for name, _, _ in fields}, reward=reward)
    a.t_index, a.n_env, a.n_agents, a.n_actions, a.t_slots, a.avail_bits = t_index.data_ptr(), N, n, A, slots, int(avail_bits) & 0xFFFFFFFF
    for k, v in constants.items():
        setattr(a, k, v)
    a.alpha, a.eta, a.eps = float(alpha), float(eta), float(eps)
    for k in ("q_env", "q_inc", "actions", "actions_inc", "reward", "terminated", "filled", "carry", "acc", "q_init"):
        setattr(a, k, keep[k].data_ptr())
    return a, keep


def rollout_priority(args, device):
    """one ssd_rollout_priority launch of the block rollout_priority_args built, on the current stream of `device`"""
    lib = abi.load_library()
    abi.check(lib, lib.ssd_rollout_priority(C.byref(args), th.cuda.current_stream(device).cuda_stream))


def copy_blocks(pairs):
    """dst <- src for every (src, dst) pair of contiguous device tensors of 4-byte elements and equal size, as ONE launch
    (ssd_copy_blocks; at most COPY_BLOCKS_MAX pairs of under 2^31 elements)."""
    if not pairs or len(pairs) > abi.COPY_BLOCKS_MAX:
        raise ValueError("ops.copy_blocks: %d pairs outside 1 .. COPY_BLOCKS_MAX = %d" % (len(pairs), abi.COPY_BLOCKS_MAX))
    for src, dst in pairs:
        if not (src.is_cuda and dst.device == src.device and src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype
                and src.element_size() == 4 and 0 < src.numel() == dst.numel() < 2 ** 31):
            raise _unfit("copy_blocks", "src", src, "contiguous device tensors of 4-byte elements, equal dtype and size expected (dst %s %s on %s)"
                         % (tuple(dst.shape), dst.dtype, dst.device))
    _copy_blocks([(s.data_ptr(), d.data_ptr(), 1, s.numel(), s.numel(), s.numel()) for s, d in pairs], pairs[0][0])


def window_grid(episode_limit, window, stride=0):
    """The window grid of a priority per training window (per_unit "window"; include/ssd_hip.h: ssd_priority_sample): (S, s, last_start)
    for episodes of T = episode_limit transitions and windows of L = `window`.  s = stride, or (L + 1) // 2 -- R2D2's half overlap -- for
    0; S = ceil((T - L) / s) + 1 windows, window k starting at min(k s, T - L): the last one is clamped so that the episode's tail is
    covered.  Raises ValueError outside 1 <= L <= T, 1 <= s <= L (a larger stride would leave gaps)."""
    T, L = int(episode_limit), int(window)
    s = int(stride) or (L + 1) // 2
    if not 1 <= L <= T or not 1 <= s <= L:
        raise ValueError("window_grid: window %r outside 1 .. %r, or stride %r outside 1 .. window" % (window, episode_limit, s))
    return -(-(T - L) // s) + 1, s, T - L


def window_starts(segments):
    """[start_0 .. start_{S - 1}] of segments = (S, s, last_start)"""
    S, s, last = segments
    return [min(k * s, last) for k in range(S)]


def priority_sample(seed, call, table, population, count, n_starts, beta, ids_out, t0_out, weights_out, log_out, segments=None, entries_out=None):
    """Prioritised replay's draw (include/ssd_hip.h: ssd_priority_sample): `count` stratified proportional draws with replacement from
    the fixed-point priorities table[0 .. population) (int32 storage of the u32 values; 0 = never trained on, drawn at the table's
    maximum), one window start each, and the importance weights (population qeff / total)^(-beta) divided by their maximum.
    ids_out, t0_out: int64 [count]; weights_out: f32 [count]; log_out: f32 [4] = mean and max of qeff / PRIORITY_ONE, the smallest
    weight, the number of distinct ids.  Device tensors: ONE launch.  Host tensors: the same arithmetic restated -- Python integers
    for the draw, float64 then f32 for the weights.  Returns (ids_out, t0_out, weights_out, log_out).
    segments = (S, s, last_start) (window_grid) with entries_out int64 [count]: a priority per window -- the table holds S entries per
    slot, `population` counts entries, the same draw runs over entries (entries_out; log[3] counts distinct entries) and every entry f
    gives ids = f // S, t0 = min((f % S) s, last_start); n_starts is not read and no start is drawn."""
    outs = (ids_out, t0_out, weights_out, log_out)
    if segments is not None:
        S, stride, last = (int(v) for v in segments)
        if not (1 <= S <= abi.PRIORITY_SEGMENTS_MAX and stride >= 1 and last >= 0 and (S - 1) * stride >= last and population % S == 0):
            raise ValueError("ops.priority_sample: segments %r: S outside 1 .. PRIORITY_SEGMENTS_MAX, stride < 1, last_start < 0, a grid that does not "
                             "reach last_start, or population %r no multiple of S" % (tuple(segments), population))
        if entries_out is None or entries_out.dtype != th.long or entries_out.numel() < count or entries_out.device != table.device or not entries_out.is_contiguous():
            raise _unfit("priority_sample", "entries_out", entries_out if entries_out is not None else table, "contiguous int64 entries_out of count elements on the table's device expected with segments")
    if not (table.dtype == th.int32 and ids_out.dtype == th.long and t0_out.dtype == th.long and weights_out.dtype == th.float32 and log_out.dtype == th.float32):
        raise _unfit("priority_sample", "table", table, "int32 table, int64 ids / t0 and f32 weights / log expected")
    if not (1 <= population <= min(table.numel(), abi.PRIORITY_POP_MAX) and 1 <= count <= abi.SAMPLE_IDS_MAX and n_starts >= 1 and 0.0 <= beta <= 1.0):
        raise ValueError("ops.priority_sample: population %r outside 1 .. min(len(table), PRIORITY_POP_MAX), count %r outside 1 .. SAMPLE_IDS_MAX, "
                         "n_starts %r < 1 or beta %r outside [0, 1]" % (population, count, n_starts, beta))
    if min(ids_out.numel(), t0_out.numel(), weights_out.numel()) < count or log_out.numel() < 4 or any(t.device != table.device or not t.is_contiguous() for t in outs + (table,)):
        raise _unfit("priority_sample", "ids_out", ids_out, "contiguous outputs of count elements (log: 4) on the table's device expected")
    if table.is_cuda:
        lib = abi.load_library()
        t = abi.SsdPrioritySampleArgs()
        t.seed, t.call, t.population, t.count, t.n_starts, t.beta = seed & (2 ** 64 - 1), call & 0xFFFFFFFF, population, count, n_starts, float(beta)
        t.table, t.ids, t.t0, t.weights, t.log = table.data_ptr(), ids_out.data_ptr(), t0_out.data_ptr(), weights_out.data_ptr(), log_out.data_ptr()
        if segments is not None:
            t.n_segments, t.seg_stride, t.last_start, t.entries = S, stride, last, entries_out.data_ptr()
        abi.check(lib, lib.ssd_priority_sample(C.byref(t), _stream(table)))
        return outs
    import bisect
    import itertools
    q = [int(v) for v in table[:population].tolist()]
    qmax = max(q) or abi.PRIORITY_ONE
    qeff = [v or qmax for v in q]
    cum = list(itertools.accumulate(qeff))
    total, call = cum[-1], call & 0xFFFFFFFF
    ids = []
    for e in range(count):
        lo, hi = total * e // count, total * (e + 1) // count
        x = lo + ((_sample_draw(seed, call, e) * (hi - lo)) >> 32)
        ids.append(bisect.bisect_right(cum, x))                      # the smallest k with cum[k] > x
    if segments is not None:                                         # ids are entries: the slot and the window start of each
        entries_out[:count] = th.tensor(ids, dtype=th.long)
        ids_out[:count] = th.tensor([f // S for f in ids], dtype=th.long)
        starts = window_starts((S, stride, last))
        t0_out[:count] = th.tensor([starts[f % S] for f in ids], dtype=th.long)
    else:
        ids_out[:count] = th.tensor(ids, dtype=th.long)
        t0_out[:count] = th.tensor([(_sample_draw(seed, call, 2 * count + e) * n_starts) >> 32 for e in range(count)], dtype=th.long)
    w = th.tensor([population * qeff[k] / total for k in ids], dtype=th.float64) ** (-float(beta))
    w = (w / w.max()).float()
    weights_out[:count] = w
    log_out[:4] = th.tensor([total / population / abi.PRIORITY_ONE, max(qeff) / abi.PRIORITY_ONE, float(w.min()), float(len(set(ids)))], dtype=th.float32)
    return outs


def priority_update(partials, ids, weights, dq_env, dq_inc, q_new, table, alpha, eta, eps):
    """Prioritised replay's train-step half (include/ssd_hip.h: ssd_priority_update), after the loss launch that wrote `partials`
    [B T n, TD_LOSS_PARTIALS] and the gradient seeds dq_env [B, T + 1, n, A] / dq_inc [B, T + 1, n, n, 3]:
      q_new[e] = clamp(round(p^alpha PRIORITY_ONE), 1, PRIORITY_MAX),  p = eta max d + (1 - eta) sum d / max(1, sum col0) + eps over the
      sample's rows, d = sqrt(col2 + col3);  dq_env[e], dq_inc[e] *= weights[e] in place;  table[ids[e]] = the largest q_new among the
      samples of that id (an id outside the table is skipped).
    Device tensors: two launches.  Host tensors: the same arithmetic in float64 (the scaling is the one f32 multiply).  Returns q_new."""
    B, T1, n, A = dq_env.shape
    if not (partials.dtype == th.float32 and weights.dtype == th.float32 and dq_env.dtype == th.float32 and dq_inc.dtype == th.float32
            and ids.dtype == th.long and q_new.dtype == th.int32 and table.dtype == th.int32):
        raise _unfit("priority_update", "partials", partials, "f32 partials / weights / dq, int64 ids, int32 q_new / table expected")
    if not (tuple(dq_inc.shape) == (B, T1, n, n, 3) and tuple(partials.shape) == (B * (T1 - 1) * n, abi.TD_LOSS_PARTIALS) and T1 >= 2
            and 1 <= B <= abi.SAMPLE_IDS_MAX and min(ids.numel(), weights.numel(), q_new.numel()) >= B and 1 <= table.numel() <= abi.PRIORITY_POP_MAX):
        raise _unfit("priority_update", "dq_inc", dq_inc, "shapes that do not belong to one batch of 1 .. SAMPLE_IDS_MAX samples")
    if not (0.0 <= alpha <= 1.0 and 0.0 <= eta <= 1.0 and eps > 0.0):
        raise ValueError("ops.priority_update: alpha %r or eta %r outside [0, 1], or eps %r <= 0" % (alpha, eta, eps))
    every = (partials, ids, weights, dq_env, dq_inc, q_new, table)
    if any(t.device != table.device or not t.is_contiguous() for t in every):
        raise _unfit("priority_update", "table", table, "contiguous tensors on one device expected")
    if table.is_cuda:
        lib = abi.load_library()
        t = abi.SsdPriorityUpdateArgs()
        t.batch, t.t_slots, t.n_agents, t.n_actions, t.table_len = B, T1, n, A, table.numel()
        t.alpha, t.eta, t.eps = float(alpha), float(eta), float(eps)
        t.partials, t.ids, t.weights, t.dq_env, t.dq_inc = partials.data_ptr(), ids.data_ptr(), weights.data_ptr(), dq_env.data_ptr(), dq_inc.data_ptr()
        t.q_new, t.table = q_new.data_ptr(), table.data_ptr()
        abi.check(lib, lib.ssd_priority_update(C.byref(t), _stream(table)))
        return q_new
    rows = partials.double().reshape(B, (T1 - 1) * n, -1)
    d = (rows[..., 2] + rows[..., 3]).sqrt()
    p = eta * d.max(dim=1)[0] + (1.0 - eta) * d.sum(dim=1) / rows[..., 0].sum(dim=1).clamp_min(1.0) + eps
    q = th.nan_to_num((p ** alpha * abi.PRIORITY_ONE).round(), nan=float(abi.PRIORITY_MAX)).clamp(1, abi.PRIORITY_MAX).to(th.int32)
    q_new[:B] = q
    dq_env.mul_(weights[:B].reshape(B, 1, 1, 1))
    dq_inc.mul_(weights[:B].reshape(B, 1, 1, 1, 1))
    best = {}
    for e, k in enumerate(ids[:B].tolist()):
        if 0 <= k < table.numel():
            best[k] = max(best.get(k, 0), int(q[e]))
    for k, v in best.items():
        table[k] = v
    return q_new


class _CatGroups(th.autograd.Function):
    """Several last-axis concatenations as ONE launch (ssd_copy_blocks), their gradients split again by ONE launch into contiguous
    per-input tensors -- what th.cat + CatBackward + the flattening of its strided gradient views do with one launch per tensor."""

    @staticmethod
    def forward(ctx, sizes, *tensors):
        ctx.sizes, ctx.shapes = sizes, [t.shape for t in tensors]
        tensors = [t.contiguous() for t in tensors]
        outs, entries, k = [], [], 0
        for cnt in sizes:
            grp = tensors[k:k + cnt]
            k += cnt
            total = sum(t.shape[-1] for t in grp)
            out = th.empty(grp[0].shape[:-1] + (total,), dtype=th.float32, device=grp[0].device)
            col = 0
            for t in grp:
                c = t.shape[-1]
                entries.append((t.data_ptr(), out.data_ptr() + 4 * col, t.numel() // c, c, c, total))
                col += c
            outs.append(out)
        _copy_blocks(entries, tensors[0])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        dev = next(g for g in grads if g is not None).device
        k = 0
        full = []
        for cnt, g in zip(ctx.sizes, grads):      # an unused output has no gradient: zeros
            if g is None:
                sh = ctx.shapes[k]
                g = th.zeros(tuple(sh[:-1]) + (sum(s_[-1] for s_ in ctx.shapes[k:k + cnt]),), dtype=th.float32, device=dev)
            full.append(g.contiguous())
            k += cnt
        grads = full
        flat = th.empty(sum(int(th.Size(sh).numel()) for sh in ctx.shapes), dtype=th.float32, device=dev)
        res, entries, k, off = [], [], 0, 0
        for cnt, g in zip(ctx.sizes, grads):
            total, col = g.shape[-1], 0
            for sh in ctx.shapes[k:k + cnt]:
                c, numel = sh[-1], int(th.Size(sh).numel())
                d = flat[off:off + numel]
                entries.append((g.data_ptr() + 4 * col, d.data_ptr(), numel // c, c, total, c))
                res.append(d.view(sh))
                col += c
                off += numel
            k += cnt
        _copy_blocks(entries, flat)
        return (None,) + tuple(res)


def cat_groups(groups):
    """[th.cat(g, dim=-1) for g in groups] for f32 tensors whose leading axes agree within a group.  On the device (at most
    abi.COPY_BLOCKS_MAX tensors): one launch forward, one backward, contiguous gradients."""
    flat = [t for g in groups for t in g]
    if (flat[0].is_cuda and len(flat) <= abi.COPY_BLOCKS_MAX and all(t.dtype == th.float32 and t.is_cuda for t in flat)
            and all(t.shape[:-1] == g[0].shape[:-1] for g in groups for t in g)):
        return list(_CatGroups.apply(tuple(len(g) for g in groups), *flat))
    _leaving_kernels("cat_groups", flat[0], "%d tensors / dtypes / leading axes" % len(flat))
    return [th.cat(list(g), dim=-1) for g in groups]


def _baddbmm(b, x, w):
    """th.baddbmm(b, x, w), the tensor-op statement of the affine layers, in the operands' common dtype (baddbmm itself refuses mixed ones)"""
    dt = th.promote_types(th.promote_types(b.dtype, x.dtype), w.dtype)
    return th.baddbmm(b.to(dt), x.to(dt), w.to(dt))


def _bmm_kernel_ok(x, w, b):
    """ssd_bias_bmm_*: f32 x [n, R, I], w [n, I, O], b [n, 1, O] on one device -- the kernel reads w + g * I * O and b + g * O; any
    other bias baddbmm broadcasts ([1, 1, O], [O], [n, R, O]) goes to the tensor-op statement."""
    return (x.is_cuda and x.dim() == 3 and w.dim() == 3 and _f32_on(x, w, b) and w.shape[0] == x.shape[0] and w.shape[1] == x.shape[2]
            and b.shape == (x.shape[0], 1, w.shape[2]))


def _bias_bmm_fwd(x, w, b, leaky=False):
    lib = abi.load_library()
    x, w, b = x.contiguous(), w.contiguous(), b.contiguous()
    n, R, I = x.shape
    O = w.shape[2]
    y = th.empty(n, R, O, dtype=th.float32, device=x.device)
    fn = lib.ssd_bias_bmm_leaky_fwd if leaky else lib.ssd_bias_bmm_fwd
    abi.check(lib, fn(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), n, R, I, O, _stream(x)))
    return y


class _BiasBmm(th.autograd.Function):
    """baddbmm(b [n, 1, O], x [n, R, I], w [n, I, O]) on the device: one launch forward (ssd_bias_bmm_fwd) and ONE launch for the three
    gradients (ssd_bias_bmm_bwd: dx, dw and the bias gradient as column sums -- deterministic, no ATen multi-block reduction);
    csrc/ssd_bmm.hip.  leaky: the layer is followed by nn.LeakyReLU() (fc1 of both heads): applied in the forward kernel's epilogue
    and, backward, to the gradient as it is loaded (ssd_bias_bmm_leaky_fwd / _bwd) -- no elementwise launch in either direction."""

    @staticmethod
    def forward(ctx, x, w, b, leaky):
        x, w = x.contiguous(), w.contiguous()
        y = _bias_bmm_fwd(x, w, b, leaky)
        ctx.leaky = leaky
        ctx.precision = LEARNER_PRECISION
        ctx.save_for_backward(x, w, *((y,) if leaky else ()))
        return y

    @staticmethod
    def backward(ctx, g):
        with _precision(ctx.precision):
            return _BiasBmm._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        lib = abi.load_library()
        x, w = ctx.saved_tensors[:2]
        g = g.contiguous()
        n, R, I = x.shape
        O = w.shape[2]
        need = ctx.needs_input_grad
        dx = th.empty_like(x) if need[0] else None
        dw = th.empty_like(w) if need[1] else None
        db = th.empty(n, 1, O, dtype=th.float32, device=x.device) if need[2] else None
        ptr = lambda t: None if t is None else t.data_ptr()
        if ctx.leaky:
            y = ctx.saved_tensors[2]
            abi.check(lib, lib.ssd_bias_bmm_leaky_bwd(g.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(), ptr(dx), ptr(dw), ptr(db), None, n, R, I, O, _stream(x)))
        else:
            abi.check(lib, lib.ssd_bias_bmm_bwd(g.data_ptr(), x.data_ptr(), w.data_ptr(), ptr(dx), ptr(dw), ptr(db), None, n, R, I, O, _stream(x)))
        return dx, dw, db, None


def _bias_bmm_pair_fwd(x, w, b, x_t, w_t, b_t, leaky):
    lib = abi.load_library()
    x, w, b, x_t, w_t, b_t = (t.contiguous() for t in (x, w, b, x_t, w_t, b_t))
    n, R, I = x.shape
    n_t, O = x_t.shape[0], w.shape[2]
    y = th.empty(n, R, O, dtype=th.float32, device=x.device)
    y_t = th.empty(n_t, R, O, dtype=th.float32, device=x.device)
    abi.check(lib, lib.ssd_bias_bmm_pair_fwd(x.data_ptr(), None, w.data_ptr(), b.data_ptr(), y.data_ptr(), n, x_t.data_ptr(), None, w_t.data_ptr(), b_t.data_ptr(),
                                             y_t.data_ptr(), n_t, R, I, 0, O, 1, 0, int(bool(leaky)), _stream(x)))
    return y, y_t


class _BiasBmmPair(th.autograd.Function):
    """_BiasBmm of a live net (x, w, b) and the same layer of a second, frozen net (x_t, w_t, b_t: no gradient) as ONE forward launch
    (ssd_bias_bmm_pair_fwd: the sets of both nets in one grid, each computed as the single launch computes it); backward: _BiasBmm's
    single launch (ssd_bias_bmm_bwd / _leaky_bwd) on the live operands."""

    @staticmethod
    def forward(ctx, x, w, b, leaky, x_t, w_t, b_t):
        x, w = x.contiguous(), w.contiguous()
        y, y_t = _bias_bmm_pair_fwd(x, w, b, x_t, w_t, b_t, leaky)
        ctx.leaky = leaky
        ctx.precision = LEARNER_PRECISION
        ctx.save_for_backward(x, w, *((y,) if leaky else ()))
        ctx.mark_non_differentiable(y_t)
        ctx.set_materialize_grads(False)         # (no zero-filled gradient for y_t: a launch per backward otherwise)
        return y, y_t

    @staticmethod
    def backward(ctx, g, g_t):
        if g is None:
            return (None,) * 7
        with _precision(ctx.precision):
            return _BiasBmm._backward(ctx, g) + (None, None, None)


def bias_bmm_pair(x, w, b, x_t, w_t, b_t, leaky=False):
    """(bias_bmm(x, w, b, leaky), bias_bmm(x_t, w_t, b_t, leaky) without a gradient): one layer of a live net and of a frozen copy (the
    learner's target network) with the same shapes.  On the device ONE forward launch computes both; anywhere else, or when the second
    net asks for a gradient, the two calls one after the other."""
    frozen = not (th.is_grad_enabled() and (x_t.requires_grad or w_t.requires_grad or b_t.requires_grad))
    if (frozen and _bmm_kernel_ok(x, w, b) and _bmm_kernel_ok(x_t, w_t, b_t) and x_t.device == x.device and tuple(x_t.shape[1:]) == tuple(x.shape[1:])
            and tuple(w_t.shape[1:]) == tuple(w.shape[1:])):
        if th.is_grad_enabled() and (w.requires_grad or b.requires_grad or x.requires_grad):
            return _BiasBmmPair.apply(x, w, b, leaky, x_t, w_t, b_t)
        return _bias_bmm_pair_fwd(x, w, b, x_t, w_t, b_t, leaky)
    y = bias_bmm(x, w, b, leaky)
    with th.no_grad() if frozen else th.enable_grad():
        y_t = bias_bmm(x_t, w_t, b_t, leaky)
    return y, y_t


class _Fc1Rows(th.autograd.Function):
    """fc1_rows on the device: ONE launch writes the rows of both fc1 layers, of both nets when feat_t is given (ssd_fc1_rows_fwd), and
    one returns the live features' gradient (ssd_fc1_rows_bwd: the two layers' input gradients added and transposed back)."""

    @staticmethod
    def forward(ctx, feat, tail, act, B, T, n, feat_t):
        lib = abi.load_library()
        feat, tail, act = feat.contiguous(), tail.contiguous(), act.contiguous()
        F0, F1, A = feat.shape[1], tail.shape[1], act.shape[2]
        new = lambda w: th.empty(n, T * B, w, dtype=th.float32, device=feat.device)
        xe, xi = new(F0 + F1), new(F0 + F1 + A)
        xe_t = xi_t = None
        if feat_t is not None:
            feat_t, xe_t, xi_t = feat_t.contiguous(), new(F0 + F1), new(F0 + F1 + A)
        ptr = lambda t: None if t is None else t.data_ptr()
        abi.check(lib, lib.ssd_fc1_rows_fwd(feat.data_ptr(), ptr(feat_t), tail.data_ptr(), act.data_ptr(), xe.data_ptr(), xi.data_ptr(), ptr(xe_t), ptr(xi_t),
                                            B, T, n, F0, F1, A, _stream(feat)))
        ctx.dims = (B, T, n, F0, F1, A)
        ctx.set_materialize_grads(False)         # (no zero-filled gradients for the second net's rows: a launch each per backward otherwise)
        if feat_t is None:
            return xe, xi
        ctx.mark_non_differentiable(xe_t, xi_t)
        return xe, xi, xe_t, xi_t

    @staticmethod
    def backward(ctx, dxe, dxi, *unused):
        lib = abi.load_library()
        B, T, n, F0, F1, A = ctx.dims
        if dxe is None and dxi is None:
            return (None,) * 7
        like = dxe if dxe is not None else dxi
        dxe = like.new_zeros(n, T * B, F0 + F1) if dxe is None else dxe.contiguous()
        dxi = like.new_zeros(n, T * B, F0 + F1 + A) if dxi is None else dxi.contiguous()
        # the leading F0 columns of rows F0 + F1 wide: the layout the slice of th.cat([feat, tail])'s gradient has, so whatever reads
        # it (a library GEMM of the tensor-op encoder chooses its kernel by the strides too) is handed what it was handed before
        d_in = th.empty(B * T * n, F0 + F1, dtype=th.float32, device=dxe.device)
        abi.check(lib, lib.ssd_fc1_rows_bwd(dxe.data_ptr(), dxi.data_ptr(), d_in.data_ptr(), B, T, n, F0, F1, A, F0 + F1, _stream(dxe)))
        return d_in[:, :F0], None, None, None, None, None, None


def fc1_rows(feat, tail, act, B, T, n, feat_t=None):
    """The input rows of the two fc1 layers in the learner's set-major, time-major layout, from the pieces where they lie: feat
    [B * T * n, F0] (the encoder's output, rows (b * T + t) * n + i), tail [B * T * n, F1] (the non-visual input columns, same rows), act
    [n, T * B, A] (the one-hot actions, rows t * B + b) -> (x_env [n, T * B, F0 + F1] = [feat | tail], x_inc [n, T * B, F0 + F1 + A] =
    [feat | tail | act]); with feat_t (the features of a frozen second net: no gradient) also (x_env_t, x_inc_t).  The values of
    th.cat([feat, tail], 1) transposed to time-major rows, and of its concatenation with act."""
    for name, t, shape in (("tail", tail, (B * T * n, tail.shape[-1])), ("act", act, (n, T * B, act.shape[-1]))) + (
            () if feat_t is None else (("feat_t", feat_t, tuple(feat.shape)),)):
        if tuple(t.shape) != shape or t.device != feat.device:
            raise _unfit("fc1_rows", name, t, "%s on the device of feat expected" % (shape,))
    if feat.dim() != 2 or feat.shape[0] != B * T * n:
        raise _unfit("fc1_rows", "feat", feat, "[B * T * n = %d, F0] expected" % (B * T * n))
    frozen = feat_t is None or not (th.is_grad_enabled() and feat_t.requires_grad)
    if feat.is_cuda and frozen and _f32_on(feat, tail, act, *(() if feat_t is None else (feat_t,))) and tail.shape[1] >= 1 and not (
            th.is_grad_enabled() and (tail.requires_grad or act.requires_grad)):
        return _Fc1Rows.apply(feat, tail, act, B, T, n, feat_t)
    _leaving_kernels("fc1_rows", feat, "dtypes / a tail or actions that ask for a gradient")
    tm = lambda x: x.reshape(B, T, n, -1).permute(2, 1, 0, 3).reshape(n, T * B, -1)
    out = ()
    for f in (feat,) + (() if feat_t is None else (feat_t,)):
        x = tm(th.cat([f, tail.to(f.dtype)], dim=1))
        out += (x, th.cat([x, act.to(f.dtype)], dim=-1))
    return out


def bias_bmm(x, w, b, leaky=False):
    """x @ w + b for per-agent weights: x [n, R, I], w [n, I, O], b [n, 1, O]; leaky: followed by LeakyReLU (slope 0.01)."""
    if _bmm_kernel_ok(x, w, b):
        if th.is_grad_enabled() and (w.requires_grad or b.requires_grad or x.requires_grad):
            return _BiasBmm.apply(x, w, b, leaky)
        return _bias_bmm_fwd(x, w, b, leaky)
    if x.dim() != 3:
        raise _unfit("bias_bmm", "x", x, "[n, R, I] expected")
    if w.dim() != 3 or tuple(w.shape[:2]) != (x.shape[0], x.shape[2]) or w.device != x.device:
        raise _unfit("bias_bmm", "w", w, "[n = %d, I = %d, O] on the device of x expected" % (x.shape[0], x.shape[2]))
    if b.device != x.device:
        raise _unfit("bias_bmm", "b", b, "the device of x expected")
    _leaving_kernels("bias_bmm", x, "dtypes %s, %s, %s / a bias that is not [n, 1, O]" % (x.dtype, w.dtype, b.dtype))
    y = _baddbmm(b, x, w)
    return th.nn.functional.leaky_relu(y) if leaky else y


class _BiasLinear(th.autograd.Function):
    """F.linear(x [R, I], w [O, I], b [O]) with the bias gradient from ops.column_sums."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return th.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        return (g @ w if ctx.needs_input_grad[0] else None, g.t() @ x if ctx.needs_input_grad[1] else None,
                column_sums(g) if ctx.needs_input_grad[2] else None)


class _ChannelBias(th.autograd.Function):
    """y [R, C, H, W] + b [C] (the bias of a convolution) with the bias gradient from ops.column_sums over the R rows followed by a
    short per-channel sum."""

    @staticmethod
    def forward(ctx, y, b):
        return y + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        R, C = g.shape[0], g.shape[1]
        # rows first (k_column_sums), then the H x W positions of a channel as the rows of a second k_column_sums: no ATen reduction
        db = column_sums(column_sums(g.reshape(R, -1)).view(C, -1).t().contiguous()) if ctx.needs_input_grad[1] else None
        return g, db


def channel_bias(y, b):
    return _ChannelBias.apply(y, b)


def bias_linear(x, w, b):
    if x.is_cuda and (w.requires_grad or b.requires_grad or x.requires_grad):
        return _BiasLinear.apply(x, w, b)
    return th.nn.functional.linear(x, w, b)


def expand_codes(codes):
    """u8 class codes [..., V, V] of the simplified palette (0 nothing, 1 apple, 2 waste, 3 wall / agent; include/ssd_hip.h
    SSD_OBS_CODE) -> f32 [..., 3, V, V]: waste = R, apple = G, wall / agent = B at 255/256 -- the observation the env emits in
    f32 form (map_env.py:945, cleanup.py:96-105)."""
    c = codes.unsqueeze(-3)
    return th.cat([c == 2, c == 1, c == 3], dim=-3).float() * (255.0 / 256.0)


def encode_codes_supported(codes):
    return codes.is_cuda and codes.dtype == th.uint8 and codes.shape[-1] == codes.shape[-2] and abi.encode_edge_supported(codes.shape[-1])


class _EncodeCodes(th.autograd.Function):
    """rgb_preprocess (Conv2d 3->6 3x3 + LeakyReLU + Flatten + Linear -> 32 + LeakyReLU; homophily_agent.py:20-27,213-214) of windows
    given as u8 class codes [R, V, V], forward on the matrix cores (ssd_policy_encode: the rollout's encoder kernel, f32-equivalent
    products): 2 launches (weight fragments, encoder) instead of the expansion to f32 planes + MIOpen convolution + GEMM + 4
    elementwise kernels.  With gradients the kernel also emits LeakyReLU(conv) [R, 6, O, O]; the backward is the reference's
    arithmetic on it: two GEMMs for the Linear, the convolution's weight gradient (MIOpen) on the re-expanded planes, the bias
    gradients by ops.column_sums."""

    @staticmethod
    def forward(ctx, codes, conv_w, conv_b, lin_w, lin_b):
        lib = abi.load_library()
        codes = codes.contiguous()
        R, V = codes.shape[0], codes.shape[-1]
        O = V - 2
        dev = codes.device
        st = _stream(codes)
        cw, lw = conv_w.detach().contiguous(), lin_w.detach().contiguous()
        cb, lb = conv_b.detach().contiguous(), lin_b.detach().contiguous()
        prec = LEARNER_PRECISION
        need = any(ctx.needs_input_grad[1:])
        # the training forward also emits LeakyReLU(conv) and runs on the Toeplitz images; a forward without gradients (the target net)
        # takes the class-LUT layout: the conv as a table sum, a third of the matrix-core work.  Other window edges than 15 / 31 have
        # the class-LUT kernel only, which then also emits LeakyReLU(conv).
        layout = abi.ENCODE_LAYOUT_TOEPLITZ if need and V in (15, 31) else abi.ENCODE_LAYOUT_LUT
        cbytes, lbytes = abi.encode_frag_bytes(V, prec, layout)
        cf, lf = th.empty(cbytes, dtype=th.uint8, device=dev), th.empty(lbytes, dtype=th.uint8, device=dev)
        pack = lib.ssd_policy_pack_encoder if layout == abi.ENCODE_LAYOUT_TOEPLITZ else lib.ssd_policy_pack_encoder_lut
        abi.check(lib, pack(cw.data_ptr(), cb.data_ptr(), lw.data_ptr(), V, prec, cf.data_ptr(), lf.data_ptr(), st))
        act = th.empty(R, 6, O, O, dtype=th.float32, device=dev) if need else None
        bands = abi.encode_bands(V)
        ea = abi.SsdPolicyEncodeArgs()
        ea.codes, ea.code_bytes = codes.data_ptr(), codes.numel()
        ea.env_stride, ea.slot_stride, ea.agent_stride, ea.slot_t = V * V, 0, V * V, None
        ea.rows, ea.view_edge, ea.n_agents, ea.agent_major, ea.precision = R, V, 1, 0, prec
        ea.layout = layout
        ea.alphabet = abi.CODE_CLASS
        ea.conv_frags, ea.lin_frags, ea.conv_b, ea.lin_b = cf.data_ptr(), lf.data_ptr(), cb.data_ptr(), lb.data_ptr()
        ea.act = None if act is None else act.data_ptr()
        if bands == 1:
            feat = th.empty(R, 32, dtype=th.float32, device=dev)
            ea.out, ea.out_stride = feat.data_ptr(), 32
            abi.check(lib, lib.ssd_policy_encode(C.byref(ea), st))
        else:       # 31 x 31 windows and up: per-band partial sums of the Linear, finished here (each output adds `bands` values)
            part = th.empty(bands, R, 32, dtype=th.float32, device=dev)
            ea.part = part.data_ptr()
            abi.check(lib, lib.ssd_policy_encode(C.byref(ea), st))
            feat = th.nn.functional.leaky_relu(column_sums(part.view(bands, R * 32)).view(R, 32) + lb)
        if need:
            ctx.save_for_backward(codes, act, feat, cw, lw)
        ctx.precision = prec
        return feat

    @staticmethod
    def backward(ctx, d_feat):
        with _precision(ctx.precision):
            return _EncodeCodes._backward(ctx, d_feat)

    @staticmethod
    def _backward(ctx, d_feat):
        lib = abi.load_library()
        codes, act, feat, cw, lw = ctx.saved_tensors
        R = codes.shape[0]
        K = act[0].numel()
        st = _stream(codes)
        # dL/d(Linear output): LeakyReLU'(x) from the sign of LeakyReLU(x), one launch (it reads a row-strided d_feat where it lies)
        g2 = th.ops.aten.leaky_relu_backward(d_feat, feat, 0.01, True).contiguous()
        d_lin_b = column_sums(g2)
        # the two products of the Linear's backward on the per-agent-layer kernels (csrc/ssd_bmm.hip, one weight set):
        #   d_lin_w [32, K] = g2^T act   (its "dw" role: rows = K of the product, split over 16 waves per tile)
        #   d_act   [R, K]  = (g2 lin_w) * LeakyReLU'(conv)   (its "dx" role with w = lin_w^T [K, 32]; the slope from the sign of act)
        d_lin_w = th.empty(32, K, dtype=th.float32, device=codes.device)
        abi.check(lib, lib.ssd_bias_bmm_bwd(act.data_ptr(), g2.data_ptr(), None, None, d_lin_w.data_ptr(), None, None, 1, R, 32, K, st))
        d_act = th.empty_like(act)
        lwt = lw.t().contiguous()
        abi.check(lib, lib.ssd_bias_bmm_bwd(g2.data_ptr(), None, lwt.data_ptr(), d_act.data_ptr(), None, None, act.data_ptr(), 1, R, K, 32, st))
        # conv weight / bias gradient straight from the class codes (no f32 planes, no im2col): per-wave partial sums + one column sum
        P = lib.ssd_conv_wgrad_partial_rows(R)
        part = th.empty(P, 168, dtype=th.float32, device=codes.device)
        abi.check(lib, lib.ssd_conv_wgrad_codes(codes.data_ptr(), d_act.data_ptr(), part.data_ptr(), R, codes.shape[-1], st))
        tot = column_sums(part)
        return None, tot[:162].view(cw.shape), tot[162:], d_lin_w, d_lin_b


def encode_codes(codes, conv_w, conv_b, lin_w, lin_b):
    """features [R, 32] of windows given as u8 class codes [R, V, V] (V odd, 3 .. 63, on the device): see _EncodeCodes.  Host tensors,
    other edges and other integer dtypes of the codes: the layers themselves on expand_codes (homophily_agent.py:20-27,213-214)."""
    if codes.dim() != 3 or codes.shape[-1] != codes.shape[-2] or codes.shape[-1] < 3:
        raise _unfit("encode_codes", "codes", codes, "[R, V, V] with V >= 3 expected")
    K = 6 * (codes.shape[-1] - 2) ** 2
    for name, t, shape in (("conv_w", conv_w, (6, 3, 3, 3)), ("conv_b", conv_b, (6,)), ("lin_w", lin_w, (32, K)), ("lin_b", lin_b, (32,))):
        if t.shape != shape or t.device != codes.device:       # the pack kernels read exactly these sizes
            raise _unfit("encode_codes", name, t, "%s on the device of codes expected" % (shape,))
    if encode_codes_supported(codes) and _f32_on(conv_w, conv_b, lin_w, lin_b):
        return _EncodeCodes.apply(codes, conv_w, conv_b, lin_w, lin_b)
    _leaving_kernels("encode_codes", codes, "dtype %s / edge %d" % (codes.dtype, codes.shape[-1]))
    act = th.nn.functional.leaky_relu(th.nn.functional.conv2d(expand_codes(codes).to(conv_w.dtype), conv_w, conv_b))
    return th.nn.functional.leaky_relu(th.nn.functional.linear(act.flatten(1), lin_w, lin_b))


class _GruGates(th.autograd.Function):
    """h' = GRU gate arithmetic (homophily_agent.py:162-165,188-191) on gi = x W_i + b_i, gh = h W_h + b_h ([R, 3H], (r, z, n)
    order) as ONE forward and ONE backward HIP kernel instead of ~9 + ~20 pointwise launches per recurrence step."""

    @staticmethod
    def forward(ctx, gi, gh, h):
        lib = abi.load_library()
        gi, gh, h = gi.contiguous(), gh.contiguous(), h.contiguous()
        R, H = h.numel() // h.shape[-1], h.shape[-1]
        h_new, rzn = th.empty_like(h), th.empty_like(gi)
        abi.check(lib, lib.ssd_gru_gates_fwd(gi.data_ptr(), gh.data_ptr(), h.data_ptr(), h_new.data_ptr(), rzn.data_ptr(), R, H, _stream(h)))
        ctx.save_for_backward(rzn, gh, h)
        return h_new

    @staticmethod
    def backward(ctx, dh):
        lib = abi.load_library()
        rzn, gh, h = ctx.saved_tensors
        dh = dh.contiguous()
        R, H = h.numel() // h.shape[-1], h.shape[-1]
        d_gi, d_gh, dh_prev = th.empty_like(rzn), th.empty_like(rzn), th.empty_like(h)
        abi.check(lib, lib.ssd_gru_gates_bwd(dh.data_ptr(), rzn.data_ptr(), gh.data_ptr(), h.data_ptr(), d_gi.data_ptr(), d_gh.data_ptr(),
                                             dh_prev.data_ptr(), R, H, _stream(h)))
        return d_gi, d_gh, dh_prev


class _GruSeq(th.autograd.Function):
    """The whole recurrence h_t = GRU(gi_t, h_{t-1}) for t = 0..T-1 as one forward and one backward launch (csrc/ssd_gru_seq.hip).
    gi [T, G, B, 3H], wh [G, H, 3H], bh [G, 1, 3H] -> hs [G, T, B, H].  h0 None: from h = 0 (ssd_gru_seq_fwd); else a state
    [G, B, H]: hs[:, 0] := h0, steps 1 .. T - 1 computed (ssd_gru_seq_fwd_h0, time-major form: n_parts 0); h0 is data (no gradient)."""

    @staticmethod
    def forward(ctx, gi, wh, bh, h0):
        lib = abi.load_library()
        gi, wh, bh = gi.contiguous(), wh.contiguous(), bh.contiguous()
        T, G, B, H3 = gi.shape
        H = H3 // 3
        Bp = (B + 15) // 16 * 16                    # the kernels walk whole 16-row tiles: ragged batches are padded with zero rows
        if Bp != B:
            gi = th.nn.functional.pad(gi, (0, 0, 0, Bp - B))
        hs = th.empty(G, T, Bp, H, dtype=gi.dtype, device=gi.device)
        need = any(ctx.needs_input_grad)
        rzn = th.empty_like(gi) if need else None
        ghn = th.empty(T, G, Bp, H, dtype=gi.dtype, device=gi.device) if need else None
        if h0 is None:
            abi.check(lib, lib.ssd_gru_seq_fwd(gi.data_ptr(), wh.data_ptr(), bh.data_ptr(), hs.data_ptr(), None if rzn is None else rzn.data_ptr(),
                                               None if ghn is None else ghn.data_ptr(), T, G, Bp, _stream(gi)))
        else:
            h0 = h0.contiguous() if Bp == B else th.nn.functional.pad(h0, (0, 0, 0, Bp - B))      # the given state is padded with the batch
            one = lambda t: (C.c_void_p * 1)(t.data_ptr())
            abi.check(lib, lib.ssd_gru_seq_fwd_h0(one(gi), 0, one(wh), one(bh), 1, one(h0), Bp * H, H, hs.data_ptr(), None if rzn is None else rzn.data_ptr(),
                                                  None if ghn is None else ghn.data_ptr(), T, G, Bp, _stream(gi)))
        ctx.h0 = h0 is not None
        if need:
            ctx.save_for_backward(hs, rzn, ghn, wh)
            ctx.B = B
        ctx.precision = LEARNER_PRECISION
        return hs if Bp == B else hs[:, :, :B].contiguous()

    @staticmethod
    def backward(ctx, dhs):
        with _precision(ctx.precision):
            return _GruSeq._backward(ctx, dhs)

    @staticmethod
    def _backward(ctx, dhs):
        lib = abi.load_library()
        hs, rzn, ghn, wh = ctx.saved_tensors
        T, G, Bp, H3 = rzn.shape
        B = ctx.B
        dhs = dhs.contiguous() if Bp == B else th.nn.functional.pad(dhs, (0, 0, 0, Bp - B))      # padded rows: zero gradient
        tiles = Bp // 16
        d_gi = th.empty_like(rzn)
        dgh = th.empty(G, T, Bp, H3, dtype=rzn.dtype, device=rzn.device)      # workspace: dL/dgh_t, the operand of the W_h gradient
        d_wh = th.empty(G, H3 // 3, H3, dtype=rzn.dtype, device=rzn.device)
        d_bh = th.empty(G, tiles, H3, dtype=rzn.dtype, device=rzn.device)
        if ctx.h0:
            one = lambda t: (C.c_void_p * 1)(t.data_ptr())
            abi.check(lib, lib.ssd_gru_seq_bwd_h0(one(dhs), hs.data_ptr(), rzn.data_ptr(), ghn.data_ptr(), one(wh), 1, one(d_gi), 0, dgh.data_ptr(),
                                                  d_wh.data_ptr(), d_bh.data_ptr(), T, G, G, Bp, _stream(rzn)))
        else:
            abi.check(lib, lib.ssd_gru_seq_bwd(dhs.data_ptr(), hs.data_ptr(), rzn.data_ptr(), ghn.data_ptr(), wh.data_ptr(), d_gi.data_ptr(),
                                               dgh.data_ptr(), d_wh.data_ptr(), d_bh.data_ptr(), T, G, Bp, _stream(rzn)))
        if Bp != B:
            d_gi = d_gi[:, :, :B].contiguous()
        return d_gi, d_wh, (column_sums(d_bh) if tiles > 1 else d_bh[:, 0]).unsqueeze(1), None      # per-tile bias sums: k_column_sums (no ATen reduction); h0 is data


class _GruSeqParts(th.autograd.Function):
    """_GruSeq with the input-side projections given as separately allocated set-major parts [sets, T * B, 3H] (the per-agent affine
    layers' outputs as they are: ssd_gru_seq_fwd_parts / _bwd_parts) -- no concatenation / transpose copies, and the gradients come back
    per part, contiguous.  The recurrence weights come as n_w separately allocated parts too (wh [sets, H, 3H], bh [sets, 1, 3H]: the
    live net's and the target net's images as they are).  B is a multiple of 16 here (gru_sequence_parts falls back otherwise).
    h0 None: from zero (ssd_gru_seq_fwd_parts); else (views [sets, B, H] per projection part, set stride, row stride in elements), read
    in place by ssd_gru_seq_fwd_h0 (the learner: batch["hidden"][:, 0] of the static batch, no copy launch); hs[:, 0] := h0, no gradient
    into it."""
    LEAD = 4          # non-tensor arguments in front of the tensors: T, B, n_w, h0

    @staticmethod
    def forward(ctx, T, B, n_w, h0, *tensors):
        lib = abi.load_library()
        whs, bhs = [t.contiguous() for t in tensors[:n_w]], [t.contiguous() for t in tensors[n_w:2 * n_w]]
        parts = [p.contiguous() for p in tensors[2 * n_w:]]
        G, H3 = sum(p.shape[0] for p in parts), parts[0].shape[-1]
        H = H3 // 3
        dev = parts[0].device
        hs = th.empty(G, T, B, H, dtype=th.float32, device=dev)
        need = any(ctx.needs_input_grad)
        rzn = th.empty(T, G, B, H3, dtype=th.float32, device=dev) if need else None
        ghn = th.empty(T, G, B, H, dtype=th.float32, device=dev) if need else None
        ptrs = (C.c_void_p * len(parts))(*[p.data_ptr() for p in parts])
        wptrs = (C.c_void_p * n_w)(*[w.data_ptr() for w in whs])
        bptrs = (C.c_void_p * n_w)(*[b.data_ptr() for b in bhs])
        if h0 is None:
            abi.check(lib, lib.ssd_gru_seq_fwd_parts(ptrs, len(parts), wptrs, bptrs, n_w, hs.data_ptr(), None if rzn is None else rzn.data_ptr(),
                                                     None if ghn is None else ghn.data_ptr(), T, G, B, _stream(hs)))
        else:
            views, set_stride, row_stride = h0
            hptrs = (C.c_void_p * len(parts))(*[v.data_ptr() for v in views])
            abi.check(lib, lib.ssd_gru_seq_fwd_h0(ptrs, len(parts), wptrs, bptrs, n_w, hptrs, set_stride, row_stride, hs.data_ptr(),
                                                  None if rzn is None else rzn.data_ptr(), None if ghn is None else ghn.data_ptr(), T, G, B, _stream(hs)))
        ctx.h0 = h0 is not None
        if need:
            ctx.save_for_backward(hs, rzn, ghn, *whs)
            ctx.shapes = [p.shape for p in parts]
            ctx.n_w = n_w
        ctx.precision = LEARNER_PRECISION
        ctx.set_materialize_grads(False)       # states without a gradient (the target net's) arrive as None, not as zero tensors
        spp = parts[0].shape[0]
        # one output per projection part: views of the one state buffer (slicing a single output would cost a zero-fill + copy + add per
        # slice in the backward pass)
        return tuple(hs[k * spp:(k + 1) * spp] for k in range(len(parts)))

    @staticmethod
    def backward(ctx, *dhs_parts):
        with _precision(ctx.precision):
            return _GruSeqParts._backward(ctx, *dhs_parts)

    @staticmethod
    def _backward(ctx, *dhs_parts):
        lib = abi.load_library()
        hs, rzn, ghn = ctx.saved_tensors[:3]
        whs = ctx.saved_tensors[3:]
        n_w = ctx.n_w
        T, G, B, H3 = rzn.shape
        n_parts = len(ctx.shapes)
        spp = G // n_parts
        need, lead = ctx.needs_input_grad, _GruSeqParts.LEAD
        # the sets whose states carry a gradient form a prefix (the live net's parts come first); the kernel walks only those
        last = max([k for k, d in enumerate(dhs_parts) if d is not None], default=-1)
        if last < 0:
            return (None,) * len(need)
        Gn = (last + 1) * spp
        dhs = [(d.contiguous() if d is not None else th.zeros(spp, T, B, H3 // 3, dtype=th.float32, device=rzn.device)) for d in dhs_parts[:last + 1]]
        d_parts = [th.empty(sh, dtype=th.float32, device=rzn.device) for sh in ctx.shapes[:last + 1]]
        dgh = th.empty(Gn, T, B, H3, dtype=th.float32, device=rzn.device)
        d_wh = th.empty(Gn, H3 // 3, H3, dtype=th.float32, device=rzn.device)
        tiles = B // 16
        d_bh = th.empty(Gn, tiles, H3, dtype=th.float32, device=rzn.device)
        pad = lambda xs: [x.data_ptr() for x in xs] + [xs[0].data_ptr()] * (n_parts - len(xs))       # parts past Gn: never touched
        ptrs = (C.c_void_p * n_parts)(*pad(d_parts))
        dptrs = (C.c_void_p * n_parts)(*pad(dhs))
        wptrs = (C.c_void_p * n_w)(*[w.data_ptr() for w in whs])
        launch = lib.ssd_gru_seq_bwd_h0 if ctx.h0 else lib.ssd_gru_seq_bwd_parts
        abi.check(lib, launch(dptrs, hs.data_ptr(), rzn.data_ptr(), ghn.data_ptr(), wptrs, n_w, ptrs, n_parts,
                              dgh.data_ptr(), d_wh.data_ptr(), d_bh.data_ptr(), T, G, Gn, B, _stream(rzn)))
        d_bh_all = (column_sums(d_bh) if tiles > 1 else d_bh[:, 0]).unsqueeze(1)                    # [Gn, 1, 3H]
        spw = G // n_w

        def of_part(full, k):
            """weight part k's share of a [Gn, ...] output: a view where the part lies inside the walked sets (the learner's form: no
            copies, no launch), None where no set of it was walked, and for a part the walk ends inside (one weight tensor for live and
            target parts) its full size with exact zeros for the sets not walked"""
            lo, hi = k * spw, (k + 1) * spw
            if hi <= Gn:
                return full[lo:hi]
            if lo >= Gn:
                return None
            out = full.new_zeros((spw,) + tuple(full.shape[1:]))
            out[:Gn - lo] = full[lo:Gn]
            return out
        g_wh = tuple(of_part(d_wh, k) if need[lead + k] else None for k in range(n_w))
        g_bh = tuple(of_part(d_bh_all, k) if need[lead + n_w + k] else None for k in range(n_w))
        g_parts = tuple(d_parts[k] if (k <= last and need[lead + 2 * n_w + k]) else None for k in range(n_parts))
        return (None,) * lead + g_wh + g_bh + g_parts


def _gru_h0_views(op, h0, like, n_parts, spp, B, H):
    """The given initial state of `op` as one view [spp, B, H] per projection part: h0 is ONE tensor [n_parts * spp, B, H] or a list
    of n_parts tensors / strided views [spp, B, H].  It is data: a state that asks for a gradient is refused."""
    views = [h0[k * spp:(k + 1) * spp] for k in range(n_parts)] if isinstance(h0, th.Tensor) else list(h0)
    if isinstance(h0, th.Tensor) and (h0.dim() != 3 or tuple(h0.shape) != (n_parts * spp, B, H)):
        raise _unfit(op, "h0", h0, "[G = %d, B = %d, H = %d] or one view [sets, B, H] per projection part expected" % (n_parts * spp, B, H))
    if len(views) != n_parts:
        raise ValueError("ops.%s: h0 comes as %d parts for %d projection parts" % (op, len(views), n_parts))
    for k, v in enumerate(views):
        if not isinstance(v, th.Tensor) or tuple(v.shape) != (spp, B, H) or v.device != like.device:
            raise _unfit(op, "h0[%d]" % k, v, "[sets = %d, B = %d, H = %d] on the device of the projections expected" % (spp, B, H))
        if v.requires_grad:
            raise ValueError("ops.%s: h0 requires a gradient; the given state is data (the recurrence sends no gradient into it): detach it" % op)
    return views


def _gru_h0_in_place(views):
    """(set stride, row stride) if the sequence kernel can read these views where they lie, else None"""
    v0 = views[0]
    ss, rs = (v0.stride(0) if v0.shape[0] > 1 else 0), (v0.stride(1) if v0.shape[1] > 1 else 0)
    for v in views:
        if (v.dtype != th.float32 or v.stride(2) != 1 or (v.shape[0] > 1 and v.stride(0) != ss) or (v.shape[1] > 1 and v.stride(1) != rs)
                or v.data_ptr() % 16):
            return None
    if ss < 0 or rs < 0 or ss % 4 or rs % 4:
        return None
    return ss, rs


def gru_sequence_parts(parts, T, B, wh, bh, h0=None):
    """gru_sequence for projections held as equally sized set-major parts [sets, T * B, 3H] (rows t * B + b); wh [G, H, 3H], bh [G, 1, 3H]
    over all sets in part order -- each either ONE tensor or a list of 1..4 equally sized parts over the sets (no concatenation).
    Returns the states as a LIST with one tensor [sets, T, B, H] per projection part.  A weight part whose sets' states carry no
    gradient gets none (the learner puts the target net's parts last); one that only partly lies among the sets with a gradient gets
    its full size, zeros for the rest.
    h0 (None: from zero): the state the sequences start from, ONE tensor [G, B, H] or one (strided) view [sets, B, H] per projection
    part; then hs[:, 0] = h0, steps 1 .. T - 1 are computed and the projections of step 0 are not read.  h0 is data."""
    H3 = parts[0].shape[-1]
    whs, bhs = (list(wh) if isinstance(wh, (list, tuple)) else [wh]), (list(bh) if isinstance(bh, (list, tuple)) else [bh])
    G = sum(p.shape[0] for p in parts)
    H = H3 // 3
    for k, p in enumerate(parts):
        if p.dim() != 3 or p.shape[1] != T * B or p.shape[2] != H3 or p.device != parts[0].device:
            raise _unfit("gru_sequence_parts", "parts[%d]" % k, p, "[sets, T * B = %d, 3H = %d] on one device expected" % (T * B, H3))
    _gru_weights_fit("gru_sequence_parts", parts[0], whs, bhs, G, H)
    if h0 is not None:
        if any(p.shape != parts[0].shape for p in parts):
            raise _unfit("gru_sequence_parts", "parts", parts[0], "equally sized parts expected with h0")
        h0 = _gru_h0_views("gru_sequence_parts", h0, parts[0], len(parts), parts[0].shape[0], B, H)
    if (parts[0].is_cuda and H3 == 192 and B % 16 == 0 and 1 <= len(parts) <= 4 and all(p.shape == parts[0].shape for p in parts)
            and _f32_on(*parts, *whs, *bhs) and 1 <= len(whs) <= 4 and all(w.shape == whs[0].shape for w in whs)
            and all(b.shape == bhs[0].shape for b in bhs) and whs[0].shape[0] * len(whs) == G):
        if h0 is None:
            return list(_GruSeqParts.apply(T, B, len(whs), None, *whs, *bhs, *parts))
        if _f32_on(*h0):
            strides = _gru_h0_in_place(h0)
            if strides is None:         # a layout the kernel does not index (odd strides, misaligned): one contiguous copy
                full = th.stack([v.contiguous() for v in h0], dim=0).reshape(G, B, H)
                h0 = [full[k * parts[0].shape[0]:(k + 1) * parts[0].shape[0]] for k in range(len(parts))]
                strides = (B * H, H)
            return list(_GruSeqParts.apply(T, B, len(whs), (h0, strides[0], strides[1]), *whs, *bhs, *parts))
    wh, bh = (whs[0] if len(whs) == 1 else th.cat(whs, dim=0)), (bhs[0] if len(bhs) == 1 else th.cat(bhs, dim=0))
    if H3 != 192 or parts[0].dtype != th.float32:
        _leaving_kernels("gru_sequence_parts", parts[0], "hidden size %d / dtype" % (H3 // 3))
    # ragged batches (B % 16) and other part counts: the time-major launch (it pads the batch itself); still the HIP recurrence
    gi = th.cat([p.reshape(p.shape[0], T, B, H3) for p in parts], dim=0).transpose(0, 1).contiguous()      # [T, G, B, 3H]
    hs = gru_sequence(gi, wh, bh) if h0 is None else gru_sequence(gi, wh, bh, th.cat(list(h0), dim=0))
    spp = parts[0].shape[0]
    return [hs[k * spp:(k + 1) * spp] for k in range(len(parts))]


def _gru_weights_fit(op, like, whs, bhs, G, H):
    """the recurrence weights as the sequence launches index them: wh parts [sets, H, 3H] and bh parts [sets, 1, 3H] on the projections'
    device that cover the G sets, else the error names the argument"""
    if len(whs) != len(bhs):
        raise ValueError("ops.%s: wh comes as %d parts and bh as %d" % (op, len(whs), len(bhs)))
    for name, ts, mid in (("wh", whs, H), ("bh", bhs, 1)):
        for t in ts:
            if t.dim() != 3 or tuple(t.shape[1:]) != (mid, 3 * H) or t.device != like.device:
                raise _unfit(op, name, t, "[sets, %d, 3H = %d] on the device of the projections expected" % (mid, 3 * H))
        if sum(t.shape[0] for t in ts) != G:
            raise _unfit(op, name, ts[0], "%d sets in all expected, got %d" % (G, sum(t.shape[0] for t in ts)))


def gru_sequence(gi, wh, bh, h0=None):
    """hs [G, T, B, H]: the GRU states h_1..h_T for the input-side projections gi [T, G, B, 3H] from a zero initial state.
    h0 [G, B, H] (data, no gradient): hs[:, 0] = h0 and steps 1 .. T - 1 are computed from it; gi[0] is not read."""
    if gi.dim() != 4 or gi.shape[3] % 3:
        raise _unfit("gru_sequence", "gi", gi, "[T, G, B, 3H] expected")
    T, G, B, H3 = gi.shape
    _gru_weights_fit("gru_sequence", gi, [wh], [bh], G, H3 // 3)
    if h0 is not None:
        h0 = _gru_h0_views("gru_sequence", h0, gi, 1, G, B, H3 // 3)[0]
    if gi.is_cuda and H3 == 192 and _f32_on(gi, wh, bh) and (h0 is None or _f32_on(h0)):
        return _GruSeq.apply(gi, wh, bh, h0)
    _leaving_kernels("gru_sequence", gi, "hidden size %d (the sequence kernels are instantiated for 64) / dtypes %s, %s, %s" % (H3 // 3, gi.dtype, wh.dtype, bh.dtype))
    h = gi.new_zeros(G, B, H3 // 3) if h0 is None else h0.to(gi.dtype)
    hs = [] if h0 is None else [h]                  # the given state IS the state after step 0
    for t in range(len(hs), T):
        h = gru_gates(gi[t], _baddbmm(bh, h, wh), h)
        hs.append(h)
    return th.stack(hs, dim=1)


def gru_gates(gi, gh, h):
    """h' from the two projections and the previous state; [..., 3H], [..., 3H], [..., H] -> [..., H]."""
    H = h.shape[-1]
    if gi.shape[-1] != 3 * H or gi.shape[:-1] != h.shape[:-1] or gi.device != h.device:
        raise _unfit("gru_gates", "gi", gi, "%s on the device of h expected" % (tuple(h.shape[:-1]) + (3 * H,),))
    if gh.shape != gi.shape or gh.device != h.device:
        raise _unfit("gru_gates", "gh", gh, "%s on the device of h expected" % (tuple(gi.shape),))
    if gi.is_cuda and _f32_on(gi, gh, h):
        return _GruGates.apply(gi, gh, h)
    _leaving_kernels("gru_gates", gi, "dtypes %s, %s, %s" % (gi.dtype, gh.dtype, h.dtype))
    r = th.sigmoid(gi[..., :H] + gh[..., :H])
    z = th.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    cand = th.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * cand + z * h
