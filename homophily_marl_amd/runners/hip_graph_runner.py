"""HipGraphRunner: the vectorised rollout of HipVecRunner as hipGraph replays (10 timesteps per replay by default).

Same data flow and stored batch as HipVecRunner / the reference loop (episode_runner.py:57-119); what changes is the
mechanics that make a timestep capturable and replayable for every t:
  * the episode storage is persistent and indexed by a device-side time counter; when the replay buffer's size is a small
    multiple of the env batch the storage IS the next slots of the replay buffer (ReplayBuffer.reserve), so inserting the
    finished batch moves no data.  Everything that holds pointers into a storage lives in a per-storage bundle;
  * the controller state (hidden states, previous action / reward / incentives) lives in static tensors; the t == 0 history
    features are zeros because the previous action is -1 (all-zero one-hot);
  * with FastPolicy's fused kernels (default) a timestep is 3 launches (pipelined): k_head<env> on the features the previous
    timestep's launch left, the fused env step + observe (writes obs[:, t + 1] of the storage), and k_inc_encode = k_head<inc> of
    t together with k_encode of slot t + 1 (they share no data; the input rows live in a buffer pair indexed by the parity of t);
    the heads file actions / pose / rewards in slot t, carry the runner state and hand the device-side counters over.  An odd number
    of timesteps per graph takes the four standalone launches (k_encode, k_head<env>, env, k_head<inc>).
    obs_others_last_action with fused_others_last_action takes the same four launches (the heads gather fc1's rows; the previous actions
    of all agents travel in FastPolicy.prev_rec, a buffer pair indexed by the parity of t like the input rows).  fused_onehot_gather:
    the same four launches for ANY flag set at any team size (every one-hot block is gathered; the same record pair).  With
    pipeline_gathered both take the three pipelined launches at every window edge, the third being k_inc_encode_gather: the env head of
    t reads prev_rec[t & 1] and writes the other buffer, the inc head inside the third launch reads prev_rec[t & 1]; the exploration
    draws are those of the four-launch timestep.
    Other configurations (obs_others_last_action without that key, fast_policy=False) take the generic torch timestep, captured the same way;
  * train_stored_state (default off): the episode field "hidden" receives the recurrent state AFTER the controller consumed slot t
    (the state the heads of slot t produced Q_t from), [h_env | h_inc] per agent: one ssd_store_hidden launch ends every timestep,
    the slot-T pass included, reading the device-side slot index the heads of slot t filed under;
  * per_initial_priority "rollout" (prioritised replay; default "max"): both heads write their Q-values into static buffers (q_out) and one
    ssd_rollout_priority launch ends every timestep (behind ssd_store_hidden where both are on), the slot-T pass included: it forms the
    one-step TD errors of slot t - 1 online and, at slot T, the fixed-point priority every episode enters the table with
    (initial_priorities()).  Test episodes take the same launches on their own storage's state; nothing reads their result;
  * epsilon is a device scalar; exploration uses the package's counter generator (no multinomial, no host sync).
Which of these a runner takes is decided once, on the host: plan_rollout (fast_policy.py) for the controller, plan_runner below for
the storage format, the graph length and the config keys.
The first episode runs eagerly (warm-up of hipBLASLt plans and the allocator); graphs are captured from the second on.
The returned EpisodeBatch is the persistent storage: consume it (buffer.insert_episode_batch) before the next run(), as the
training loop does (run.py:184-185).
"""
import ctypes as C
from typing import NamedTuple

import torch as th
import torch.nn.functional as F

from .. import abi, ops

from ..components.episode_buffer import EpisodeBatch
from ..fast_policy import FastPolicy, plan_rollout
from .hip_vec_runner import HipVecRunner


class RunnerPlan(NamedTuple):
    fast: bool              # the FastPolicy kernels; else the generic torch timestep
    direct_obs: bool        # fused encoder: the env kernel writes obs[:, t + 1] of the storage itself (and the class codes the encoder reads)
    fold_store: bool        # the two heads file their results in the storage themselves: no store-step launch
    graph_steps: int        # timesteps per rollout hipGraph; 0: eager timesteps
    pipe: bool              # the pipelined timestep of 3 launches
    counter_start: int      # what the exploration draw counter starts at


def plan_runner(plan, args, episode_limit, obs_fmt):
    """The runner's own choices for a controller whose RolloutPlan is `plan` (computed with fused = fused_policy and the simplified
    palette).  Pure: it is called before anything is allocated."""
    a = args
    fast = bool(getattr(a, "fast_policy", True)) and plan.supported
    direct_obs = fast and plan.fused_enc
    fold_store = direct_obs and bool(getattr(a, "fold_store", True))
    if obs_fmt == abi.OBS_CODE and not direct_obs:
        # class-code storage is consumed by the fused encoder only; windows it does not take (view 0) take the generic timestep
        # (the torch controller expands the codes itself)
        fast = False
    # Pipelined timestep (3 launches): env head -> env step -> [inc head of t + encoder of t + 1] as one launch
    # (FastPolicy.act_inc_encode).  The encoder writes the OTHER buffer of FastPolicy.inputs_pair, so the buffer of a timestep is
    # its parity -- baked into the captured graph, hence an even number of timesteps per graph.
    K = max(1, int(getattr(a, "steps_per_graph", 10)))
    while episode_limit % K:
        K -= 1
    if fast and plan.needs_prev_rec and K % 2:
        # the previous-action records alternate with the parity of t, which a captured graph bakes in: an even number of timesteps
        # per graph, or (odd episode lengths) eager timesteps
        K = max([k for k in range(2, K, 2) if episode_limit % k == 0], default=0)
    use_graph = bool(getattr(a, "rollout_graph", True))
    # (fold_store implies that the encoder has class codes to read: the storage's under OBS_CODE, else the env's side buffer)
    pipe = bool(fold_store and plan.fused and plan.inc_encode and getattr(a, "pipeline_encode", True) and (K % 2 == 0 or not use_graph))
    # pipeline_any_view / pipeline_gathered change the launches of a timestep, not its draws: in the four-launch timestep the
    # encoder advances the draw counter BEFORE the heads of that timestep read it, in the pipelined one the inc head advances it
    # AFTER they did -- so the counter starts one ahead there and both runners draw the same exploration (the dense layouts at
    # 15 / 31 keep their sequence; the gathered ones had no pipelined sequence before the key, so the rule holds there too)
    ahead = pipe and (plan.V not in (15, 31) or plan.needs_prev_rec)
    return RunnerPlan(fast=fast, direct_obs=direct_obs, fold_store=fold_store, graph_steps=K, pipe=pipe, counter_start=int(ahead))


class HipGraphRunner(HipVecRunner):
    def setup(self, scheme, groups, preprocess, mac):
        super().setup(scheme, groups, preprocess, mac)
        self._scheme, self._groups, self._preprocess = scheme, groups, preprocess
        self._graph = None
        self._episodes = 0
        self._ready = False
        self._bundles, self._own_store, self._replay = {}, None, None
        self._graph_steps = 1

    def set_replay_buffer(self, buffer):
        """Write training episodes directly into `buffer` (ReplayBuffer.reserve) when its size is a small multiple (<= 8) of the env
        batch and it lives on the env's device; buffer.insert_episode_batch(batch) then moves no data."""
        N = self.batch_size
        ok = (buffer is not None and buffer.buffer_size % N == 0 and buffer.buffer_size // N <= 8
              and th.device(buffer.device) == th.device(self.args.device) and buffer.max_seq_length == self.episode_limit + 1)
        self._replay = buffer if ok else None
        return ok

    def _runner_plan(self):
        """(whether the fused heads are allowed, the RunnerPlan): pure, from the controller, the config and the env's palette"""
        a = self.args
        use_fused = bool(getattr(a, "fused_policy", True)) and self.env.native.cfg.obs_color == abi.COLOR_SIMPLIFIED
        return use_fused, plan_runner(plan_rollout(self.mac, use_fused), a, self.episode_limit, self.obs_fmt)

    def plans_fused_heads(self):
        """whether the rollout will run on the fused heads (FastPolicy with .fused) -- known after setup(), before anything is allocated"""
        use_fused, rp = self._runner_plan()
        return bool(rp.fast and plan_rollout(self.mac, use_fused).fused)

    def _ladder_total(self):
        """all envs of the job: batch_size_run x ranks"""
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        return self.batch_size * world

    # ---- static state ---------------------------------------------------------------------------------------------
    def _allocate(self):
        a, N, n, T = self.args, self.batch_size, self.args.n_agents, self.episode_limit
        dev = self.env.device
        simplified = self.env.native.cfg.obs_color == abi.COLOR_SIMPLIFIED
        # the fused encoder reads u8 class codes: the env kernel emits them next to the f32 observation (format R storage) or the
        # storage itself holds them (format C)
        self._want_code = bool(getattr(a, "fast_policy", True) and getattr(a, "fused_policy", True) and simplified
                               and self.obs_fmt != abi.OBS_CODE and abi.encode_edge_supported(self.env.native.V))
        self._dense_cur = self.env.native.obs_buffers(self.obs_fmt, want_code=self._want_code)   # obs / pos / orient written by the env kernel
        self.cur = self._dense_cur
        use_fused, rp = self._runner_plan()
        self.direct_obs, self.fold_store, self.pipe, self._graph_steps_planned = rp.direct_obs, rp.fold_store, rp.pipe, rp.graph_steps
        self.t_dev = th.zeros(1, dtype=th.long, device=dev)
        self.rng_ctr = th.full((1,), rp.counter_start, dtype=th.long, device=dev)   # never reset: exploration draws differ between episodes
        self.prev_actions = th.full((N, n), -1, dtype=th.long, device=dev)
        self.prev_reward = th.zeros(N, n, device=dev)
        self.prev_inc = th.zeros(N, n, n, dtype=th.long, device=dev)
        # the same incentive actions as receiver-major bytes [n(receiver), N, 16] (ssd_policy_head.recv_inc): what the fused env head reads
        self.recv_inc = th.zeros(n, N, 16, dtype=th.uint8, device=dev) if n <= 16 else None
        H = a.rnn_hidden_dim
        self.h_env = th.zeros(N, n, 1, H, device=dev)
        self.h_inc = th.zeros(N, n, 1, H, device=dev)
        self.eps = th.zeros((), device=dev)
        self.ep_return = th.zeros(N, n, device=dev)
        avail = self.env.avail_actions_batch[0, 0]
        self.avail_idx = th.nonzero(avail).squeeze(-1)                  # constant table of available env actions
        self.avail_mask = self.env.avail_actions_batch                  # [N, n, A]
        self.inc_mask = (1 - th.eye(n, device=dev, dtype=th.long)).reshape(1, n, n)
        self.fast = None
        if rp.fast:         # else: the generic captured timestep
            # one exploration seed for every rank: the draws are keyed by the GLOBAL env id (env_id_base + local env)
            self.fast = FastPolicy(self.mac, N, avail, seed=int(self.env.native.cfg.seed) * 2654435761 + 12345, fused=use_fused,
                                   precision=1 if str(getattr(a, "qnet_dtype", "fp32")).lower() in ("bf16", "bfloat16") else 2,
                                   env_id_base=int(self.env.native.cfg.env_id_base))
            self._zeros_nn = th.zeros(N, n, device=dev)
            self.pos_t, self.orient_t = th.zeros(N, n, 2, device=dev), th.zeros(N, n, 2, device=dev)   # pose before the env step
            self.actions_i32 = th.zeros(N, n, dtype=th.int32, device=dev)
            self.t_store = th.zeros(1, dtype=th.long, device=dev)     # the encoder's copy of t_dev, read by the store-step launch
        # epsilon_ladder_alpha > 0: a rate per env, eps ** expo[b], as a persistent table the captured graphs bake in like self.eps;
        # refreshed from the scalar by one device op wherever the scalar is filled (_set_eps).  Off: no table, epsilon_rows stays NULL
        self.ladder_alpha = float(getattr(a, "epsilon_ladder_alpha", 0.0) or 0.0)
        self.expo = self.eps_rows = None
        if self.ladder_alpha > 0.0:
            if self.fast is None or not self.fast.fused:
                raise ValueError("epsilon_ladder_alpha > 0 needs the fused rollout heads; this runner planned %s"
                                 % ("the generic timestep" if self.fast is None else "the per-layer heads"))
            from ..components.epsilon_schedules import ladder_exponents
            self.expo = th.from_numpy(ladder_exponents(self.ladder_alpha, int(self.env.native.cfg.env_id_base), N, self._ladder_total())).to(dev)
            self.eps_rows = th.zeros(N, device=dev)
        self.rng_copy = th.zeros(1, dtype=th.long, device=dev)          # pipelined: the env head's copy of rng_ctr for the inc head
        self.stored_state = bool(getattr(a, "train_stored_state", False))
        # per_initial_priority "rollout": the heads' Q-values of the current slot (FastPolicy's q_out is agent-major, the generic
        # timestep's copy env-major) and the constants of the one-step TD error, from where the loss launch takes them
        self.initial_priority = getattr(a, "per_initial_priority", "max") == "rollout"
        self.q_env = self.q_inc = None
        self.priority_windows = None
        if self.initial_priority:
            A = a.n_actions
            self.q_env = th.zeros((n, N, A) if rp.fast else (N, n, A), device=dev)
            self.q_inc = th.zeros((n, N, n, 3) if rp.fast else (N, n, n, 3), device=dev)
            self._avail_bits = sum(1 << k for k, v in enumerate(avail.reshape(-1).tolist()) if v)
            norm = ops.window_reward_norm(getattr(a, "train_window_norm", "episode"), T + 1, int(getattr(a, "train_window", 0) or 0))
            self._td_constants = ops.td_constants(a, norm)
            # per_unit "window": one priority per training window of the stride grid, (S, L, s, K) (run.setup resolved the stride)
            if getattr(a, "per_unit", "episode") == "window":
                L = int(a.train_window)
                self.priority_windows = (ops.window_grid(T, L, int(a.per_window_stride))[0], L, int(a.per_window_stride), int(a.train_burn_in))
        self._par = 0
        self._ready = True

    def _bind_store(self, store):
        """Select the episode storage of this episode.  Everything that holds pointers into a storage (output buffers of the env
        kernel, store-step arguments, the captured graph) lives in a per-storage bundle created on first use."""
        from types import SimpleNamespace
        st = store.data.transition_data
        key = st["obs"].data_ptr()
        b = self._bundles.get(key)
        self.store = store
        if b is None:
            st["filled"].fill_(1)                                       # fixed-length episodes: every slot is filled
            st["avail_actions"].copy_(self.env.avail_actions_batch.unsqueeze(1).expand(-1, self.episode_limit + 1, -1, -1))
            b = SimpleNamespace(graph=None, cur=self._dense_cur, ss=None, ss_last=None, file_env=None, file_inc=None, file_inc_last=None,
                                begin_graph=None, finish_graph=None, hidden=None, priority=None, priority_state=None)
            # the slot index the heads of slot t filed under, which the two launches below only read: the encoder's / env head's copy
            # where one is written (direct_obs), else the master before it is advanced
            fast = self.fast is not None
            t_filed = self.t_store if (fast and self.direct_obs) else self.t_dev
            if self.stored_state:
                b.hidden = ops.store_hidden_args(t_filed, self.fast.h_env if fast else self.h_env, self.fast.h_inc if fast else self.h_inc, st["hidden"])
            if self.initial_priority:
                b.priority, b.priority_state = ops.rollout_priority_args(t_filed, self.q_env, self.q_inc, fast, self._avail_bits, st, self._td_constants,
                                                                         self.args.per_alpha, self.args.per_eta, self.args.per_eps,
                                                                         windows=self.priority_windows)
            if self.fast is not None:
                if self.direct_obs:
                    b.cur = self.env.native.storage_obs_buffers(st["obs"], self.obs_fmt, want_code=self._want_code)
                b.ss, b.ss_last = self._make_store_args(True), self._make_store_args(False)
                if self.fold_store:     # the two heads file their results in the storage themselves: no store-step launch
                    out, slots = self.env.native.out, self.episode_limit + 1
                    common = dict(t_index=self.t_store.data_ptr(), t_slots=slots)
                    b.file_env = dict(common, dst_pos=st["agent_pos"].data_ptr(), dst_orient=st["agent_orientation"].data_ptr(),
                                      dst_actions=st["actions"].data_ptr(), dst_actions_onehot=st["actions_onehot"].data_ptr(),
                                      prev_actions_out=self.prev_actions.data_ptr())
                    b.file_inc_last = dict(common, dst_actions_inc=st["actions_inc"].data_ptr())
                    if self.recv_inc is not None:
                        b.file_env = dict(b.file_env, recv_inc=self.recv_inc.data_ptr())
                    b.file_inc = dict(b.file_inc_last, prev_actions_inc_out=self.prev_inc.data_ptr(), dst_reward=st["reward"].data_ptr(),
                                      dst_clean_num=st["clean_num"].data_ptr(), dst_apple_den=st["apple_den"].data_ptr(),
                                      dst_terminated=st["terminated"].data_ptr(), terminated=out["terminated"].data_ptr(),
                                      prev_reward_out=self.prev_reward.data_ptr(), ep_return=self.ep_return.data_ptr(),
                                      next_t_out=self.t_dev.data_ptr())
                    if self.recv_inc is not None:
                        b.file_inc = dict(b.file_inc, recv_inc_out=self.recv_inc.data_ptr())
                    if self.pipe:
                        # counter hand-over without a launch writing a scalar it reads: the env head reads the masters (t_dev, rng_ctr)
                        # and writes the copies (t_store, rng_copy); the inc head reads the copies and writes the masters' next values
                        b.file_env = dict(b.file_env, t_index=self.t_dev.data_ptr(), t_copy_out=self.t_store.data_ptr(),
                                          step_copy_out=self.rng_copy.data_ptr())
                        b.file_inc = dict(b.file_inc, next_step_out=self.rng_ctr.data_ptr())
                        b.file_inc_last = dict(b.file_inc_last, next_step_out=self.rng_ctr.data_ptr())
            self._bundles[key] = b
        self._bundle, self.cur, self._ss, self._ss_last, self._graph = b, b.cur, b.ss, b.ss_last, b.graph

    def _pick(self, q, avail_mask, idx_table, k):
        """epsilon-greedy (action_selectors.py:44-68) without host sync: random AVAILABLE action = table[floor(u * k)]."""
        if avail_mask is not None:
            q = q.masked_fill(avail_mask == 0, -float("inf"))
        greedy = q.argmax(dim=-1)
        u = th.rand(greedy.shape, device=q.device)
        r = th.clamp((th.rand(greedy.shape, device=q.device) * k).long(), max=k - 1)
        rand = idx_table[r] if idx_table is not None else r
        return th.where(u < self.eps, rand, greedy)

    def _fast_stages(self, store_env_step):
        """The launches of one timestep with the FastPolicy kernels, in order, as (kernel name, key, closure).  Fused path
        (default): k_encode reads obs[:, t] from the storage where the env kernel put it, the two head kernels file actions / pose /
        rewards into slot t and carry the previous-step inputs, return and counters themselves -- a timestep is 4 launches
        (encode, env head, env step+observe, inc head), or 3 when pipelined (self.pipe: env head, env step+observe, inc head of t +
        encoder of t + 1 as one launch).  Otherwise one store-step launch writes the nine small fields.
        The pipelined timestep differs from the four-launch one in three things only: no encoder launch of its own, the input buffer
        `buf` (its parity instead of 0) and the draw counter the inc head reads (the env head's copy instead of the master)."""
        st = self.store.data.transition_data
        td = self.t_dev
        fast, bundle, pipe, fused = self.fast, self._bundle, self.pipe, self.fast.fused
        obs, pos, orient = self.cur["obs"], self.cur["pos"], self.cur["orient"]
        codes = st["obs"] if self.obs_fmt == abi.OBS_CODE else self.cur.get("code")     # what the fused encoder reads
        actions = fast.actions
        pos_t, orient_t = self.pos_t, self.orient_t                     # forward_inc sees the PRE-step pose (controller :78-82)
        par = self._par
        buf = par if pipe else 0                                        # pipelined: the buffer of a timestep is its parity
        inc_step = self.rng_copy if pipe else self.rng_ctr
        inc_encode = pipe and store_env_step                            # slot T: nothing left to encode

        def encode():
            if self.direct_obs:     # the observation is already in the storage; the encoder reads its class codes
                fast.encode(None, codes=codes, slot_t=td, t_copy=self.t_store, counter_inc=self.rng_ctr if self.fold_store else None)
            else:
                fast.encode(obs, codes=codes, store_obs=st["obs"], store_t=td)

        def env_head():
            extra = dict(orient=orient, actions_i32=self.actions_i32, pos_copy=pos_t, orient_copy=orient_t) if fused else {}
            fast.head_env(self.prev_actions, self.prev_reward, self.prev_inc, pos, self.eps, self.rng_ctr, file=bundle.file_env,
                          buf=buf, par=par, q_out=self.q_env, eps_rows=self.eps_rows, **extra)

        def env_step():
            if not fused:
                pos_t.copy_(pos); orient_t.copy_(orient)
                self.actions_i32.copy_(actions)
            if store_env_step:
                self.env.step_batch(self.actions_i32, observe=True, fmt=self.obs_fmt, out=self.cur if self.direct_obs else None)

        def inc_head():
            if store_env_step:
                out = self.env.native.out
                reward, clean, den = out["reward"], out["clean_num"], out["apple_den"]
            else:       # slot T: zeros for reward / clean_num / apple_den
                reward = clean = den = self._zeros_nn
            file = bundle.file_inc if store_env_step else bundle.file_inc_last
            if inc_encode:
                fast.act_inc_encode(actions, pos_t, orient_t, reward, clean, den, self.eps, inc_step, codes, slot_t=self.t_store, slot_add=1,
                                    buf=buf, file=file, par=par, q_out=self.q_inc, eps_rows=self.eps_rows)
            else:
                fast.act_inc(actions, pos_t, orient_t, reward, clean, den, self.eps, inc_step, file=file, buf=buf, par=par, q_out=self.q_inc,
                             eps_rows=self.eps_rows)

        def store_hidden():     # train_stored_state: the state after slot t, behind the inc head that produced it
            ops.store_hidden(bundle.hidden, self.env.device)

        return ([] if pipe else [("ssd::k_encode", "encode", encode)]) + [("ssd::k_head<env>", "head_env", env_head)] + \
            ([("ssd::k_env<MODE_STEP_OBS>", "env", env_step)] if store_env_step or not pipe else []) + \
            [("ssd::k_inc_encode", "inc_encode", inc_head) if inc_encode else ("ssd::k_head<inc>", "head_inc", inc_head)] + \
            ([("ssd::k_store_hidden", "store_hidden", store_hidden)] if self.stored_state else []) + \
            ([("ssd::k_rollout_priority_seq" if self.priority_windows else "ssd::k_rollout_priority", "rollout_priority", self._rollout_priority)]
             if self.initial_priority and self.fold_store else [])

    def _rollout_priority(self):
        """per_initial_priority "rollout": row t - 1 of the one-step TD errors from this slot's Q-values, behind the launches that
        filed slot t's actions and before the slot index is advanced"""
        ops.rollout_priority(self._bundle.priority, self.env.device)

    def initial_priorities(self):
        """int32 [N] (per_unit "window": [N, S], one per window of the grid): the fixed-point priorities of the episodes the last
        TRAINING rollout produced (ssd_rollout_priority), for
        ReplayBuffer.insert_episode_batch; None with per_initial_priority "max" (or after a test episode): the slots are zeroed"""
        if not self._ready or not self.initial_priority or getattr(self, "_test_mode", True):
            return None
        return self._bundle.priority_state["q_init"]

    def timestep_launches(self):
        """(kernel name, key, closure) of the launches of one rollout timestep on the live buffers -- what the rollout hipGraph was
        captured from; bench.py times them one by one with HIP events (a graph replay has no host call to bracket)."""
        if self.fast is None or not self.fast.fused or not self.fold_store:
            return []
        self._par = self.t & 1
        return self._fast_stages(True)

    def _select_fast(self, store_env_step):
        """_select with the FastPolicy kernels (see _fast_stages)."""
        td = self.t_dev
        for _, _, fn in self._fast_stages(store_env_step):
            fn()
        if self.fold_store:
            return
        ss = self._ss if store_env_step else self._ss_last
        # ONE launch: the nine small fields of slot t, the controller's "previous step" inputs, the episode return and the
        # time / exploration counters (incremented after every block has read t)
        abi.check(self.fast.lib, self.fast.lib.ssd_store_step_launch(C.byref(ss), th.cuda.current_stream(self.env.device).cuda_stream))
        if self.initial_priority:       # the store step filed slot t's actions; the counters are advanced below / by the next encoder
            self._rollout_priority()
        if not self.direct_obs:     # without the encoder's t copy the counters are advanced by two small torch kernels
            self.rng_ctr += 1
            if store_env_step:
                td += 1

    def _make_store_args(self, with_step_outputs):
        st, out, fp = self.store.data.transition_data, self.env.native.out, self.fast
        ss = abi.SsdStoreStep()
        ss.t_index = self.t_dev.data_ptr()
        ss.n_env, ss.n_agents, ss.n_actions, ss.t_slots = self.batch_size, self.args.n_agents, self.args.n_actions, self.episode_limit + 1
        ss.actions, ss.actions_inc = fp.actions.data_ptr(), fp.actions_inc.data_ptr()
        ss.pos, ss.orient = self.pos_t.data_ptr(), self.orient_t.data_ptr()
        ss.dst_pos, ss.dst_orient = st["agent_pos"].data_ptr(), st["agent_orientation"].data_ptr()
        if self.direct_obs:
            ss.t_index, ss.counter_inc = self.t_store.data_ptr(), self.rng_ctr.data_ptr()
        ss.dst_actions, ss.dst_actions_onehot, ss.dst_actions_inc = st["actions"].data_ptr(), st["actions_onehot"].data_ptr(), st["actions_inc"].data_ptr()
        if with_step_outputs:
            ss.reward, ss.clean_num, ss.apple_den, ss.terminated = (out["reward"].data_ptr(), out["clean_num"].data_ptr(),
                                                                      out["apple_den"].data_ptr(), out["terminated"].data_ptr())
            ss.dst_reward, ss.dst_clean_num, ss.dst_apple_den, ss.dst_terminated = (st["reward"].data_ptr(), st["clean_num"].data_ptr(),
                                                                                    st["apple_den"].data_ptr(), st["terminated"].data_ptr())
            ss.prev_actions, ss.prev_reward, ss.prev_actions_inc = (self.prev_actions.data_ptr(), self.prev_reward.data_ptr(),
                                                                    self.prev_inc.data_ptr())
            ss.ep_return = self.ep_return.data_ptr()
            if self.direct_obs:
                ss.next_t_out = self.t_dev.data_ptr()
        return ss

    def _select(self, store_env_step):
        """One controller evaluation on the current observation; with store_env_step also the env transition."""
        if self.fast is not None:
            return self._select_fast(store_env_step)
        a, mac, st = self.args, self.mac, self.store.data.transition_data
        td = self.t_dev
        obs, pos, orient = self.cur["obs"], self.cur["pos"], self.cur["orient"]
        st["obs"].index_copy_(1, td, obs.unsqueeze(1))
        st["agent_pos"].index_copy_(1, td, pos.unsqueeze(1))
        st["agent_orientation"].index_copy_(1, td, orient.unsqueeze(1))
        feat = mac.encode_obs(obs)
        inputs = mac.assemble_inputs(feat, self.prev_actions, self.prev_reward, self.prev_inc, pos, False)
        q_env, h_env, _ = mac.agent.forward_env(inputs, self.h_env)
        self.h_env.copy_(h_env)
        actions = self._pick(q_env, self.avail_mask, self.avail_idx, self.avail_idx.numel())      # [N, n]
        pos_t, orient_t = pos.clone(), orient.clone()                   # forward_inc sees the PRE-step pose (controller :78-82)
        if store_env_step:
            out = self.env.step_batch((actions % a.n_actions).to(th.int32), observe=True, fmt=self.obs_fmt)
            reward, clean, den = out["reward"], out["clean_num"], out["apple_den"]
            st["reward"].index_copy_(1, td, reward.unsqueeze(1))
            st["terminated"].index_copy_(1, td, out["terminated"].reshape(-1, 1, 1))
            st["clean_num"].index_copy_(1, td, clean.unsqueeze(1))
            st["apple_den"].index_copy_(1, td, den.unsqueeze(1))
            self.ep_return += reward
        else:   # slot T: the batch holds zeros for reward / clean_num / apple_den (episode_runner.py:108-119)
            reward = clean = den = th.zeros_like(self.prev_reward)
        onehot = F.one_hot(actions, num_classes=a.n_actions)
        st["actions"].index_copy_(1, td, actions.reshape(actions.shape[0], 1, -1, 1))
        st["actions_onehot"].index_copy_(1, td, onehot.float().unsqueeze(1))
        q_inc, h_inc, _ = mac.agent.forward_inc(inputs, self.h_inc, onehot, pos_t / mac.pos_scale, orient_t, reward.unsqueeze(-1),
                                                clean.unsqueeze(-1), den.unsqueeze(-1))
        self.h_inc.copy_(h_inc)
        if self.stored_state:       # both states of slot t are in place; t_dev is advanced below
            ops.store_hidden(self._bundle.hidden, self.env.device)
        actions_inc = self._pick(q_inc, None, None, a.n_inc_actions) * self.inc_mask              # [N, n, n]
        st["actions_inc"].index_copy_(1, td, actions_inc.reshape(actions_inc.shape[0], 1, actions_inc.shape[1], -1, 1))
        if self.initial_priority:       # slot t is filed; t_dev is advanced below
            self.q_env.copy_(q_env.reshape(self.q_env.shape))
            self.q_inc.copy_(q_inc.reshape(self.q_inc.shape))
            self._rollout_priority()
        if store_env_step:
            self.prev_actions.copy_(actions)
            self.prev_reward.copy_(reward)
            self.prev_inc.copy_(actions_inc)
            td += 1

    # ---- runner surface ---------------------------------------------------------------------------------------------
    def begin_episode(self, test_mode=False):
        if not self._ready:
            self._allocate()
        self._test_mode = test_mode
        store = self._replay.reserve(self.batch_size) if (self._replay is not None and not test_mode) else None
        if store is None:
            if self._own_store is None:
                self._own_store = EpisodeBatch(self._scheme, self._groups, self.batch_size, self.episode_limit + 1,
                                               preprocess=self._preprocess, device=self.args.device)
            store = self._own_store
        self._bind_store(store)
        self.batch = self.store
        sel = self.mac.action_selector
        sel.epsilon = 0.0 if test_mode else sel.schedule.eval(self.sched_t)
        zero_after = getattr(self.args, "epsilon_zero", None)
        if zero_after is not None and self.t_env > zero_after:
            sel.epsilon = 0.0
        self.t = 0
        self._episodes += 1
        b = self._bundle
        if self._begin_recording(test_mode):
            # a recorded test episode takes the eager launch sequence (no graph is replayed or captured): frame t is one ssd_render
            # launch after the env step of t
            self._begin_launches()
            self._set_eps(sel.epsilon)
            self._recorder.frame()
            return
        # The episode's opening launches (env reset + first observation, the runner state's fills, the weight packs, the encoder of
        # slot 0) and its closing ones (slot-T pass, statistics) are ~25 small launches the host issues one by one while the GPU waits
        # for them (0.4 of a 7.5 ms iteration); from the third episode of a storage on they are two more hipGraph replays.
        if b.begin_graph is not None:
            self._set_eps(sel.epsilon)
            b.begin_graph.replay()
            return
        self._begin_launches()
        self._set_eps(sel.epsilon)
        if self._graph is None and self._episodes >= 2 and getattr(self.args, "rollout_graph", True) and self._graph_steps_planned:
            th.cuda.synchronize()
            g = th.cuda.CUDAGraph()
            # K consecutive timesteps per graph (the device-side time index makes every step of the replay land in its own
            # slot); K divides the episode length, so an episode is episode_limit / K replays
            K = self._graph_steps_planned
            self._graph_steps = K
            with th.no_grad(), ops.capture(g, capture_error_mode="thread_local"):
                for k in range(K):
                    self._par = k & 1        # a replay starts at a multiple of K (even when pipelined)
                    self._select(True)
            self._graph = self._bundle.graph = g
            # capture records but does not run: re-establish the episode start state
            self.t_dev.zero_()
        elif (self._graph is not None and self.fast is not None and getattr(self.fast, "_pack_graph", None) is not None
              and getattr(self.args, "rollout_graph", True) and getattr(self.args, "episode_edge_graphs", True)):
            # third episode of this storage: everything is warm (the pack graph exists) -- capture the opening launches; they were
            # just run eagerly for THIS episode, the capture itself runs nothing
            th.cuda.synchronize()
            g = th.cuda.CUDAGraph()
            with th.no_grad(), ops.capture(g, capture_error_mode="thread_local"):
                self._begin_launches(in_capture=True)
            b.begin_graph = g

    def _set_eps(self, epsilon):
        """the episode's exploration rate: the device scalar and, under epsilon_ladder_alpha, the table of the envs' own rates
        eps ** (1 + alpha g / (G - 1)) from it -- one device op, no upload (the host runs several rollouts ahead of the device)"""
        self.eps.fill_(epsilon)
        if self.eps_rows is not None:
            th.pow(self.eps, self.expo, out=self.eps_rows)

    def _stat_extra(self, test_mode):
        return 4 if (not test_mode and float(getattr(self.args, "epsilon_ladder_alpha", 0.0) or 0.0) > 0.0) else 0

    def _ladder_greedy_envs(self):
        """the rank's ceil(N / 8) highest-id envs: the greediest rungs of the ladder"""
        return -(-self.batch_size // 8)

    def _stats_device(self, out, ep_return, test_mode):
        super()._stats_device(out, ep_return, test_mode)
        if self._stat_extra(test_mode):     # the same sums over the greediest eighth of the envs, behind the four of all envs
            k = self._ladder_greedy_envs()
            ops.runner_stats(out["collective_return"][-k:], out["equality"][-k:], ep_return[-k:], self._stat_buf(test_mode)[4:])

    def _log_extra(self, sums, stats, prefix, test_mode):
        if len(sums) == 4:
            # return_mean now mixes rates from epsilon down to epsilon ** (1 + alpha); this stays comparable with near-greedy play
            rollouts = max(1, stats["n_episodes"] // self.batch_size)
            self.logger.log_stat("ladder_greedy_return_mean", sums[0] / (rollouts * self._ladder_greedy_envs()), self.t_env)
            eps = float(self.mac.action_selector.epsilon)
            self.logger.log_stat("epsilon_ladder_min", eps ** (1.0 + self.ladder_alpha) if eps > 0.0 else 0.0, self.t_env)

    def _begin_launches(self, in_capture=False):
        """the device work that opens an episode on the bound storage (everything but the epsilon scalar, which the host computes)"""
        self.env.reset_batch()
        self.env.observe_batch(self.obs_fmt, out=self.cur if getattr(self, "direct_obs", False) else None)   # fills self.cur (or obs[:, 0])
        # the runner state an episode opens with, as ONE launch: time index, previous actions (-1) / reward / incentive actions, the
        # episode returns, the hidden states (the generic timestep's, or FastPolicy's own)
        hidden = [self.h_env, self.h_inc] if self.fast is None else [self.fast.h_env, self.fast.h_inc]
        ops.fill_blocks([(self.t_dev, 0), (self.prev_actions, 0xFFFFFFFF), (self.prev_reward, 0), (self.prev_inc, 0), (self.ep_return, 0)]
                        + ([(self.recv_inc, 0)] if self.recv_inc is not None else []) + [(h, 0) for h in hidden]
                        + ([(self.fast.prev_rec, 0xFFFFFFFF)] if self.fast is not None and self.fast.prev_rec is not None else []))
        if self.fast is not None:
            if in_capture:
                self.fast._pack_eager()   # the learner may have stepped the weights since the last episode (packs are shared)
            else:
                self.fast.pack()
        if self.pipe:       # the encoder runs one timestep ahead of the heads: the observation of slot 0 is encoded here
            with th.no_grad():
                codes = self.store.data.transition_data["obs"] if self.obs_fmt == abi.OBS_CODE else self.cur["code"]
                self.fast.encode(None, codes=codes, slot_t=self.t_dev, buf=0)

    @th.no_grad()
    def step_once(self):
        if self.t >= self.episode_limit:
            raise RuntimeError("step_once() past episode_limit: the episode storage has no slot left (finish_episode / begin_episode first)")
        if self._graph is not None and not self._recording:
            if self.t % self._graph_steps == 0:       # one replay advances _graph_steps timesteps
                self._graph.replay()
        else:
            self._par = self.t & 1
            self._select(True)
            if self._recording:
                self._recorder.frame()
        self.t += 1
        return self.t >= self.episode_limit

    @th.no_grad()
    def finish_episode(self):
        self._par = self.t & 1
        b = self._bundle
        self._out = dict(collective_return=self.env.native.out["collective_return"], equality=self.env.native.out["equality"])
        self._ep_return = self.ep_return
        stats_on = bool(getattr(self.args, "runner_stats", True))
        if b.finish_graph is not None and not self._test_mode:
            b.finish_graph.replay()                                     # the slot-T pass + this rollout's statistics
            self._stats_on_device_done = stats_on
            return self._finish_stats()
        self._select(False)
        self._finish_recording()
        if (b.begin_graph is not None and b.finish_graph is None and not self._test_mode and self._par == 0
                and getattr(self.args, "episode_edge_graphs", True)):
            # the closing launches of a training episode on this storage as a graph (captured after they ran eagerly for this episode)
            if stats_on:
                self._stat_acc(False)                                   # the accumulator exists before the capture
            th.cuda.synchronize()
            g = th.cuda.CUDAGraph()
            with ops.capture(g, capture_error_mode="thread_local"):
                self._select(False)
                if stats_on:
                    self._stats_device(self._out, self._ep_return, False)
            b.finish_graph = g
        return self._finish_stats()
