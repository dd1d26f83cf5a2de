"""HipVecRunner: episode rollouts of N vectorised envs resident on the GPU, behind the reference's runner surface
(src/runners/episode_runner.py:7-152: __init__(args, logger), setup, get_env_info, run(test_mode) -> EpisodeBatch,
reset, close_env, save_replay, attrs t_env / batch_size).

Per timestep (episode_runner.py:57-97): store obs -> env-head action selection -> env.step -> store rewards ->
incentive-head action selection -> store.  Here the env transition and the observation of the NEXT state come from one
fused kernel launch (ssd_step_observe) and nothing leaves the device.  `runner: "episode"` is the same loop with the
reference's restriction batch_size_run == 1.
"""
import os
from functools import partial

import torch as th

from .. import abi
from ..components.episode_buffer import EpisodeBatch
from ..envs import REGISTRY as env_REGISTRY


class HipVecRunner:
    single_env_only = False
    fixed_length_episodes = True       # the SSD envs terminate at episode_limit only: every stored episode fills all T + 1 slots

    def __init__(self, args, logger):
        self.args, self.logger = args, logger
        self.batch_size = args.batch_size_run
        if self.single_env_only:
            assert self.batch_size == 1                                   # episode_runner.py:13
        env_args = dict(args.env_args)
        # replay_envs: the envs whose test episodes are recorded when the env is in render mode (render / is_replay)
        self.replay_envs = list(env_args.pop("replay_envs", None) or [0])
        env_args.setdefault("n_env", self.batch_size)
        env_args.setdefault("device", getattr(args, "device_index", 0))
        env_args.setdefault("env_id_base", getattr(args, "env_id_base", 0))
        self.env = env_REGISTRY[args.env](**env_args)
        self.episode_limit = self.env.episode_limit
        self.t = 0
        self.t_env = 0
        self.rollouts = 0          # training rollouts finished (schedule_unit "rollouts": the epsilon clock, see sched_t)
        self.train_returns, self.test_returns = [], []          # reference attributes; the statistics live on the device (_finish_stats)
        self.train_stats, self.test_stats = {}, {}
        self.log_train_stats_t = -1000000
        # obs_storage: "code" keeps observations as u8 class codes (simplified palette; 12x fewer bytes in the storage and the
        # replay buffer); the controller expands them where it consumes them
        self.obs_fmt = abi.OBS_CODE if getattr(self.args, "obs_storage", "f32") == "code" else abi.OBS_F32
        self._recorder, self._recording, self.replays = None, False, []

    @property
    def sched_t(self):
        """The clock of the epsilon schedule (epsilon_schedules.py; reference: t_env, episode_runner.py:72).  The reference only
        ever runs ONE env, where t_env advances by episode_limit per rollout and per learner.train.  schedule_unit "env_steps"
        keeps that literally; "rollouts" (the default for batch_size_run > 1, run.py setup) advances the clock by episode_limit per
        ROLLOUT, so that epsilon_anneal_time spans the same number of rollouts / optimisation steps as in the reference instead of
        collapsing to the first rollout (4096 envs x 100 steps >> 50000)."""
        if getattr(self.args, "schedule_unit", "env_steps") == "rollouts":
            return self.rollouts * self.episode_limit
        return self.t_env

    def setup(self, scheme, groups, preprocess, mac):
        self.new_batch = partial(EpisodeBatch, scheme, groups, self.batch_size, self.episode_limit + 1, preprocess=preprocess,
                                 device=self.args.device)
        self.mac = mac
        self.store_state = "state" in scheme and getattr(self.args, "store_state", True)

    def get_env_info(self):
        return self.env.get_env_info()

    def save_replay(self, out_dir=None):
        """Recorded test episodes (render mode) -> <local_results_path>/replays/replay-<timestamp>/episode_<i>/env_<e>/ (<k>.png,
        frames.npz, replay.gif); without recordings, the env's own replay (n_env = 1, is_replay)."""
        if not self.replays:
            return self.env.save_replay()
        from ..utils import replay
        out_dir = out_dir or replay.replay_dir(getattr(self.args, "local_results_path", "results"))
        for i, rec in enumerate(self.replays):
            replay.write_replay(os.path.join(out_dir, "episode_%d" % i), rec, self.env.env_name, self.replay_envs)
        self.replays = []
        return out_dir

    # ---- replay recording (test episodes of a render-mode env) ----------------------------------------------------
    def _begin_recording(self, test_mode):
        self._recording = bool(test_mode and getattr(self.env, "native", None) is not None and self.env.native.render_on)
        if self._recording:
            if self._recorder is None:
                from ..utils.replay import ReplayRecorder
                self._recorder = ReplayRecorder(self.env.native, self.replay_envs, self.episode_limit)
            self._recorder.begin()
        return self._recording

    def _finish_recording(self):
        if self._recording:
            self.replays.append(self._recorder.finish(self.batch))
            self._recording = False

    def close_env(self):
        self.env.close()

    def reset(self):
        self.batch = self.new_batch()
        self.env.reset_batch()
        self.t = 0

    def _store_observation(self, o, t):
        data = {"avail_actions": self.env.avail_actions_batch, "obs": o["obs"], "agent_pos": o["pos"], "agent_orientation": o["orient"]}
        if self.store_state:
            data["state"] = self.env.observe_batch(self.obs_fmt, want_state=True)["state"]
        self.batch.update(data, ts=t)

    # The rollout is exposed timestep by timestep (begin_episode / step_once / finish_episode) so that a caller such as
    # bench.py can time an exact number of transitions; run() is the reference-shaped whole-episode call.
    def begin_episode(self, test_mode=False):
        self.reset()
        self._test_mode = test_mode
        self._ep_return = th.zeros(self.batch_size, self.args.n_agents, device=self.env.device)
        self.mac.init_hidden(batch_size=self.batch_size)
        self._o = self.env.observe_batch(self.obs_fmt)
        self._out = None
        if self._begin_recording(test_mode):
            self._recorder.frame()                                      # frame 0: the state after the reset

    @th.no_grad()
    def step_once(self):
        t, test_mode = self.t, self._test_mode
        self._store_observation(self._o, t)
        actions = self.mac.select_actions_env(self.batch, t_ep=t, t_env=self.sched_t, test_mode=test_mode)
        out = self.env.step_batch((actions.squeeze(-1) % self.args.n_actions).to(th.int32), observe=True, fmt=self.obs_fmt)
        self._ep_return += out["reward"]
        # `terminated` is stored as the env flag: episode_limit never appears in info (episode_runner.py:83)
        self.batch.update({"actions": actions, "reward": out["reward"], "terminated": out["terminated"].unsqueeze(-1),
                           "clean_num": out["clean_num"], "apple_den": out["apple_den"]}, ts=t)
        actions_inc = self.mac.select_actions_inc(actions, self.batch, t_ep=t, t_env=self.sched_t, test_mode=test_mode)
        self.batch.update({"actions_inc": actions_inc}, ts=t)
        self._o = self._out = out
        if self._recording:
            self._recorder.frame()
        self.t += 1
        return self.t >= self.episode_limit

    @th.no_grad()
    def finish_episode(self):
        """slot T: last observation and the bootstrapping actions (episode_runner.py:99-119), then stats."""
        test_mode = self._test_mode
        self._store_observation(self._o, self.t)
        actions = self.mac.select_actions_env(self.batch, t_ep=self.t, t_env=self.sched_t, test_mode=test_mode)
        actions_inc = self.mac.select_actions_inc(actions, self.batch, t_ep=self.t, t_env=self.sched_t, test_mode=test_mode)
        self.batch.update({"actions_inc": actions_inc}, ts=self.t)
        self.batch.update({"actions": actions}, ts=self.t)
        self._finish_recording()
        return self._finish_stats()

    def _finish_stats(self):
        """Episode statistics of episode_runner.py:121-152 (collective_return / equality_metric / ep_length sums over the episodes,
        mean and standard deviation of the per-agent returns), accumulated ON THE DEVICE: a rollout adds its sums to a small f64
        tensor with a handful of device ops and no host synchronisation; the host reads the tensor once per log interval (_log)."""
        test_mode = self._test_mode
        out, ep_return = self._out, self._ep_return
        stats = self.test_stats if test_mode else self.train_stats
        prefix = "test_" if test_mode else ""
        if getattr(self.args, "runner_stats", True):
            if not getattr(self, "_stats_on_device_done", False):
                self._stats_device(out, ep_return, test_mode)
            self._stats_on_device_done = False
            stats["n_episodes"] = self.batch_size + stats.get("n_episodes", 0)
            stats["ep_length"] = self.t * self.batch_size + stats.get("ep_length", 0)
            stats["n_returns"] = ep_return.numel() + stats.get("n_returns", 0)
        if getattr(self.args, "behaviour_stats", False):
            self._behaviour_device(test_mode)
        if not test_mode and self._reward_model_on():
            self._reward_model_device()
        if not test_mode:
            self.t_env += self.t * self.batch_size
            self.rollouts += 1
        if getattr(self.args, "runner_stats", True):
            if test_mode and stats["n_episodes"] >= self.args.test_nepisode:
                self._log(stats, prefix, test_mode)
            # runner_log_interval is measured on the schedule clock: under schedule_unit "rollouts" a rollout of all envs advances it
            # by episode_limit, so the host reads the device sums every runner_log_interval / episode_limit rollouts (the reference's
            # cadence) instead of after every rollout (4096 envs advance t_env by 409 600)
            elif not test_mode and self.sched_t - self.log_train_stats_t >= self.args.runner_log_interval:
                self._log(stats, prefix, test_mode)
                if hasattr(self.mac.action_selector, "epsilon"):
                    self.logger.log_stat("epsilon", self.mac.action_selector.epsilon, self.t_env)
                self.log_train_stats_t = self.sched_t
        return self.batch

    def _stats_device(self, out, ep_return, test_mode):
        """the device side of _finish_stats: this rollout's sums added to the accumulator (a handful of launches, no synchronisation;
        the graph runner replays them as part of its episode-closing graph)"""
        from .. import ops
        ops.runner_stats(out["collective_return"], out["equality"], ep_return, self._stat_acc(test_mode))

    def _stat_buf(self, test_mode):
        """the device accumulator of a mode as the host reads it (_log): the four sums of _stat_acc and, behind them, whatever
        _stat_extra says the runner accumulates as well -- one tensor, so a log event stays one device -> host read"""
        key = "_acc_test" if test_mode else "_acc_train"
        if getattr(self, key, None) is None:
            setattr(self, key, th.zeros(4 + self._stat_extra(test_mode), dtype=th.float64, device=self.env.device))
        return getattr(self, key)

    def _stat_extra(self, test_mode):
        return 0

    def _stat_acc(self, test_mode):
        """device accumulator [sum collective_return, sum equality_metric, sum of returns, sum of squared returns]"""
        return self._stat_buf(test_mode)[:4]

    # ---- behaviour statistics (config key behaviour_stats, default off) ---------------------------------------------------------------
    def _behaviour_acc(self, test_mode):
        """(f64 accumulator [abi.behaviour_len(n, A)], int64 workspace) of ssd_behaviour_stats, one pair per mode, allocated on first use"""
        from .. import ops
        key = "_beh_test" if test_mode else "_beh_train"
        if getattr(self, key, None) is None:
            n, A = self.args.n_agents, self.args.n_actions
            setattr(self, key, (th.zeros(abi.behaviour_len(n, A), dtype=th.float64, device=self.env.device),
                                ops.behaviour_workspace(n, A, self.env.device)))
        return getattr(self, key)

    def _behaviour_device(self, test_mode):
        """this rollout's per-agent behaviour statistics added to the accumulator: two eager launches over the episode's storage
        (self.batch: the runner's own, or the replay buffer's reserved slots), on the current stream, never inside a stream capture"""
        from .. import ops
        if th.cuda.is_available() and th.cuda.is_current_stream_capturing():
            raise RuntimeError("behaviour_stats is launched eagerly: _finish_stats was reached inside a stream capture")
        st = self.batch.data.transition_data
        acc, ws = self._behaviour_acc(test_mode)
        ops.behaviour_stats(st["actions"], st["actions_inc"], st["reward"], st["clean_num"], self.args.n_actions, acc, ws)

    # ---- reward model (config key reward_model, default "individual" = off) -------------------------------------------------------------
    def _reward_model_on(self):
        """the predicate of the learner and the scheme (ops.reward_field): a model is named (absent, None and "individual" are off)"""
        from .. import ops
        return ops.reward_field(self.args) != "reward"

    def _reward_model_device(self):
        """this training rollout's rewards shaped by the reward model, storage field "reward" -> "reward_model" (what the loss reads):
        one eager launch over the episode's storage (self.batch: the runner's own, or the replay buffer's reserved slots) before the
        batch is returned for insertion, on the current stream, never inside a stream capture.  The launch adds the per-(env, agent)
        sums of the shaped reward and of its two model terms to an f64 accumulator that _log reads and zeroes."""
        from .. import ops
        if th.cuda.is_available() and th.cuda.is_current_stream_capturing():
            raise RuntimeError("reward_model is launched eagerly: _finish_stats was reached inside a stream capture")
        st = self.batch.data.transition_data
        if getattr(self, "_reward_acc", None) is None:
            self._reward_acc = th.zeros(self.batch_size, self.args.n_agents, 3, dtype=th.float64, device=st["reward"].device)
            self._reward_rollouts = 0
        a = self.args
        if getattr(a, "reward_model_scalars", None) is None:        # a runner built without run.setup
            a.reward_model_scalars = ops.social_reward_scalars(a.reward_model, a.n_agents, **{k: getattr(a, k) for k in (
                "ia_alpha", "ia_beta", "ia_decay", "prosocial_weight") if hasattr(a, k)})
        ops.social_reward(st["reward"], st["reward_model"], a.reward_model, a.reward_model_scalars, self._reward_acc)
        self._reward_rollouts += 1

    def reward_model_means(self, reset=True):
        """{name: mean} of the shaped reward and of its two model terms per (env, slot < T, agent) over the training rollouts since the
        accumulator was last zeroed ({} before the first).  The accumulator [N, n, 3] is copied to the host once and each column summed
        there in a stated order -- ascending (env, agent), left to right from 0 (a running sum, not a tree) -- then divided once by the
        count, so a logged mean equals its restatement in plain loops to the bit.  Synchronises; eager, outside any capture."""
        if getattr(self, "_reward_acc", None) is None or not self._reward_rollouts:
            return {}
        import numpy as np
        cells = self._reward_acc.cpu().numpy().reshape(-1, 3)
        sums = np.add.accumulate(cells, axis=0)[-1].tolist()         # accumulate is sequential: ((c0 + c1) + c2) + ...
        count = float(self._reward_rollouts * self.batch_size * self.episode_limit * self.args.n_agents)
        if reset:
            self._reward_acc.zero_()
            self._reward_rollouts = 0
        names = ("reward_model_mean", "ia_envy_mean", "ia_guilt_mean") if self.args.reward_model == "inequity_aversion" else ("reward_model_mean", "prosocial_others_mean")
        return {k: v / count for k, v in zip(names, sums)}

    def behaviour(self, test_mode=False, reset=False):
        """The behaviour accumulator of the training (or test) episodes since it was last zeroed, by block name (abi.behaviour_layout):
        dict[str, np.ndarray] of f64 integers.  Synchronises.  Rank-local under data parallelism, like the other runner statistics."""
        if not getattr(self.args, "behaviour_stats", False):
            raise RuntimeError("runner.behaviour() needs the config key behaviour_stats")
        acc, _ = self._behaviour_acc(test_mode)
        blocks = abi.behaviour_blocks(acc.cpu().numpy(), self.args.n_agents, self.args.n_actions)
        if reset:
            acc.zero_()
        return blocks

    def run(self, test_mode=False):
        self.begin_episode(test_mode)
        while not self.step_once():
            pass
        return self.finish_episode()

    def _log(self, stats, prefix, test_mode):
        acc = self._stat_buf(test_mode)
        sums = acc.cpu().tolist()                       # the one device -> host read of the log interval
        coll, eq, rs, rss = sums[:4]
        acc.zero_()
        n_ep, n_ret = stats["n_episodes"], max(1, stats.get("n_returns", 0))
        mean = rs / n_ret
        self.logger.log_stat(prefix + "return_mean", mean, self.t_env)
        self.logger.log_stat(prefix + "return_std", max(0.0, rss / n_ret - mean * mean) ** 0.5, self.t_env)    # np.std: population
        for k, v in (("collective_return", coll), ("equality_metric", eq), ("ep_length", stats.get("ep_length", 0))):
            self.logger.log_stat(prefix + k + "_mean", v / n_ep, self.t_env)
        self._log_extra(sums[4:], stats, prefix, test_mode)
        if getattr(self.args, "behaviour_stats", False):
            bacc, _ = self._behaviour_acc(test_mode)
            vec = bacc.cpu().numpy()
            bacc.zero_()
            for k, v in abi.behaviour_summary(vec, self.args.n_agents, self.args.n_actions).items():
                self.logger.log_stat(prefix + k, v, self.t_env)
        if not test_mode and self._reward_model_on():
            for k, v in self.reward_model_means().items():
                self.logger.log_stat(k, v, self.t_env)
        stats.clear()

    def _log_extra(self, sums, stats, prefix, test_mode):
        """what a runner logs from the sums behind the first four (_stat_extra)"""


class EpisodeRunner(HipVecRunner):
    """`runner: "episode"`: one env, as the reference asserts (episode_runner.py:13)."""
    single_env_only = True
