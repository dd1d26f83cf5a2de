"""One rank of a data-parallel test job (a helper, no test in it; tests/dp_util.run_ranks starts it):

    python -m tests.dp_worker --case NAME --rank R --world W --port P --device cpu|cuda --out DIR

For W > 1 (and for the forced one-rank case) the rank joins a gloo group -- gloo carries device tensors, so two ranks share one GPU --
builds ITS SHARD of a golden fixture (tests/learner_util.build(..., sl=...)) or its own training loop (run.setup), runs the case and
writes DIR/rank<R>.npz: the logged values of every step (added over the group by _FusedLogs.synced where the learner is distributed),
the parameter checksums, the flat parameters, both optimisers' state, the flat gradient as clip_and_step met it (after the
all-reduce), the priority results, and the number of dist.all_reduce calls this rank issued.  It asserts nothing about numbers (the
tests do, against the reference recordings and the CPU tensor-op learner); it reads tests/golden/ only."""
import argparse
import os
import sys
import time
from datetime import timedelta

import numpy as np
import torch as th
import torch.distributed as dist

from homophily_marl_amd.learners.homophily_learner import _FusedLogs

LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")
ROWS_OF_EPISODES = [4, 1, 6, 3]                       # where the four episodes lie among the decoy rows of a window case's buffer
PRIORITY_IDS = [[5, 1], [3, 3]]                       # per rank, into its own 8-entry table (rank 1: both samples name one slot)
PRIORITY_WEIGHTS = [[1.0, 0.37], [0.61, 0.25]]
TABLE_LEN = 8
LOOP_ENVS, LOOP_T, LOOP_ITERS = 16, 12, 4
LOOP_ALL_ON = dict(train_window=5, train_burn_in=2, train_stored_state=True, prioritized_replay=True, td_lambda=0.8)

# code: class-code storage under strict_device_ops; graph: the captured step -- both on the device only (--device cpu runs the same case
# in f32 storage, eagerly, through the tensor-op learner)
F = lambda base, code, graph, **kw: dict(kind="fixture", base=base, code=code, graph=graph, **kw)
CASES = {
    "fixture-cleanup5-f32-eager": F("learner_cleanup5.npz", False, False),
    "fixture-harvest5-code-graph": F("learner_harvest5.npz", True, True),
    "fixture-cleanup5_w4-code-graph": F("learner_cleanup5_w4.npz", True, True),
    "lambda-cleanup5-code-graph": F("learner_cleanup5.npz", True, True, overrides=dict(td_lambda=0.8), perturb=True, more_replays=3),
    "weights-episodes": dict(kind="weights", golden=None),
    "weights-windows": dict(kind="weights", golden="cleanup5_L6_K2_dq1_oth0"),
    "five-forced": dict(kind="five", force=True),
    "five-plain": dict(kind="five", force=False),
    "exit3": dict(kind="exit3"),
    "loop-plain": dict(kind="loop", keys={}),
    "loop-all": dict(kind="loop", keys=LOOP_ALL_ON),
    "rollout32-plain": dict(kind="rollout32", keys={}),
    "rollout32-all": dict(kind="rollout32", keys=LOOP_ALL_ON),
}
for _g in ("cleanup5_L6_K2_dq1_oth0", "harvest5_L3_K1_dq0_oth1"):
    for _graph in (False, True):
        CASES["window-%s-%s" % (_g, "graph" if _graph else "eager")] = dict(kind="window", golden=_g, graph=_graph)


class Rank:
    """what the cases share: the group, the counted all-reduce, the shard, the taps on the learner and the record that is written"""

    def __init__(self, a):
        self.rank, self.world, self.out = a.rank, a.world, a.out
        self.on_gpu = a.device == "cuda"
        self.device = "cuda:0" if self.on_gpu else "cpu"
        self.rec = {}
        self.n_all_reduce = 0
        self.grads = []
        inner = dist.all_reduce

        def counted(*args, **kw):
            self.n_all_reduce += 1
            return inner(*args, **kw)
        dist.all_reduce = counted

    def join(self):
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(self.port), RANK=str(self.rank), WORLD_SIZE=str(self.world))
        dist.init_process_group("gloo", rank=self.rank, world_size=self.world, timeout=timedelta(seconds=60))

    @property
    def shard(self):
        per = 4 // self.world
        return slice(self.rank * per, (self.rank + 1) * per)

    def build(self, base, overrides=None, code=False):
        from tests.learner_util import build, load_fixture
        z, meta = load_fixture(base)
        args, batch, mac, learner = build(z, meta, device=self.device, sl=self.shard, overrides=overrides, code_obs=code and self.on_gpu)
        assert learner.distributed == (dist.is_initialized() and (self.world > 1 or os.environ.get("SSD_FORCE_DIST") == "1"))
        assert learner._fused(batch) == self.on_gpu
        self.tap(learner)
        return args, batch, mac, learner

    def tap(self, learner):
        """the flat gradient as clip_and_step meets it (a captured step: as the second graph's replay meets it), and the denominators
        the step was handed"""
        inner_clip, inner_dens = learner.clip_and_step, learner.denominators

        def clip_and_step():
            if not (self.on_gpu and th.cuda.is_current_stream_capturing()):
                self.grads.append(learner._flat_grad.detach().clone())
            inner_clip()

        def denominators(batch):
            self.dens = inner_dens(batch)
            return self.dens
        learner.clip_and_step, learner.denominators = clip_and_step, denominators

    def tap_graph(self, learner):
        g1, g2 = learner._graph
        grads = self.grads

        class Second:
            def replay(self):
                grads.append(learner._flat_grad.detach().clone())
                g2.replay()
        learner._graph = (g1, Second())

    def past_capture(self, learner, mac, batch):
        """the rewind of tests/test_hip_learner_path._learner_fixture_body: three train calls on a scratch copy of the weights (the third
        captures), then weights, target net and optimiser state back to the start"""
        sd0 = {k: v.clone() for k, v in mac.agent.state_dict().items()}
        for _ in range(3):
            learner.train(batch, 0, 0)
        assert learner._graph is not None
        self.tap_graph(learner)
        return sd0

    @staticmethod
    def rewind(learner, mac, sd0):
        mac.agent.load_state_dict(sd0)
        learner.target_mac.load_state(mac)
        for opt in (learner.optimiser_env, learner.optimiser_inc):
            for st in opt.state.values():
                st["step"].zero_(); st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()

    def local_dens(self, learner, batch):
        """this rank's own denominators (no collective)"""
        was, learner.distributed = learner.distributed, False
        try:
            return learner.denominators(batch).detach().cpu().double().numpy()
        finally:
            learner.distributed = was

    def global_logs(self, learner, logs, batch):
        """the nine logged values of the GLOBAL batch: the kernel's sums -- on CPU tensors the sums behind the tensor-op learner's
        quotients, in float64 -- added over the group by _FusedLogs.synced()"""
        if not isinstance(logs, _FusedLogs):
            n = learner.n_agents
            rows = float(batch.batch_size * (batch.max_seq_length - 1) * n)
            d = self.dens.detach().double()
            v = {k: logs[k].detach().double() for k in LOG_KEYS}
            clean = (batch["clean_num"][:, :-1] > 0).double().sum()
            rew = (batch["reward"][:, :-1].double() / learner.args.reward_scale).sum()
            s = th.zeros(13, dtype=th.float64)
            s[2], s[3], s[4] = v["loss_value_env"] * d[0], v["loss_value_inc"] * d[0], v["loss_sim"] * (1 + d[1])
            s[5], s[6] = v["q_env_taken_mean"] * rows, v["q_inc_taken_mean"] * rows * n
            s[7], s[8] = v["value_give_mean"] * rows, v["value_receive_mean"] * rows
            s[10], s[12] = clean, rew
            s[9], s[11] = v["incentives_to_cleanup_per"] * (clean + 1e-6), v["incentives_to_harvest_per"] * (rew + 1e-6)
            logs = _FusedLogs(s, d, rows, n)
        if learner.distributed:
            logs = logs.synced()
        return np.array([float(logs[k]) for k in LOG_KEYS])

    def record_step(self, learner, mac, logs, batch):
        from tests.learner_util import param_checksums
        if self.on_gpu:
            th.cuda.synchronize()
        sums, sqs, heads = param_checksums(mac)
        for k, v in (("logs", self.global_logs(learner, logs, batch)), ("sums", sums), ("sqs", sqs), ("heads", heads),
                     ("grads", self.grads[-1].cpu().numpy())):
            self.rec.setdefault(k, []).append(v)

    def record_state(self, learner, key=None):
        """flat parameters and both optimisers' state (key: appended to per-iteration lists, else written once)"""
        cat = lambda xs: th.cat([x.detach().reshape(-1).float().cpu() for x in xs]).numpy()
        got = {"flat": cat(learner.params)}
        for name, opt in (("env", learner.optimiser_env), ("inc", learner.optimiser_inc)):
            st = [opt.state[p] for p in opt.param_groups[0]["params"]]
            got[name + "_exp_avg"], got[name + "_exp_avg_sq"] = cat([s["exp_avg"] for s in st]), cat([s["exp_avg_sq"] for s in st])
            got[name + "_step"] = np.array([float(s["step"]) for s in st])
        for k, v in got.items():
            if key is None:
                self.rec[k] = v
            else:
                self.rec.setdefault(key + k, []).append(v)

    def write(self, learner=None):
        if learner is not None:
            self.rec["distributed"] = np.array(bool(learner.distributed))
        self.rec["n_all_reduce"] = np.array(self.n_all_reduce)
        np.savez(os.path.join(self.out, "rank%d.npz" % self.rank), **{k: np.asarray(v) for k, v in self.rec.items()})
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()


# ---- the learner-level cases ---------------------------------------------------------------------------------------------------------------
def run_fixture(r, c):
    """two optimisation steps on the shard of a learner fixture, eager or replayed from the captured step"""
    from homophily_marl_amd import ops
    from tests.test_learner_options import perturb_target
    graph = c["graph"] and r.on_gpu
    args, batch, mac, learner = r.build(c["base"], dict(c.get("overrides", {}), train_graph=graph), c["code"])
    ops.set_strict(c["code"] and r.on_gpu)
    assert learner.use_graph == graph
    if graph:
        sd0 = r.past_capture(learner, mac, batch)
        r.rewind(learner, mac, sd0)
    if c.get("perturb"):
        perturb_target(learner)
    for step in range(2):
        if graph:
            learner.train(batch, 0, 0)
            logs = learner._static_logs
        else:
            logs = learner.cal_loss_and_step(batch)
        r.record_step(learner, mac, logs, batch)
    r.record_state(learner)
    if graph:
        for _ in range(c.get("more_replays", 0)):
            learner.train(batch, 0, 0)
        th.cuda.synchronize()
        r.rec["graph_checks"] = np.array(getattr(learner, "_check_n", 0))
        r.rec["finite"] = np.array(all(bool(th.isfinite(p).all()) for p in mac.parameters()))
    r.write(learner)


def _windows(r, name, overrides, code):
    """(recorded case, mac, learner, buffer, ids, t0, this rank's windows): the rank's two episodes among decoy rows of a ReplayBuffer
    on its device, gathered at its half of the golden's (ids, t0), norm "window" """
    from tests import train_window_util as W
    rec, c = W.golden_case(name)
    args, batch, mac, learner = r.build(c["base"], dict(c["overrides"], **overrides), code)
    rows = ROWS_OF_EPISODES[r.shard]
    buf = W.buffer_of(batch, rows=rows, size=8, norm="window")
    ids, t0 = th.tensor(rows, device=r.device), th.tensor(c["t0"][r.shard], device=r.device)
    win = buf.gather_windows(ids, t0, c["window"], c["burn_in"])
    assert win.reward_norm == c["window"] + 1.0 and learner._fused(win) == r.on_gpu
    assert [int((win["filled"][e] == 0).sum()) for e in range(win.batch_size)] == c["k_e"][r.shard]
    return c, mac, learner, buf, ids, t0, win


def run_window(r, c):
    from homophily_marl_amd import ops
    from tests.test_learner_options import perturb_target
    graph = c["graph"] and r.on_gpu
    g, mac, learner, buf, ids, t0, win = _windows(r, c["golden"], dict(train_graph=graph), True)
    ops.set_strict(r.on_gpu)
    # the windows' burn-in rows differ per episode, so the ranks' own denominators differ: the global ones are no multiple of either
    local = r.local_dens(learner, win)
    r.rec["local_dens"] = local
    if r.world > 1:
        every = [th.zeros(2, dtype=th.float64) for _ in range(r.world)]
        dist.all_gather(every, th.as_tensor(local))
        assert len({tuple(e.tolist()) for e in every}) == r.world, every
    if graph:
        sd0 = r.past_capture(learner, mac, win)
        out = learner.sample_out()
        assert (out.batch_size, out.max_seq_length, out.reward_norm) == (win.batch_size, g["window"] + 1, g["window"] + 1.0)
        assert buf.gather_windows(ids, t0, g["window"], g["burn_in"], out=out) is out       # after capture: straight into the static batch
        win = out
        r.rewind(learner, mac, sd0)
    perturb_target(learner)
    for step in range(2):
        if graph:
            learner.train(win, 0, 0)
            logs = learner._static_logs
        else:
            logs = learner.cal_loss_and_step(win)
        r.record_step(learner, mac, logs, win)
    r.record_state(learner)
    r.write(learner)


def run_weights(r, c):
    """one eager step on a batch that carries this rank's own priority tuple"""
    from tests.test_learner_options import perturb_target
    if c["golden"] is None:
        args, batch, mac, learner = r.build("learner_cleanup5.npz", None, False)
    else:
        g, mac, learner, buf, ids, t0, batch = _windows(r, c["golden"], {}, False)
    perturb_target(learner)
    table = th.zeros(TABLE_LEN, dtype=th.int32, device=r.device)
    table[3] = 70000                                                     # an entry a smaller q_new must still replace
    batch.priority = (table, th.tensor(PRIORITY_IDS[r.rank], device=r.device), th.tensor(PRIORITY_WEIGHTS[r.rank], device=r.device))
    r.rec["table_before"] = table.cpu().numpy()
    logs = learner.cal_loss_and_step(batch)
    r.record_step(learner, mac, logs, batch)
    r.rec["q_new"], r.rec["table_after"] = learner.last_q_new.cpu().numpy(), table.cpu().numpy()
    r.record_state(learner)
    r.write(learner)


def run_five(r, c):
    """five train() calls on the whole fixture by ONE rank (eager, eager, capture, two replays): with a one-rank group under
    SSD_FORCE_DIST=1, or with no group"""
    from homophily_marl_amd import ops
    assert r.world == 1 and (os.environ.get("SSD_FORCE_DIST") == "1") == c["force"]
    args, batch, mac, learner = r.build("learner_cleanup5.npz", dict(train_graph=r.on_gpu), True)
    ops.set_strict(r.on_gpu)
    for call in range(5):
        seen = len(r.grads)
        learner.train(batch, 0, 0)
        if learner._graph is not None and call == 2:
            r.tap_graph(learner)
        # (the capturing call replays its second graph before the tap exists: zeros stand for its gradient in both runs)
        r.rec.setdefault("call_grads", []).append(r.grads[-1].cpu().numpy() if len(r.grads) > seen else np.zeros(learner._flat_grad.numel(), np.float32))
        r.record_state(learner, key="call_")
        dens = learner._static_logs.dens if learner._graph is not None else r.dens          # what the step divided by
        r.rec.setdefault("call_dens", []).append(dens.detach().cpu().numpy())
    r.rec["graph"] = np.array(learner._graph is not None)
    r.write(learner)


def run_exit3(r, c):
    """rank 1 leaves with status 3 before its first collective; rank 0 goes into the step and waits for it"""
    if r.rank == 1:
        sys.exit(3)
    args, batch, mac, learner = r.build("learner_harvest5.npz")
    learner.cal_loss_and_step(batch)
    r.write(learner)


# ---- the loop-level cases ------------------------------------------------------------------------------------------------------------------
def _loop_ctx(r, n_env, keys, base):
    from homophily_marl_amd.run import load_config, setup
    th.manual_seed(0)
    np.random.seed(11)
    cfg = load_config("cleanup", overrides=dict(dict(
        runner="hip_graph", batch_size_run=n_env, batch_size=4, buffer_size=4 * n_env, replay_in_place=True, buffer_cpu_only=False, store_state=False,
        obs_storage="code", env_args=dict(num_agents=3, map="default3", episode_limit=LOOP_T, seed=3), use_cuda=True, save_model=False,
        runner_stats=False, learner_log_interval=LOOP_T, strict_device_ops=True, train_graph=True, train_steps_per_rollout=2, env_id_base=base), **keys))
    ctx = setup(cfg)
    first = []
    inner = ctx.buffer.insert_episode_batch

    def insert(b):
        if not first:
            th.cuda.synchronize()
            first.append({k: v.detach().cpu().numpy().copy() for k, v in b.data.transition_data.items()})
        return inner(b)
    ctx.buffer.insert_episode_batch = insert
    return ctx, first


def run_loop(r, c):
    """four iterations of run.train_iteration on 16 envs of this rank's own (global env ids 16 rank ..): eager, eager | capture, replay | ..."""
    from homophily_marl_amd import ops
    from homophily_marl_amd.run import train_iteration
    ctx, first = _loop_ctx(r, LOOP_ENVS, c["keys"], LOOP_ENVS * r.rank)
    try:
        assert ctx.learner.distributed == (r.world > 1)
        ep = 0
        for _ in range(LOOP_ITERS):
            ep = train_iteration(ctx, ep)
            th.cuda.synchronize()
            r.record_state(ctx.learner, key="iter_")
        for k, v in first[0].items():
            r.rec["roll_" + k] = v
        stats = ctx.logger.stats
        for k in _FusedLogs.KEYS:
            r.rec["stat_" + k] = np.array([v for _, v in stats[k]], dtype=np.float64)
        r.rec["train_steps"] = np.array(ctx.train_steps)
        r.rec["graph"] = np.array(ctx.learner._graph is not None)
        r.rec["finite"] = np.array(all(bool(th.isfinite(p).all()) for p in ctx.mac.parameters()))
        r.rec["poll_error"] = np.array(ctx.runner.env.native.poll_error())
        r.rec["numeric_status"] = np.array(ops.numeric_status())
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()
    r.write(ctx.learner)


def run_rollout32(r, c):
    """no group: the first rollout of 32 envs with global ids 0 .. 31 under the same seed"""
    from homophily_marl_amd import ops
    assert r.world == 1
    ctx, first = _loop_ctx(r, 2 * LOOP_ENVS, c["keys"], 0)
    try:
        assert not ctx.learner.distributed
        ctx.buffer.insert_episode_batch(ctx.runner.run(test_mode=False))
        for k, v in first[0].items():
            r.rec["roll_" + k] = v
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()
    r.write(ctx.learner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--device", choices=("cpu", "cuda"), required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    t0 = time.perf_counter()
    th.set_num_threads(1)
    th.backends.cuda.matmul.allow_tf32 = False
    c = CASES[a.case]
    r = Rank(a)
    r.port = a.port
    if a.world > 1 or c.get("force"):
        r.join()
    r.rec["case"] = np.array(a.case)
    {"fixture": run_fixture, "window": run_window, "weights": run_weights, "five": run_five, "exit3": run_exit3, "loop": run_loop,
     "rollout32": run_rollout32}[c["kind"]](r, c)
    print("rank %d of %d, case %s: %.1f s, %d all-reduces" % (a.rank, a.world, a.case, time.perf_counter() - t0, r.n_all_reduce), flush=True)


if __name__ == "__main__":
    main()
