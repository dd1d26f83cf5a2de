"""Launcher of the data-parallel tests (a helper, no test in it): run_ranks starts one fresh `python -m tests.dp_worker` per rank (the
way tests/test_bench_contract.py starts bench.py), waits for the job under ONE time limit, and returns what the ranks wrote.  A rank
that exits non-zero, or the limit passing, ends the job: the other ranks are killed and the failure carries the tail of every rank's
stderr.  Nothing is retried.  The ranks' gloo timeout (60 s) ends a rank whose peer died even if nobody kills it."""
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_LIMIT = 180.0            # seconds per job; a job that reaches it counts as hung
MAX_RANKS = 3                # processes with the device open at once (pytest itself not counted)


class RankFailure(AssertionError):
    """a job that did not end well: .procs are its (ended) processes, .codes their exit codes (None: killed at the limit)"""

    def __init__(self, message, procs, codes):
        super().__init__(message)
        self.procs, self.codes = procs, codes


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tail(path, n=25):
    with open(path, errors="replace") as f:
        return "".join(f.readlines()[-n:])


def run_ranks(case, world, device, env=None, limit=JOB_LIMIT):
    """[{key: array} per rank] of one job of `world` ranks on `device` ("cpu" / "cuda"); env: extra environment of the ranks.  Prints
    the job's wall time (the summary of a pull request reads it from there)."""
    assert 1 <= world <= MAX_RANKS and device in ("cpu", "cuda")
    port = free_port()
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SSD_FORCE_DIST",
                                                              "SSD_GRAPH_CHECK")}
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory() as d:
        procs, logs = [], []
        try:
            for rank in range(world):
                err = open(os.path.join(d, "rank%d.err" % rank), "w")
                logs.append(err)
                procs.append(subprocess.Popen([sys.executable, "-m", "tests.dp_worker", "--case", case, "--rank", str(rank), "--world", str(world),
                                               "--port", str(port), "--device", device, "--out", d],
                                              cwd=ROOT, env=dict(base, **(env or {})), stdin=subprocess.DEVNULL, stdout=err, stderr=subprocess.STDOUT))
            failed = None
            while failed is None and any(p.poll() is None for p in procs):
                if any(p.poll() not in (None, 0) for p in procs):
                    failed = "a rank exited non-zero"
                elif time.perf_counter() - t0 > limit:
                    failed = "the job passed its limit of %g s (hung)" % limit
                else:
                    time.sleep(0.05)
            if failed is None and any(p.returncode != 0 for p in procs):
                failed = "a rank exited non-zero"
            codes = [p.poll() for p in procs]
        finally:
            for p in procs:                                              # on every way out: nothing of the job stays behind
                if p.poll() is None:
                    p.kill()
            for p in procs:
                p.wait()
            for f in logs:
                f.close()
        wall = time.perf_counter() - t0
        print("dp job %s, %d rank(s) on %s: %.1f s" % (case, world, device, wall))
        if failed is not None:
            tails = "\n".join("---- rank %d (exit %s) ----\n%s" % (r, codes[r], _tail(os.path.join(d, "rank%d.err" % r))) for r in range(world))
            raise RankFailure("%s: %s after %.1f s\n%s" % (case, failed, wall, tails), procs, codes)
        out = []
        for rank in range(world):
            with np.load(os.path.join(d, "rank%d.npz" % rank)) as z:
                out.append({k: z[k] for k in z.files})
        return out


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


STATE_KEYS = ("flat", "env_exp_avg", "env_exp_avg_sq", "env_step", "inc_exp_avg", "inc_exp_avg_sq", "inc_step")


def assert_replicas_equal(ranks, prefix="", extra=("grads",)):
    """parameters, both optimisers' moments and step counters (and the all-reduced gradients) of every rank equal rank 0's bit for bit"""
    for k in tuple(prefix + s for s in STATE_KEYS) + tuple(extra):
        for r, other in enumerate(ranks[1:], 1):
            assert bit_equal(ranks[0][k], other[k]), "rank %d differs from rank 0 in %s by %.3e" % (
                r, k, float(np.abs(ranks[0][k].astype(np.float64) - other[k]).max()))
    assert len({int(r["n_all_reduce"]) for r in ranks}) == 1, [int(r["n_all_reduce"]) for r in ranks]


# ---- what the two test files share: the bars (each named after the test it comes from) and the references -----------------------------------
LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")


def check_recorded_steps(ranks, rec, label):
    """every rank's two steps against a reference recording `rec` (keys step<k>_<name>): the bars of
    tests/test_hip_learner_path.py::test_learner_on_device_matches_reference_fixture (= tests/test_learner_options.check_step)"""
    for step in range(2):
        ref = np.array([float(rec["step%d_%s" % (step, k)]) for k in LOG_KEYS])
        sq = rec["step%d_param_sq" % step]
        for r, z in enumerate(ranks):
            e_log = np.abs(z["logs"][step] - ref)
            e_head = float(np.abs(z["heads"][step] - rec["step%d_param_head" % step]).max())
            e_sq = float(np.abs(z["sqs"][step] - sq).max() / np.abs(sq).max())
            print("%s step %d rank %d: logs %.3e (%s; bar 1e-5), param heads %.3e (bar 2e-5), squared checksums %.3e (bar 1e-5)" % (
                label, step, r, e_log.max(), LOG_KEYS[int(e_log.argmax())], e_head, e_sq))
            assert (e_log < 1e-5).all(), (step, r, dict(zip(LOG_KEYS, zip(z["logs"][step].tolist(), ref.tolist()))))
            assert e_head < 2e-5 and e_sq < 1e-5, (step, r, e_head, e_sq)


_refs = {}


def lambda_reference():
    """two steps of the CPU tensor-op learner at td_lambda 0.8 on the whole cleanup fixture (made once, never written)"""
    if "lambda" not in _refs:
        from tests.learner_util import build, load_fixture, param_checksums
        from tests.test_learner_options import perturb_target
        z, meta = load_fixture("learner_cleanup5.npz")
        args, batch, mac, learner = build(z, meta, overrides=dict(td_lambda=0.8))
        assert not learner.distributed and not learner._fused(batch)
        perturb_target(learner)
        want = []
        for step in range(2):
            logs = learner.cal_loss_and_step(batch)
            want.append((np.array([float(logs[k]) for k in LOG_KEYS]), param_checksums(mac)))
        _refs["lambda"] = want
    return _refs["lambda"]


def check_lambda_steps(ranks, label):
    """the bars of tests/test_td_lambda_gpu.py::test_device_learner_matches_the_tensor_op_learner"""
    for step, (ref_logs, (sums, sqs, heads)) in enumerate(lambda_reference()):
        for r, z in enumerate(ranks):
            e_log = np.abs(z["logs"][step] - ref_logs)
            e_head = float(np.abs(z["heads"][step] - heads).max())
            e_sum = np.abs(z["sums"][step] - sums) / np.maximum(1.0, np.abs(sums))
            e_sq = np.abs(z["sqs"][step] - sqs) / np.maximum(1.0, np.abs(sqs))
            print("%s step %d rank %d: logs %.3e (%s), param heads %.3e, checksums %.3e / %.3e over max(1, |ref|) (bar 1e-5 each)" % (
                label, step, r, e_log.max(), LOG_KEYS[int(e_log.argmax())], e_head, e_sum.max(), e_sq.max()))
            assert (e_log < 1e-5).all(), (step, r, dict(zip(LOG_KEYS, zip(z["logs"][step].tolist(), ref_logs.tolist()))))
            assert e_head < 1e-5 and (e_sum <= 1e-5).all() and (e_sq <= 1e-5).all(), (step, r, e_head, float(e_sum.max()), float(e_sq.max()))


def weights_reference(golden):
    """(flat gradient, q_new [4]) of the CPU tensor-op learner (fused_loss off) on the four episodes -- or the golden case's four windows
    -- with the ranks' weights concatenated and a host table"""
    if ("weights", golden) not in _refs:
        import torch as th
        from tests import train_window_util as W
        from tests.dp_worker import PRIORITY_IDS, PRIORITY_WEIGHTS, ROWS_OF_EPISODES, TABLE_LEN
        from tests.learner_util import build, load_fixture
        from tests.test_learner_options import perturb_target
        if golden is None:
            z, meta = load_fixture("learner_cleanup5.npz")
            args, batch, mac, learner = build(z, meta, overrides=dict(fused_loss=False))
        else:
            rec, c = W.golden_case(golden)
            args, whole, mac, learner = W.build_case(c, overrides=dict(fused_loss=False))
            batch = W.buffer_of(whole, rows=ROWS_OF_EPISODES, size=8, norm="window").gather_windows(ROWS_OF_EPISODES, c["t0"], c["window"], c["burn_in"])
        perturb_target(learner)
        batch.priority = (th.zeros(TABLE_LEN, dtype=th.int32), th.tensor(sum(PRIORITY_IDS, [])), th.tensor(sum(PRIORITY_WEIGHTS, [])))
        learner.forward_backward(batch)
        _refs[("weights", golden)] = (learner._flat_grad.detach().numpy().copy(), learner.last_q_new.numpy().astype(np.int64))
    return _refs[("weights", golden)]


def check_weights(ranks, golden, label):
    """the all-reduced gradient within 1e-5 max(1, |g| max) of the reference's (the bar of tests/test_priority_gpu.py::
    test_weighted_fused_gradient_matches_the_weighted_tensor_op_learner), every rank's table the restated write-back of its own q_new,
    the four q_new within 1 + 1e-4 q of the reference's (the bar of test_captured_replays_are_the_eager_run)"""
    from tests import priority_util as P
    from tests.dp_worker import PRIORITY_IDS
    grad, q_ref = weights_reference(golden)
    top = float(np.abs(grad).max())
    assert top > 0
    for r, z in enumerate(ranks):
        err = float(np.abs(z["grads"][0] - grad).max())
        print("%s rank %d: all-reduced weighted gradient against the tensor-op learner %.3e (bar %.3e, |g| max %.3e)" % (label, r, err, 1e-5 * max(1.0, top), top))
        assert err <= 1e-5 * max(1.0, top), (r, err, top)
        q = z["q_new"].astype(np.int64)
        assert q.min() >= 1 and np.array_equal(z["table_after"].astype(np.int64), P.write_back(z["table_before"], PRIORITY_IDS[r], q)), (r, q, z["table_after"])
    q = np.concatenate([z["q_new"].astype(np.int64) for z in ranks])
    print("%s: q_new %s, reference %s (bar 1 + 1e-4 q)" % (label, q.tolist(), q_ref.tolist()))
    assert (np.abs(q - q_ref) <= 1 + 1e-4 * q_ref).all(), (q, q_ref)
