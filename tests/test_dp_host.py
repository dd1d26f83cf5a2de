"""CPU suite: two gloo ranks of tests/dp_worker.py on CPU tensors, where the tensor-op learner serves the data-parallel path beyond
default flags (TD(lambda), windows with per-episode burn-in, importance weights), held to the reference recordings and to the
single-process tensor-op learner on the whole batch; and the launcher itself (tests/dp_util.run_ranks): its time limit and the
kill-on-failure path.  The GPU counterpart is tests/test_dp_device.py."""
import time

import numpy as np
import pytest

from tests import dp_util as D
from tests import train_window_util as W
from tests.learner_util import load_fixture


def test_two_ranks_on_a_fixture_match_the_reference_recording():
    """A: cleanup fixture, two episodes per rank: every logged value (the ranks' sums added by _FusedLogs.synced over global
    denominators) and the parameters after both recorded steps; replicas, moments and the all-reduced gradient equal bit for bit"""
    ranks = D.run_ranks("fixture-cleanup5-f32-eager", 2, "cpu")
    z, meta = load_fixture("learner_cleanup5.npz")
    assert all(bool(r["distributed"]) for r in ranks)
    D.check_recorded_steps(ranks, z, "cleanup5 / cpu")
    D.assert_replicas_equal(ranks)
    assert int(ranks[0]["n_all_reduce"]) == 2 * 3                           # per step: denominators, gradient, the logged sums


def test_two_ranks_with_lambda_returns_match_the_whole_batch():
    """B: td_lambda 0.8 against the single-process tensor-op learner on the four episodes"""
    ranks = D.run_ranks("lambda-cleanup5-code-graph", 2, "cpu")
    D.check_lambda_steps(ranks, "td_lambda 0.8 / cpu")
    D.assert_replicas_equal(ranks)


def test_two_ranks_on_windows_match_the_reference_on_slices():
    """C: each rank gathers its two windows (burn-in rows 0 + 2 against 2 + 2: the ranks' own denominators differ, which the ranks
    assert); the steps against what the reference recorded on the four slices"""
    name = "cleanup5_L6_K2_dq1_oth0"
    ranks = D.run_ranks("window-%s-eager" % name, 2, "cpu")
    rec, c = W.golden_case(name)
    assert not np.array_equal(ranks[0]["local_dens"], ranks[1]["local_dens"]), ranks[0]["local_dens"]
    print("local denominators", ranks[0]["local_dens"].tolist(), ranks[1]["local_dens"].tolist())
    D.check_recorded_steps(ranks, rec, name + " / cpu")
    D.assert_replicas_equal(ranks)


@pytest.mark.parametrize("case,golden", [("weights-episodes", None), ("weights-windows", "cleanup5_L6_K2_dq1_oth0")])
def test_two_ranks_with_importance_weights_match_the_weighted_whole_batch(case, golden):
    """D: per-rank priority tuples; the all-reduced gradient, the tables and the new priorities"""
    ranks = D.run_ranks(case, 2, "cpu")
    D.check_weights(ranks, golden, case + " / cpu")
    D.assert_replicas_equal(ranks)


def test_a_rank_that_exits_ends_the_job_and_nothing_stays_behind():
    """rank 1 exits 3 before its first collective while rank 0 waits in its own: the job fails long before its limit, names the exit
    code, and both processes are gone"""
    t0 = time.perf_counter()
    with pytest.raises(D.RankFailure, match="exited non-zero") as e:
        D.run_ranks("exit3", 2, "cpu")
    wall = time.perf_counter() - t0
    print("failed job ended after %.1f s (limit %g s)" % (wall, D.JOB_LIMIT))
    assert wall < D.JOB_LIMIT and 3 in e.value.codes
    assert len(e.value.procs) == 2 and all(p.poll() is not None for p in e.value.procs)
    assert "rank 1 (exit 3)" in str(e.value)


def test_a_job_past_its_limit_is_killed():
    """a job under a limit shorter than an interpreter's start: reported as hung, both processes killed"""
    with pytest.raises(D.RankFailure, match="hung") as e:
        D.run_ranks("fixture-cleanup5-f32-eager", 2, "cpu", limit=0.2)
    assert all(p.poll() is not None for p in e.value.procs)
