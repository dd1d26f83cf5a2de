"""GPU suite: the data-parallel DEVICE learner.  Two gloo ranks of tests/dp_worker.py share the one GPU (gloo carries device tensors;
RCCL cannot put two ranks on one device), each on its shard with global denominators: the fused loss kernels with denominators
handed in, ssd_clip_adam_step behind the all-reduce, the three-stage split of the captured step (denominators outside the graph, the
collective between the two graphs), _FusedLogs.synced and SSD_FORCE_DIST -- against the reference recordings and the CPU tensor-op
learner on the whole batch (never against a device run), and the training loop under a process group.  This file is the way to check a
change to the collective path on a one-GPU machine; tests/test_dp_host.py runs the same worker on CPU tensors."""
import numpy as np
import pytest

from tests import dp_util as D
from tests import train_window_util as W
from tests.learner_util import load_fixture

pytestmark = pytest.mark.gpu


# ---- A. the fixture steps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,base", [("fixture-cleanup5-f32-eager", "learner_cleanup5.npz"), ("fixture-harvest5-code-graph", "learner_harvest5.npz"),
                                       ("fixture-cleanup5_w4-code-graph", "learner_cleanup5_w4.npz")])
def test_two_ranks_on_a_fixture_match_the_reference_recording(case, base):
    """f32 storage eager; code storage under strict_device_ops with the step captured (replayed past the capture after a rewind): both
    recorded steps at the bars of test_learner_on_device_matches_reference_fixture, the replicas equal bit for bit"""
    ranks = D.run_ranks(case, 2, "cuda")
    z, meta = load_fixture(base)
    assert all(bool(r["distributed"]) for r in ranks)
    D.check_recorded_steps(ranks, z, case)
    D.assert_replicas_equal(ranks)


# ---- B. TD(lambda) -------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_with_lambda_returns_match_the_tensor_op_learner():
    """td_lambda 0.8, captured, every replay checked against an eager evaluation by SSD_GRAPH_CHECK (six replays in all)"""
    ranks = D.run_ranks("lambda-cleanup5-code-graph", 2, "cuda", env=dict(SSD_GRAPH_CHECK="1"))
    D.check_lambda_steps(ranks, "td_lambda 0.8")
    D.assert_replicas_equal(ranks)
    assert all(int(r["graph_checks"]) == 6 and bool(r["finite"]) for r in ranks), [int(r["graph_checks"]) for r in ranks]


# ---- C. windows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("name", ["cleanup5_L6_K2_dq1_oth0", "harvest5_L3_K1_dq0_oth1"])
def test_two_ranks_on_gathered_windows_match_the_reference(name, mode):
    """the split 0, 1 | 2, 3 of the golden's episodes: burn-in rows 0 + 2 against 2 + 2 (L6) and 1 + 0 against 1 + 1 (L3), so the ranks'
    own denominators differ (asserted by the ranks before their first all-reduce, and here)"""
    ranks = D.run_ranks("window-%s-%s" % (name, mode), 2, "cuda")
    rec, c = W.golden_case(name)
    print("local denominators", ranks[0]["local_dens"].tolist(), ranks[1]["local_dens"].tolist())
    assert not np.array_equal(ranks[0]["local_dens"], ranks[1]["local_dens"])
    D.check_recorded_steps(ranks, rec, "%s / %s" % (name, mode))
    D.assert_replicas_equal(ranks)


# ---- D. importance weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,golden", [("weights-episodes", None), ("weights-windows", "cleanup5_L6_K2_dq1_oth0")])
def test_two_ranks_with_importance_weights_match_the_weighted_tensor_op_learner(case, golden):
    ranks = D.run_ranks(case, 2, "cuda")
    D.check_weights(ranks, golden, case)
    D.assert_replicas_equal(ranks)


# ---- E. one forced rank --------------------------------------------------------------------------------------------------------------------
def test_one_forced_rank_is_the_run_without_a_group():
    """SSD_FORCE_DIST=1 with a one-rank group against no group, five train() calls (eager, eager, capture, replay, replay): the same
    kernels on the same inputs -- only the place where the denominators are computed moves (outside the graph and copied in, against
    inside it) -- so parameters and moments are equal bit for bit.  On a difference the first call and stage that differ are named."""
    forced = D.run_ranks("five-forced", 1, "cuda", env=dict(SSD_FORCE_DIST="1"))[0]
    plain = D.run_ranks("five-plain", 1, "cuda")[0]
    assert bool(forced["distributed"]) and not bool(plain["distributed"]) and bool(forced["graph"]) and bool(plain["graph"])
    assert int(forced["n_all_reduce"]) > 0 and int(plain["n_all_reduce"]) == 0
    for call in range(5):
        for stage, key in (("denominators", "call_dens"), ("gradient", "call_grads"), ("parameters", "call_flat")) + tuple(
                ("optimiser state " + k, "call_" + k) for k in D.STATE_KEYS[1:]):
            a, b = forced[key][call], plain[key][call]
            assert D.bit_equal(a, b), "train call %d: %s differ by %.3e (first stage of the step that does)" % (
                call, stage, float(np.abs(a.astype(np.float64) - b).max()))
    print("five train calls: denominators %s, gradients, parameters and moments equal bit for bit; %d all-reduces against 0" % (
        forced["call_dens"][-1].tolist(), int(forced["n_all_reduce"])))


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "all"])
def test_two_ranks_of_the_training_loop_stay_replicas(variant):
    """run.setup + four run.train_iteration per rank (Cleanup-3, 16 envs per rank with global env ids 16 rank .., batch 4, two train
    steps per rollout, the step captured at the third call; `all`: windows with burn-in from the stored recurrent state, prioritised
    replay, TD(lambda)): the replicas never diverge, the ranks issue the same collectives, the logger of both ranks receives the same
    synced values, and the ranks' first rollouts are the two halves of one 32-env rollout of a group-less process, byte for byte"""
    ranks = D.run_ranks("loop-" + variant, 2, "cuda")
    whole = D.run_ranks("rollout32-" + variant, 1, "cuda")[0]
    for it in range(4):
        for k in D.STATE_KEYS:
            assert D.bit_equal(ranks[0]["iter_" + k][it], ranks[1]["iter_" + k][it]), "iteration %d: the ranks differ in %s" % (it, k)
    assert int(ranks[0]["n_all_reduce"]) == int(ranks[1]["n_all_reduce"]) > 0
    for k in D.LOG_KEYS:
        a, b = ranks[0]["stat_" + k], ranks[1]["stat_" + k]
        assert a.size >= 2 and D.bit_equal(a, b) and np.isfinite(a).all(), (k, a, b)
    # eight train steps: denominators + gradient each, and the logged sums at every log event
    assert int(ranks[0]["n_all_reduce"]) == 2 * 8 + ranks[0]["stat_loss_sim"].size
    fields = [k for k in whole if k.startswith("roll_")]
    assert ("roll_hidden" in fields) == (variant == "all") and "roll_obs" in fields and "roll_actions_inc" in fields
    for k in fields:
        for r, z in enumerate(ranks):
            assert D.bit_equal(z[k], whole[k][16 * r:16 * r + 16]), "first rollout of rank %d differs from envs %d .. in %s" % (r, 16 * r, k)
    print("loop %s: %d all-reduces per rank, %d log events, %d stored fields of the first rollout equal byte for byte" % (
        variant, int(ranks[0]["n_all_reduce"]), ranks[0]["stat_loss_sim"].size, len(fields)))
    for z in ranks:
        assert bool(z["distributed"]) and bool(z["graph"]) and bool(z["finite"]) and int(z["train_steps"]) == 8
        assert int(z["poll_error"]) == 0 and int(z["numeric_status"]) == 0
