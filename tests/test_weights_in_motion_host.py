"""CPU suite: the derived copies of the weights while training moves them (tests/motion_util.py; the device half is
tests/test_weights_in_motion_gpu.py).

  (a) six learner.train calls across three target syncs (target_update_interval 2) against the reference's own train() on the same
      batch (tests/golden/learner_target_sync.npz, oracle/gen_target_sync_golden.py).  Bar of call k: max(the two-step bar of
      tests/test_learner_parity.py, 8 x the sensitivity the generator measured for that call by perturbing the reference's initial
      weights by one f32 rounding).  Measured sensitivities (printed): losses <= 1.2e-7, param_head 3.0e-8, param_sq 5.4e-9 relative at
      every call -- the six-step Adam trajectory does not amplify them, so every bar is the two-step bar.
  (b) power: with the sync replaced by a no-op, call 3 (the fixture's power_call) misses the reference by more than 10 bars.  The
      reference's own unsynced run (fixture, nosync3_*) misses its synced run by 294 bars (loss_value_env) and 1041 bars (loss_value_inc).
  (c) the target net's caches after every sync: bit-equal to fresh concatenations of the live parameters, at unchanged addresses.
  (d) the float64 stepwise controller of motion_util (the GPU tests' reference for whole rollouts) on the three learner fixtures
      within 2e-6 of the reference's Q-values; the share of rows its greedy comparison leaves out; what one train step does to its
      states (the power of the GPU tests' stale-weights arm)."""
import numpy as np
import pytest
import torch as th

from tests import motion_util as mu
from tests.learner_util import build, load_fixture

FIXTURES = ["learner_cleanup5.npz", "learner_harvest5.npz", "learner_cleanup5_w4.npz"]


def _learner(no_sync=False):
    zs, _ = load_fixture("learner_target_sync.npz")
    z, meta = load_fixture("learner_cleanup5.npz")
    args, batch, mac, learner = build(z, meta, overrides=dict(target_update_interval=2))
    assert args.target_update_interval == 2
    if no_sync:
        mu.suppress_sync(learner)
    seen = []
    inner = learner.cal_loss_and_step

    def step(b):
        seen.append(inner(b))
        return seen[-1]
    learner.cal_loss_and_step = step
    return zs, batch, mac, learner, seen


def test_fixture_holds_results_only_and_its_syncs_are_measurable():
    zs, meta = load_fixture("learner_target_sync.npz")
    assert meta["batch"] == "learner_cleanup5.npz" and meta["overrides"] == dict(target_update_interval=2)
    assert not [k for k in zs.files if k.startswith("batch_") or k.startswith("w_")]
    n_calls, power = int(zs["n_calls"]), int(zs["power_call"])
    assert n_calls == 6 and zs["sync_after"].tolist() == [2, 4, 6] and power == 3
    for k in range(1, n_calls + 1):
        print("call %d sensitivity: %s param_head %.2e param_sq (rel) %.2e" % (
            k, {key: "%.1e" % float(zs["sens%d_%s" % (k, key)]) for key in mu.LOG_KEYS}, float(zs["sens%d_param_head" % k]),
            float(zs["sens%d_param_sq_rel" % k])))
    assert max(float(zs["sens6_" + key]) for key in mu.LOG_KEYS[:3]) <= 1e-4          # else the generator cuts the trajectory
    # the reference's own numbers: its unsynced run leaves its synced run at the power call by more than 10 bars
    log_bars = mu.bars(zs, power)[0]
    gaps = {key: abs(float(zs["nosync%d_%s" % (power, key)]) - float(zs["call%d_%s" % (power, key)])) / log_bars[key]
            for key in ("loss_value_env", "loss_value_inc")}
    print("reference, sync suppressed, call %d: gap / bar %s" % (power, gaps))
    assert max(gaps.values()) > 10
    for k in (1, 2):                                                                  # nothing differs before the first sync
        assert float(zs["nosync%d_loss_value_env" % k]) == float(zs["call%d_loss_value_env" % k])


def test_six_train_calls_across_target_syncs_match_the_reference():
    zs, batch, mac, learner, seen = _learner()
    assert [str(x) for x in zs["param_names"]] == list(mac.agent.state_dict().keys())
    for k in range(1, 7):
        learner.train(batch, 0, k)
        assert len(seen) == k and learner.last_target_update_episode == k - k % 2
        errors = mu.call_errors(zs, k, seen[-1], mac)
        print("call %d: worst %s at %.3f of its bar; losses %s" % ((k,) + mu.worst(errors) + (
            {key: "%.2e" % errors[key][0] for key in mu.LOG_KEYS[:3]},)))
        for name, (err, bar) in errors.items():
            assert err < bar, (k, name, err, bar)


def test_a_suppressed_target_sync_misses_the_reference():
    zs, batch, mac, learner, seen = _learner(no_sync=True)
    power = int(zs["power_call"])
    for k in range(1, power + 1):
        learner.train(batch, 0, k)
        errors = mu.call_errors(zs, k, seen[-1], mac)
        if k < 3:
            assert mu.worst(errors)[1] < 1, (k, errors)                               # the arms are one up to the first sync
    ratios = {key: errors[key][0] / errors[key][1] for key in ("loss_value_env", "loss_value_inc")}
    print("sync suppressed, call %d: error / bar %s" % (power, ratios))
    assert max(ratios.values()) > 10, ratios
    # and it is the reference's own unsynced run it follows
    for key in ratios:
        assert abs(float(seen[-1][key]) - float(zs["nosync%d_%s" % (power, key)])) < mu.bars(zs, power)[0][key], key


@pytest.mark.parametrize("grad", ["on", "off"])
def test_target_caches_follow_every_sync_at_unchanged_addresses(grad):
    """grad "on": the target net is first touched with gradients enabled (no cache may be kept from there: it would be a graph
    output) and synced with them enabled; "off": the caches are built before the first call and every sync runs under no_grad."""
    zs, batch, mac, learner, seen = _learner()
    tgt = learner.target_mac.agent
    if grad == "on":
        tgt._gru_weights_both(); tgt._fc2_merged()
        assert tgt._gru_cache is None and tgt._fc2_cache is None
    else:
        with th.no_grad():
            tgt._gru_weights_both(); tgt._fc2_merged()
        inner = learner._update_targets

        def sync():
            with th.no_grad():
                inner()
        learner._update_targets = sync
    syncs = []
    for k in range(1, 7):
        before = None if tgt._gru_cache is None else [t.data_ptr() for t in mu.cache_tensors(tgt)]
        was = learner.last_target_update_episode
        learner.train(batch, 0, k)
        ptrs = [t.data_ptr() for t in mu.cache_tensors(tgt)]                         # the learner's own evaluation built them by now
        assert before is None or ptrs == before, k
        if learner.last_target_update_episode != was:
            syncs.append(k)
            mu.assert_caches_follow(tgt, mac.agent, ptrs, "after the sync of call %d" % k)
        else:                                                                         # between syncs the live net has moved on
            assert not all(th.equal(x, y) for x, y in zip(mu.cache_tensors(tgt), mu.fresh_concatenations(mac.agent))), k
            mu.assert_caches_follow(tgt, tgt, ptrs, "call %d, no sync" % k)
    assert syncs == [2, 4, 6]


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_controller_matches_the_reference_q_values(name):
    z, meta = load_fixture(name)
    args, batch, mac, learner = build(z, meta)
    ep = mu.episode_fields(batch)
    q_env, q_inc, h_env, h_inc = mu.controller64(mac, mu.agent64(mac), ep)
    de, di = np.abs(q_env.numpy() - z["q_env"]).max(), np.abs(q_inc.numpy() - z["q_inc"]).max()
    # a property of the float64 controller and the inputs alone: the share of rows the greedy comparison leaves out
    _, clear, _, clear_i, off = mu.greedy_rows(q_env, q_inc, th.as_tensor(z["batch_avail_actions"][0, 0, 0]))
    share = mu.excluded_share(clear, clear_i, off)
    print("%s: float64 controller against the reference: q_env %.2e q_inc %.2e; rows left out: env %.4f inc %.4f" % ((name, de, di) + share))
    assert de < 2e-6 and di < 2e-6
    assert h_env.shape == (batch.batch_size, batch.max_seq_length, args.n_agents, 64) and h_env[:, 0].abs().max() > 0
    assert max(share) < mu.EXCLUDED_CAP


def test_one_train_step_moves_the_float64_states_by_100_bars():
    """The GPU tests hold a rollout's stored state to the float64 controller with the weights it was played with and expect the
    weights of one train step earlier to miss by more than 10 STATE_TOL.  That expectation is licensed here, on the host: between any
    two consecutive weight sets of the six-call trajectory the float64 states on the fixture batch differ by at least 100 STATE_TOL."""
    zs, batch, mac, learner, seen = _learner()
    ep = mu.episode_fields(batch)
    states = [mu.controller64(mac, mu.agent64(mac), ep)[2:]]
    for k in range(1, 7):
        learner.train(batch, 0, k)
        states.append(mu.controller64(mac, mu.agent64(mac), ep)[2:])
    moves = [max(float((a - b).abs().max()) for a, b in zip(x, y)) for x, y in zip(states, states[1:])]
    print("max |delta h| of one train step, calls 1..6: %s" % ["%.2e" % m for m in moves])
    assert min(moves) >= 100 * mu.STATE_TOL, moves
