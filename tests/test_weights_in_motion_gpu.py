"""GPU suite: the four derived copies of the network follow the parameters as training moves them (host half and the bars:
tests/test_weights_in_motion_host.py, tests/motion_util.py; DESIGN section 2 "Weights in motion").

  * the target net's GRU images and merged dueling layers (_gru_cache / _fc2_cache), refreshed in place by load_state_dict under a
    captured train step: six learner.train calls across three target syncs against the REFERENCE's own train() on the same batch
    (tests/golden/learner_target_sync.npz), eager and captured, f32 and class-code storage, and the bf16 variant.  With the sync
    suppressed the same run misses the reference at call 3 by more than 10 bars (the reference's own unsynced run: 294 / 1041 bars).
  * the rollout's weight images (FastPolicy.pack: eager, its own hipGraph, part of the captured opening graph): every rollout of a
    training loop is held to a float64 stepwise controller with the weights it was played with -- the stored recurrent state of all
    13 slots within STATE_TOL = 1e-5 -- and must MISS the weights of one train step earlier by more than 10 STATE_TOL.  Licence for the
    latter, measured on the host (test_one_train_step_moves_the_float64_states_by_100_bars): one train step moves the float64 states
    by 1.87e-2 .. 4.11e-2 on the fixture batch, >= 100 STATE_TOL, so the one-step-earlier copy is used.  The packed images are
    bit-equal to those of a FastPolicy constructed afresh (an eager pack) at the moment the rollout ends.
  * a greedy test rollout after the last step: every stored action is the masked float64 argmax wherever the top two are more than
    4 TOL_Q apart.  Rows left out: the three learner fixtures stay under the 1 % cap (0.0000, host test), a greedy rollout cannot be
    held to it -- its envs are copies of each other, one near-tie takes 1 / 65 of the rows -- and is capped at 5 %
    (motion_util.ROLLOUT_EXCLUDED_CAP, with the reasoning; measured 0.0154 pipelined, 0.0000 four_launch).
Every case prints its max state error, stale-copy error, excluded-row share and the pack states it reached."""
import pytest
import torch as th

from homophily_marl_amd import ops
from tests import motion_util as mu
from tests.test_stored_state_gpu import N_ENV, T_EP, _ctx

pytestmark = pytest.mark.gpu

BF16_Q_TOL = 2e-2            # tests/test_hip_learner_path.py: the bf16 variant's bar


# ---- the trajectory across target syncs on the device -----------------------------------------------------------------------------------
def _device_learner(train_graph, storage, **over):
    from tests.learner_util import build, load_fixture
    th.backends.cuda.matmul.allow_tf32 = False
    zs, _ = load_fixture("learner_target_sync.npz")
    z, meta = load_fixture("learner_cleanup5.npz")
    args, batch, mac, learner = build(z, meta, device="cuda:0", overrides=dict(dict(target_update_interval=2, train_graph=train_graph), **over),
                                      code_obs=storage == "code")
    assert learner._fused(batch) and learner.use_graph == train_graph and args.target_update_interval == 2
    seen = []
    name = "_graph_step" if train_graph else "cal_loss_and_step"
    inner = getattr(learner, name)

    def step(b):
        seen.append(inner(b))
        return seen[-1]
    setattr(learner, name, step)
    return zs, batch, mac, learner, seen


@pytest.mark.parametrize("train_graph,storage", [(False, "f32"), (True, "f32"), (False, "code"), (True, "code")])
def test_six_train_calls_across_target_syncs_on_the_device(train_graph, storage):
    """With train_graph the step is captured at call 3 and replayed at calls 3 .. 6: call 5 is a replay that bootstraps from the target
    net synced after call 4, through caches whose addresses the graph baked in.  Measured on an MI355X: every call within 0.024 of
    its bar in all four arms (losses <= 3.4e-8 off the reference)."""
    zs, batch, mac, learner, seen = _device_learner(train_graph, storage)
    tgt = learner.target_mac.agent
    ops.set_strict(storage == "code")
    try:
        ptrs = None
        for k in range(1, 7):
            learner.train(batch, 0, k)
            errors = mu.call_errors(zs, k, seen[-1], mac)
            print("graph %s %s call %d: worst %s at %.3f of its bar; losses %s" % ((train_graph, storage, k) + mu.worst(errors) + (
                {key: "%.2e" % errors[key][0] for key in mu.LOG_KEYS[:3]},)))
            for name, (err, bar) in errors.items():
                assert err < bar, (k, name, err, bar)
            assert (learner._graph is not None) == (train_graph and k >= 3)
            if k == 1:
                ptrs = [t.data_ptr() for t in mu.cache_tensors(tgt)]
            if k % 2 == 0:
                assert learner.last_target_update_episode == k
                mu.assert_caches_follow(tgt, mac.agent, ptrs, "after the sync of call %d" % k)
        assert [t.data_ptr() for t in mu.cache_tensors(tgt)] == ptrs
    finally:
        ops.set_strict(False)


def test_a_suppressed_target_sync_misses_the_reference_on_the_device():
    zs, batch, mac, learner, seen = _device_learner(True, "code")
    mu.suppress_sync(learner)
    power = int(zs["power_call"])
    ops.set_strict(True)
    try:
        for k in range(1, power + 1):
            learner.train(batch, 0, k)
            errors = mu.call_errors(zs, k, seen[-1], mac)
            if k < 3:
                assert mu.worst(errors)[1] < 1, (k, errors)
        ratios = {key: errors[key][0] / errors[key][1] for key in ("loss_value_env", "loss_value_inc")}
        print("sync suppressed, call %d (captured): error / bar %s" % (power, ratios))
        assert learner._graph is not None and max(ratios.values()) > 10, ratios
    finally:
        ops.set_strict(False)


def test_bf16_variant_across_target_syncs():
    """learner_dtype bf16, its own captured step: the TD losses of calls 3 and 5 (each right after a sync) at the variant's bar.
    Measured: |error| <= 7.4e-6 at both calls.  The bar is the variant's Q bar and cannot see a stale target net here (with the GRU
    cache refresh removed the errors are 1.0e-2 / 1.3e-2): this arm holds that the variant's own captured step runs across syncs and
    stays at the reference; the staleness is held by the f32 arms (1037 bars at call 3, 1280 at call 5 under the same removal)."""
    zs, batch, mac, learner, seen = _device_learner(True, "code", learner_dtype="bf16")
    assert learner.precision == 1
    ops.set_strict(True)
    try:
        for k in range(1, 7):
            learner.train(batch, 0, k)
            if k in (3, 5):
                for key in ("loss_value_env", "loss_value_inc", "loss_sim"):
                    err = abs(float(seen[-1][key]) - float(zs["call%d_%s" % (k, key)]))
                    print("bf16 call %d %s: |error| %.2e" % (k, key, err))
                    assert err < BF16_Q_TOL, (k, key, err)
        assert learner._graph is not None
        assert all(bool(th.isfinite(p).all()) for p in mac.parameters())
    finally:
        ops.set_strict(False)
        ops.set_learner_precision(2)


# ---- rollouts follow the weights the learner has just stepped ---------------------------------------------------------------------------
IMAGES = ("img_env", "img_inc", "conv_frags", "lin_frags")


def _loop_ctx(**over):
    return _ctx(train_stored_state=True, target_update_interval=2, **over)


def _fresh_images(ctx, keys):
    """the images of a FastPolicy constructed now on the same controller (an eager pack of the current weights)"""
    from homophily_marl_amd.fast_policy import FastPolicy
    fast = ctx.runner.fast
    fresh = FastPolicy(ctx.mac, fast.N, fast.avail, seed=fast.seed, fused=fast.fused, precision=fast.precision, env_id_base=fast.env_id_base)
    assert getattr(fresh, "_pack_graph", None) is None and fresh._pack_calls == 1
    th.cuda.synchronize()
    return {k: fresh.p[k].clone() for k in keys}


def _rollout(ctx, host_mac, played, stale, keys, tag, test_mode=False):
    """one rollout: its images against a fresh policy's, its stored state against the float64 controller with `played` (must hold) and
    with `stale` (None, or must miss).  Returns (batch, the episode's fields, the float64 controller's outputs)."""
    runner = ctx.runner
    batch = runner.run(test_mode=test_mode)
    th.cuda.synchronize()
    images = {k: runner.fast.p[k].clone() for k in keys}
    fresh = _fresh_images(ctx, keys)
    for k in keys:
        assert th.equal(images[k], fresh[k]), (tag, k)
    ep = mu.episode_fields(batch.data.transition_data)
    hidden = batch["hidden"]
    assert hidden.shape == (N_ENV, T_EP + 1, 5, 128)
    out = mu.controller64(host_mac, played, ep)
    err = mu.state_error(hidden, out[2], out[3])
    stale_err = None if stale is None else mu.state_error(hidden, *mu.controller64(host_mac, stale, ep)[2:])
    print("%s: stored state against the float64 controller: %.3e (bar %.0e); one train step earlier: %s" % (
        tag, err, mu.STATE_TOL, "-" if stale_err is None else "%.3e" % stale_err))
    assert err < mu.STATE_TOL, (tag, err)
    assert stale_err is None or stale_err > 10 * mu.STATE_TOL, (tag, stale_err)
    return batch, ep, out


def _train(ctx, batch):
    a = ctx.args
    ctx.buffer.insert_episode_batch(batch)
    sample = ctx.buffer.sample_windows(a.batch_size, a.train_window, a.train_burn_in, out=ctx.learner.sample_out())
    ctx.learner.train(sample, ctx.runner.t_env, ctx.train_steps)
    ctx.train_steps += 1


@pytest.mark.parametrize("form,over", [("pipelined", {}), ("four_launch", dict(pipeline_encode=False))], ids=["pipelined", "four_launch"])
def test_rollouts_follow_the_weights_the_learner_has_just_stepped(form, over):
    """Seven training rollouts with a train step after each (captured from the third; target syncs after steps 2, 4, 6), then one
    greedy test rollout.  Measured on the host (tests/test_weights_in_motion_host.py): one train step moves the float64 states by
    >= 1.87e-2 = 1870 STATE_TOL, so every rollout from the second on must miss the previous weights by more than 10 STATE_TOL."""
    ctx = _loop_ctx(**over)
    try:
        runner, mac = ctx.runner, ctx.mac
        host_mac = mu.host_controller(mac, ctx.buffer.scheme)
        copies, pure, packs = [], 0, []
        for e in range(1, 8):
            had_opening = {id(b) for b in runner._bundles.values() if b.begin_graph is not None}
            played = mu.agent64(mac)                                          # the weights after the previous train step
            batch, _, _ = _rollout(ctx, host_mac, played, copies[-1] if copies else None, IMAGES, "%s rollout %d" % (form, e))
            assert (runner.fast is not None, runner.pipe) == (True, form == "pipelined")
            pure += int(id(runner._bundle) in had_opening)
            packs.append("opening graph" if id(runner._bundle) in had_opening else
                         "pack graph" if getattr(runner.fast, "_pack_graph", None) is not None else "eager")
            copies.append(played)
            _train(ctx, batch)
        th.cuda.synchronize()
        print("%s: pack states reached: %s; pure-replay openings %d" % (form, packs, pure))
        assert runner.fast._pack_graph is not None and runner._bundle.begin_graph is not None and pure >= 2
        assert packs[0] == "eager" and "pack graph" in packs and "opening graph" in packs
        assert ctx.learner._graph is not None and ctx.learner.last_target_update_episode == 6
        # a greedy rollout with the weights of the last train step
        net = mu.agent64(mac)
        batch, ep, (q_env, q_inc, _, _) = _rollout(ctx, host_mac, net, copies[-1], IMAGES, "%s test rollout" % form, test_mode=True)
        assert float(runner.eps) == 0.0
        ref_a, clear, ref_i, clear_i, off = mu.greedy_rows(q_env, q_inc, runner.env.avail_actions_batch[0, 0])
        share = mu.excluded_share(clear, clear_i, off)
        print("%s test rollout: rows left out of the greedy comparison: env %.4f inc %.4f" % ((form,) + share))
        out_rows = (~clear).nonzero()
        print("    left out (slot, agent): envs  %s" % {(int(t), int(i)): int(((out_rows[:, 1] == t) & (out_rows[:, 2] == i)).sum())
                                                       for t, i in {(int(r[1]), int(r[2])) for r in out_rows}})
        assert max(share) < mu.ROLLOUT_EXCLUDED_CAP
        acts, inc = ep["actions"].squeeze(-1), ep["actions_inc"].squeeze(-1)
        assert (acts == ref_a)[clear].all()
        assert (inc == ref_i)[clear_i & off].all() and not inc.diagonal(dim1=2, dim2=3).any()
        assert runner.env.native.poll_error() == 0
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


@pytest.mark.parametrize("case,flags,rows", [
    ("gathered", dict(fused_onehot_gather=True, obs_distance=True), ("onehot_env", "onehot_inc")),
    ("others", dict(obs_others_last_action=True, fused_others_last_action=True), ("rows_env", "rows_inc")),
    ("per_layer", dict(fused_policy=False, obs_storage="f32"), ("w1e", "w2e", "w1i_x", "w1i_a", "wie", "whe", "wii", "whi", "w2i_h", "w2i_o", "b2i", "lw_t"))],
    ids=["gathered", "others", "per_layer"])
def test_row_tables_follow_a_train_step(case, flags, rows):
    """rollout - train - rollout under the gathered input layouts (tests/test_heads_onehot_gather.py "shipped_distance",
    tests/test_heads_others_last_action.py "shipped_others"): the fc1 row tables the pack launch writes, with the images; and on the
    per-layer heads (fused_policy off), whose GEMM-ready packs p[...] the same pack() copies"""
    ctx = _loop_ctx(strict_device_ops=False, **flags)
    try:
        host_mac = mu.host_controller(ctx.mac, ctx.buffer.scheme)
        keys = (IMAGES if case != "per_layer" else ()) + rows
        first = mu.agent64(ctx.mac)
        batch, _, _ = _rollout(ctx, host_mac, first, None, keys, "%s rollout 1" % case)
        fast = ctx.runner.fast
        assert fast.fused == (case != "per_layer") and (fast.gather, fast.others) == (case == "gathered", case == "others")
        tables = {k: fast.p[k].clone() for k in rows}
        _train(ctx, batch)
        _rollout(ctx, host_mac, mu.agent64(ctx.mac), first, keys, "%s rollout 2" % case)
        assert not any(th.equal(tables[k], fast.p[k]) for k in rows)            # the tables moved with the weights
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()


def test_rollout_after_load_models_plays_the_loaded_weights(tmp_path):
    """saved after train step 2, trained and rolled out to episode 5, loaded: rollout 6 (a replayed opening graph on its storage)
    follows the LOADED weights and misses those of just before the load"""
    ctx = _loop_ctx()
    try:
        runner, mac, learner = ctx.runner, ctx.mac, ctx.learner
        host_mac = mu.host_controller(mac, ctx.buffer.scheme)
        saved = None
        for e in range(1, 6):
            batch = runner.run(test_mode=False)
            _train(ctx, batch)
            if e == 2:
                learner.save_models(str(tmp_path))
                saved = mu.agent64(mac)
        before = mu.agent64(mac)
        had_opening = {id(b) for b in runner._bundles.values() if b.begin_graph is not None}
        learner.load_models(str(tmp_path))
        loaded = mu.agent64(mac)
        for (name, x), y in zip(loaded.state_dict().items(), saved.state_dict().values()):
            assert th.equal(x, y), name
        assert learner._graph is None
        _rollout(ctx, host_mac, loaded, before, IMAGES, "rollout after load_models")
        assert id(runner._bundle) in had_opening                              # the pack ran inside the replayed opening graph
        mu.assert_caches_follow(learner.target_mac.agent, mac.agent, [t.data_ptr() for t in mu.cache_tensors(learner.target_mac.agent)],
                                "after load_models")
    finally:
        ops.set_strict(False)
        ctx.runner.close_env()
