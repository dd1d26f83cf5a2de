"""GPU suite: the loss flags double_q: False and consider_others_inc: True on the fused loss kernel (k_td_sim_loss) and in the captured
train step -- against the numbers the reference's learner recorded (tests/golden/learner_options.npz), against the tensor-op statement
on random batches, and captured against eager."""
import numpy as np
import pytest
import torch as th

from tests.test_learner_options import CASES, LOG_KEYS, case, check_step, perturb_target

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("train_graph,storage", [(False, "f32"), (True, "f32"), (False, "code"), (True, "code")])
@pytest.mark.parametrize("name", CASES)
def test_fused_learner_matches_reference_options(name, train_graph, storage):
    """Two optimisation steps on the device under the case's flags, every logged value within 1e-5 and every parameter after each step,
    eagerly and replayed from the captured train step; code storage with every operator on the HIP kernels (strict_device_ops)."""
    from homophily_marl_amd import ops
    from tests.learner_util import build
    th.backends.cuda.matmul.allow_tf32 = False
    rec, (z, meta), overrides = case(name)
    args, batch, mac, learner = build(z, meta, device="cuda:0", overrides=dict(overrides, train_graph=train_graph),
                                      code_obs=storage == "code")
    ops.set_strict(storage == "code")
    try:
        assert learner._fused(batch) and learner.use_graph == train_graph
        assert (args.double_q, args.consider_others_inc) == (overrides["double_q"], overrides["consider_others_inc"])
        if train_graph:
            # past the capture (third call) on a scratch copy of the weights, then rewind weights, target net and optimiser state
            sd0 = {k: v.clone() for k, v in mac.agent.state_dict().items()}
            for _ in range(3):
                learner.train(batch, 0, 0)
            assert learner._graph is not None
            mac.agent.load_state_dict(sd0)
            learner.target_mac.load_state(mac)
            for opt in (learner.optimiser_env, learner.optimiser_inc):
                for st in opt.state.values():
                    st["step"].zero_(); st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
        perturb_target(learner)
        for step in range(2):
            if train_graph:
                learner.train(batch, 0, 0)
                logs = learner._static_logs
            else:
                logs = learner.cal_loss_and_step(batch)
            check_step(logs, mac, rec, step)
        if train_graph:
            assert learner._graph is not None
    finally:
        ops.set_strict(False)


@pytest.mark.parametrize("double_q,others", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("B,T,n,kind", [(16, 100, 5, "cleanup"), (5, 23, 10, "cleanup"), (7, 31, 5, "harvest")])
def test_fused_loss_kernel_matches_the_tensor_op_loss_options(B, T, n, kind, double_q, others):
    """k_td_sim_loss against the tensor-op statement + autograd on the same batch and weights under every combination of the two flags:
    every logged value (1e-5 relative) and the whole flat parameter gradient (2e-6 relative)."""
    from tests.test_hip_learner_path import _random_learner_batch
    batch, fused, plain = _random_learner_batch(B, T, n, kind, seed=B + T)
    for lr in (fused, plain):
        lr.args.double_q, lr.args.consider_others_inc = double_q, others
    assert fused._fused(batch) and not plain._fused(batch)
    d1, d2 = fused.denominators(batch), plain.denominators(batch)
    assert d1[0] == d2[0] and d1[1] == d2[1]
    l1 = fused.forward_backward(batch, d1)
    l2 = plain.forward_backward(batch, d2)
    for k in LOG_KEYS:
        assert abs(float(l1[k]) - float(l2[k])) < 1e-5 * max(1.0, abs(float(l2[k]))), (k, float(l1[k]), float(l2[k]))
    g1, g2 = fused._flat_grad, plain._flat_grad
    assert float(g2.abs().max()) > 1e-4
    assert float((g1 - g2).abs().max()) < 2e-6 * max(1.0, float(g2.abs().max())), (float((g1 - g2).abs().max()), float(g2.abs().max()))


def test_captured_consider_others_inc_step_equals_the_eager_step():
    """Five train calls with consider_others_inc: the hipGraph learner (eager twice, captured at the third call, replayed after) and an
    eager learner from the same weights and target net stay within 1e-5 in every logged value and every parameter."""
    from types import SimpleNamespace
    from homophily_marl_amd.controllers import REGISTRY as mac_REGISTRY
    from homophily_marl_amd.learners import REGISTRY as le_REGISTRY
    from tests.test_hip_learner_path import _random_learner_batch
    batch, eager, _ = _random_learner_batch(16, 100, 5, "cleanup", seed=3)
    eager.args.consider_others_inc = True
    a = SimpleNamespace(**vars(eager.args)); a.train_graph = True
    mac = mac_REGISTRY[a.mac](batch.scheme, {"agents": 5}, a).cuda()
    mac.agent.load_state_dict(eager.mac.agent.state_dict())
    graph = le_REGISTRY[a.learner](mac, batch.scheme, SimpleNamespace(log_stat=lambda *x, **k: None, console_logger=None), a)
    graph.cuda()
    graph.target_mac.load_state(eager.target_mac)
    assert graph._fused(batch)
    for call in range(5):
        lg = graph._graph_step(batch)
        le = eager.cal_loss_and_step(batch)
        for k in LOG_KEYS:
            assert abs(float(lg[k]) - float(le[k])) < 1e-5, (call, k, float(lg[k]), float(le[k]))
        pg = th.cat([p.detach().reshape(-1) for p in graph.mac.parameters()])
        pe = th.cat([p.detach().reshape(-1) for p in eager.mac.parameters()])
        assert float((pg - pe).abs().max()) < 1e-5, call
    assert graph._graph is not None and graph._graph_calls == 5
    assert np.isfinite(float(le["loss_value_inc"]))
