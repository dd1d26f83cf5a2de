"""GPU: the learner's unroll of the live and the target net with every affine layer and dueling combination launched once for both, on
fc1 rows assembled by one launch (HomophilyLearner.unroll_pair -> HomophilyMAC.unroll_rows_pair, HomophilyAgent.unroll_pre_pair /
unroll_post_pair) against the two nets unrolled separately (mac.unroll, target_mac.unroll: the single launches and the tensor-op
assembly), at B = 2, T = 5, n = 2 and 5, view 7: the four Q tensors and the flat parameter gradient of a fixed scalar of (q_env,
q_inc) are equal bit for bit (torch.equal) -- eager, and as a captured and replayed step -- under strict_device_ops.

Two observation storages.  `code` (u8 class codes: the encoder kernels, the storage the train step is benchmarked with): every kernel
on the path is deterministic, so the reference is held to reproduce itself and every parameter's gradient is compared.  `f32` (float
planes: the encoder as tensor operations, torch's convolution backward): the reference is evaluated a second time after the paired
step, and a parameter enters the comparison when the two reference evaluations agree on it bit for bit.  Measured on MI355X: the
weight gradient of the library convolution (conv_to_fc.0.weight) differs between two evaluations of the same step by 5e-9; only
parameters of that encoder may drop out, all others must be reproduced, and on those the paired step must equal the reference."""
import pytest
import torch as th

from homophily_marl_amd import ops

pytestmark = pytest.mark.gpu
NAMES = ("q_env", "q_inc", "tq_env", "tq_inc", "flat gradient")


def _separate(learner, batch):
    q_env, q_inc = learner.mac.unroll(batch)
    with th.no_grad():
        tq_env, tq_inc = learner.target_mac.unroll(batch)
    return q_env, q_inc, tq_env, tq_inc


def _step(learner, batch, unroll, seeds):
    """the four Q tensors and the flat gradient of sum(q_env * seeds[0]) + sum(q_inc * seeds[1]) (learner._backward: the train step's own)"""
    q_env, q_inc, tq_env, tq_inc = unroll(learner, batch)
    learner._backward([q_env, q_inc], seeds=seeds)
    return [q_env.detach(), q_inc.detach(), tq_env, tq_inc, learner._flat_grad]


def _diverging(learner, a, b):
    """the parameters on whose slices two flat gradients differ (the first names the faulty part)"""
    assert a.numel() == b.numel() == sum(p.numel() for p in learner.params)
    names = {id(p): k for k, p in learner.mac.named_parameters()}
    out, off = [], 0
    for p in learner.params:
        if not th.equal(a[off:off + p.numel()], b[off:off + p.numel()]):
            out.append(names[id(p)])
        off += p.numel()
    return out


def _compare(learner, tag, got, want, unstable):
    for name, a, b in zip(NAMES[:4], got, want):
        assert a.shape == b.shape and th.equal(a, b), (tag, name, float((a - b).abs().max()))
    differ = _diverging(learner, got[4], want[4])
    print(tag, "gradient differs on", differ, "reference differs from itself on", unstable)
    assert set(differ) <= set(unstable), (tag, differ, unstable, float((got[4] - want[4]).abs().max()))


@pytest.mark.parametrize("storage", ["f32", "code"])
@pytest.mark.parametrize("n", [2, 5])
def test_unroll_pair_equals_the_separate_unrolls_eager_and_replayed(n, storage):
    from tests.test_hip_learner_path import _random_learner_batch
    B, T = 2, 5
    batch, learner, _ = _random_learner_batch(B, T, n, "cleanup", seed=11 + n)
    if storage == "code":
        codes = th.randint(0, 4, (B, T + 1, n, 15, 15), generator=th.Generator().manual_seed(n), dtype=th.uint8).cuda()
        batch.data.transition_data["obs"] = codes
        assert learner.mac.unroll_shared(batch)["codes"] is not None
    A = learner.n_actions
    g = th.Generator().manual_seed(n)
    seeds = [th.randn(B, T + 1, n, A, generator=g).cuda(), th.randn(B, T + 1, n, n, 3, generator=g).cuda()]
    pair = lambda l, b: l.unroll_pair(b)
    was = ops.STRICT
    ops.set_strict(True)
    try:
        want = [t.clone() for t in _step(learner, batch, _separate, seeds)]
        assert not th.equal(want[0], want[2]) and float(want[4].abs().max()) > 0          # the target net differs; the gradient is there
        got = [t.clone() for t in _step(learner, batch, pair, seeds)]
        again = [t.clone() for t in _step(learner, batch, _separate, seeds)]
        # the reference against itself: everything but the library convolution's parameters is reproduced (all of it with class codes)
        for name, a, b in zip(NAMES[:4], again, want):
            assert th.equal(a, b), ("reference", name)
        unstable = _diverging(learner, again[4], want[4])
        assert all(k.startswith("agent.conv_to_fc.") for k in unstable) and (storage == "f32" or not unstable), unstable
        _compare(learner, "eager", got, want, unstable)
        # captured and replayed (the train step's own capture: a stream of its own, the affine backward's scratch reserved before)
        th.cuda.synchronize()
        stream = th.cuda.Stream()
        ops.reserve_bmm_scratch(stream)
        graph = th.cuda.CUDAGraph()
        with ops.capture(graph, stream=stream, capture_error_mode="thread_local"):
            static = _step(learner, batch, pair, seeds)
        for t in static:
            t.zero_()
        graph.replay()
        th.cuda.synchronize()
        _compare(learner, "replayed", static, want, unstable)
    finally:
        ops.set_strict(was)
