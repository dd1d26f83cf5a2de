"""The host (tensor-op) branch of every operator of homophily_marl_amd/ops.py against the independent float64 statements of
tests/ops_contract_util.py: outputs and gradients, at the shapes the device suite (tests/test_ops_contract_gpu.py) uses.  This proves
the statements before they are used on the device and pins the semantics the device branch has to match: the bias forms th.baddbmm
broadcasts, the gradient of `other`, one recurrence-weight tensor with a gradient on a prefix of the states.

Bar: 1e-6 * max(1, max |ref|) (ops_contract_util.HOST_BAR): the two sides differ by the f32 rounding of short sums only."""
import numpy as np
import pytest
import torch as th

from homophily_marl_amd import ops
from tests import ops_contract_util as U

BMM_SHAPES = [(2, 17, 5, 20), (3, 33, 80, 3), (1, 4100, 5, 3)]
GRU_SHAPES = [(3, 2, 5), (2, 3, 16)]
HEAD_SHAPES = [(2, 2, 4, 1, 8, 0), (3, 3, 5, 3, 3, 16), (3, 3, 5, 3, 3, 15)]
Q_SHAPES = [(3, 3, 5, 3, 3), (2, 2, 4, 1, 16)]
GATE_SHAPES = [(17, 64), (5, 3)]
ENCODE_SHAPES = [(5, 5), (4, 15), (3, 31)]
# (projection parts, weight parts, parts whose states enter the loss), T = 2, B = 16, sets per part 1 and 2
PARTS_CASES = [(4, 4, (0, 1)), (4, 1, (0, 1)), (2, 1, (0,)), (4, 2, (0,)), (4, 2, (0, 1, 2)), (4, 4, (1,)), (3, 1, (0, 1, 2))]


def _check(case, outs, leaves):
    """outputs and, after one backward with the case's cotangents, the gradient of every leaf that asked for one"""
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    for k, (o, r) in enumerate(zip(outs, case["outs"])):
        U.close_host(o.detach().numpy(), r, "output %d" % k)
    loss = sum((o * th.tensor(np.array(c))).sum() for o, c in zip(outs, case["cots"]) if c is not None)
    loss.backward()
    for name, t in leaves.items():
        if t.requires_grad:
            assert t.grad is not None, name
            U.close_host(t.grad.numpy(), case["grads"][name], "d_" + name)


@pytest.mark.parametrize("fn,args", [(U.bias_bmm_case, (2, 17, 5, 20, True)), (U.gru_case, (3, 2, 5)), (U.gru_parts_case, (2, 16, 1, 4, (0, 1))),
                                     (U.gru_gates_case, (5, 3)), (U.dueling_q_case, (3, 3, 5, 3, 3)), (U.dueling_head_case, (3, 3, 5, 3, 3, 15)),
                                     (U.cat_case, ((0,),)), (U.row_sums_case, ((3, 7, 5),)), (U.encode_case, (4, 15))])
def test_a_statement_reproduces_itself(fn, args):
    U.rerun_is_identical(fn, *args)


@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("n,R,I,O", BMM_SHAPES)
def test_bias_bmm(n, R, I, O, leaky):
    case = U.bias_bmm_case(n, R, I, O, leaky)
    t = U.tensors(case, "cpu", requires=("x", "w", "b"))
    _check(case, ops.bias_bmm(t["x"], t["w"], t["b"], leaky=leaky), t)


@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("bias", ["11O", "O", "nRO"])
def test_bias_bmm_takes_every_bias_baddbmm_broadcasts(bias, leaky):
    case = U.bias_bmm_case(2, 17, 5, 20, leaky, bias)
    t = U.tensors(case, "cpu", requires=("x", "w", "b"))
    _check(case, ops.bias_bmm(t["x"], t["w"], t["b"], leaky=leaky), t)


@pytest.mark.parametrize("T,G,B", GRU_SHAPES)
def test_gru_sequence(T, G, B):
    case = U.gru_case(T, G, B)
    t = U.tensors(case, "cpu", requires=("gi", "wh", "bh"))
    _check(case, ops.gru_sequence(t["gi"], t["wh"], t["bh"]), t)


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("n_parts,n_w,used", PARTS_CASES)
def test_gru_sequence_parts(n_parts, n_w, used, spp):
    """the weights as ONE tensor or as n_w parts, a cotangent on the `used` parts only: every weight part gets its full-size
    gradient (zeros for the sets whose states carry none)"""
    T, B, G = 2, 16, spp * n_parts
    case = U.gru_parts_case(T, B, spp, n_parts, used)
    inp = case["inputs"]
    parts = [th.tensor(U.set_major(inp["gi"], k, spp), requires_grad=True) for k in range(n_parts)]
    spw = G // n_w
    whs = [th.tensor(np.array(inp["wh"][k * spw:(k + 1) * spw]), requires_grad=True) for k in range(n_w)]
    bhs = [th.tensor(np.array(inp["bh"][k * spw:(k + 1) * spw]), requires_grad=True) for k in range(n_w)]
    hs = ops.gru_sequence_parts(parts, T, B, whs[0] if n_w == 1 else whs, bhs[0] if n_w == 1 else bhs)
    assert len(hs) == n_parts
    U.close_host(th.cat([h.detach() for h in hs]).numpy(), case["outs"][0], "hs")
    cot = th.tensor(np.array(case["cots"][0]))
    sum((hs[k] * cot[k * spp:(k + 1) * spp]).sum() for k in used).backward()
    d_gi = np.concatenate([U.set_major(case["grads"]["gi"], k, spp) for k in range(n_parts)])
    got = np.concatenate([(p.grad if p.grad is not None else th.zeros_like(p)).numpy() for p in parts])
    U.close_host(got, d_gi, "d_gi")
    for name, ts in (("wh", whs), ("bh", bhs)):
        for k, w in enumerate(ts):
            assert w.grad is not None, (name, k)
            U.close_host(w.grad.numpy(), case["grads"][name][k * spw:(k + 1) * spw], "d_%s part %d" % (name, k))


@pytest.mark.parametrize("R,H", GATE_SHAPES)
def test_gru_gates(R, H):
    case = U.gru_gates_case(R, H)
    t = U.tensors(case, "cpu", requires=("gi", "gh", "h"))
    _check(case, ops.gru_gates(t["gi"], t["gh"], t["h"]), t)


@pytest.mark.parametrize("n,T,B,inner,K", Q_SHAPES)
def test_dueling_q(n, T, B, inner, K):
    case = U.dueling_q_case(n, T, B, inner, K)
    t = U.tensors(case, "cpu", requires=("a", "v"))
    q = ops.dueling_q(t["a"], t["v"], B, T, inner)
    assert q.shape == ((B, T, n, K) if inner == 1 else (B, T, n, inner, K))
    _check(case, q.reshape(B, T, n, inner, K), t)


@pytest.mark.parametrize("n,T,B,inner,K,E", HEAD_SHAPES)
def test_dueling_head_with_a_gradient_for_other(n, T, B, inner, K, E):
    case = U.dueling_head_case(n, T, B, inner, K, E)
    t = U.tensors(case, "cpu", requires=("h", "other", "w", "b"))
    q = ops.dueling_head(t["h"], t.get("other"), t["w"], t["b"], B, T, inner)
    assert q.shape == ((B, T, n, K) if inner == 1 else (B, T, n, inner, K))
    _check(case, q.reshape(B, T, n, inner, K), t)


def test_dueling_head_with_a_broadcast_bias():
    case = U.dueling_head_case(3, 3, 5, 3, 3, 16, 64, "11K")
    t = U.tensors(case, "cpu", requires=("h", "other", "w", "b"))
    _check(case, ops.dueling_head(t["h"], t["other"], t["w"], t["b"], 5, 3, 3), t)


@pytest.mark.parametrize("used", [(0,), (1,), (0, 1)])
def test_cat_groups(used):
    case = U.cat_case(used)
    t = U.tensors(case, "cpu", requires=tuple(case["inputs"]))
    groups = [[t["t%d_%d" % (i, j)] for j in range(len(grp))] for i, grp in enumerate(U.CAT_SHAPES)]
    outs = ops.cat_groups(groups)
    for k, (o, r) in enumerate(zip(outs, case["outs"])):
        assert np.array_equal(o.detach().numpy(), r.astype(np.float32)), k      # a copy: exact
    sum((o * th.tensor(np.array(c))).sum() for o, c in zip(outs, case["cots"]) if c is not None).backward()
    for i, grp in enumerate(U.CAT_SHAPES):
        for j in range(len(grp)):
            g = t["t%d_%d" % (i, j)].grad
            if i in used:
                assert np.array_equal(g.numpy(), case["grads"]["t%d_%d" % (i, j)].astype(np.float32))
            else:
                assert g is None or not g.any()


@pytest.mark.parametrize("shape", [(17, 5), (3, 7, 5), (2, 3, 7, 5)])
def test_column_sums(shape):
    case = U.row_sums_case(shape)
    U.close_host(ops.column_sums(th.tensor(np.array(case["inputs"]["x"]))).numpy(), case["outs"][0], "sums")


def test_column_sums_refuses_a_vector_by_name():
    with pytest.raises(ValueError, match=r"\bx\b"):
        ops.column_sums(th.zeros(5))


@pytest.mark.parametrize("R,V", ENCODE_SHAPES)
def test_encode_codes(R, V):
    case = U.encode_case(R, V)
    t = U.tensors(case, "cpu", requires=("conv_w", "conv_b", "lin_w", "lin_b"))
    assert np.array_equal(ops.expand_codes(t["codes"]).double().numpy(), U.st_planes(t["codes"]).numpy())
    _check(case, ops.encode_codes(t["codes"], t["conv_w"], t["conv_b"], t["lin_w"], t["lin_b"]), t)


def test_a_precision_block_restores_what_it_found_also_when_it_raises():
    """ops._precision (the backward of every Function, HomophilyLearner.train): nothing is set when nothing changes; what was found
    comes back when the block raises, too (the library call replaced: no device here)"""
    assert ops.LEARNER_PRECISION == 2
    with ops._precision(2):
        assert ops.LEARNER_PRECISION == 2
    calls = []
    real = ops.set_learner_precision
    try:
        def fake(p):
            calls.append(p)
            ops.LEARNER_PRECISION = p
        ops.set_learner_precision = fake
        with pytest.raises(KeyError):
            with ops._precision(1):
                assert ops.LEARNER_PRECISION == 1
                raise KeyError("x")
        assert calls == [1, 2] and ops.LEARNER_PRECISION == 2
    finally:
        ops.set_learner_precision = real
        ops.LEARNER_PRECISION = 2
