"""GPU: the paired forward launches of the train step (ssd_bias_bmm_pair_fwd, ssd_dueling_head_pair_fwd: one layer, or one dueling
combination, of the learner's live and target net in ONE grid) against the single launches, which stay the reference: every output of a
pair equals the single launch's bit for bit (np.array_equal / torch.equal), because a weight set's arithmetic does not depend on the
other sets of its grid.  All operands and outputs of a case sit in a poisoned arena (tests/arena_util.py), so a write outside an
output, an output element left out and a read of the surroundings that reaches the arithmetic all show.

Shapes: set counts 1, 2, 5 for either group (all nine pairs cycle through the cases); 1, 17 and 33 rows (one ragged 16-row tile, one
and two whole tiles plus one row); the layer shapes of the train step -- (50, 64) fc1 (scalar row loads: 50 is not a multiple of 4),
(64, 192) the GRU projection (three output tiles per wave, two groups), (64, 10) the env head's [advantage | value] layer -- and the
two-source rows [50 | 9] -> 64 (per-column source select; the single reference is the single launch on the concatenated rows, the
single two-source launch takes first sources of whole 16-column chunks only) and [64 | 16] -> 4 with the first source shared by
x1_div = 5 rows (the incentive head's layer); LeakyReLU on and off; both learner precisions."""
import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests.arena_util import Arena

pytestmark = pytest.mark.gpu

COUNTS = [(a, b) for a in (1, 2, 5) for b in (1, 2, 5)]
ROWS = (1, 17, 33)
OFFS = (4, 8, 12, 0)
# (I1, I2, O, x1_div, x2_shared)
LAYERS = [(50, 0, 64, 1, 0), (64, 0, 192, 1, 0), (64, 0, 10, 1, 0), (50, 9, 64, 1, 0), (64, 16, 4, 5, 1)]
CASES = [(LAYERS[k], ROWS[r], COUNTS[(3 * k + r + 4 * (p - 1)) % 9], p) for k in range(len(LAYERS)) for r in range(3) for p in (2, 1)]


def call(name, *args):
    lib = abi.load_library()
    abi.check(lib, getattr(lib, name)(*args))


def f32(a):
    return np.asarray(a, dtype=np.float32)


class precision:
    def __init__(self, p):
        self.p = p

    def __enter__(self):
        call("ssd_set_learner_precision", self.p)

    def __exit__(self, *exc):
        call("ssd_set_learner_precision", 2)


def test_the_cases_meet_every_set_count_pair_and_precision():
    assert {c[2] for c in CASES} == set(COUNTS) and {c[3] for c in CASES} == {1, 2} and {c[1] for c in CASES} == set(ROWS)


@pytest.mark.parametrize("layer,R,counts,prec", CASES, ids=["%dx%d_%d-R%d-n%d_%d-p%d" % (c[0][0], c[0][1], c[0][2], c[1], c[2][0], c[2][1], c[3]) for c in CASES])
def test_paired_layer_equals_the_two_single_launches(layer, R, counts, prec):
    I1, I2, O, div, shared = layer
    R = R * div                                                    # rows of the launch: `div` rows share a row of the first source
    rng = np.random.default_rng(1000 * I1 + 10 * R + prec)
    A = Arena()
    groups = []
    for g, n in enumerate(counts):
        x1 = f32(rng.standard_normal((n, R // div, I1)))
        x1[:, 0] = 0                                               # (with b[:, 0] = 0 and single-source rows: an exact zero at the LeakyReLU's kink)
        w = f32(rng.standard_normal((n, I1 + I2, O)) * 0.2)
        b = f32(rng.standard_normal((n, O)) * 0.1)
        b[:, 0] = 0
        x2 = f32(rng.standard_normal(((R, I2) if shared else (n, R, I2)))) if I2 else None
        o = OFFS[(g + R) % 4]
        reg = dict(n=n, x1=A.place("x1_%d" % g, x1, offset_in_16=o), w=A.place("w_%d" % g, w, offset_in_16=OFFS[(g + 1) % 4]),
                   b=A.place("b_%d" % g, b, offset_in_16=OFFS[(g + 2) % 4]), x2=None if x2 is None else A.place("x2_%d" % g, x2, offset_in_16=OFFS[(g + 3) % 4]))
        if I2 and (I1 & 15):                                       # the single reference of these rows: one source, concatenated on the host
            assert div == 1 and not shared
            reg["cat"] = A.place("cat_%d" % g, np.concatenate([x1, x2], axis=-1), offset_in_16=o)
        for kind in ("ref", "ref_leaky", "pair", "pair_leaky"):
            reg[kind] = A.reserve("y_%s_%d" % (kind, g), (n, R, O), offset_in_16=OFFS[(g + len(kind)) % 4])
        groups.append(reg)
    a, b = groups
    p2 = lambda r: None if r["x2"] is None else r["x2"].ptr
    with precision(prec):
        for r in groups:
            if not I2:
                call("ssd_bias_bmm_fwd", r["x1"].ptr, r["w"].ptr, r["b"].ptr, r["ref"].ptr, r["n"], R, I1, O, None)
                call("ssd_bias_bmm_leaky_fwd", r["x1"].ptr, r["w"].ptr, r["b"].ptr, r["ref_leaky"].ptr, r["n"], R, I1, O, None)
            elif "cat" in r:
                call("ssd_bias_bmm_fwd", r["cat"].ptr, r["w"].ptr, r["b"].ptr, r["ref"].ptr, r["n"], R, I1 + I2, O, None)
                call("ssd_bias_bmm_leaky_fwd", r["cat"].ptr, r["w"].ptr, r["b"].ptr, r["ref_leaky"].ptr, r["n"], R, I1 + I2, O, None)
            else:
                call("ssd_bias_bmm2_fwd", r["x1"].ptr, r["x2"].ptr, r["w"].ptr, r["b"].ptr, r["ref"].ptr, r["n"], R, I1, I2, O, div, shared, None)
        for kind, lk in (("pair", 0), ("pair_leaky", 1)):
            call("ssd_bias_bmm_pair_fwd", a["x1"].ptr, p2(a), a["w"].ptr, a["b"].ptr, a[kind].ptr, a["n"], b["x1"].ptr, p2(b), b["w"].ptr, b["b"].ptr, b[kind].ptr,
                 b["n"], R, I1, I2, O, div, shared, lk, None)
    no_leaky_ref = bool(I2) and "cat" not in a                     # (the single two-source launch has no leaky form: its outputs keep the pre-fill)
    if no_leaky_ref:
        for r in groups:
            r["ref_leaky"].written = False
    A.check()
    for r in groups:
        ref = r["ref"].array()
        assert np.array_equal(r["pair"].array(), ref), (r["n"], float(np.abs(r["pair"].array() - ref).max()))
        leaky_ref = np.where(ref > 0, ref, np.float32(0.01) * ref) if no_leaky_ref else r["ref_leaky"].array()
        assert np.array_equal(r["pair_leaky"].array(), leaky_ref)
        assert (ref < 0).any() and not np.array_equal(leaky_ref, ref)                  # the two forms differ: the flag reached the kernel
    if prec == 2 and not I2:                                       # and the values are the layer's: f32 against float64 (the bound of test_learner_kernel_bounds.py)
        x, w, bias = (a[k].array().astype(np.float64) for k in ("x1", "w", "b"))
        pre = bias[:, None, :] + x @ w
        assert float(np.abs(a["pair"].array() - pre).max()) < 1e-5 * max(1.0, float(np.abs(pre).max()))


DUEL = [((5, 2, 1, 9), (5, 5)), ((3, 3, 5, 3), (2, 5)), ((1, 1, 1, 1), (1, 2)), ((4, 65, 2, 15), (5, 1)), ((2, 7, 3, 4), (2, 2))]


@pytest.mark.parametrize("dims,counts", DUEL, ids=["T%d_B%d_inner%d_K%d-n%d_%d" % (d + c) for d, c in DUEL])
def test_paired_dueling_combination_equals_the_two_single_launches(dims, counts):
    T, B, inner, K = dims
    rng = np.random.default_rng(T * 100 + K)
    A = Arena()
    groups = []
    for g, n in enumerate(counts):
        y = A.place("y_%d" % g, f32(rng.standard_normal((n, T * B * inner, K + 1))), offset_in_16=OFFS[g])
        groups.append((n, y, A.reserve("q_ref_%d" % g, (B, T, n, inner, K), offset_in_16=OFFS[g + 1]), A.reserve("q_pair_%d" % g, (B, T, n, inner, K), offset_in_16=OFFS[g + 2])))
    for n, y, ref, _ in groups:
        call("ssd_dueling_head_fwd", y.ptr, ref.ptr, n, T, B, inner, K, None)
    (na, ya, _, qa), (nb, yb, _, qb) = groups
    call("ssd_dueling_head_pair_fwd", ya.ptr, qa.ptr, na, yb.ptr, qb.ptr, nb, T, B, inner, K, None)
    A.check()
    for n, y, ref, got in groups:
        assert np.array_equal(got.array(), ref.array())
        v = y.array()
        want = (v[..., K:] + v[..., :K] - v[..., :K].mean(-1, keepdims=True)).reshape(n, T, B, inner, K).transpose(2, 1, 0, 3, 4)
        assert float(np.abs(got.array() - want).max()) < 1e-5


def _grads(outs, seeds, wrt):
    return th.autograd.grad(outs, wrt, grad_outputs=seeds)


@pytest.mark.parametrize("prec", [2, 1])
@pytest.mark.parametrize("n,n_t,R,I,O,leaky", [(5, 5, 33, 50, 64, True), (2, 5, 17, 64, 192, False), (5, 1, 1, 59, 64, True)])
def test_paired_function_returns_the_single_functions_outputs_and_gradients(n, n_t, R, I, O, leaky, prec):
    """ops.bias_bmm_pair against ops.bias_bmm of each net: both outputs, and dx / dw / db of the live operands (_BiasBmm's backward
    launch on the same operands), bit for bit; the second net's output carries no gradient."""
    g = th.Generator().manual_seed(R + I)
    mk = lambda *s: th.randn(*s, generator=g).cuda()
    x, w, b = mk(n, R, I).requires_grad_(), (mk(n, I, O) * 0.2).requires_grad_(), (mk(n, 1, O) * 0.1).requires_grad_()
    x_t, w_t, b_t, seed = mk(n_t, R, I), mk(n_t, I, O) * 0.2, mk(n_t, 1, O) * 0.1, mk(n, R, O)
    was = ops.STRICT
    ops.set_strict(True)
    try:
        with ops._precision(prec):
            y, y_t = ops.bias_bmm_pair(x, w, b, x_t, w_t, b_t, leaky=leaky)
            ref, ref_t = ops.bias_bmm(x, w, b, leaky=leaky), ops.bias_bmm(x_t, w_t, b_t, leaky=leaky)
        got, want = _grads([y], [seed], [x, w, b]), _grads([ref], [seed], [x, w, b])      # (outside the block: the forward's precision is recorded)
    finally:
        ops.set_strict(was)
    assert th.equal(y, ref) and th.equal(y_t, ref_t) and y.requires_grad and not y_t.requires_grad
    for a, c in zip(got, want):
        assert th.equal(a, c) and float(c.abs().max()) > 0


@pytest.mark.parametrize("prec", [2, 1])
@pytest.mark.parametrize("n,n_t,T,B,inner,K,E", [(5, 5, 5, 2, 1, 9, 0), (5, 5, 5, 2, 5, 3, 16), (2, 5, 3, 3, 2, 3, 15)])
def test_paired_dueling_head_returns_the_single_heads_outputs_and_gradients(n, n_t, T, B, inner, K, E, prec):
    g = th.Generator().manual_seed(T + K)
    mk = lambda *s: th.randn(*s, generator=g).cuda()
    H = 64
    h, w, b = mk(n, T * B, H).requires_grad_(), (mk(n, H + E, K + 1) * 0.2).requires_grad_(), (mk(n, 1, K + 1) * 0.1).requires_grad_()
    h_t, w_t, b_t = mk(n_t, T * B, H), mk(n_t, H + E, K + 1) * 0.2, mk(n_t, 1, K + 1) * 0.1
    other = mk(T * B, inner, E) if E else None
    was = ops.STRICT
    ops.set_strict(True)
    try:
        with ops._precision(prec):
            q, q_t = ops.dueling_head_pair(h, other, w, b, h_t, w_t, b_t, B, T, inner)
            ref, ref_t = ops.dueling_head(h, other, w, b, B, T, inner), ops.dueling_head(h_t, other, w_t, b_t, B, T, inner)
        seed = mk(*q.shape)
        got, want = _grads([q], [seed], [h, w, b]), _grads([ref], [seed], [h, w, b])
    finally:
        ops.set_strict(was)
    assert q.shape == ref.shape and th.equal(q, ref) and th.equal(q_t, ref_t) and not q_t.requires_grad
    for a, c in zip(got, want):
        assert th.equal(a, c) and float(c.abs().max()) > 0
