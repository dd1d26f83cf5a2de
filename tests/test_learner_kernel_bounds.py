"""Bounds tests of the learner's HIP kernels: every operand of a launch lives in a poisoned arena (tests/arena_util.py), the shapes are
swept around the kernels' own tile constants, and the results are compared with a plain float64 host reference.

What a case asserts: (1) no byte of a band, of the slack or of an INPUT changed; (2) every output element the contract writes was
written, none outside it; (3) no NaN in an output -- the bands around f32 operands are NaN, so an over-read that reaches the
arithmetic shows, also when it is "masked" by a multiplication with 0; (4) the values, within the tolerance the existing test of the
same kernel states (cited at each case) applied to the float64 reference, `==` for the bit-exact kernels.  The f32 matrix kernels run
a second time under ssd_set_learner_precision(1): same (1)-(3), values within the bound bf16 rounding of both operands gives,
|err| <= 2^-7 (|x| @ |w|) elementwise (unit round-off 2^-8 per operand, two operands; the rest is margin for the f32 accumulation).

Calls go through abi.load_library() with raw pointers; ops.py (whose th.empty outputs hide a stray store) is bypassed on purpose.
Operands sit at dword addresses that are NOT 16-byte aligned wherever the header allows it (offset_in_16 = 4 / 8 / 12).

Covered entry points: ssd_bias_bmm_fwd, ssd_bias_bmm_leaky_fwd, ssd_bias_bmm_bwd, ssd_bias_bmm_leaky_bwd, ssd_bias_bmm2_fwd,
ssd_bias_bmm2_bwd_w, ssd_bias_bmm_bwd_x, ssd_dueling_head_fwd, ssd_dueling_head_bwd, ssd_dueling_q_fwd, ssd_dueling_q_bwd, ssd_gru_gates,
ssd_gru_gates_fwd, ssd_gru_gates_bwd, ssd_column_sums, ssd_copy_blocks, ssd_fill_blocks, ssd_gather_rows, ssd_sample_ids,
ssd_runner_stats, ssd_unroll_other, ssd_incentive_transfer, ssd_conv_wgrad_codes (+ ssd_conv_wgrad_partial_rows), ssd_build_inputs,
ssd_build_inputs_flags, ssd_gru_seq_fwd, ssd_gru_seq_bwd, ssd_gru_seq_fwd_parts, ssd_gru_seq_bwd_parts, ssd_clip_adam_step, ssd_td_sim_loss
(bounds and the closed-form columns; its TD values stay with the tensor-op comparison of tests/test_hip_learner_path.py:233),
ssd_policy_encode (with `act`, `out` and `part`)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from homophily_marl_amd import abi
from tests.arena_util import Arena

pytestmark = pytest.mark.gpu



def _csrc_int(source, pattern):
    """an integer constant read from the kernel source, so that the sweeps follow the code's own tile sizes and grid caps"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(abi.__file__)), "csrc", source)).read()
    found = re.findall(pattern, text)
    assert found and len(set(found)) == 1, (source, pattern, found)
    return int(found[0])


BMM_TPW = _csrc_int("ssd_bmm.hip", r"constexpr int BMM_TPW = (\d+);")
BMM_BWD_WAVES = _csrc_int("ssd_bmm.hip", r"constexpr int BMM_BWD_WAVES = (\d+);")
CW_ROWS = _csrc_int("ssd_bmm.hip", r"constexpr int CW_ROWS = (\d+),")
GRID_CAP = _csrc_int("ssd_policy.hip", r"want > (\d+) \? \1 : \(int\)want")          # the gate launchers' workgroup cap
assert GRID_CAP == _csrc_int("ssd_learner.hip", r"b > (\d+) \? \1 : b\)")             # grid_for: the same cap in ssd_learner.hip
COPY_GX, GATHER_GX, FILL_GX = (_csrc_int("ssd_learner.hip", p) for p in (r"if \(gx > (\d+)\) gx = \1;\n    hipLaunchKernelGGL\(k_copy_blocks",
                                                                        r"if \(gx > (\d+)\) gx = \1;\n    hipLaunchKernelGGL\(k_gather_rows",
                                                                        r"if \(gx > (\d+)\) gx = \1;\n    hipLaunchKernelGGL\(k_fill_blocks"))
CHUNK_AT = 4 * 64 * BMM_BWD_WAVES - 3               # first row count with (R + 3) / 4 >= 64 * BMM_BWD_WAVES: the row-chunked dw
ROWS = [1, 15, 16, 17, 33, 255, 257]
INS = [1, 3, 4, 5, 15, 16, 17, 64, 73, 80]
OUTS = [1, 3, 4, 9, 15, 16, 17, 16 * BMM_TPW - 1, 16 * BMM_TPW, 16 * BMM_TPW + 1, 64, 192]
NS = [1, 2, 5, 10]
OFFS = [4, 8, 12, 0]


def _lib():
    return abi.load_library()


def call(name, *args):
    lib = _lib()
    abi.check(lib, getattr(lib, name)(*args))


def f32(a):
    return np.asarray(a, dtype=np.float32)


class bf16_products:
    """ssd_set_learner_precision(1) for the block, 2 restored in a finally"""

    def __enter__(self):
        call("ssd_set_learner_precision", 1)

    def __exit__(self, *exc):
        call("ssd_set_learner_precision", 2)


def close_f32(got, ref, rel, name):
    """|got - ref| < rel * max(1, max |ref|): the form of tests/test_hip_learner_path.py:715,717"""
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    assert err < rel * max(1.0, float(np.abs(ref).max())), (name, err)


def close_bf16(got, ref, bound, name):
    """elementwise |got - ref| <= 2^-7 * bound (bound = |x| @ |w| of the product) + 2^-22 |ref|.  The second term is the f32 form of
    the OUTPUT, which the product bound does not hold when the product is exactly 0 (the all-zero x row below: y = b, and the leaky
    layer's 0.01f * b is one f32 multiplication by a constant that is itself 0.01 rounded -- under 3 * 2^-24 |ref| in all)."""
    err = np.abs(got.astype(np.float64) - ref)
    lim = 2.0 ** -7 * bound + 2.0 ** -22 * np.abs(ref)
    assert (err <= lim).all(), (name, float((err - lim).max()))


def leaky(v):
    return np.where(v > 0, v, 0.01 * v)


# ---- ssd_bias_bmm_fwd / _leaky_fwd / _bwd / _leaky_bwd ------------------------------------------------------------------------------
def _bmm_shapes():
    """every (in, out) pair of the two lists (both XV and both OV paths, every tail of the 48-column wave); rows and n cycle through
    their lists so that every rows x in, rows x out, n x in, n x out pair value meets several partners; then the row-chunk threshold
    (one below, at, one above) with few dw tiles, and the encoder-backward uses (ops.py:707,710: one set, K = 6 (V - 2)^2)."""
    out = []
    for j, O in enumerate(OUTS):
        for i, I in enumerate(INS):
            out.append((NS[(i + 2 * j) % 4], ROWS[(i + j) % len(ROWS)], I, O))
    for R in (CHUNK_AT - 1, CHUNK_AT, CHUNK_AT + 1):
        out += [(3, R, 80, 3), (1, R, 16, 16), (5, R, 64, 9), (5, R, 5, 1)]
    return out


def _bmm_case(n, R, I, O, seed, bf, variants):
    rng = np.random.default_rng(seed)
    x, w, b, g = f32(rng.standard_normal((n, R, I))), f32(rng.standard_normal((n, I, O)) * 0.2), f32(rng.standard_normal((n, O)) * 0.1), f32(rng.standard_normal((n, R, O)))
    x[:, 0] = 0; b[:, 0] = 0                                     # an exact zero pre-activation (test_hip_learner_path.py:730)
    X, W, Bv, G = (t.astype(np.float64) for t in (x, w, b, g))
    pre = Bv[:, None, :] + X @ W
    aX, aW, aG = np.abs(X), np.abs(W), np.abs(G)
    o = OFFS[seed % 4]
    if "fwd" in variants:
        A = Arena()
        px, pw, pb = A.place("x", x, offset_in_16=o), A.place("w", w, offset_in_16=OFFS[(seed + 1) % 4]), A.place("b", b, offset_in_16=OFFS[(seed + 2) % 4])
        y, yl = A.reserve("y", (n, R, O), offset_in_16=OFFS[(seed + 3) % 4]), A.reserve("y_leaky", (n, R, O), offset_in_16=o)
        call("ssd_bias_bmm_fwd", px.ptr, pw.ptr, pb.ptr, y.ptr, n, R, I, O, None)
        call("ssd_bias_bmm_leaky_fwd", px.ptr, pw.ptr, pb.ptr, yl.ptr, n, R, I, O, None)
        A.check()
        for got, ref, nm in ((y.array(), pre, "y"), (yl.array(), leaky(pre), "y_leaky")):
            if bf:
                close_bf16(got, ref, aX @ aW, nm)
            else:
                close_f32(got, ref, 1e-5, nm)                    # test_hip_learner_path.py:715,741
    if "bwd" in variants:
        yf = f32(leaky(pre))                                     # the leaky layer's output as the forward leaves it (its sign is the slope)
        sl = np.where(x > 0, 1.0, 0.01)                          # slope_of = x itself: LeakyReLU'(.) from the sign of slope_of
        gs = G * np.where(yf > 0, 1.0, 0.01)
        Wt = np.swapaxes(W, 1, 2)
        A = Arena()
        pg, py = A.place("g", g, offset_in_16=o), A.place("y", yf, offset_in_16=OFFS[(seed + 1) % 4])
        px, pw = A.place("x", x, offset_in_16=OFFS[(seed + 2) % 4]), A.place("w", w, offset_in_16=OFFS[(seed + 3) % 4])
        r = lambda nm, shape, k: A.reserve(nm, shape, offset_in_16=OFFS[(seed + k) % 4])
        dx1, dw1, db1 = r("dx(all, slope_of)", (n, R, I), 1), r("dw(all)", (n, I, O), 2), r("db(all)", (n, O), 3)
        dx2 = r("dx(alone)", (n, R, I), 2)
        dw3, db3 = r("dw(dw db)", (n, I, O), 3), r("db(dw db)", (n, O), 0)
        dw4 = r("dw(alone)", (n, I, O), 1)
        dx5, dw5, db5 = r("dx(leaky)", (n, R, I), 3), r("dw(leaky)", (n, I, O), 0), r("db(leaky)", (n, O), 1)
        call("ssd_bias_bmm_bwd", pg.ptr, px.ptr, pw.ptr, dx1.ptr, dw1.ptr, db1.ptr, px.ptr, n, R, I, O, None)
        call("ssd_bias_bmm_bwd", pg.ptr, None, pw.ptr, dx2.ptr, None, None, None, n, R, I, O, None)         # (x null: the encoder's d_act form)
        call("ssd_bias_bmm_bwd", pg.ptr, px.ptr, None, None, dw3.ptr, db3.ptr, None, n, R, I, O, None)
        call("ssd_bias_bmm_bwd", pg.ptr, px.ptr, None, None, dw4.ptr, None, None, n, R, I, O, None)         # (w null: the encoder's d_lin_w form)
        call("ssd_bias_bmm_leaky_bwd", pg.ptr, py.ptr, px.ptr, pw.ptr, dx5.ptr, dw5.ptr, db5.ptr, None, n, R, I, O, None)
        A.check()
        Xt = np.swapaxes(X, 1, 2)
        refs = [(dx1, (G @ Wt) * sl, (aG @ np.swapaxes(aW, 1, 2)) * sl), (dw1, Xt @ G, np.swapaxes(aX, 1, 2) @ aG), (db1, G.sum(1), aG.sum(1)),
                (dx2, G @ Wt, aG @ np.swapaxes(aW, 1, 2)), (dw3, Xt @ G, np.swapaxes(aX, 1, 2) @ aG), (db3, G.sum(1), aG.sum(1)),
                (dw4, Xt @ G, np.swapaxes(aX, 1, 2) @ aG),
                (dx5, gs @ Wt, np.abs(gs) @ np.swapaxes(aW, 1, 2)), (dw5, Xt @ gs, np.swapaxes(aX, 1, 2) @ np.abs(gs)), (db5, gs.sum(1), np.abs(gs).sum(1))]
        for reg, ref, bound in refs:
            if bf:
                close_bf16(reg.array(), ref, bound, reg.name)
            else:
                close_f32(reg.array(), ref, 2e-5, reg.name)      # test_hip_learner_path.py:717,743


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,R,I,O", _bmm_shapes())
def test_bias_bmm_forward_and_backward_in_the_arena(n, R, I, O, bf):
    if bf:
        with bf16_products():
            _bmm_case(n, R, I, O, R + I + O, True, ("fwd", "bwd"))
    else:
        _bmm_case(n, R, I, O, R + I + O, False, ("fwd", "bwd"))


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [3, 15, 31])
@pytest.mark.parametrize("R", [5, 203])
def test_bias_bmm_bwd_in_the_encoder_backward_forms(R, V, bf):
    """ops.py:707 (dw alone: rows = R, in = 32, out = K, x = act role swapped: g = act [R, K]... as called: g = act, x = g2) and :710
    (dx alone with slope_of, in = K, out = 32), one weight set, K = 6 (V - 2)^2 -- up to 5046 columns."""
    K = 6 * (V - 2) ** 2
    rng = np.random.default_rng(R + V)
    act, g2, lwt = f32(rng.standard_normal((1, R, K))), f32(rng.standard_normal((1, R, 32))), f32(rng.standard_normal((1, K, 32)) * 0.05)
    A = Arena()
    pa, pg, pl = A.place("act", act, offset_in_16=4), A.place("g2", g2, offset_in_16=8), A.place("lin_w^T", lwt, offset_in_16=12)
    dlw, dact = A.reserve("d_lin_w", (1, 32, K), offset_in_16=4), A.reserve("d_act", (1, R, K), offset_in_16=12)

    def run():
        call("ssd_bias_bmm_bwd", pa.ptr, pg.ptr, None, None, dlw.ptr, None, None, 1, R, 32, K, None)
        call("ssd_bias_bmm_bwd", pg.ptr, None, pl.ptr, dact.ptr, None, None, pa.ptr, 1, R, K, 32, None)
    if bf:
        with bf16_products():
            run()
    else:
        run()
    A.check()
    Ad, Gd, Ld = act.astype(np.float64), g2.astype(np.float64), lwt.astype(np.float64)
    sl = np.where(act > 0, 1.0, 0.01)
    for reg, ref, bound in ((dlw, np.swapaxes(Gd, 1, 2) @ Ad, np.swapaxes(np.abs(Gd), 1, 2) @ np.abs(Ad)),
                            (dact, (Gd @ np.swapaxes(Ld, 1, 2)) * sl, (np.abs(Gd) @ np.swapaxes(np.abs(Ld), 1, 2)) * sl)):
        if bf:
            close_bf16(reg.array(), ref, bound, reg.name)
        else:
            close_f32(reg.array(), ref, 2e-5, reg.name)          # test_hip_learner_path.py:717


# ---- ssd_bias_bmm2_fwd / ssd_bias_bmm2_bwd_w / ssd_bias_bmm_bwd_x ----------------------------------------------------------------------
def _bmm2_shapes():
    out, k = [], 0
    for I1 in (16, 64):
        for I2 in (1, 3, 4, 15, 16):
            for div in (1, 2, 5, 10):
                out.append((NS[k % 4], div * (1, 7, 33, 26)[k % 4], I1, I2, (4, 10, 16, 17)[(k // 2) % 4], div, k % 2))
                k += 1
    return out + [(3, 10 * 410, 64, 16, 4, 10, 1), (1, CHUNK_AT + 2, 16, 3, 4, 5, 0)]        # the row-chunked dw with two-source rows


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,R,I1,I2,O,div,shared", _bmm2_shapes())
def test_two_source_layer_in_the_arena(n, R, I1, I2, O, div, shared, bf):
    """y = b + [x1[r / x1_div] | x2[r]] w, its dw / db, and dx1 = g w[:in1]^T with w_set = (in1 + in2) out > in1 out."""
    rng = np.random.default_rng(R + I1 + I2 + O)
    I = I1 + I2
    x1, x2 = f32(rng.standard_normal((n, R // div, I1)) * 0.5), f32(rng.standard_normal((R, I2) if shared else (n, R, I2)))
    w, b, g = f32(rng.standard_normal((n, I, O)) * 0.2), f32(rng.standard_normal((n, O)) * 0.2), f32(rng.standard_normal((n, R, O)))
    gsum = f32(rng.standard_normal((n, R // div, O)))
    A = Arena()
    p1, p2, pw, pb = A.place("x1", x1, offset_in_16=4), A.place("x2", x2, offset_in_16=12), A.place("w", w, offset_in_16=8), A.place("b", b, offset_in_16=4)
    pg, pgs = A.place("g", g, offset_in_16=12), A.place("gs", gsum, offset_in_16=8)
    y, dw, db = A.reserve("y", (n, R, O), offset_in_16=4), A.reserve("dw", (n, I, O), offset_in_16=8), A.reserve("db", (n, O), offset_in_16=12)
    dw2, db2 = A.reserve("dw(alone)", (n, I, O), offset_in_16=4), A.reserve("db(alone)", (n, O), offset_in_16=8)
    dx1 = A.reserve("dx1", (n, R // div, I1), offset_in_16=12)

    def run():
        call("ssd_bias_bmm2_fwd", p1.ptr, p2.ptr, pw.ptr, pb.ptr, y.ptr, n, R, I1, I2, O, div, shared, None)
        call("ssd_bias_bmm2_bwd_w", pg.ptr, p1.ptr, p2.ptr, dw.ptr, db.ptr, n, R, I1, I2, O, div, shared, None)
        call("ssd_bias_bmm2_bwd_w", pg.ptr, p1.ptr, p2.ptr, dw2.ptr, None, n, R, I1, I2, O, div, shared, None)
        call("ssd_bias_bmm2_bwd_w", pg.ptr, p1.ptr, p2.ptr, None, db2.ptr, n, R, I1, I2, O, div, shared, None)
        call("ssd_bias_bmm_bwd_x", pgs.ptr, pw.ptr, dx1.ptr, n, R // div, I1, O, I * O, None)
    if bf:
        with bf16_products():
            run()
    else:
        run()
    A.check()
    X = np.concatenate([np.repeat(x1.astype(np.float64), div, axis=1), np.broadcast_to(x2.astype(np.float64), (n, R, I2))], axis=2)
    W, G, GS = w.astype(np.float64), g.astype(np.float64), gsum.astype(np.float64)
    Xt, W1t = np.swapaxes(X, 1, 2), np.swapaxes(W[:, :I1], 1, 2)
    refs = [(y, b.astype(np.float64)[:, None] + X @ W, np.abs(X) @ np.abs(W), 1e-5), (dw, Xt @ G, np.abs(Xt) @ np.abs(G), 2e-5), (db, G.sum(1), np.abs(G).sum(1), 2e-5),
            (dw2, Xt @ G, np.abs(Xt) @ np.abs(G), 2e-5), (db2, G.sum(1), np.abs(G).sum(1), 2e-5), (dx1, GS @ W1t, np.abs(GS) @ np.abs(W1t), 2e-5)]
    for reg, ref, bound, rel in refs:
        if bf:
            close_bf16(reg.array(), ref, bound, reg.name)
        else:
            close_f32(reg.array(), ref, rel, reg.name)           # test_hip_learner_path.py:715,717 (the same kernels)


# ---- ssd_dueling_head_fwd / _bwd, ssd_dueling_q_fwd / _bwd -----------------------------------------------------------------------------
def _dueling_shapes(kmax):
    tb = [(1, 1), (3, 5), (7, 37), (2, 129)]
    return [(NS[1:][k % 3] if k % 4 else 1, tb[k % 4][0], tb[(k + k // 4) % 4][1], (1, 2, 5, 10)[(k + k // 3) % 4], k) for k in range(1, kmax + 1)]


def _q_layout(a_rows, n, T, B, inner, K):
    """[n, T * B * inner, K] rows r = (t B + b) inner + j  ->  [B, T, n, inner, K]"""
    return a_rows.reshape(n, T, B, inner, K).transpose(2, 1, 0, 3, 4)


@pytest.mark.parametrize("n,T,B,inner,K", _dueling_shapes(15))
def test_dueling_head_in_the_arena(n, T, B, inner, K):
    rng = np.random.default_rng(n + T + B + inner + K)
    rows = T * B * inner
    yv, dq = f32(rng.standard_normal((n, rows, K + 1))), f32(rng.standard_normal((B, T, n, inner, K)))
    A = Arena()
    py, pdq = A.place("y", yv, offset_in_16=4), A.place("dq", dq, offset_in_16=12)
    q, dy, dy2, gs = A.reserve("q", (B, T, n, inner, K), offset_in_16=8), A.reserve("dy", (n, rows, K + 1), offset_in_16=4), \
        A.reserve("dy(with gs)", (n, rows, K + 1), offset_in_16=12), A.reserve("gs", (n, T * B, K + 1), offset_in_16=8)
    call("ssd_dueling_head_fwd", py.ptr, q.ptr, n, T, B, inner, K, None)
    call("ssd_dueling_head_bwd", pdq.ptr, dy.ptr, None, n, T, B, inner, K, None)
    call("ssd_dueling_head_bwd", pdq.ptr, dy2.ptr, gs.ptr, n, T, B, inner, K, None)
    A.check()
    Y, DQ = yv.astype(np.float64), dq.astype(np.float64)
    a, v = Y[..., :K], Y[..., K:]
    assert np.abs(q.array() - _q_layout(v + a - a.mean(-1, keepdims=True), n, T, B, inner, K)).max() < 2e-6      # test_hip_learner_path.py:788
    dqr = DQ.transpose(2, 1, 0, 3, 4).reshape(n, rows, K)
    ref = np.concatenate([dqr - dqr.mean(-1, keepdims=True), dqr.sum(-1, keepdims=True)], axis=-1)
    close_f32(dy.array(), ref, 2e-5, "dy")                       # test_hip_learner_path.py:792
    assert np.array_equal(dy.array(), dy2.array())
    close_f32(gs.array(), ref.reshape(n, T * B, inner, K + 1).sum(2), 2e-5, "gs")


@pytest.mark.parametrize("n,T,B,inner,K", _dueling_shapes(16))
def test_dueling_q_in_the_arena(n, T, B, inner, K):
    rng = np.random.default_rng(n + T + B + inner + K)
    rows = T * B * inner
    a, v, dq = f32(rng.standard_normal((n, rows, K))), f32(rng.standard_normal((n, rows, 1))), f32(rng.standard_normal((B, T, n, inner, K)))
    A = Arena()
    pa, pv, pdq = A.place("a", a, offset_in_16=4), A.place("v", v, offset_in_16=8), A.place("dq", dq, offset_in_16=12)
    q, da, dv = A.reserve("q", (B, T, n, inner, K), offset_in_16=12), A.reserve("da", (n, rows, K), offset_in_16=4), A.reserve("dv", (n, rows, 1), offset_in_16=8)
    call("ssd_dueling_q_fwd", pa.ptr, pv.ptr, q.ptr, n, T, B, inner, K, None)
    call("ssd_dueling_q_bwd", pdq.ptr, da.ptr, dv.ptr, n, T, B, inner, K, None)
    A.check()
    a64, v64 = a.astype(np.float64), v.astype(np.float64)
    dqr = dq.astype(np.float64).transpose(2, 1, 0, 3, 4).reshape(n, rows, K)
    assert np.abs(q.array() - _q_layout(v64 + a64 - a64.mean(-1, keepdims=True), n, T, B, inner, K)).max() < 1e-6      # test_hip_learner_path.py:1098
    assert np.abs(da.array() - (dqr - dqr.mean(-1, keepdims=True))).max() < 2e-6                                        # test_hip_learner_path.py:1103
    assert np.abs(dv.array() - dqr.sum(-1, keepdims=True)).max() < 2e-6


# ---- ssd_gru_gates / _fwd / _bwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,H", [(1, 64), (255, 64), (257, 64), (GRID_CAP * 256 // 64 + 1, 64), (1, 1), (257, 1), (85, 3), (17, 65), (GRID_CAP * 256 // 65 + 1, 65)])
def test_gru_gate_kernels_in_the_arena(R, H):
    """any rows >= 1 and any hidden >= 1 (the header says so): hidden 64 and 1, 3, 65; rows past the grid cap of 4096 workgroups."""
    rng = np.random.default_rng(R + H)
    gi, gh, h, dh = (f32(rng.standard_normal(s)) for s in ((R, 3 * H), (R, 3 * H), (R, H), (R, H)))
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    GI, GHd, Hd, DH = (t.astype(np.float64) for t in (gi, gh, h, dh))
    r, z = sig(GI[:, :H] + GHd[:, :H]), sig(GI[:, H:2 * H] + GHd[:, H:2 * H])
    c = np.tanh(GI[:, 2 * H:] + r * GHd[:, 2 * H:])
    hn = (1 - z) * c + z * Hd
    A = Arena()
    pgi, pgh, ph = A.place("gi", gi, offset_in_16=4), A.place("gh", gh, offset_in_16=8), A.place("h", h, offset_in_16=12)
    hin = A.place("h(in place)", h, offset_in_16=4, inout=True)
    hnew, rzn = A.reserve("h_new", (R, H), offset_in_16=8), A.reserve("rzn", (R, 3 * H), offset_in_16=12)
    call("ssd_gru_gates_fwd", pgi.ptr, pgh.ptr, ph.ptr, hnew.ptr, rzn.ptr, R, H, None)
    call("ssd_gru_gates", pgi.ptr, pgh.ptr, hin.ptr, R, H, None)
    A.check()
    tol = 2e-6                                                   # test_hip_learner_path.py:662
    assert np.abs(hnew.array() - hn).max() < tol and np.abs(rzn.array() - np.concatenate([r, z, c], 1)).max() < tol
    assert np.abs(hin.array() - hn).max() < tol
    saved = rzn.array()
    A = Arena()
    pdh, prz, pgh, ph = A.place("dh", dh, offset_in_16=12), A.place("rzn", saved, offset_in_16=4), A.place("gh", gh, offset_in_16=8), A.place("h", h, offset_in_16=4)
    dgi, dgh, dhp = A.reserve("d_gi", (R, 3 * H), offset_in_16=8), A.reserve("d_gh", (R, 3 * H), offset_in_16=12), A.reserve("dh_prev", (R, H), offset_in_16=4)
    call("ssd_gru_gates_bwd", pdh.ptr, prz.ptr, pgh.ptr, ph.ptr, dgi.ptr, dgh.ptr, dhp.ptr, R, H, None)
    A.check()
    S = saved.astype(np.float64)
    rs, zs, ns = S[:, :H], S[:, H:2 * H], S[:, 2 * H:]
    d_n = DH * (1 - zs) * (1 - ns * ns); d_z = DH * (Hd - ns) * zs * (1 - zs); d_r = d_n * GHd[:, 2 * H:] * rs * (1 - rs)
    assert np.abs(dgi.array() - np.concatenate([d_r, d_z, d_n], 1)).max() < tol
    assert np.abs(dgh.array() - np.concatenate([d_r, d_z, d_n * rs], 1)).max() < tol
    assert np.abs(dhp.array() - DH * zs).max() < tol


# ---- ssd_column_sums ---------------------------------------------------------------------------------------------------------------
def _colsum_shapes():
    ch = abi.COLSUM_CHUNK
    rows, cols, out = [1, ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch + 1, 8080], [1, 3, 63, 64, 65, 1014], []
    for i, R in enumerate(rows):
        for j, Cc in enumerate(cols):
            G = 5 if (i + j) % 2 and R * Cc * 5 * 4 <= (12 << 20) else 1
            out.append((G, R, Cc, (i + j // 2) % 2))
    return out + [(5, 8080, 3, 1), (5, 8080, 65, 0), (5, 1, 1014, 1), (1, 8080, 1014, 0)]


@pytest.mark.parametrize("G,R,Cc,ws", _colsum_shapes())
def test_column_sums_in_the_arena(G, R, Cc, ws):
    rng = np.random.default_rng(G + R + Cc)
    x = f32(rng.standard_normal((G, R, Cc)))
    chunks = (R + abi.COLSUM_CHUNK - 1) // abi.COLSUM_CHUNK
    A = Arena()
    px, out = A.place("x", x, offset_in_16=4), A.reserve("out", (G, Cc), offset_in_16=12)
    work = A.reserve("workspace", (G, chunks, Cc), offset_in_16=8, written=chunks > 1) if ws else None
    call("ssd_column_sums", px.ptr, out.ptr, G, R, Cc, work.ptr if ws else None, None)
    A.check()
    ref = x.astype(np.float64).sum(1)
    close_f32(out.array(), ref, 1e-5, "out")                     # test_hip_learner_path.py:849
    if ws and chunks > 1:
        pad = np.zeros((G, chunks * abi.COLSUM_CHUNK, Cc)); pad[:, :R] = x
        close_f32(work.array(), pad.reshape(G, chunks, abi.COLSUM_CHUNK, Cc).sum(2), 1e-5, "workspace")


# ---- ssd_copy_blocks / ssd_fill_blocks / ssd_gather_rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, abi.COPY_BLOCKS_MAX])
def test_copy_blocks_in_the_arena(count):
    """strided blocks, cols 1 / 3 / 4 / 5 with stride > cols: the gaps between a destination's rows are bands too (written = False
    there); one block larger than a grid sweep of 64 x 256 x 4 elements; bit-exact."""
    rng = np.random.default_rng(count)
    A, blocks, expect = Arena(), [], []
    for k in range(count):
        cols = (1, 3, 4, 5)[k % 4]
        rows, ss, ds = ((COPY_GX * 256 * 4 + 4464, cols + 1, cols + 2) if k == 0 else ((1, 2, 17, 300)[(k // 4) % 4], cols + k % 3, cols + (k + 1) % 3))
        if count > 1 and k < 3 and k:
            ss = ds = cols                                        # dense blocks as well
        src = f32(rng.standard_normal((rows, ss)))
        w = np.zeros((rows, ds), dtype=bool); w[:, :cols] = True
        ps = A.place("src%d" % k, src, offset_in_16=OFFS[k % 4])
        pd = A.reserve("dst%d" % k, (rows, ds), offset_in_16=OFFS[(k + 1) % 4], written=w)
        blocks.append((ps, pd, rows, cols, ss, ds)); expect.append((pd, src[:, :cols], cols))
    table = (abi.SsdBlockCopy * count)(*[abi.SsdBlockCopy(ps.ptr, pd.ptr, *rest) for ps, pd, *rest in blocks])
    call("ssd_copy_blocks", table, count, None)
    A.check()
    for pd, ref, cols in expect:
        assert np.array_equal(pd.array()[:, :cols], ref), pd.name


@pytest.mark.parametrize("count", [1, abi.FILL_BLOCKS_MAX])
def test_fill_blocks_in_the_arena(count):
    """fills of 4 bytes, of an i64 -1 pattern, of odd word counts and one past a grid sweep (256 x 256 words); neighbours are bands."""
    A, blocks, regs = Arena(), [], []
    sizes = [4, 8 * 5, 4 * 3, 4 * (FILL_GX * 256 * 4 + 3), 4 * 255, 4 * 257, 4 * 1025, 8]
    for k in range(count):
        nb, val = sizes[k % len(sizes)], (0xFFFFFFFF if k % 2 else (0, 0x3F800000)[k % 4 // 2])
        reg = A.reserve("block%d" % k, (nb // 4,), dtype=np.uint32, offset_in_16=OFFS[k % 4], fill=0x5A5A5A5A)
        blocks.append((reg, nb, val)); regs.append((reg, val))
    call("ssd_fill_blocks", (abi.SsdBlockFill * count)(*[abi.SsdBlockFill(reg.ptr, nb, val, 0) for reg, nb, val in blocks]), count, None)
    A.check()
    for reg, val in regs:
        assert (reg.array() == val).all(), reg.name
    if count > 1:
        assert (regs[1][0].array().view(np.int64) == -1).all()      # the i64 -1 the runner opens an episode with


@pytest.mark.parametrize("count,n_ids", [(1, 1), (abi.COPY_BLOCKS_MAX, 5), (6, 16)])
def test_gather_rows_in_the_arena(count, n_ids):
    """row_bytes 1, 3, 4, 5, 17 and 131072 + 4 (longer than one sweep of the 32 x 256 x 4-byte grid: the kernel strides); sources and
    destinations at odd byte addresses; the ids are surrounded by a VALID id (the destination bands catch an over-read)."""
    rng = np.random.default_rng(count + n_ids)
    rb = [1, 3, 4, 5, 17, GATHER_GX * 256 * 4 * 4 + 4]
    src_rows = 9
    ids = rng.integers(0, src_rows, n_ids).astype(np.int64)
    A = Arena()
    pid = A.place("ids", ids, align=8, fill=0)
    fields, regs = [], []
    for k in range(count):
        nb = rb[k % len(rb)] if (k < len(rb) or count <= len(rb)) else rb[k % 5]
        src = rng.integers(0, 256, (src_rows, nb)).astype(np.uint8)
        ps = A.place("src%d" % k, src, align=1, fill=0xFF)
        pd = A.reserve("dst%d" % k, (n_ids, nb), dtype=np.uint8, align=1, written=None)       # u8: a byte may equal the pre-fill; compared with == below
        fields.append((ps, pd, nb)); regs.append((pd, src))
    call("ssd_gather_rows", (abi.SsdRowGather * count)(*[abi.SsdRowGather(ps.ptr, pd.ptr, nb) for ps, pd, nb in fields]), count, pid.ptr, n_ids, None)
    A.check()
    for pd, src in regs:
        assert np.array_equal(pd.array(), src[ids]), pd.name


# ---- ssd_sample_ids / ssd_runner_stats -----------------------------------------------------------------------------------------------
# (with the register-slot edges of the wave kernel: 64 / 128 / 256 picks and one past each)
SAMPLE_IDS_CASES = [(1, 1), (1, 7), (2, 2), (2, 4096), (16, 8192), (64, 64), (65, 70), (128, 128), (129, 4096), (256, 256), (257, 300),
                    (abi.SAMPLE_IDS_MAX, abi.SAMPLE_IDS_MAX), (abi.SAMPLE_IDS_MAX, 5000)]      # (count, population)


@pytest.mark.parametrize("count,population", SAMPLE_IDS_CASES)
def test_sample_ids_in_the_arena(count, population):
    """the expected ids come from ops.sample_ids on a HOST tensor: that branch is a pure-Python restatement of the generator and of
    Floyd's sampling (no library call), i.e. a second implementation, not the kernel; distinctness and range are asserted on their own."""
    import torch as th
    from homophily_marl_amd import ops
    A = Arena()
    ids = A.reserve("ids", (count,), dtype=np.int64, align=8)
    call("ssd_sample_ids", 0x123456789ABCDEF, 11, population, count, ids.ptr, None)
    A.check()
    ref = ops.sample_ids(0x123456789ABCDEF, 11, population, count, th.zeros(count, dtype=th.long)).numpy()
    got = ids.array()
    assert np.array_equal(got, ref) and len(set(got.tolist())) == count and got.min() >= 0 and got.max() < population


@pytest.mark.parametrize("n_env", [1, 255, 4097])
def test_runner_stats_in_the_arena(n_env):
    rng = np.random.default_rng(n_env)
    coll, eq, ret = f32(rng.standard_normal(n_env) * 30), f32(rng.random(n_env)), f32(rng.standard_normal(n_env * 5) * 8)
    acc0 = np.array([1.0, 2.0, 3.0, 4.0])
    A = Arena()
    pc, pe, pr = A.place("collective_return", coll, offset_in_16=4), A.place("equality", eq, offset_in_16=12), A.place("episode_return", ret, offset_in_16=8)
    acc = A.place("acc", acc0, align=8, fill=float("nan"), inout=True)
    call("ssd_runner_stats", pc.ptr, pe.ptr, pr.ptr, n_env, n_env * 5, acc.ptr, None)
    A.check()
    r = ret.astype(np.float64)
    ref = acc0 + np.array([coll.astype(np.float64).sum(), eq.astype(np.float64).sum(), r.sum(), (r * r).sum()])
    assert np.abs(acc.array() - ref).max() < 1e-9 * np.abs(ref).max()          # test_hip_learner_path.py:815


# ---- ssd_unroll_other / ssd_incentive_transfer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,n,Aa", [(1, 1, 2, 8), (3, 17, 5, 9), (5, 5, 10, 9), (2, 64, 2, 8), (16, 8, 2, 9), (3, 7, 12, 3)])
def test_unroll_other_in_the_arena(B, T, n, Aa):
    """B T n ragged against the 256-thread workgroup (and exactly 256 / 250 / 2), n_actions 8 / 9, actions of -1 (an all-zero
    one-hot), a team of 12; the actions' bands hold n_actions (outside the domain, harmless as an index); bit-exact."""
    rng = np.random.default_rng(B + T + n)
    acts = rng.integers(-1, Aa, (B, T, n)).astype(np.int64)
    pos, ori = f32(rng.integers(0, 25, (B, T, n, 2))), f32(rng.integers(-1, 2, (B, T, n, 2)))
    rew, cln, den = (f32(rng.random((B, T, n))) for _ in range(3))
    scale = np.float32(30.805843601498726)
    A = Arena()
    pa = A.place("actions", acts, align=8, fill=Aa)
    pp, po, pr, pc, pdn = (A.place(nm, t, offset_in_16=OFFS[k % 4]) for k, (nm, t) in enumerate((("pos", pos), ("orient", ori), ("reward", rew), ("clean_num", cln), ("apple_den", den))))
    other, act_tm = A.reserve("other", (T * B, n, Aa + 7), offset_in_16=4), A.reserve("act_tm", (n, T * B, Aa), offset_in_16=12)
    call("ssd_unroll_other", pa.ptr, pp.ptr, po.ptr, pr.ptr, pc.ptr, pdn.ptr, float(scale), B, T, n, Aa, other.ptr, act_tm.ptr, None)
    A.check()
    onehot = (acts[..., None] == np.arange(Aa)).astype(np.float32)
    ref = np.concatenate([onehot, pos / scale, ori, rew[..., None], cln[..., None], den[..., None]], axis=-1)      # f32 division, as the kernel
    assert np.array_equal(other.array(), ref.transpose(1, 0, 2, 3).reshape(T * B, n, Aa + 7))                      # test_hip_learner_path.py:764 (th.equal)
    assert np.array_equal(act_tm.array(), onehot.transpose(2, 1, 0, 3).reshape(n, T * B, Aa))


@pytest.mark.parametrize("B,T,n", [(1, 2, 2), (3, 17, 5), (5, 5, 10), (64, 2, 2), (6500, 81, 2)])
def test_incentive_transfer_in_the_arena(B, T, n):
    """B T n below, at and ragged against 256, and past the grid cap (4096 x 256 threads: the kernel strides); incentive actions'
    bands hold 3 (outside 0 .. 2)."""
    rng = np.random.default_rng(B + T + n)
    ainc = rng.integers(0, 3, (B, T, n, n)).astype(np.int64)
    rew = f32(rng.standard_normal((B, T - 1, n)))
    eff, cost, inc, seq = np.float32(1.5), np.float32(0.5), np.float32(2.0), np.float32(T)
    A = Arena()
    pa, pr = A.place("actions_inc", ainc, align=8, fill=3), A.place("rewards", rew, offset_in_16=4)
    give, renv, rinc = (A.reserve(nm, (B, T - 1, n), offset_in_16=o) for nm, o in (("give", 8), ("rewards_for_env", 12), ("rewards_for_inc", 4)))
    rp, rn, rz = (A.reserve(nm, (B, T, n), offset_in_16=o) for nm, o in (("recv_pos", 12), ("recv_neg", 8), ("recv_zero", 4)))
    call("ssd_incentive_transfer", B, T, n, pa.ptr, pr.ptr, float(eff), float(cost), float(inc), float(seq), give.ptr, rp.ptr, rn.ptr, rz.ptr, renv.ptr, rinc.ptr, None)
    A.check()
    off = ~np.eye(n, dtype=bool)
    g = ((ainc != 0) & off).sum(3).astype(np.float32)                                   # giver i over receivers j
    p, m = ((ainc == 1) & off).sum(2).astype(np.float32), ((ainc == 2) & off).sum(2).astype(np.float32)      # receiver i over givers j
    assert np.array_equal(rp.array(), p) and np.array_equal(rn.array(), m) and np.array_equal(rz.array(), n - 1 - p - m)
    assert np.array_equal(give.array(), g[:, :-1])
    # f32 arithmetic in the kernel's order ((r + k e i) / s): small integers times exact constants, so == up to the final division
    env = (rew + (p - m)[:, :-1] * eff * inc) / seq
    incr = (rew - g[:, :-1] * cost * inc) / seq
    assert np.array_equal(renv.array(), env.astype(np.float32)) and np.array_equal(rinc.array(), incr.astype(np.float32))


# ---- ssd_conv_wgrad_codes (+ ssd_conv_wgrad_partial_rows) -----------------------------------------------------------------------------
CONV_WGRAD_CASES = [(1, 3), (3, 5), (4, 15), (5, 17), (203, 31), (5, 63), (203, 3), (1, 63), (3, 31), (4, 5), (5, 15), (203, 17)]      # (R, V)


@pytest.mark.parametrize("R,V", CONV_WGRAD_CASES)
def test_conv_wgrad_codes_in_the_arena(R, V):
    """rows around CW_ROWS = 4 windows per wave and 203; V = 3 .. 63; `partial` has exactly ssd_conv_wgrad_partial_rows(R) rows -- the
    row behind it is a band; the class codes' bands hold 0xFF (no class)."""
    lib = _lib()
    P = lib.ssd_conv_wgrad_partial_rows(R)
    assert P == ((R + CW_ROWS - 1) // CW_ROWS + 3) // 4 * 4
    O = V - 2
    rng = np.random.default_rng(R + V)
    codes, dconv = rng.integers(0, 4, (R, V, V)).astype(np.uint8), f32(rng.standard_normal((R, 6, O, O)))
    A = Arena()
    pc, pd = A.place("codes", codes, align=1, fill=0xFF, row_bytes=V * V), A.place("d_conv", dconv, offset_in_16=4, row_bytes=6 * O * O * 4)
    part = A.reserve("partial", (P, 168), offset_in_16=12)
    call("ssd_conv_wgrad_codes", pc.ptr, pd.ptr, part.ptr, R, V, None)
    A.check()
    D = dconv.astype(np.float64)
    ref = np.zeros((6, 3, 3, 3))
    for ch, cls in enumerate((2, 1, 3)):                       # waste -> R, apple -> G, wall / agent -> B
        lit = (codes == cls).astype(np.float64)
        for dy in range(3):
            for dx in range(3):
                ref[:, ch, dy, dx] = np.einsum("royx,ryx->o", D, lit[:, dy:dy + O, dx:dx + O]) * (255.0 / 256.0)
    got = part.array().astype(np.float64).sum(0)
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.abs(got[:162] - ref.reshape(-1)).max() < 2e-5 * scale            # the gradient tolerance of test_hip_learner_path.py:717
    assert np.abs(got[162:] - D.sum((0, 2, 3))).max() < 2e-5 * max(1.0, float(np.abs(D.sum((0, 2, 3))).max()))
    waves = (R + CW_ROWS - 1) // CW_ROWS
    assert not part.array()[waves:].any()                                      # "rows past the last wave's windows are written as zeros"


# ---- ssd_build_inputs / ssd_build_inputs_flags ---------------------------------------------------------------------------------------
def _inputs_ref(flags, rows_bt, n, Aa, t0, acts, rew, ainc, pos, scale):
    """[rows_bt, n, width] of the _build_inputs tail in the reference's block order (homophily_controller.py:137-184); t0: bit 0 = the
    t == 0 branch, bits 8.. = T (the history tensors hold every step's own values: the previous row, none at an episode's first)."""
    hist = t0 >> 8
    tz = np.array([(t0 & 1) or (hist and b % hist == 0) for b in range(rows_bt)], dtype=bool)
    prev = np.arange(rows_bt) - 1 if hist else np.arange(rows_bt)
    prev = np.where(tz, 0, prev)
    la, lr, li = acts[prev], rew[prev], ainc[prev]
    live = (~tz)[:, None]
    blocks = []
    onehot = ((la[..., None] == np.arange(Aa)) & live[..., None]).astype(np.float32)
    if flags & 1: blocks.append(onehot)
    if flags & 2: blocks.append(np.broadcast_to(np.eye(n, dtype=np.float32), (rows_bt, n, n)))
    if flags & 4: blocks.append((np.sign(lr) * live).astype(np.float32)[..., None])
    if flags & 8:
        off = ~np.eye(n, dtype=bool)
        recv = (((li == 1) & off).sum(1) - ((li == 2) & off).sum(1)) * live            # receiver i over givers g
        blocks.append(np.sign(recv).astype(np.float32)[..., None])
    if flags & 64: blocks.append(np.broadcast_to(onehot.reshape(rows_bt, 1, n * Aa), (rows_bt, n, n * Aa)))
    if flags & 16:
        d = pos[:, :, None, :] - pos[:, None, :, :]
        blocks.append((np.float32(1) - np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) / scale).astype(np.float32))
    if flags & 32: blocks.append((pos / scale).astype(np.float32))
    return np.concatenate(blocks, axis=-1) if blocks else np.zeros((rows_bt, n, 0), np.float32)


ALL_FLAG_WORDS = list(range(128))          # the 128 combinations tests/test_learner_parity.py:130 enumerates


@pytest.mark.parametrize("B,T,n,Aa", [(1, 1, 2, 8), (3, 17, 5, 9), (5, 5, 10, 9), (16, 8, 2, 9)])
def test_build_inputs_in_the_arena(B, T, n, Aa):
    """ssd_build_inputs (the shipped blocks) and ssd_build_inputs_flags with every one of the 128 flag words, in the t0 = 1, t0 = 0,
    agent-major and seq_len (t0 = T << 8) forms; `out` is wider than the block with out_offset > 0 -- the untouched columns are bands
    (they must keep the pre-fill); rows x width ragged against 256; last actions of -1; bit-exact (test_hip_learner_path.py:929 holds the
    reference controller to 1e-6; the blocks are one-hots, signs and one f32 division / square root)."""
    rng = np.random.default_rng(B + T + n)
    rows = B * T
    acts = rng.integers(-1, Aa, (rows, n)).astype(np.int64)
    rew, ainc = f32(rng.integers(-1, 2, (rows, n))), rng.integers(0, 3, (rows, n, n)).astype(np.int64)
    pos, scale = f32(rng.integers(0, 25, (rows, n, 2))), np.float32(30.805843601498726)
    lib = _lib()
    words = [None] + [abi.INPUT_EXPLICIT | w for w in ALL_FLAG_WORDS]
    forms = [1, 0, 2, T << 8, (T << 8) | 2]
    for k, word in enumerate(words):
        t0 = forms[k % len(forms)]
        flags = 1 | 2 | 4 | 8 | 32 if word is None else word & 127
        ref = _inputs_ref(flags, rows, n, Aa, t0, acts, rew, ainc, pos, scale)
        width = ref.shape[-1]
        if word is not None:
            assert lib.ssd_build_inputs_width(n, Aa, word) == width
        off, stride = 1 + k % 5, width + 1 + k % 5 + k % 3
        A = Arena()
        pa, pr = A.place("last_actions", acts, align=8, fill=Aa), A.place("last_reward", rew, offset_in_16=4)
        pi, pp = A.place("last_actions_inc", ainc, align=8, fill=3), A.place("pos", pos, offset_in_16=12)
        w = np.zeros((rows * n, stride), dtype=bool); w[:, off:off + width] = True
        out = A.reserve("out", (rows * n, stride), offset_in_16=8, written=w)
        if word is None:
            call("ssd_build_inputs", rows, n, Aa, t0, pa.ptr, pr.ptr, pi.ptr, pp.ptr, float(scale), out.ptr, stride, off, None)
        else:
            call("ssd_build_inputs_flags", rows, n, Aa, t0, word, pa.ptr, pr.ptr, pi.ptr, pp.ptr, float(scale), out.ptr, stride, off, None)
        A.check()
        exp = ref.transpose(1, 0, 2) if t0 & 2 else ref                   # agent-major rows i * rows + b
        assert np.array_equal(out.array()[:, off:off + width], exp.reshape(rows * n, width)), (word, t0)


# ---- ssd_gru_seq_fwd / _bwd / _fwd_parts / _bwd_parts ----------------------------------------------------------------------------------
def _gru_reference(gi, wh, bh, dhs):
    """float64 unroll of the cell from a zero state (homophily_agent.py:162-165) + autograd: gi [T, G, B, 192], wh [G, 64, 192],
    bh [G, 192], dhs [G, T, B, 64] -> hs [G, T, B, 64], rzn [T, G, B, 192], ghn [T, G, B, 64], d_gi, d_wh, d_bh"""
    import torch as th
    gi, wh, bh = (th.tensor(t, dtype=th.float64, requires_grad=True) for t in (gi, wh, bh))
    T, G, B = gi.shape[:3]
    h, hs, rzn, ghn = th.zeros(G, B, 64, dtype=th.float64), [], [], []
    for t in range(T):
        gh = th.baddbmm(bh[:, None, :], h, wh)
        r, z = th.sigmoid(gi[t][..., :64] + gh[..., :64]), th.sigmoid(gi[t][..., 64:128] + gh[..., 64:128])
        c = th.tanh(gi[t][..., 128:] + r * gh[..., 128:])
        h = (1 - z) * c + z * h
        hs.append(h); rzn.append(th.cat([r, z, c], -1)); ghn.append(gh[..., 128:])
    hs = th.stack(hs, 1)
    (hs * th.tensor(dhs, dtype=th.float64)).sum().backward()
    return [t.detach().numpy() for t in (hs, th.stack(rzn), th.stack(ghn), gi.grad, wh.grad, bh.grad)]


def _gru_data(T, G, B, seed):
    rng = np.random.default_rng(seed)
    return (f32(rng.standard_normal((T, G, B, 192)) * 0.7), f32(rng.standard_normal((G, 64, 192)) * 0.15), f32(rng.standard_normal((G, 192)) * 0.1),
            f32(rng.standard_normal((G, T, B, 64))))                    # scaled as test_hip_learner_path.py:671-674


def _status_clear():
    from homophily_marl_amd import ops
    assert ops.numeric_status() == 0


GRU_SEQ_CASES = [(1, 1, 16, 1), (2, 3, 48, 1), (101, 3, 16, 1), (2, 10, 16, 0), (1, 20, 48, 1), (101, 1, 48, 0), (2, 20, 16, 1)]      # (T, G, B, train)


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("T,G,B,train", GRU_SEQ_CASES)
def test_gru_sequence_in_the_arena(T, G, B, train, bf):
    """ssd_gru_seq_fwd (with and without rzn / ghn) and ssd_gru_seq_bwd, every tensor 16-byte aligned as the header requires (the
    refusal of anything else: tests/test_learner_abi_refusals.py).  f32: states < 1e-5, gradients < 2e-5 of their scale
    (test_hip_learner_path.py:690,692).  bf16 products: the bands / written / no-NaN checks only (no elementwise bound is derived for
    T chained steps)."""
    gi, wh, bh, dhs = _gru_data(T, G, B, T * 100 + G + B)
    hs_r, rzn_r, ghn_r, dgi_r, dwh_r, dbh_r = _gru_reference(gi, wh, bh, dhs)
    tiles = B // 16

    def run():
        A = Arena()
        pgi, pwh, pbh = (A.place(nm, t, align=16) for nm, t in (("gi", gi), ("wh", wh), ("bh", bh)))
        hs = A.reserve("hs", (G, T, B, 64), align=16)
        rzn, ghn = (A.reserve("rzn", (T, G, B, 192), align=16), A.reserve("ghn", (T, G, B, 64), align=16)) if train else (None, None)
        call("ssd_gru_seq_fwd", pgi.ptr, pwh.ptr, pbh.ptr, hs.ptr, rzn.ptr if train else None, ghn.ptr if train else None, T, G, B, None)
        A.check()
        _status_clear()
        if not train:
            return hs.array(), None
        saved = (hs.array(), rzn.array(), ghn.array())
        A2 = Arena()
        pd, ph, pr, pn, pw = (A2.place(nm, t, align=16) for nm, t in (("dhs", dhs), ("hs", saved[0]), ("rzn", saved[1]), ("ghn", saved[2]), ("wh", wh)))
        dgi, dgh = A2.reserve("d_gi", (T, G, B, 192), align=16), A2.reserve("dgh", (G, T, B, 192), align=16, written=None)
        dwh, dbp = A2.reserve("d_wh", (G, 64, 192), offset_in_16=4), A2.reserve("d_bh_part", (G, tiles, 192), offset_in_16=12)
        call("ssd_gru_seq_bwd", pd.ptr, ph.ptr, pr.ptr, pn.ptr, pw.ptr, dgi.ptr, dgh.ptr, dwh.ptr, dbp.ptr, T, G, B, None)
        A2.check(allow_nan=("dgh",))
        _status_clear()
        return saved, (dgi.array(), dwh.array(), dbp.array().astype(np.float64).sum(1))
    if bf:
        with bf16_products():
            run()
        return
    fwd, grads = run()
    if not train:
        assert np.abs(fwd - hs_r).max() < 1e-5
        return
    assert np.abs(fwd[0] - hs_r).max() < 1e-5 and np.abs(fwd[1] - rzn_r).max() < 1e-5 and np.abs(fwd[2] - ghn_r).max() < 1e-5
    for got, ref, nm in zip(grads, (dgi_r, dwh_r, dbh_r), ("d_gi", "d_wh", "d_bh")):
        close_f32(got, ref, 2e-5, nm)


@pytest.mark.parametrize("T,spp,B,n_parts,n_wparts,grad_parts", [(2, 1, 16, 1, 1, 1), (2, 1, 48, 2, 1, 1), (1, 1, 16, 3, 3, 2), (2, 5, 16, 4, 2, 2), (101, 1, 16, 4, 4, 3),
                                                                 (2, 3, 16, 2, 2, 2), (2, 1, 16, 4, 1, 1), (1, 5, 48, 2, 1, 1), (2, 1, 16, 3, 1, 3), (2, 1, 16, 4, 4, 4)])
def test_gru_sequence_parts_in_the_arena(T, spp, B, n_parts, n_wparts, grad_parts):
    """ssd_gru_seq_fwd_parts / _bwd_parts: gi parts 1 .. 4 x weight parts 1 .. 4 as separately placed tensors, G_grad < G (the target
    net's sets carry no gradient): the d_gi parts past G_grad and the tail of d_wh / dgh / d_bh_part must stay unwritten AND their
    bands clean.  Values as test_gru_sequence_in_the_arena."""
    G = spp * n_parts
    if G % n_wparts:
        G = spp * n_parts * n_wparts; spp = G // n_parts
    Gn, tiles, wpp = grad_parts * spp, B // 16, G // n_wparts
    gi, wh, bh, dhs = _gru_data(T, G, B, T + G + B + n_parts)
    dhs[Gn:] = 0                                                     # the sets without a gradient
    hs_r, rzn_r, ghn_r, dgi_r, dwh_r, dbh_r = _gru_reference(gi, wh, bh, dhs)
    set_major = lambda t: np.ascontiguousarray(np.swapaxes(t, 0, 1))      # [T, G, ...] -> [G, T, ...]
    gis = set_major(gi)
    A = Arena()
    pgi = [A.place("gi part %d" % k, gis[k * spp:(k + 1) * spp], align=16) for k in range(n_parts)]
    pwh = [A.place("wh part %d" % k, wh[k * wpp:(k + 1) * wpp], align=16) for k in range(n_wparts)]
    pbh = [A.place("bh part %d" % k, bh[k * wpp:(k + 1) * wpp], align=16) for k in range(n_wparts)]
    hs, rzn, ghn = A.reserve("hs", (G, T, B, 64), align=16), A.reserve("rzn", (T, G, B, 192), align=16), A.reserve("ghn", (T, G, B, 64), align=16)
    tab = lambda regs: (C.c_void_p * 4)(*[r.ptr for r in regs])
    call("ssd_gru_seq_fwd_parts", tab(pgi), n_parts, tab(pwh), tab(pbh), n_wparts, hs.ptr, rzn.ptr, ghn.ptr, T, G, B, None)
    A.check()
    _status_clear()
    assert np.abs(hs.array() - hs_r).max() < 1e-5 and np.abs(rzn.array() - rzn_r).max() < 1e-5 and np.abs(ghn.array() - ghn_r).max() < 1e-5
    A2 = Arena()
    dh = dhs.reshape(G, T, B, 64)
    pdh = [A2.place("dhs part %d" % k, dh[k * spp:(k + 1) * spp], align=16) for k in range(n_parts)]
    ph, pr, pn = A2.place("hs", hs.array(), align=16), A2.place("rzn", rzn.array(), align=16), A2.place("ghn", ghn.array(), align=16)
    pwh = [A2.place("wh part %d" % k, wh[k * wpp:(k + 1) * wpp], align=16) for k in range(n_wparts)]
    dgi = [A2.reserve("d_gi part %d" % k, (spp, T, B, 192), align=16, written=k < grad_parts) for k in range(n_parts)]
    head = lambda shape: np.broadcast_to((np.arange(G) < Gn).reshape((G,) + (1,) * (len(shape) - 1)), shape)
    dgh = A2.reserve("dgh", (G, T, B, 192), align=16, written=None)
    dwh = A2.reserve("d_wh", (G, 64, 192), offset_in_16=8, written=head((G, 64, 192)))
    dbp = A2.reserve("d_bh_part", (G, tiles, 192), offset_in_16=4, written=head((G, tiles, 192)))
    call("ssd_gru_seq_bwd_parts", tab(pdh), ph.ptr, pr.ptr, pn.ptr, tab(pwh), n_wparts, tab(dgi), n_parts, dgh.ptr, dwh.ptr, dbp.ptr, T, G, Gn, B, None)
    A2.check(allow_nan=("dgh",))
    _status_clear()
    pre = np.frombuffer(np.full(1, 0x7FE0BEEF, dtype="<u4").tobytes(), dtype=np.float32)[0]
    assert (dgh.array()[Gn:].view(np.uint32) == np.float32(pre).view(np.uint32)).all()                 # the workspace's tail: untouched
    got_gi = np.concatenate([d.array() for d in dgi[:grad_parts]], axis=0)
    close_f32(got_gi, set_major(dgi_r)[:Gn], 2e-5, "d_gi")                                               # test_hip_learner_path.py:692
    close_f32(dwh.array()[:Gn], dwh_r[:Gn], 2e-5, "d_wh")
    close_f32(dbp.array()[:Gn].astype(np.float64).sum(1), dbh_r[:Gn], 2e-5, "d_bh")


# ---- ssd_clip_adam_step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numels", [[1], [1000], [1024, 1, 1023, 2049, 7], [3] * abi.ADAM_MAX_JOBS, [1 + (37 * k) % 300 for k in range(abi.ADAM_MAX_JOBS)]],
                         ids=["one element", "one job", "ragged jobs", "64 small jobs", "64 ragged jobs"])
def test_clip_adam_step_in_the_arena(numels):
    """job boundaries that are not multiples of the 1024-element workgroup span, a one-element job, n_jobs = 1 and SSD_ADAM_MAX_JOBS;
    parameters, both optimisers' moments, the step counters, flat_grad and partials all banded.  Reference: the statement of
    include/ssd_hip.h (clip_grad_norm_ x 2 + torch.optim.Adam x 2) in float64; parameters < 2e-6, moments < 1e-4 of their largest
    (test_hip_learner_path.py:956,963)."""
    rng = np.random.default_rng(len(numels) + numels[0])
    total, chunks = sum(numels), (sum(numels) + 1023) // 1024
    lr, b1, b2, eps, clip = (np.float32(5e-4), np.float32(1e-3)), np.float32(0.9), np.float32(0.999), np.float32(1e-8), np.float32(0.05)
    grad = f32(rng.standard_normal(total) * 0.1)
    A = Arena()
    pg = A.place("flat_grad", grad, offset_in_16=4, inout=True)
    steps0 = np.full((len(numels), 2), 3.0, dtype=np.float32)
    pst = A.place("steps", steps0, offset_in_16=8, inout=True)
    part = A.reserve("partials", (chunks, 3), offset_in_16=12)
    jobs, host = [], []
    off = 0
    for k, ne in enumerate(numels):
        seg = k % 3
        opts = (0, 1) if seg == 0 else ((1,) if seg == 1 else (0,))
        p0 = f32(rng.standard_normal(ne))
        rp = A.place("param %d" % k, p0, offset_in_16=OFFS[k % 4], inout=True)
        mom = {o: (f32(rng.standard_normal(ne) * 0.01), f32(rng.random(ne) * 1e-3)) for o in opts}
        rm = {o: (A.place("exp_avg %d.%d" % (k, o), mom[o][0], offset_in_16=OFFS[(k + o) % 4], inout=True),
                  A.place("exp_avg_sq %d.%d" % (k, o), mom[o][1], offset_in_16=OFFS[(k + o + 1) % 4], inout=True)) for o in opts}
        jobs.append((rp, off, ne, seg, rm)); host.append((p0, mom))
        off += ne
    table = (abi.SsdAdamJob * len(numels))()
    for k, (rp, o0, ne, seg, rm) in enumerate(jobs):
        table[k].param, table[k].offset, table[k].numel, table[k].segment = rp.ptr, o0, ne, seg
        for o in (0, 1):
            if o in rm:
                table[k].exp_avg[o], table[k].exp_avg_sq[o], table[k].step[o] = rm[o][0].ptr, rm[o][1].ptr, pst.ptr + 4 * (2 * k + o)
    import torch as th
    jt = th.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).cuda()                # the job table: a device array the kernels only read
    args = abi.SsdClipAdamArgs(flat_grad=pg.ptr, total=total, jobs=jt.data_ptr(), n_jobs=len(numels), partials=part.ptr, lr_inc=float(lr[0]),
                               lr_env=float(lr[1]), beta1=float(b1), beta2=float(b2), eps=float(eps), clip=float(clip))
    call("ssd_clip_adam_step", C.byref(args), None)
    A.check()
    assert th.equal(jt.cpu(), th.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()))
    g64, S, o0 = grad.astype(np.float64), [0.0, 0.0, 0.0], 0
    for rp, o0, ne, seg, rm in jobs:
        S[seg] += (g64[o0:o0 + ne] ** 2).sum()
    c_inc = min(1.0, float(clip) / (np.sqrt(S[0] + S[2]) + 1e-6))
    c_env = min(1.0, float(clip) / (np.sqrt(c_inc * c_inc * S[0] + S[1]) + 1e-6))
    assert c_inc < 1.0 or total < 20                                                             # the clips really scale
    B1, B2, st = float(b1), float(b2), 4.0
    got_g, got_s = pg.array(), pst.array()
    for k, ((rp, o0, ne, seg, rm), (p0, mom)) in enumerate(zip(jobs, host)):
        g = g64[o0:o0 + ne] * (c_inc * c_env if seg == 0 else (c_env if seg == 1 else c_inc))
        assert np.abs(got_g[o0:o0 + ne] - g).max() < 2e-6
        p = p0.astype(np.float64)
        for o in (0, 1):
            if o not in rm:
                assert got_s[k, o] == 3.0
                continue
            assert got_s[k, o] == 4.0
            m, v = mom[o][0].astype(np.float64), mom[o][1].astype(np.float64)
            m = m + (1 - B1) * (g - m); v = B2 * v + (1 - B2) * g * g
            p = p - (float(lr[o]) / (1 - B1 ** st)) * m / (np.sqrt(v) / np.sqrt(1 - B2 ** st) + float(eps))
            assert np.abs(rm[o][0].array() - m).max() <= 1e-4 * max(1e-12, np.abs(m).max())
            assert np.abs(rm[o][1].array() - v).max() <= 1e-4 * max(1e-12, np.abs(v).max())
        assert np.abs(rp.array() - p).max() < 2e-6, k
    ps = part.array().astype(np.float64).sum(0)
    assert np.allclose(ps, S, rtol=1e-5, atol=1e-12)


# ---- ssd_td_sim_loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double_q,others", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("B,T,n", [(16, 100, 5), (5, 23, 10), (7, 31, 5), (1, 3, 2), (3, 9, 2)])
def test_td_sim_loss_in_the_arena(B, T, n, double_q, others):
    """mode 0 and mode 1 with the four (double_q, consider_others_inc) sets at the (B, T, n) of tests/test_learner_options_gpu.py:54 plus
    B = 1 and n = 2, every tensor in the arena: bands, inputs untouched, every dq element written (the bootstrap slot as zeros), no NaN,
    `partials` columns 13 .. 15 (and, in mode 0, 2 .. 15) keep the pre-fill.  Values compared here are the ones with a closed form that
    does not restate the kernel: mask, similarity-mask sum, give, received difference, clean flag, reward -- exact; the TD / similarity
    terms and the gradient are held to the tensor-op loss by tests/test_hip_learner_path.py:233 and test_learner_options_gpu.py."""
    rng = np.random.default_rng(B + T + n + 2 * double_q + others)
    T1, Aa, H = T + 1, 9, 3
    q_env, tq_env = f32(rng.standard_normal((B, T1, n, Aa))), f32(rng.standard_normal((B, T1, n, Aa)))
    q_inc, tq_inc = f32(rng.standard_normal((B, T1, n, n, 3))), f32(rng.standard_normal((B, T1, n, n, 3)))
    avail = (rng.random((B, T1, n, Aa)) < 0.7).astype(np.int32); avail[..., 4] = 1
    acts = rng.integers(0, Aa, (B, T1, n)).astype(np.int64)
    ainc = (rng.integers(0, 3, (B, T1, n, n)) * (1 - np.eye(n, dtype=np.int64))).astype(np.int64)
    rew = f32(rng.integers(-1, 3, (B, T1, n)) * (rng.random((B, T1, n)) < 0.3))
    cln = f32(rng.integers(0, 3, (B, T1, n)) * (rng.random((B, T1, n)) < 0.3))
    term = np.zeros((B, T1), dtype=np.uint8)
    for b in range(B):
        term[b, max(0, T - 1 - (b % 3) * 2)] = 1
    filled = np.ones((B, T1), dtype=np.int64)
    filled[:, 1:] = 1 - np.minimum(1, np.cumsum(term, 1)[:, :-1])
    for mode in (0, 1):
        A = Arena()
        P = lambda nm, t, **kw: A.place(nm, t, **kw)
        a = abi.SsdTdLossArgs(batch=B, t_slots=T1, n_agents=n, n_actions=Aa, sim_horizon=H, double_q=double_q, gamma_env=0.99, gamma_inc=0.99, reward_scale=1.0,
                              incentive_ratio=1.0, incentive_cost=0.5, incentive=2.0, seq_len=float(T1), sim_threshold=0.1, sim_loss_weight=0.1,
                              consider_others_inc=others)
        regs = dict(q_env=P("q_env", q_env, offset_in_16=4), q_inc=P("q_inc", q_inc, offset_in_16=8), tq_env=P("tq_env", tq_env, offset_in_16=12),
                    tq_inc=P("tq_inc", tq_inc, offset_in_16=4), actions=P("actions", acts, align=8, fill=Aa), actions_inc=P("actions_inc", ainc, align=8, fill=3),
                    avail=A.place("avail", avail, fill=0), reward=P("reward", rew, offset_in_16=8), clean_num=P("clean_num", cln, offset_in_16=12),
                    terminated=P("terminated", term, align=1, fill=1), filled=P("filled", filled, align=8, fill=0))
        mask = filled[:, :T] * np.concatenate([np.ones((B, 1), np.int64), 1 - term[:, :T - 1].astype(np.int64)], 1) if T > 1 else filled[:, :T]
        regs["dens"] = P("dens", f32([max(1.0, float(mask.sum() * n)), 3.0]), offset_in_16=4)
        wp = np.zeros((B * T * n, abi.TD_LOSS_PARTIALS), dtype=bool); wp[:, :13 if mode else 2] = True
        regs["partials"] = A.reserve("partials", wp.shape, offset_in_16=8, written=wp)
        regs["dq_env"] = A.reserve("dq_env", q_env.shape, offset_in_16=12, written=bool(mode))
        regs["dq_inc"] = A.reserve("dq_inc", q_inc.shape, offset_in_16=4, written=bool(mode))
        for k, r in regs.items():
            setattr(a, k, r.ptr)
        call("ssd_td_sim_loss", C.byref(a), mode, None)
        A.check()
        part = regs["partials"].array().reshape(B, T, n, abi.TD_LOSS_PARTIALS)
        assert np.array_equal(part[..., 0], np.broadcast_to(mask[..., None].astype(np.float32), (B, T, n)))
        # window flags -> cluster / idle -> sum over k != i of [cluster equal] idle_i idle_k (n - 2)   (homophily_learner.py:184-206)
        cn, rw = np.zeros((B, T, n)), np.zeros((B, T, n))
        for t in range(T):
            lo = max(0, t - H + 1)
            cn[:, t] = (cln[:, lo:t + 1] > 0).sum(1) > 0
            rw[:, t] = rew[:, lo:t + 1].astype(np.float64).sum(1) > 0
        cl, idle = 2 * rw + cn, cn + rw
        same = (cl[..., :, None] == cl[..., None, :]) & ~np.eye(n, dtype=bool)
        sim = (same * idle[..., :, None] * idle[..., None, :]).sum(-1) * (n - 2)
        assert np.array_equal(part[..., 1], sim.astype(np.float32))
        if mode:
            off = ~np.eye(n, dtype=bool)
            give = ((ainc != 0) & off).sum(3)[:, :T]
            rv = (((ainc == 1) & off).sum(2) - ((ainc == 2) & off).sum(2))[:, :T]
            assert np.array_equal(part[..., 7], give.astype(np.float32)) and np.array_equal(part[..., 8], rv.astype(np.float32))
            assert np.array_equal(part[..., 10], (cln[:, :T] > 0).astype(np.float32)) and np.array_equal(part[..., 12], rew[:, :T])
            assert not regs["dq_env"].array()[:, T].any() and not regs["dq_inc"].array()[:, T].any()          # the bootstrap slot: zeros
            assert np.count_nonzero(regs["dq_env"].array()[:, :T]) <= B * T * n                               # one action per (b, t, i)


# ---- ssd_policy_encode (the learner's call form: ops._EncodeCodes) -------------------------------------------------------------------
@pytest.mark.parametrize("R,V", [(1, 3), (3, 5), (4, 15), (5, 17), (203, 31), (5, 63), (203, 3), (1, 63), (3, 31), (4, 5), (5, 15), (203, 17), (203, 15), (1, 31)])
def test_policy_encode_with_act_in_the_arena(R, V):
    """the training forward: class codes u8 [R, V, V] at a byte address of any alignment -> `act` = LeakyReLU(conv) [R, 6, O, O] and
    the features (`out` [R, 32] for one band, else `part` [bands, R, 32], 16-byte aligned as the header requires); the fragment images are
    packed into the arena as well.  Features within 1e-5 of the float64 encoder (tests/test_encoder_any_view.py:112); the codes' bands
    hold 0xFF (no class)."""
    O = V - 2
    rng = np.random.default_rng(R * 100 + V)
    codes = rng.integers(0, 4, (R, V, V)).astype(np.uint8)
    k1, k2 = 1 / np.sqrt(27.0), 1 / np.sqrt(6.0 * O * O)                  # nn.Conv2d / nn.Linear default initialisation ranges
    cw, cb = f32(rng.uniform(-k1, k1, (6, 3, 3, 3))), f32(rng.uniform(-k1, k1, 6))
    lw, lb = f32(rng.uniform(-k2, k2, (32, 6 * O * O))), f32(rng.uniform(-k2, k2, 32))
    layout = abi.ENCODE_LAYOUT_TOEPLITZ if V in (15, 31) else abi.ENCODE_LAYOUT_LUT
    cbytes, lbytes = abi.encode_frag_bytes(V, 2, layout)
    bands = abi.encode_bands(V)
    A = Arena()
    pc = A.place("codes", codes, align=1, fill=0xFF, row_bytes=V * V)
    pcw, pcb, plw, plb = A.place("conv_w", cw, offset_in_16=4), A.place("conv_b", cb, offset_in_16=8), A.place("lin_w", lw, offset_in_16=12), A.place("lin_b", lb, offset_in_16=4)
    cf = A.reserve("conv image", (cbytes,), dtype=np.uint8, align=16, written=None)
    lf = A.reserve("lin image", (lbytes,), dtype=np.uint8, align=16, written=None)
    act = A.reserve("act", (R, 6, O, O), offset_in_16=8, row_bytes=6 * O * O * 4)
    feat = A.reserve("out", (R, 32), offset_in_16=12) if bands == 1 else A.reserve("part", (bands, R, 32), align=16)
    pack = "ssd_policy_pack_encoder" if layout == abi.ENCODE_LAYOUT_TOEPLITZ else "ssd_policy_pack_encoder_lut"
    call(pack, pcw.ptr, pcb.ptr, plw.ptr, V, 2, cf.ptr, lf.ptr, None)
    ea = abi.SsdPolicyEncodeArgs(codes=pc.ptr, code_bytes=codes.size, env_stride=V * V, slot_stride=0, agent_stride=V * V, rows=R, view_edge=V, n_agents=1,
                                 agent_major=0, precision=2, layout=layout, alphabet=abi.CODE_CLASS, conv_frags=cf.ptr, lin_frags=lf.ptr, conv_b=pcb.ptr,
                                 lin_b=plb.ptr, act=act.ptr)
    if bands == 1:
        ea.out, ea.out_stride = feat.ptr, 32
    else:
        ea.part = feat.ptr
    call("ssd_policy_encode", C.byref(ea), None)
    A.check()
    planes = np.stack([(codes == c) for c in (2, 1, 3)], 1).astype(np.float64) * (255.0 / 256.0)
    conv = np.zeros((R, 6, O, O)) + cb.astype(np.float64)[None, :, None, None]
    for dy in range(3):
        for dx in range(3):
            conv += np.einsum("oc,rcyx->royx", cw.astype(np.float64)[:, :, dy, dx], planes[:, :, dy:dy + O, dx:dx + O])
    a_ref = leaky(conv)
    lin = a_ref.reshape(R, -1) @ lw.astype(np.float64).T
    assert np.abs(act.array() - a_ref).max() < 1e-5                                                      # tests/test_encoder_any_view.py:112
    if bands == 1:
        assert np.abs(feat.array() - leaky(lin + lb.astype(np.float64))).max() < 1e-5
    else:
        assert np.abs(feat.array().astype(np.float64).sum(0) - lin).max() < 1e-5
