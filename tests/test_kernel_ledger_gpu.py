"""GPU cases of the kernel ledger (tests/kernel_cases.py, tests/test_kernel_ledger_host.py): the two per-layer encoder entry points no other
test launches at more than one window size -- ssd_conv_leaky (k_conv_leaky<6, 0 / 15 / 31>) and ssd_encoder (k_encoder<6, 32, 1>) --
against Conv2d(3, 6, 3) + LeakyReLU(0.01) (+ Flatten + Linear + LeakyReLU) restated in float64 on random planes and weights of both signs.

Every operand stands in a poisoned arena (tests/arena_util.py): bands and inputs come back bit-identical, every output element the
contract writes is written and none beside it, no poison reaches an output.  Each case makes four launches into four outputs of one
arena: row order env-major and agent-major, without and with the copy of the observation into an episode storage
[N, 3 slots, n, 3, V, V] whose env stride is larger than the block (*store_t = 2: slot 2 bit-equal to obs, slots 0 and 1 and the
padding keep their fill); ssd_encoder writes rows of 32 features at stride 32, and at stride 64 from column 9 (inside an input matrix).

Tolerances are forward-error bounds per element, computed from the float64 magnitudes of the case (u = 2^-24, every rounding on the
longest chain counted once, first order):
    conv    e_c = 32 u (|b| + sum |w x|)                                   27 fmas, the bias, the activation
    linear  e_f = (6 ceil(P / 64) + 14) u sum |lw a| + sum |lw| e_c         the per-lane chain of 6 ceil(P / 64) fmas, six butterfly adds, the
                                                                           bias, the activation; and the conv's error carried through
Each case prints max(error / bound) before it asserts error <= bound.  Every launch is a valid call: the refusals are tested on the
CPU (tests/test_kernel_ledger_host.py)."""
import numpy as np
import pytest

from homophily_marl_amd import abi
from tests import kernel_cases as kc
from tests.arena_util import Arena

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLOTS, STORE_T, STORE_PAD = 3, 2, 8                       # the storage's time slots, the slot the launches file into, floats between env blocks
STRIDES = ((32, 0), (64, 9))                              # (out_stride, first column) of ssd_encoder's feature rows


def f32(a):
    return np.asarray(a, dtype=np.float32)


def leaky(v):
    return np.where(v > 0, v, 0.01 * v)


def _case(V, rows, seed, linear):
    """random f32 operands: planes N(0, 1), weights uniform in the default initialisation ranges of Conv2d / Linear (both signs)"""
    rng = np.random.default_rng(seed)
    P = (V - 2) ** 2
    k1, k2 = 1 / np.sqrt(27.0), 1 / np.sqrt(6.0 * P)
    d = dict(obs=f32(rng.standard_normal((rows, 3, V, V))), cw=f32(rng.uniform(-k1, k1, (6, 3, 3, 3))), cb=f32(rng.uniform(-k1, k1, 6)))
    if linear:
        d.update(lw=f32(rng.uniform(-k2, k2, (32, 6 * P))), lb=f32(rng.uniform(-k2, k2, 32)))
    return d


def conv_reference(d):
    """(LeakyReLU(conv) in float64 [R, 6, O, O], its error bound e_c) -- the convolution as 27 tap products"""
    X, W, Bv = (d[k].astype(np.float64) for k in ("obs", "cw", "cb"))
    R, _, V, _ = X.shape
    O = V - 2
    pre = np.zeros((R, 6, O, O)) + Bv[None, :, None, None]
    mag = np.zeros((R, 6, O, O)) + np.abs(Bv)[None, :, None, None]
    for ch in range(3):
        for dy in range(3):
            for dx in range(3):
                patch = X[:, ch, dy:dy + O, dx:dx + O][:, None]
                w = W[:, ch, dy, dx][None, :, None, None]
                pre += w * patch
                mag += np.abs(w) * np.abs(patch)
    return leaky(pre), 32 * U * mag


def linear_reference(d, act, e_conv):
    """(the features in float64 [R, 32], their error bound e_f)"""
    R = act.shape[0]
    P = act.shape[2] * act.shape[3]
    a, e = act.reshape(R, -1), e_conv.reshape(R, -1)
    LW, LB = d["lw"].astype(np.float64), d["lb"].astype(np.float64)
    chain = 6 * ((P + 63) // 64) + 14
    return leaky(a @ LW.T + LB), chain * U * (np.abs(a) @ np.abs(LW).T) + e @ np.abs(LW).T


def _agent_major(x, rows, n):
    """rows (b, i) -> rows (i, b)"""
    return np.ascontiguousarray(x.reshape((rows // n, n) + x.shape[1:]).swapaxes(0, 1)).reshape(x.shape)


def _storage(A, name, rows, n, L):
    """an episode storage [N, SLOTS, n, L] with STORE_PAD floats between env blocks; the contract writes slot STORE_T of every env"""
    N, stride = rows // n, SLOTS * n * L + STORE_PAD
    w = np.zeros((N, stride), dtype=bool)
    w[:, STORE_T * n * L:(STORE_T + 1) * n * L] = True
    return A.reserve(name, (N, stride), offset_in_16=8, row_bytes=L * 4, written=w), stride


def _check_storage(reg, d, rows, n, L):
    got = reg.array()[:, STORE_T * n * L:(STORE_T + 1) * n * L]
    assert np.array_equal(got.view(np.uint32), d["obs"].reshape(rows // n, n * L).view(np.uint32)), reg.name      # the copied slot: bit-equal


def _held_to(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / bound).max())
    print("%s: max error %.3e, max error / bound %.3f" % (what, float(err.max()), ratio))
    assert (err <= bound).all(), (what, ratio, tuple(int(i) for i in np.argwhere(err > bound)[0]))
    return ratio


@pytest.mark.parametrize("rows,n", kc.CONV_LEAKY_ROWS, ids=["rows%d_n%d" % c for c in kc.CONV_LEAKY_ROWS])
@pytest.mark.parametrize("V", kc.CONV_LEAKY_EDGES)
def test_conv_leaky_matches_the_float64_convolution_in_the_arena(V, rows, n):
    lib = abi.load_library()
    O = V - 2
    K, L = 6 * O * O, 3 * V * V
    d = _case(V, rows, 1000 * V + rows, linear=False)
    ref, bound = conv_reference(d)
    A = Arena()
    po = A.place("obs", d["obs"], offset_in_16=4, row_bytes=L * 4)
    pw, pb = A.place("conv_w", d["cw"], offset_in_16=12), A.place("conv_b", d["cb"], offset_in_16=8)
    pt = A.place("store_t", np.array([STORE_T], dtype=np.int64), align=8, fill=0)
    runs = []
    for am in (0, 1):
        for store in (False, True):
            out = A.reserve("out(agent_major %d, store %d)" % (am, store), (rows, K), offset_in_16=(4, 12)[am], row_bytes=K * 4)
            st, stride = _storage(A, "storage(agent_major %d)" % am, rows, n, L) if store else (None, 0)
            runs.append((am, out, st, stride))
    for am, out, st, stride in runs:
        abi.check(lib, lib.ssd_conv_leaky(po.ptr, rows, V, 6, pw.ptr, pb.ptr, out.ptr, n, am, st.ptr if st else None, stride, pt.ptr if st else None, None))
    A.check()
    worst = 0.0
    for am, out, st, stride in runs:
        want, lim = (ref.reshape(rows, K), bound.reshape(rows, K)) if not am else (_agent_major(ref.reshape(rows, K), rows, n), _agent_major(bound.reshape(rows, K), rows, n))
        worst = max(worst, _held_to(out.array(), want, lim, "%s V=%d %s" % (kc.conv_leaky(V), V, out.name)))
        if st:
            _check_storage(st, d, rows, n, L)
    assert worst > 0.0                                                          # f32 against float64: some rounding shows


@pytest.mark.parametrize("rows,n", kc.ENCODER_ROWS, ids=["rows%d_n%d" % c for c in kc.ENCODER_ROWS])
@pytest.mark.parametrize("V", kc.ENCODER_EDGES)
def test_encoder_matches_the_float64_encoder_in_the_arena(V, rows, n):
    lib = abi.load_library()
    L = 3 * V * V
    d = _case(V, rows, 2000 * V + rows, linear=True)
    act, e_conv = conv_reference(d)
    ref, bound = linear_reference(d, act, e_conv)
    A = Arena()
    po = A.place("obs", d["obs"], offset_in_16=12, row_bytes=L * 4)
    pw, pb = A.place("conv_w", d["cw"], offset_in_16=4), A.place("conv_b", d["cb"], offset_in_16=8)
    plw, plb = A.place("lin_w", d["lw"], offset_in_16=8), A.place("lin_b", d["lb"], offset_in_16=12)
    pt = A.place("store_t", np.array([STORE_T], dtype=np.int64), align=8, fill=0)
    runs = []
    for k, (am, (stride, col), store) in enumerate(((0, STRIDES[0], False), (1, STRIDES[1], True), (0, STRIDES[1], True), (1, STRIDES[0], False))):
        w = np.zeros((rows, stride), dtype=bool)
        w[:, col:col + 32] = True
        out = A.reserve("out(agent_major %d, stride %d, store %d)" % (am, stride, store), (rows, stride), offset_in_16=(4, 8, 12, 0)[k], written=w)
        st, env_stride = _storage(A, "storage(agent_major %d)" % am, rows, n, L) if store else (None, 0)
        runs.append((am, stride, col, out, st, env_stride))
    for am, stride, col, out, st, env_stride in runs:
        abi.check(lib, lib.ssd_encoder(po.ptr, rows, V, 6, 32, pw.ptr, pb.ptr, plw.ptr, plb.ptr, out.ptr + 4 * col, stride, n, am,
                                       st.ptr if st else None, env_stride, pt.ptr if st else None, None))
    A.check()
    for am, stride, col, out, st, env_stride in runs:
        want, lim = (ref, bound) if not am else (_agent_major(ref, rows, n), _agent_major(bound, rows, n))
        _held_to(out.array()[:, col:col + 32], want, lim, "%s V=%d %s" % (kc.encoder(), V, out.name))
        if st:
            _check_storage(st, d, rows, n, L)

