"""GPU: the row assembly in front of the learner's two fc1 layers (csrc/ssd_train_rows.hip: ssd_fc1_rows_fwd / _bwd, ops.fc1_rows) against
the tensor operations it replaces -- th.cat([feat, tail]), the transposition to set-major, time-major rows, th.cat([x, act]) and, on the
way back, the addition of the two layers' input gradients, its slice and its transposition.  Copies and one addition of two f32 values:
the comparison is `==` throughout.  Kernel calls with raw pointers into a poisoned arena (tests/arena_util.py): no write outside an
output, every output element written, no read of the surroundings.

Shapes: one and two nets; the train step's widths (32 | 18 | 9) at B = 2, T = 5, n = 5; another team and Harvest's widths; a single
element of everything; a batch of more than one workgroup; no tail."""
import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops
from tests.arena_util import Arena

pytestmark = pytest.mark.gpu

# B, T, n, feat_w, tail_w, act_w, nets
SHAPES = [(2, 5, 5, 32, 18, 9, 2), (3, 4, 2, 32, 15, 8, 2), (1, 1, 1, 1, 1, 1, 2), (16, 7, 5, 32, 18, 9, 1), (2, 3, 10, 32, 0, 9, 2), (5, 2, 3, 7, 3, 2, 1)]
OFFS = (4, 8, 12, 0)


def call(name, *args):
    lib = abi.load_library()
    abi.check(lib, getattr(lib, name)(*args))


def _tm(x, B, T, n):
    """rows (b * T + t) * n + i -> [n, T * B, .], rows t * B + b"""
    return np.ascontiguousarray(x.reshape(B, T, n, -1).transpose(2, 1, 0, 3)).reshape(n, T * B, -1)


@pytest.mark.parametrize("B,T,n,F0,F1,A,nets", SHAPES)
def test_row_assembly_kernels_equal_the_concatenations_and_transpositions(B, T, n, F0, F1, A, nets):
    rng = np.random.default_rng(B * 100 + T * 10 + n)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    feats, tail, act = [f(B * T * n, F0) for _ in range(nets)], f(B * T * n, F1), f(n, T * B, A)
    arena = Arena()
    pf = [arena.place("feat_%d" % k, x, offset_in_16=OFFS[k]) for k, x in enumerate(feats)]
    pt = arena.place("tail", tail, offset_in_16=8) if F1 else None
    pa = arena.place("act", act, offset_in_16=12)
    xe = [arena.reserve("x_env_%d" % k, (n, T * B, F0 + F1), offset_in_16=OFFS[k + 1]) for k in range(nets)]
    xi = [arena.reserve("x_inc_%d" % k, (n, T * B, F0 + F1 + A), offset_in_16=OFFS[k + 2]) for k in range(nets)]
    dxe, dxi = f(n, T * B, F0 + F1), f(n, T * B, F0 + F1 + A)
    pde, pdi = arena.place("d_x_env", dxe, offset_in_16=4), arena.place("d_x_inc", dxi, offset_in_16=8)
    ld = F0 + (F1 if (B + T) % 2 else 0)                           # dense rows, or the leading columns of rows F0 + F1 wide
    written = np.zeros((B * T * n, ld), dtype=bool)
    written[:, :F0] = True
    d_feat = arena.reserve("d_feat", (B * T * n, ld), offset_in_16=12, written=written)
    second = lambda regs: regs[1].ptr if nets == 2 else None
    call("ssd_fc1_rows_fwd", pf[0].ptr, second(pf), None if pt is None else pt.ptr, pa.ptr, xe[0].ptr, xi[0].ptr, second(xe), second(xi), B, T, n, F0, F1, A, None)
    call("ssd_fc1_rows_bwd", pde.ptr, pdi.ptr, d_feat.ptr, B, T, n, F0, F1, A, ld, None)
    arena.check()
    for k in range(nets):
        x = _tm(np.concatenate([feats[k], tail], axis=1), B, T, n)
        assert np.array_equal(xe[k].array(), x) and np.array_equal(xi[k].array(), np.concatenate([x, act], axis=-1)), k
    want = (dxe[..., :F0] + dxi[..., :F0]).reshape(n, T, B, F0).transpose(2, 1, 0, 3).reshape(B * T * n, F0)
    assert np.array_equal(d_feat.array()[:, :F0], want)


@pytest.mark.parametrize("B,T,n,F0,F1,A", [(2, 5, 5, 32, 18, 9), (3, 4, 2, 32, 15, 8)])
def test_fc1_rows_function_equals_the_tensor_operations_with_their_gradient(B, T, n, F0, F1, A):
    """ops.fc1_rows against the statement HomophilyMAC.unroll_inputs / HomophilyAgent.unroll_pre make with tensor operations: the four
    outputs, and the features' gradient of a fixed scalar of (x_env, x_inc) -- autograd's own add, slice and transposition."""
    g = th.Generator().manual_seed(B + T)
    mk = lambda *s: th.randn(*s, generator=g).cuda()
    feat, feat_t, tail, act = mk(B * T * n, F0).requires_grad_(), mk(B * T * n, F0), mk(B * T * n, F1), mk(n, T * B, A)
    seeds = [mk(n, T * B, F0 + F1), mk(n, T * B, F0 + F1 + A)]
    was = ops.STRICT
    ops.set_strict(True)
    try:
        xe, xi, xe_t, xi_t = ops.fc1_rows(feat, tail, act, B, T, n, feat_t)
        got = th.autograd.grad([xe, xi], [feat], grad_outputs=seeds)[0]
    finally:
        ops.set_strict(was)
    tm = lambda x: x.reshape(B, T, n, -1).permute(2, 1, 0, 3).reshape(n, T * B, -1)
    x, x_t = tm(th.cat([feat, tail], dim=1)), tm(th.cat([feat_t, tail], dim=1))
    xa = th.cat([x, act], dim=-1)
    want = th.autograd.grad([x, xa], [feat], grad_outputs=seeds)[0]
    assert th.equal(xe, x) and th.equal(xi, xa) and th.equal(xe_t, x_t) and th.equal(xi_t, th.cat([x_t, act], dim=-1))
    assert not xe_t.requires_grad and not xi_t.requires_grad and th.equal(got, want) and float(want.abs().max()) > 0
