"""Helpers of the stored-state suites (tests/test_stored_state_host.py, tests/test_stored_state_gpu.py): no test in it.

The reference of the sequence kernels from a given state is a plain stepwise unroll of the GRU cell (homophily_agent.py:162-165) in
float64 that treats h0 as a constant: hs[0] = h0, steps 1 .. T - 1 computed, gradients by torch autograd."""
import torch as th


def gru_case(T, G, B, seed):
    """(gi [T, G, B, 192], wh [G, 64, 192], bh [G, 1, 192], h0 [G, B, 64] with |h0| < 0.9, wout [G, T, B, 64]) as CPU f32 tensors"""
    g = th.Generator().manual_seed(seed)
    gi = th.randn(T, G, B, 192, generator=g) * 0.7
    wh = th.randn(G, 64, 192, generator=g) * 0.15
    bh = th.randn(G, 1, 192, generator=g) * 0.1
    h0 = th.tanh(th.randn(G, B, 64, generator=g)) * 0.9
    wout = th.randn(G, T, B, 64, generator=g)
    return gi, wh, bh, h0, wout


def gru_step(gi_t, h, wh, bh):
    gh = th.baddbmm(bh, h, wh)
    r = th.sigmoid(gi_t[..., :64] + gh[..., :64])
    z = th.sigmoid(gi_t[..., 64:128] + gh[..., 64:128])
    cand = th.tanh(gi_t[..., 128:] + r * gh[..., 128:])
    return (1 - z) * cand + z * h


def gru_unroll_ref(gi, wh, bh, h0, wout, grad_sets=None):
    """float64: states [G, T, B, 64] with hs[:, 0] = h0 (a constant) and the gradients of sum(hs[:grad_sets] * wout[:grad_sets]) w.r.t.
    gi, wh, bh"""
    gi, wh, bh = (x.double().clone().requires_grad_() for x in (gi, wh, bh))
    h = h0.double()
    hs = [h]
    for t in range(1, gi.shape[0]):
        h = gru_step(gi[t], h, wh, bh)
        hs.append(h)
    hs = th.stack(hs, dim=1)
    k = hs.shape[0] if grad_sets is None else grad_sets
    loss = (hs[:k] * wout[:k].double()).sum()
    if loss.requires_grad:
        loss.backward()
    grads = tuple(x.grad if x.grad is not None else th.zeros_like(x) for x in (gi, wh, bh))
    return hs.detach(), grads
