"""Independent statements of the operators of homophily_marl_amd/ops.py, their test data and the launch recorder: a helper, no test
in it (tests/test_ops_contract_host.py, tests/test_ops_contract_gpu.py).

Every statement is float64 torch written from the reference's lines the operator cites, NOT from ops.py's host branches, and returns
(outputs, gradients of sum_k <output_k, cotangent_k> w.r.t. EVERY differentiable input) as numpy arrays.  The gradient of one input
does not depend on which other inputs are differentiated, so one evaluation per case serves every subset of requests; the cases are
cached (evaluated once, handed out read-only).

The launch recorder stands in for abi.load_library(): every attribute raises LaunchAttempt(name), so "this call would have launched
ssd_x" is observable without starting a kernel."""
import functools

import numpy as np
import torch as th

from tests.test_learner_kernel_bounds import _gru_reference, close_f32, f32  # noqa: F401  (re-exported to the two suites)

HOST_BAR = 1e-6         # host branch vs float64 statement: f32 rounding of short sums, relative to max(1, max |ref|)


# ---- the launch recorder ---------------------------------------------------------------------------------------------------------------
class LaunchAttempt(Exception):
    """an entry point of the HIP library was asked for: `name` would have been launched"""

    def __init__(self, name):
        super().__init__(name)
        self.name = name


class LaunchRecorder:
    def __getattr__(self, name):
        raise LaunchAttempt(name)


def install_recorder(monkeypatch):
    from homophily_marl_amd import ops
    monkeypatch.setattr(ops.abi, "load_library", lambda: LaunchRecorder())


# ---- evaluation --------------------------------------------------------------------------------------------------------------------------
def _evaluate(fn, inputs, cots):
    """fn(**float64 leaves) -> tensor or tuple; cots: one cotangent (array or None = output unused) per output.
    Returns ([outputs], {name: gradient}); an input no used output depends on has a zero gradient."""
    leaves = {k: th.tensor(np.asarray(v), dtype=th.float64, requires_grad=True) if np.asarray(v).dtype.kind == "f" else th.tensor(np.asarray(v))
              for k, v in inputs.items()}
    outs = fn(**leaves)
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    cots = list(cots) if isinstance(cots, (tuple, list)) else [cots]
    assert len(outs) == len(cots)
    loss = sum((o * th.tensor(np.asarray(c), dtype=th.float64)).sum() for o, c in zip(outs, cots) if c is not None)
    names = [k for k, v in leaves.items() if v.requires_grad]
    got = th.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True) if th.is_tensor(loss) else [None] * len(names)
    grads = {k: (np.zeros(leaves[k].shape) if g is None else g.numpy()) for k, g in zip(names, got)}
    return [o.detach().numpy() for o in outs], grads


def close_host(got, ref, name):
    """|got - ref| <= HOST_BAR * max(1, max |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= HOST_BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0), (name, err)


def leaky(y):
    """nn.LeakyReLU() (homophily_agent.py:22,26; F.leaky_relu :159,187): slope 0.01, a zero takes the negative side"""
    return th.where(y > 0, y, 0.01 * y)


# ---- the statements (float64 tensors in, tensors out) --------------------------------------------------------------------------------------
def st_bias_bmm(x, w, b, leaky_after=False):
    """th.matmul(inputs, w) + b per weight set (homophily_agent.py:159,168), b anything that broadcasts to [n, R, O]"""
    y = th.matmul(x, w) + b
    return leaky(y) if leaky_after else y


def st_gru_cell(gi, gh, h):
    """homophily_agent.py:162-165 on gi = x W_i + b_i, gh = h W_h + b_h, blocks (r, z, n)"""
    H = h.shape[-1]
    r = th.sigmoid(gi[..., :H] + gh[..., :H])
    z = th.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = th.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + z * h


def st_dueling_q(a, v, B, T, inner):
    """q = v + a - mean_k a (homophily_agent.py:170,206); rows (t * B + b) * inner + j of set i -> q[b, t, i, j]"""
    n, K = a.shape[0], a.shape[-1]
    q = v + a - a.mean(dim=-1, keepdim=True)
    return q.reshape(n, T, B, inner, K).permute(2, 1, 0, 3, 4)


def st_dueling_head(h, w, b, B, T, inner, other=None):
    """homophily_agent.py:200-206 (168-170 without `other`): the layer input of (i, tb, j) is [h[i, tb] | other[tb, j]], the advantage
    layer in columns 0..K-1 of w / b and the value layer in column K"""
    n, TB, H = h.shape
    K = w.shape[-1] - 1
    x = h.unsqueeze(2).repeat(1, 1, inner, 1)
    if other is not None:
        x = th.cat([x, other.unsqueeze(0).repeat(n, 1, 1, 1)], dim=-1)
    y = th.matmul(x, w.unsqueeze(1)) + b.reshape(b.shape[0] if b.dim() == 3 else 1, 1, 1, K + 1)
    a, v = y[..., :K], y[..., K:]
    q = v + a - a.mean(dim=-1, keepdim=True)                              # [n, TB, inner, K]
    return q.reshape(n, T, B, inner, K).permute(2, 1, 0, 3, 4)


def st_planes(codes):
    """the observation of a class-code window: waste (2) lights R, apple (1) G, wall / agent (3) B, at 255 / 256"""
    c = codes.unsqueeze(-3)
    return th.cat([c == 2, c == 1, c == 3], dim=-3).to(th.float64) * (255.0 / 256.0)


def st_encode(codes, conv_w, conv_b, lin_w, lin_b):
    """rgb_preprocess (homophily_agent.py:20-27,213-214): Conv2d 3 -> 6, 3 x 3, LeakyReLU, Flatten, Linear, LeakyReLU; the convolution
    written as the sum over the 27 taps"""
    x = st_planes(codes)                                                  # [R, 3, V, V]
    O = x.shape[-1] - 2
    y = conv_b.reshape(1, -1, 1, 1)
    for dy in range(3):
        for dx in range(3):
            y = y + th.einsum("rcyx,oc->royx", x[:, :, dy:dy + O, dx:dx + O], conv_w[:, :, dy, dx])
    y = leaky(y)
    return leaky(th.matmul(y.reshape(y.shape[0], -1), lin_w.t()) + lin_b)


# ---- cases: data (numpy f32, scaled as tests/test_hip_learner_path.py:672-674,706-707 scales it) + statement, cached ------------------------
def _rng(*key):
    return np.random.default_rng(abs(hash(tuple(int(k) for k in key))) % (2 ** 32))


def _cot(g, shape, ones):
    """a random cotangent, or all ones (what y.sum().backward() feeds: a stride-0 tensor); the generator advances the same either way"""
    c = f32(g.standard_normal(shape))
    return np.ones_like(c) if ones else c


def _ro(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def _case(inputs, outs, grads, cots, **extra):
    return dict(inputs=_ro(inputs), outs=_ro(outs), grads=_ro(grads), cots=_ro([c for c in cots]), **extra)


@functools.lru_cache(maxsize=None)
def bias_bmm_case(n, R, I, O, leaky_after, bias="n1O", ones=False):
    """bias: "n1O" (the kernel's form), "11O", "O", "nRO" -- the forms th.baddbmm broadcasts"""
    g = _rng(n, R, I, O, leaky_after)
    x, w = f32(g.standard_normal((n, R, I))), f32(g.standard_normal((n, I, O)) * 0.2)
    b = f32(g.standard_normal({"n1O": (n, 1, O), "11O": (1, 1, O), "O": (O,), "nRO": (n, R, O)}[bias]) * 0.1)
    if leaky_after and bias == "n1O":
        x[:, 0] = 0; b[:, :, 0] = 0                                       # an exact zero pre-activation in every weight set
    cot = _cot(g, (n, R, O), ones)
    inputs = dict(x=x, w=w, b=b)
    outs, grads = _evaluate(lambda x, w, b: st_bias_bmm(x, w, b, leaky_after), inputs, [cot])
    return _case(inputs, outs, grads, [cot])


@functools.lru_cache(maxsize=None)
def gru_case(T, G, B, ones=False):
    """gi [T, G, B, 192], wh [G, 64, 192], bh [G, 1, 192], cotangent [G, T, B, 64]: _gru_reference, the unroll of the cell from a zero
    state with autograd"""
    g = _rng(T, G, B)
    gi, wh = f32(g.standard_normal((T, G, B, 192)) * 0.7), f32(g.standard_normal((G, 64, 192)) * 0.15)
    bh, cot = f32(g.standard_normal((G, 1, 192)) * 0.1), _cot(g, (G, T, B, 64), ones)
    hs, _, _, d_gi, d_wh, d_bh = _gru_reference(gi, wh, bh[:, 0], cot)
    return _case(dict(gi=gi, wh=wh, bh=bh), [hs], dict(gi=d_gi, wh=d_wh, bh=d_bh[:, None, :]), [cot])


@functools.lru_cache(maxsize=None)
def gru_parts_case(T, B, spp, n_parts, used, ones=False):
    """n_parts projection parts of spp sets; `used`: the parts whose states enter the loss (the others' cotangent is zero).
    inputs: gi time-major [T, G, B, 192] (part k = sets k * spp .. as [spp, T * B, 192]: set_major), wh [G, 64, 192], bh [G, 1, 192]."""
    G = spp * n_parts
    g = _rng(T, B, spp, n_parts, *sorted(used))
    gi, wh = f32(g.standard_normal((T, G, B, 192)) * 0.7), f32(g.standard_normal((G, 64, 192)) * 0.15)
    bh, cot = f32(g.standard_normal((G, 1, 192)) * 0.1), _cot(g, (G, T, B, 64), ones)
    for k in range(n_parts):
        if k not in used:
            cot[k * spp:(k + 1) * spp] = 0
    hs, _, _, d_gi, d_wh, d_bh = _gru_reference(gi, wh, bh[:, 0], cot)
    return _case(dict(gi=gi, wh=wh, bh=bh), [hs], dict(gi=d_gi, wh=d_wh, bh=d_bh[:, None, :]), [cot])


def set_major(gi, k, spp):
    """projection part k of a time-major gi [T, G, B, 3H] as the operator takes it: [spp, T * B, 3H], rows t * B + b"""
    T, G, B, H3 = gi.shape
    return np.ascontiguousarray(np.swapaxes(gi[:, k * spp:(k + 1) * spp], 0, 1)).reshape(spp, T * B, H3)


@functools.lru_cache(maxsize=None)
def gru_gates_case(R, H, ones=False):
    g = _rng(R, H)
    inputs = dict(gi=f32(g.standard_normal((R, 3 * H))), gh=f32(g.standard_normal((R, 3 * H))), h=f32(g.standard_normal((R, H))))
    cot = _cot(g, (R, H), ones)
    outs, grads = _evaluate(st_gru_cell, inputs, [cot])
    return _case(inputs, outs, grads, [cot])


@functools.lru_cache(maxsize=None)
def dueling_q_case(n, T, B, inner, K, ones=False):
    g = _rng(n, T, B, inner, K)
    rows = T * B * inner
    inputs = dict(a=f32(g.standard_normal((n, rows, K))), v=f32(g.standard_normal((n, rows, 1))))
    cot = _cot(g, (B, T, n, inner, K), ones)
    outs, grads = _evaluate(lambda a, v: st_dueling_q(a, v, B, T, inner), inputs, [cot])
    return _case(inputs, outs, grads, [cot])


@functools.lru_cache(maxsize=None)
def dueling_head_case(n, T, B, inner, K, E, H=64, bias="n1K", ones=False):
    """E = 0: the env head (no `other`, inner = 1)"""
    g = _rng(n, T, B, inner, K, E, H)
    TB = T * B
    inputs = dict(h=f32(g.standard_normal((n, TB, H)) * 0.5), w=f32(g.standard_normal((n, H + E, K + 1)) * 0.2),
                  b=f32(g.standard_normal((n, 1, K + 1) if bias == "n1K" else (1, 1, K + 1)) * 0.1))
    if E:
        inputs["other"] = f32(g.standard_normal((TB, inner, E)))
    cot = _cot(g, (B, T, n, inner, K), ones)
    outs, grads = _evaluate(lambda **kw: st_dueling_head(B=B, T=T, inner=inner, **kw), inputs, [cot])
    return _case(inputs, outs, grads, [cot])


CAT_SHAPES = (((3, 5, 4), (3, 5, 1), (3, 5, 7)), ((2, 6), (2, 3)))       # two groups of 3 and 2 tensors (last-axis concatenation)


@functools.lru_cache(maxsize=None)
def cat_case(used=(0,), ones=False):
    """th.cat(group, dim=-1) per group (homophily_agent.py:187,200); `used`: the outputs with a cotangent"""
    g = _rng(len(CAT_SHAPES), *used)
    inputs = {"t%d_%d" % (i, j): f32(g.standard_normal(sh)) for i, grp in enumerate(CAT_SHAPES) for j, sh in enumerate(grp)}
    cots = [_cot(g, grp[0][:-1] + (sum(s[-1] for s in grp),), ones) if i in used else None for i, grp in enumerate(CAT_SHAPES)]
    fn = lambda **kw: tuple(th.cat([kw["t%d_%d" % (i, j)] for j in range(len(grp))], dim=-1) for i, grp in enumerate(CAT_SHAPES))
    outs, grads = _evaluate(fn, inputs, cots)
    return _case(inputs, outs, grads, cots)


@functools.lru_cache(maxsize=None)
def row_sums_case(shape):
    g = _rng(*shape)
    inputs = dict(x=f32(g.standard_normal(shape)))
    outs, _ = _evaluate(lambda x: x.sum(-2), inputs, [None])
    return _case(inputs, outs, {}, [None])


@functools.lru_cache(maxsize=None)
def encode_case(R, V, ones=False):
    g = _rng(R, V)
    K = 6 * (V - 2) ** 2
    codes = g.integers(0, 4, (R, V, V)).astype(np.uint8)
    inputs = dict(codes=codes, conv_w=f32(g.standard_normal((6, 3, 3, 3)) * 0.2), conv_b=f32(g.standard_normal(6) * 0.1),
                  lin_w=f32(g.standard_normal((32, K)) * (0.5 / np.sqrt(K))), lin_b=f32(g.standard_normal(32) * 0.1))
    cot = _cot(g, (R, 32), ones)
    outs, grads = _evaluate(st_encode, inputs, [cot])
    return _case(inputs, outs, grads, [cot])


def rerun_is_identical(case_fn, *args):
    """the statement alone reproduces itself to 1e-12 when evaluated again (a fresh, uncached evaluation)"""
    a, b = case_fn(*args), case_fn.__wrapped__(*args)
    for x, y in zip(a["outs"], b["outs"]):
        assert np.abs(x - y).max() <= 1e-12
    for k in a["grads"]:
        assert np.abs(a["grads"][k] - b["grads"][k]).max() <= 1e-12


def tensors(case, device, names=None, requires=()):
    """the case's inputs as fresh leaf tensors on `device` (f32 / their integer dtype), requires_grad for the names in `requires`"""
    out = {}
    for k, v in case["inputs"].items():
        if names is not None and k not in names:
            continue
        t = th.tensor(np.array(v), device=device)
        out[k] = t.requires_grad_(True) if k in requires else t
    return out
