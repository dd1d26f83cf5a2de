"""CPU suite of training windows from the rollout's stored recurrent state (config key train_stored_state; ssd_store_hidden,
ssd_gru_seq_fwd_h0 / _bwd_h0): the chain identity of the tensor-op recurrence (a window evaluated from the stored state is the same
slice of the whole unroll) with its gradients against autograd of a plain unroll, the CPU learner on gathered windows against the slice
of its whole-episode Q-values -- with the key off the same windows must MISS the slice, so the identity cannot pass vacuously --, the
exports' declarations as compiled and refusals, the setup and operator refusals, and the key off as today's scheme."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, ops, run
from tests import train_window_util as W
from tests.learner_util import build, load_fixture
from tests.stored_state_util import gru_case, gru_unroll_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. chain identity of the tensor-op path ---------------------------------------------------------------------------------------------
def test_tensor_op_window_from_a_stored_state_is_the_slice_of_the_whole_unroll():
    T, G, B = 9, 3, 5
    gi, wh, bh, _, wout = gru_case(T, G, B, seed=3)
    hs = ops.gru_sequence(gi, wh, bh)
    for t0 in (0, 1, 4, 8):
        g2, w2, b2 = gi[t0:].clone().requires_grad_(), wh.clone().requires_grad_(), bh.clone().requires_grad_()
        h0 = hs[:, t0].clone()
        win = ops.gru_sequence(g2, w2, b2, h0=h0)
        assert th.equal(win, hs[:, t0:]) and th.equal(win[:, 0], h0), t0
        ref, grads = gru_unroll_ref(gi[t0:], wh, bh, h0, wout[:, t0:])
        assert float((win.detach().double() - ref).abs().max()) < 1e-5
        if T - t0 > 1:
            (win * wout[:, t0:]).sum().backward()
            for x, r, name in zip((g2, w2, b2), grads, ("d_gi", "d_wh", "d_bh")):
                err = float((x.grad.double() - r).abs().max())
                print("t0 = %d %s: max error %.3e" % (t0, name, err))
                assert err < 2e-5 * max(1.0, float(r.abs().max())), (t0, name)
            assert not g2.grad[0].any()                                       # the projections of step 0 are not read
        else:
            assert not win.requires_grad                                      # one row: loaded, nothing computed
    parts = [gi[:, :2].permute(1, 0, 2, 3).reshape(2, T * B, 192), gi[:, 2:].permute(1, 0, 2, 3).reshape(1, T * B, 192)]
    with pytest.raises(ValueError, match="equally sized"):
        ops.gru_sequence_parts(parts, T, B, wh, bh, h0=hs[:, 0])
    parts = [gi[:, k:k + 1].permute(1, 0, 2, 3).reshape(1, T * B, 192) for k in range(3)]
    got = th.cat(ops.gru_sequence_parts([p[:, 4 * B:] for p in parts], T - 4, B, wh, bh, h0=[hs[k:k + 1, 4] for k in range(3)]), dim=0)
    assert th.equal(got, hs[:, 4:])


# ---- 2. the CPU learner: window against slice -------------------------------------------------------------------------------------------
WINDOW, ROWS = 5, [4, 1, 6, 3]


@pytest.fixture(scope="module")
def whole():
    """the x4-weights Cleanup-5 fixture (4 episodes of 13 slots), its whole-episode states written into "hidden", held in a buffer
    among decoys"""
    z, meta = load_fixture("learner_cleanup5_w4.npz")
    args, batch, mac, learner = build(z, meta)
    assert batch.max_seq_length == 13 and args.n_agents == 5 and not getattr(args, "train_stored_state", False)
    with th.no_grad():
        shared = mac.unroll_shared(batch)
        parts, wh, bh = mac.unroll_pre(batch, shared)
        he, hi = ops.gru_sequence_parts(parts, 13, batch.batch_size, wh, bh)                  # [n, T, B, H] each
        q_env, q_inc = mac.agent.unroll_post(he, hi, shared["other"])
        assert th.equal(q_env, mac.unroll(batch)[0])
    batch.scheme["hidden"] = {"vshape": (128,), "group": "agents", "dtype": th.float32}
    batch.data.transition_data["hidden"] = th.cat([he, hi], dim=-1).permute(2, 1, 0, 3).contiguous()      # [B, T, n, 128]
    buf = W.buffer_of(batch, rows=ROWS, size=8, norm="episode")
    return SimpleNamespace(args=args, mac=mac, learner=learner, buf=buf, q_env=q_env, q_inc=q_inc)


@pytest.mark.parametrize("t0", [0, 1, 7])
def test_cpu_learner_window_from_the_stored_state_is_the_slice(whole, t0):
    win = whole.buf.gather_windows(ROWS, [t0] * 4, WINDOW, 0)
    assert win["hidden"].shape == (4, WINDOW + 1, 5, 128)
    sl = slice(t0, t0 + WINDOW + 1)
    try:
        whole.args.train_stored_state = True
        with th.no_grad():
            q_env, q_inc = whole.mac.unroll(win)
            pair = whole.learner.unroll_pair(win)
    finally:
        whole.args.train_stored_state = False
    for name, got, ref in (("q_env", q_env, whole.q_env[:, sl]), ("q_inc", q_inc, whole.q_inc[:, sl])):
        err = float((got - ref).abs().max())
        print("t0 = %d, key on, %s: max difference to the slice %.3e" % (t0, name, err))
        assert err < 1e-5, (name, t0)
    # the live and the target net (equal weights here) both start from the stored state
    assert th.equal(pair[0], q_env) and th.equal(pair[1], q_inc) and th.equal(pair[2], q_env) and th.equal(pair[3], q_inc)
    h = win["hidden"][:, 0]
    assert th.equal(whole.learner.last_first_states[0], h[..., :64].transpose(0, 1)) and th.equal(whole.learner.last_first_states[1], h[..., 64:].transpose(0, 1))
    # teeth: from zeros (the key off) the same window misses the slice at row 0 wherever it starts mid-episode
    with th.no_grad():
        z_env, z_inc = whole.mac.unroll(win)
    for name, got, ref in (("q_env", z_env, whole.q_env[:, sl]), ("q_inc", z_inc, whole.q_inc[:, sl])):
        miss = float((got[:, 0] - ref[:, 0]).abs().max())
        print("t0 = %d, key off, %s: row 0 misses the slice by %.3e" % (t0, name, miss))
        if t0 > 0:
            assert miss > 1e-3, (name, t0)
        else:
            assert miss < 1e-5, (name, t0)


# ---- 3. exports, operator contract, setup -------------------------------------------------------------------------------------------------
NAMES = {"ssd_store_hidden", "ssd_gru_seq_fwd_h0", "ssd_gru_seq_bwd_h0"}


def test_exports_are_declared_exported_and_mirrored():
    """declaration, export and argtypes of every name of the table: tests/test_abi_symbols.py"""
    assert "#define SSD_ABI_VERSION 10" in open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    assert NAMES <= set(abi.HIP_SIGNATURES)
    assert abi.load_library().ssd_abi_version() == abi.ABI_VERSION == 10     # three exports more, no version change


def test_struct_size_and_declarations_as_compiled(tmp_path):
    """the three declarations are usable from C (sizeof / offsetof: tests/test_abi_symbols.py)"""
    c = tmp_path / "s.c"
    c.write_text('#include "ssd_hip.h"\nint main(){\n'
                 'int (*f)(const ssd_store_hidden_args*, void*) = ssd_store_hidden;\n'
                   'int (*g)(const float* const*, int32_t, const float* const*, const float* const*, int32_t, const float* const*, int64_t, int64_t, float*,'
                   ' float*, float*, int32_t, int32_t, int32_t, void*) = ssd_gru_seq_fwd_h0;\n'
                   'int (*h)(const float* const*, const float*, const float*, const float*, const float* const*, int32_t, float* const*, int32_t, float*,'
                   ' float*, float*, int32_t, int32_t, int32_t, int32_t, void*) = ssd_gru_seq_bwd_h0;\nreturn f == 0 || g == 0 || h == 0;}')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "s.o")])   # the declarations are usable
    # the argument counts of the two sequence exports as the header declares them
    assert len(abi.HIP_SIGNATURES["ssd_gru_seq_fwd_h0"][1]) == 15 and len(abi.HIP_SIGNATURES["ssd_gru_seq_bwd_h0"][1]) == 16


P = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched (the checks run before any launch)


def test_invalid_launches_are_refused_with_a_message_that_names_the_function():
    lib = abi.load_library()
    INV = abi.SSD_ERR_INVALID

    def store(**kw):
        a = abi.SsdStoreHiddenArgs()
        a.t_index, a.n_env, a.n_agents, a.t_slots, a.h_env, a.h_inc, a.src_agent_stride, a.src_env_stride, a.dst = P, 3, 5, 4, P, P, 192, 64, P
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ssd_store_hidden(C.byref(a), None)
    assert lib.ssd_store_hidden(None, None) == INV and b"ssd_store_hidden" in lib.ssd_last_error()
    for kw in (dict(t_index=None), dict(h_env=None), dict(h_inc=None), dict(dst=None), dict(n_env=0), dict(n_agents=0), dict(t_slots=0), dict(dst=P + 4),
               dict(h_inc=P + 8), dict(src_agent_stride=190), dict(src_env_stride=2), dict(src_env_stride=-64)):
        assert store(**kw) == INV, kw
        assert b"ssd_store_hidden" in lib.ssd_last_error(), kw
    one = lambda p=P: (C.c_void_p * 1)(p)

    def fwd(gi=P, n_parts=1, h0=P, ss=64, rs=64, hs=P, rzn=None, ghn=None, T=3, G=2, B=16):
        return lib.ssd_gru_seq_fwd_h0(one(gi), n_parts, one(), one(), 1, one(h0), ss, rs, hs, rzn, ghn, T, G, B, None)
    for kw in (dict(h0=None), dict(h0=P + 4), dict(ss=66), dict(rs=-64), dict(rs=3), dict(B=21), dict(T=0), dict(gi=None), dict(hs=None), dict(rzn=P),
               dict(n_parts=5), dict(n_parts=-1), dict(G=0)):
        assert fwd(**kw) == INV, kw
        assert b"ssd_gru_seq_fwd_h0" in lib.ssd_last_error(), kw
    assert lib.ssd_gru_seq_fwd_h0(one(), 1, one(), one(), 1, None, 64, 64, P, None, None, 3, 2, 16, None) == INV

    def bwd(dhs=P, d_gi=P, n_parts=1, T=3, G=2, Gn=2, B=16, dgh=P):
        return lib.ssd_gru_seq_bwd_h0(one(dhs), P, P, P, one(), 1, one(d_gi), n_parts, dgh, P, P, T, G, Gn, B, None)
    for kw in (dict(dhs=None), dict(d_gi=P + 4), dict(B=8), dict(Gn=3), dict(Gn=0), dict(T=0), dict(dgh=None), dict(n_parts=5)):
        assert bwd(**kw) == INV, kw
        assert b"ssd_gru_seq_bwd_h0" in lib.ssd_last_error(), kw


def test_ops_refuse_a_state_that_does_not_fit_and_name_the_argument():
    T, G, B = 3, 2, 4
    gi, wh, bh, h0, _ = gru_case(T, G, B, seed=1)
    with pytest.raises(ValueError, match=r"gru_sequence: h0 requires a gradient"):
        ops.gru_sequence(gi, wh, bh, h0=h0.clone().requires_grad_())
    with pytest.raises(ValueError, match=r"gru_sequence: h0 \(2, 5, 64\)"):
        ops.gru_sequence(gi, wh, bh, h0=th.zeros(G, B + 1, 64))
    parts = [gi[:, k:k + 1].permute(1, 0, 2, 3).reshape(1, T * B, 192) for k in range(G)]
    with pytest.raises(ValueError, match=r"gru_sequence_parts: h0 requires a gradient"):
        ops.gru_sequence_parts(parts, T, B, wh, bh, h0=[h0[:1], h0[1:].clone().requires_grad_()])
    with pytest.raises(ValueError, match=r"h0 comes as 1 parts for 2"):
        ops.gru_sequence_parts(parts, T, B, wh, bh, h0=[h0[:1]])
    with pytest.raises(ValueError, match=r"gru_sequence_parts: h0\[1\] \(1, 4, 32\)"):
        ops.gru_sequence_parts(parts, T, B, wh, bh, h0=[h0[:1], h0[1:, :, :32]])
    # every needs_input_grad combination is answered: the gradient arrives exactly where it was asked for
    for mask in range(8):
        xs = [x.clone().requires_grad_(bool(mask >> k & 1)) for k, x in enumerate((gi, wh, bh))]
        out = ops.gru_sequence(xs[0], xs[1], xs[2], h0=h0)
        assert out.requires_grad == bool(mask)
        if mask:
            out.sum().backward()
        assert [x.grad is not None for x in xs] == [bool(mask >> k & 1) for k in range(3)]
    with pytest.raises(ValueError, match="dst"):
        ops.store_hidden_args(th.zeros(1, dtype=th.long), th.zeros(5, 3, 64), th.zeros(5, 3, 64), th.zeros(3, 4, 5, 128))      # host tensors: no launch


BASE = dict(runner="hip_graph", train_window=5, buffer_cpu_only=False, use_cuda=True, rnn_hidden_dim=64)


@pytest.mark.parametrize("keys,match", [(dict(train_window=0), "train_window > 0"), (dict(runner="hip_vec"), "runner hip_graph"),
                                        (dict(runner="episode"), "runner hip_graph"), (dict(buffer_cpu_only=True), "device-resident"),
                                        (dict(use_cuda=False), "device-resident"), (dict(rnn_hidden_dim=32), "rnn_hidden_dim 64")])
def test_setup_refuses_the_key_where_it_cannot_work(keys, match):
    with pytest.raises(ValueError, match="train_stored_state.*" + match):
        run._check_stored_state(SimpleNamespace(**dict(BASE, train_stored_state=True, **keys)))
    a = SimpleNamespace(**dict(BASE, train_stored_state=False, **keys))
    assert run._check_stored_state(a) is False                                # off: nothing is asked of the other keys


def test_key_defaults_to_off_and_the_scheme_has_no_hidden_field_without_it():
    assert run.load_config("cleanup")["train_stored_state"] is False
    a = SimpleNamespace(**BASE)
    assert run._check_stored_state(a) is False and a.train_stored_state is False
    assert run._check_stored_state(SimpleNamespace(**dict(BASE, train_stored_state=True, train_burn_in=2))) is True
    info = dict(state_shape=7, obs_shape=(3, 15, 15), obs_dims=(15, 15), n_actions=9)
    for keys, has in (({}, False), (dict(train_stored_state=False), False), (dict(train_stored_state=True), True)):
        args = SimpleNamespace(ind_reward=True, n_agents=5, n_actions=9, name="homophily", rnn_hidden_dim=64, **keys)
        scheme, groups, _ = run.build_scheme(args, info)
        assert ("hidden" in scheme) == has
        if has:
            assert scheme["hidden"] == {"vshape": (128,), "group": "agents", "dtype": th.float32}
    off, absent = (run.build_scheme(SimpleNamespace(ind_reward=True, n_agents=5, n_actions=9, name="homophily", rnn_hidden_dim=64, **k), info)[0]
                   for k in (dict(train_stored_state=False), {}))
    assert off == absent
