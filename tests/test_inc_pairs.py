"""The inc head's epilogue items are the PARTNER pairs only (csrc/ssd_policy_mfma.hip, IncItems): 16 (n - 1) items per 16-row tile, 64 per
pass, the self pair a constant 0 stored without an evaluation -- except that a launch with q_out still writes the self pairs' Q values.

Cases: the standalone inc head (ssd_policy_head_inc) and the fused launch (ssd_policy_head_inc_encode, 15 x 15 windows) at
  n in {1, 2, 3, 5, 6, 10}: 0, 16, 32, 64, 80, 144 partner items -- no pass, a partial first pass, half a pass, exactly one pass, a
                            second pass of 16 live lanes, three passes;
  N in {37, 130}:           a ragged last tile (5 and 2 rows), and 9 tiles = two workgroups per agent;
  epsilon in {0, 1, 0.3}.
Each case launches twice on the same counters and seed, with q_out and without, every output inside a poisoned arena
(tests/arena_util.py), and asserts
  * both launches leave the same actions_inc, prev_actions_inc_out, recv_inc_out bytes and filed dst_actions_inc;
  * q_out is within 1e-5 (tests/test_policy_mfma.py's bar) of the torch f32 controller for all n x n pairs, self pairs included;
  * every pick equals the host restatement of the draw contract (tests/explore_util.py) applied to the launch's OWN q_out;
  * self pairs are 0 in all four outputs; the time slots other than *t_index, the record bytes from n on, and every band around the
    outputs keep their fill."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

from homophily_marl_amd import abi
from tests import arena_util as au
from tests import explore_util as xu

TOL_Q = 1e-5
SEED, BASE, STEP = 0x2545F491, 4096 * 7 + 3, 17
V, A = 15, 9
SLOTS, SLOT = 3, 1
NS = (1, 2, 3, 5, 6, 10)
ENVS = (37, 130)
EPSILONS = (0.0, 1.0, 0.3)
CASES = [(launch, n, N) for launch in ("head", "fused") for n in NS for N in ENVS]


def test_partner_items_cover_every_pass_shape():
    """the arithmetic the case list rests on: items per tile, passes of 64, live lanes of the last pass"""
    shape = {n: (16 * (n - 1), -(-16 * (n - 1) // 64), (16 * (n - 1) - 1) % 64 + 1 if n > 1 else 0) for n in NS}
    assert shape == {1: (0, 0, 0), 2: (16, 1, 16), 3: (32, 1, 32), 5: (64, 1, 64), 6: (80, 2, 16), 10: (144, 3, 16)}
    for n in range(2, 11):          # item -> (row, partner j) as the kernel maps it: a bijection onto the off-diagonal pairs of a tile
        for agent in range(n):
            seen = set()
            for it in range(16 * (n - 1)):
                row, jj = divmod(it, n - 1)
                assert row == (it * ((65536 + n - 2) // (n - 1))) >> 16
                seen.add((row, jj + (jj >= agent)))
            assert seen == {(r, j) for r in range(16) for j in range(n) if j != agent}


@functools.lru_cache(maxsize=None)
def _mac(n):
    """the controller of n agents on the device, built without an env (window 15 x 15, 9 actions, the shipped input set)"""
    from homophily_marl_amd.components.episode_buffer import ReplayBuffer
    from homophily_marl_amd.controllers import REGISTRY as mac_REGISTRY
    from homophily_marl_amd.run import build_scheme, load_config
    args = SimpleNamespace(**load_config("cleanup", overrides=dict(use_cuda=True, env_args=dict(num_agents=n, view_size=V // 2))))
    args.device = "cuda:0"
    info = dict(n_agents=n, n_actions=A, state_shape=4, obs_shape=3 * V * V, state_dims=(25, 18), obs_dims=(V, V), episode_limit=SLOTS - 1)
    args.n_agents, args.n_actions = n, A
    args.state_shape, args.obs_shape, args.state_dims, args.obs_dims = info["state_shape"], info["obs_shape"], info["state_dims"], info["obs_dims"]
    scheme, groups, pre = build_scheme(args, info)
    buf = ReplayBuffer(scheme, groups, 1, SLOTS, preprocess=pre, device="cpu")
    th.manual_seed(100 + n)
    mac = mac_REGISTRY[args.mac](buf.scheme, groups, args)
    mac.cuda()
    assert mac.n_agents == n and mac.input_shape == 32 + A + n + 4
    return mac


@functools.lru_cache(maxsize=None)
def _inputs(n, N):
    """random inputs of one timestep and the torch f32 controller's Q values of the inc head, computed once per (n, N)"""
    mac = _mac(n)
    g = th.Generator(device="cuda").manual_seed(1000 * n + N)
    r = lambda *s: th.randn(*s, generator=g, device="cuda")
    d = dict(x=r(N, n, mac.input_shape) * 0.5, h0=r(N, n, 64) * 0.3, pos=th.rand(N, n, 2, generator=g, device="cuda") * 20.0,
             orient=th.randint(-1, 2, (N, n, 2), generator=g, device="cuda").float(),
             reward=th.randint(-1, 2, (N, n), generator=g, device="cuda").float(), clean=th.randint(0, 3, (N, n), generator=g, device="cuda").float(),
             den=th.rand(N, n, generator=g, device="cuda"), act=th.randint(0, A, (N, n), generator=g, device="cuda"),
             codes=th.randint(0, 4, (N, n, abi.code_agent_stride(V)), generator=g, device="cuda").to(th.uint8))
    with th.no_grad():
        q, _, _ = mac.agent.forward_inc(d["x"].reshape(N * n, -1), d["h0"].unsqueeze(2), F.one_hot(d["act"], A), d["pos"] / mac.pos_scale, d["orient"],
                                        d["reward"].unsqueeze(-1), d["clean"].unsqueeze(-1), d["den"].unsqueeze(-1))
    d["q_ref"] = q.reshape(N, n, n, 3).cpu().numpy()
    return d


def _launch(fp, launch, d, n, N, eps, want_q):
    """one launch with every output in a fresh poisoned arena: (arena, regions)"""
    ar = au.Arena()
    i64 = np.int64
    written_slot = np.zeros((N, SLOTS, n, n), dtype=bool)
    written_slot[:, SLOT] = True
    written_rec = np.zeros((n, N, 16), dtype=bool)
    written_rec[:, :, :n] = True
    reg = dict(actions=ar.reserve("out_actions", (N, n, n), i64, align=8), p_inc=ar.reserve("prev_actions_inc_out", (N, n, n), i64, align=8),
               recv=ar.reserve("recv_inc_out", (n, N, 16), np.uint8, align=16, written=written_rec),
               filed=ar.reserve("dst_actions_inc", (N, SLOTS, n, n), i64, align=8, written=written_slot))
    if want_q:
        reg["q"] = ar.reserve("q_out", (n, N, n, 3), np.float32, align=4)
    file = dict(out_actions=reg["actions"].ptr, prev_actions_inc_out=reg["p_inc"].ptr, recv_inc_out=reg["recv"].ptr, dst_actions_inc=reg["filed"].ptr,
                t_index=d["t_index"].data_ptr(), t_slots=SLOTS)
    if want_q:
        file["q_out"] = reg["q"].ptr
    fp.inputs_pair.zero_()
    fp.inputs_pair[0, :, :, :d["x"].shape[-1]] = d["x"].transpose(0, 1)
    fp.h_inc.copy_(d["h0"].transpose(0, 1))
    args = (d["act"], d["pos"], d["orient"], d["reward"], d["clean"], d["den"], eps, d["step"])
    if launch == "fused":
        fp.act_inc_encode(*args, d["codes"], buf=0, file=file, mask_alphabet=False)
    else:
        fp.act_inc(*args, buf=0, file=file)
    th.cuda.synchronize()
    ar.check()
    return {k: v.array().copy() for k, v in reg.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("launch,n,N", CASES, ids=["%s-n%d-N%d" % c for c in CASES])
def test_inc_head_evaluates_the_partner_pairs_only(launch, n, N):
    from homophily_marl_amd.fast_policy import FastPolicy
    mac = _mac(n)
    d = dict(_inputs(n, N))
    d["step"] = th.full((1,), STEP, dtype=th.long, device="cuda")
    d["t_index"] = th.full((1,), SLOT, dtype=th.long, device="cuda")
    fp = FastPolicy(mac, N, th.ones(A, dtype=th.uint8), seed=SEED, precision=2, env_id_base=BASE)
    assert fp.fused and fp.fused_enc and fp.inc_encode and fp.V == V and fp.bands == 1
    tiles = (N + 15) // 16
    assert abi.policy_head_plan(N, n, 1 if launch == "fused" else 0)[2] == 1 and (tiles > 8) == (N == 130)
    keys = xu.inc_keys(N, n, BASE)
    diag = np.broadcast_to(np.eye(n, dtype=bool), (N, n, n))
    for eps_value in EPSILONS:
        eps = th.full((), eps_value, device="cuda")
        with_q = _launch(fp, launch, d, n, N, eps, True)
        without = _launch(fp, launch, d, n, N, eps, False)
        label = (launch, n, N, eps_value)
        for name in ("actions", "p_inc", "recv", "filed"):
            assert (with_q[name] == without[name]).all(), (label, name)
        act = with_q["actions"]
        q = np.swapaxes(with_q["q"], 0, 1)                                # [N, n(i), n(j), 3]
        err = float(np.abs(q - d["q_ref"]).max())
        print("%s n=%d N=%d eps=%.1f: max |q_out - torch f32| %.2e over %d pairs (%d self)" % (launch, n, N, eps_value, err, q[..., 0].size, N * n))
        assert err < TOL_Q, (label, err)
        want, flag = xu.expected_actions(SEED ^ xu.INC_SEED_XOR, STEP, keys, eps_value, 0b111, 3, q, zero_diagonal=True)
        bad = act != want
        assert not bad.any(), (label, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        off = ~diag
        assert flag[off].all() if eps_value >= 1 else (not flag.any() if eps_value == 0 else (n == 1 or 0 < flag[off].sum() < off.sum()))
        # the self pairs: 0 in every output
        assert (act[diag] == 0).all() and (with_q["p_inc"][diag] == 0).all() and (with_q["filed"][:, SLOT][diag] == 0).all(), label
        assert (with_q["p_inc"] == act).all() and (with_q["filed"][:, SLOT] == act).all(), label
        rec = with_q["recv"][:, :, :n]                                   # [j, b, i] = actions_inc[b, i, j]
        assert (rec == np.transpose(act, (2, 0, 1)).astype(np.uint8)).all(), label
        assert (rec[np.arange(n), :, np.arange(n)] == 0).all(), label
        if n > 1 and eps_value > 0:
            assert (act[off] > 0).any(), label                            # (the launch stores picks other than the self pairs' 0)
