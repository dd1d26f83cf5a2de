"""Host side of the gathered one-hot layout of the fused rollout heads (SSD_INPUT_GATHER_ONEHOT, config key fused_onehot_gather; CPU
suite).

  * the truth table of FastPolicy.supports over all 128 _build_inputs flag sets x n in {3, 5, 6, 10}: with the key off today's
    answers (the dense width decides), with the key on True everywhere -- n = 10 with all seven flags is the row that needs the
    feature;
  * the argument refusals of ssd_policy_head_env / _inc / _inc_encode / ssd_policy_pack_head for the new bit.  Every one of those
    checks runs before any device call, so they are pinned with dummy non-null addresses;
  * tests/golden/rollout_wide_cleanup10.npz (the REFERENCE controller with all seven flags at Cleanup-10) through this package's
    torch controller, so that the fixture the GPU file drives the kernels over is pinned where no GPU is needed.
"""
import ctypes as C
import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch as th

from homophily_marl_amd import abi
from homophily_marl_amd.fast_policy import FastPolicy, plan_rollout
from tests.policy_cases import dummy_head as _head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["obs_last_action", "obs_agent_id", "obs_reward", "obs_inc_reward", "obs_distance", "obs_agent_pos", "obs_others_last_action"]
BITS = [1, 2, 4, 8, 16, 32, 64]
SHIPPED = 1 | 2 | 4 | 8 | 32
GATHER = 0x100


def test_the_bit_is_above_the_unassigned_one_and_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    assert "#define SSD_INPUT_GATHER_ONEHOT 0x100u" in hdr
    assert abi.INPUT_GATHER_ONEHOT == GATHER and not GATHER & 0xFF
    assert abi.onehot_rows(10, 9, 127) == 1 + 18 + 90 and abi.onehot_rows(6, 9, SHIPPED | 16) == 19
    cfg = open(os.path.join(ROOT, "homophily_marl_amd", "config", "default.yaml")).read()
    assert "\nfused_onehot_gather: False" in cfg


def test_supports_truth_table_with_and_without_the_key():
    """Key off: supports is what it was -- the shipped set, or a dense row (+ the inc head's one-hot action) within 64 columns and no
    others' block.  Key on: True for every flag set at every team size; the flag word carries the bit exactly when the set holds a
    one-hot block (last action, agent id, others' last actions), else it stays the dense word, which always fits (46 + 9 columns).
    The widths are recomputed here by the reference's _get_input_shape rule."""
    from homophily_marl_amd.controllers import REGISTRY as mac_REGISTRY
    from tests.learner_util import build, load_fixture
    z, meta = load_fixture("learner_cleanup5.npz")
    args, batch, _, _ = build(z, meta)
    A = args.n_actions
    needs_feature = 0
    for n in (3, 5, 6, 10):
        widths = [A, n, 1, 1, n, 2, n * A]
        for on in itertools.product([False, True], repeat=7):
            full = 32 + sum(w for w, o in zip(widths, on) if o)
            word = sum(b for b, o in zip(BITS, on) if o)
            mk = lambda key: mac_REGISTRY[args.mac](batch.scheme, {"agents": n}, SimpleNamespace(
                **dict(vars(args), n_agents=n, fused_onehot_gather=key, **dict(zip(NAMES, on)))))
            off = mk(False)
            assert off.input_shape == full
            assert off.rollout_input_flags == off.input_flags == (None if on[6] else word)
            today = off.shipped_flags or (not on[6] and full + A <= 64)
            assert plan_rollout(off).supported == today, (n, on)
            mac = mk(True)
            assert mac.input_shape == full and mac.input_flags == off.input_flags            # untouched by the key
            assert mac.rollout_input_flags == ((word | GATHER) if word & (1 | 2 | 64) else word), (n, on)
            assert plan_rollout(mac).supported is True, (n, on)
            assert plan_rollout(mac, fused=False).supported == mac.shipped_flags
            needs_feature += not today
    assert needs_feature > 4 * 64                                                         # every set with bit 64, and the wide dense ones
    on = [True] * 7
    mac = mac_REGISTRY[args.mac](batch.scheme, {"agents": 10}, SimpleNamespace(**dict(vars(args), n_agents=10, fused_onehot_gather=True,
                                                                                     **dict(zip(NAMES, on)))))
    assert mac.input_shape == 155 and FastPolicy.supports(mac)                             # the row that fails without the feature


def test_heads_refuse_bad_gather_arguments_before_any_launch():
    """Every row returns from the argument check: the addresses are dummies, so a launch would fault."""
    lib = abi.load_library()
    P = 1 << 20
    wide = 32 + 9 + 6 + 1 + 1 + 6 + 2                                           # shipped + distance at n = 6: 57 columns, 66 with the inc one-hot
    for fn, inc in ((lib.ssd_policy_head_env, False), (lib.ssd_policy_head_inc, True)):
        a = _head(n=6)
        a.input_flags, a.input_shape = abi.INPUT_EXPLICIT | SHIPPED | 16, wide
        assert fn(C.byref(a), None) == abi.SSD_ERR_UNSUPPORTED                 # dense, as before: does not fit
        a.input_flags |= GATHER
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # the bit without its table
        a.prev_record = P
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # still no table (others_rows does not stand in for it)
        a.others_rows = P
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID
        a.others_rows, a.onehot_rows, a.prev_record = None, P, None
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # the record is missing
        a.onehot_rows, a.prev_record = P + 4, P
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # a misaligned table
        a.onehot_rows, a.prev_record = P, P + 8
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID
        a.onehot_rows, a.prev_record, a.prev_record_out = P, P, P
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # writes the buffer it reads (inc: writes at all)
        a.prev_record_out = None
        a.input_shape = wide - 6                                               # obs_distance flagged, its columns missing
        assert fn(C.byref(a), None) == abi.SSD_ERR_UNSUPPORTED
        a.input_shape = wide + 6 * 9                                           # the others' block not flagged
        assert fn(C.byref(a), None) == abi.SSD_ERR_UNSUPPORTED
        a.input_shape, a.input_flags = wide, a.input_flags | 128
        assert fn(C.byref(a), None) == abi.SSD_ERR_UNSUPPORTED                 # bit 128: still no head builds it
        a.input_flags, a.n_agents = (a.input_flags & ~128), 11
        a.input_shape = 32 + 9 + 11 + 1 + 1 + 11 + 2
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # more agents than a record holds
    a = _head(n=6)
    a.input_flags, a.input_shape, a.onehot_rows, a.prev_record = abi.INPUT_EXPLICIT | SHIPPED | 16 | GATHER, wide, P, P
    e = abi.SsdPolicyEncodeArgs()
    assert lib.ssd_policy_head_inc_encode(C.byref(a), C.byref(e), None) == abi.SSD_ERR_UNSUPPORTED
    assert b"SSD_INPUT_GATHER_ONEHOT" in lib.ssd_last_error()


def test_pack_head_refuses_bad_gather_arguments_before_any_launch():
    lib = abi.load_library()
    P = 1 << 20
    hp = abi.SsdPolicyHeadParams()
    for f in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc2_v_w", "fc2_v_b"):
        setattr(hp, f, P)
    for k in range(3):
        hp.w_i[k] = hp.w_h[k] = hp.b_i[k] = hp.b_h[k] = P
    full = 32 + 9 + 10 + 1 + 1 + 90 + 10 + 2                                    # all seven blocks at n = 10
    hp.n_agents, hp.fc1_in, hp.fc2_in, hp.fc2_out = 10, full, 64, 9
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_UNSUPPORTED     # 155 rows without a flag word: as before
    hp.input_flags, hp.n_actions, hp.others_rows = abi.INPUT_EXPLICIT | 127, 9, P
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_UNSUPPORTED     # dense 65 with bit 64 alone: as before
    hp.input_flags |= GATHER
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_INVALID         # a null snapshot pointer (others_rows is not it)
    hp.onehot_rows = P + 8
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_INVALID         # alignment
    hp.onehot_rows = P
    hp.n_actions = 0
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_INVALID         # n_actions missing
    hp.n_actions = 9
    for bad in (full - 1, full + 1, full + 8, 64):                                          # neither the env head's nor the inc head's width
        hp.fc1_in = bad
        assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_UNSUPPORTED, bad
    hp.fc1_in, hp.input_flags = full, hp.input_flags | 128
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_UNSUPPORTED


class _Files(dict):
    files = property(lambda self: list(self))


def load_wide_fixture(device="cpu", key=True):
    """(z, meta, args, batch, mac) of tests/golden/rollout_wide_cleanup10.npz.  The fixture holds no weights: they are drawn again from
    its seed (tools/gen_rollout_wide_golden.py draw_weights, numpy's frozen RandomState stream) and checked against the recorded
    per-tensor sums."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_rollout_wide_golden import checksums, draw_weights
    from tests.learner_util import GOLDEN, build
    z = np.load(os.path.join(GOLDEN, "rollout_wide_cleanup10.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    shapes = json.loads(bytes(z["weight_shapes"]).decode())
    assert list(shapes) == list(z["weight_names"])
    weights = draw_weights(shapes, meta["seed"])
    assert np.array_equal(checksums(weights), z["weight_sums"])
    files = _Files({k: z[k] for k in z.files if k.startswith("batch_")})
    files.update({"w_" + k: v for k, v in weights.items()})
    args, batch, mac, _ = build(files, meta, device=device, overrides=dict(meta["overrides"], fused_onehot_gather=key))
    assert mac.input_shape == meta["input_shape"] == 155 and args.n_agents == 10
    return z, meta, args, batch, mac


def test_wide_reference_fixture_through_the_torch_controller():
    """The recorded q_env / q_inc are the REFERENCE's; this package's torch controller, stepped the same way on the CPU, reproduces
    them within the project's bar (1e-5)."""
    z, meta, args, batch, mac = load_wide_fixture()
    B, n = batch.batch_size, args.n_agents
    assert B == 2 and meta["steps"] == 6 and mac.rollout_input_flags == 127 | GATHER and mac.input_flags is None
    assert np.abs(z["q_env"]).max() > 0.1 and np.abs(z["q_inc"]).max() > 0.1                # not a fixture of zeros
    mac.init_hidden(B)
    with th.no_grad():
        for t in range(meta["steps"]):
            q_env, q_inc, _ = mac.forward(batch, t)
            de = (q_env.reshape(B, n, -1) - th.as_tensor(z["q_env"][:, t])).abs().max().item()
            di = (q_inc.reshape(B, n, n, -1) - th.as_tensor(z["q_inc"][:, t])).abs().max().item()
            assert de < 1e-5 and di < 1e-5, (t, de, di)
