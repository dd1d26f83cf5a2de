"""Host side of obs_others_last_action on the fused rollout heads (config key fused_others_last_action; CPU suite).

  * all 128 _build_inputs flag combinations: the rollout flag word, the dense width and FastPolicy.supports with the key on, and
    today's values with the key off;
  * the argument refusals of ssd_policy_head_env / _inc / _inc_encode / ssd_policy_pack_head for bit 64: every one of those checks
    runs before any device call, so they are pinned here with dummy non-null addresses (as test_learner_abi_refusals.py does for the
    learner exports) -- the GPU file only repeats the one that needs a real launch to follow it;
  * the reference fixture tests/golden/rollout_others_cleanup5.npz through the torch controller (the GPU file drives the kernels
    over the same numbers).
"""
import ctypes as C
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from homophily_marl_amd.fast_policy import plan_rollout
from tests.policy_cases import dummy_head as _head

NAMES = ["obs_last_action", "obs_agent_id", "obs_reward", "obs_inc_reward", "obs_distance", "obs_agent_pos", "obs_others_last_action"]
BITS = [1, 2, 4, 8, 16, 32, 64]


def _base(name):
    from tests.learner_util import build, load_fixture
    z, meta = load_fixture(name)
    args, batch, _, _ = build(z, meta)
    return args, batch


@pytest.mark.parametrize("name", ["learner_cleanup5.npz", "learner_harvest5.npz"])
def test_rollout_flag_word_and_support_for_every_flag_combination(name):
    """Key on: rollout_input_flags is the seven-bit word, the dense width is input_shape less the others' block, and supports() is true
    exactly when dense + A <= 64 (or the set is the shipped one), with and without bit 64.  Key off: input_flags / supports are what
    they were (None / False with obs_others_last_action).  The widths are recomputed here by the reference's _get_input_shape rule."""
    from homophily_marl_amd.controllers import REGISTRY as mac_REGISTRY
    args, batch = _base(name)
    lib = abi.load_library()
    n, A = args.n_agents, args.n_actions
    widths = [A, n, 1, 1, n, 2, n * A]
    seen = 0
    for on in itertools.product([False, True], repeat=7):
        full = 32 + sum(w for w, o in zip(widths, on) if o)
        dense = full - (n * A if on[6] else 0)
        word = sum(b for b, o in zip(BITS, on) if o)
        mk = lambda key: mac_REGISTRY[args.mac](batch.scheme, {"agents": n},
                                                SimpleNamespace(**dict(vars(args), fused_others_last_action=key, **dict(zip(NAMES, on)))))
        mac = mk(True)
        assert mac.input_shape == full
        assert mac.rollout_input_flags == word and mac.input_flags_all == word
        assert mac.input_flags == (None if on[6] else word)                    # untouched by the key
        assert plan_rollout(mac).supported == (mac.shipped_flags or dense + A <= 64), (on, dense)
        assert plan_rollout(mac, fused=False).supported == mac.shipped_flags
        off = mk(False)
        assert off.input_flags == (None if on[6] else word) and off.rollout_input_flags == off.input_flags
        assert plan_rollout(off).supported == (off.shipped_flags or (not on[6] and full + A <= 64)), on
        assert lib.ssd_build_inputs_width(n, A, abi.INPUT_EXPLICIT | word) == full - 32
        seen += on[6] and plan_rollout(mac).supported
    assert seen == 64                      # n = 5: every set with the block fits (dense <= 55)


SHIPPED = 1 | 2 | 4 | 8 | 32


def test_heads_refuse_bad_others_last_action_arguments_before_any_launch():
    """Every row returns from the argument check: the addresses are dummies, so a launch would fault."""
    lib = abi.load_library()
    P = 1 << 20
    for fn, inc in ((lib.ssd_policy_head_env, False), (lib.ssd_policy_head_inc, True)):
        a = _head()
        a.input_flags = abi.INPUT_EXPLICIT | SHIPPED | 64
        a.input_shape = 32 + 18 + 45
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # null table / record
        a.others_rows = P
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # record still missing
        a.others_rows, a.prev_record = P + 4, P
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # alignment
        a.others_rows, a.prev_record, a.prev_record_out = P, P, P
        assert fn(C.byref(a), None) == abi.SSD_ERR_INVALID                     # writes the buffer it reads (inc: writes at all)
        a.prev_record_out = None
        a.input_shape = 50                                                     # width without the block
        assert fn(C.byref(a), None) == abi.SSD_ERR_UNSUPPORTED
        a.input_shape = 32 + 18 + 45 + 5                                       # + obs_distance not flagged
        assert fn(C.byref(a), None) == abi.SSD_ERR_UNSUPPORTED
        b = _head(n=10)                                                        # n = 10 with all seven blocks: dense 65 columns
        b.others_rows, b.prev_record = P, P
        b.input_flags = abi.INPUT_EXPLICIT | 127
        b.input_shape = 32 + 9 + 10 + 1 + 1 + 10 + 2 + 90
        assert fn(C.byref(b), None) == abi.SSD_ERR_UNSUPPORTED
        b.input_flags = abi.INPUT_EXPLICIT | 255
        assert fn(C.byref(b), None) == abi.SSD_ERR_UNSUPPORTED                 # a bit no head builds
    a = _head()
    a.input_flags, a.input_shape, a.others_rows, a.prev_record = abi.INPUT_EXPLICIT | SHIPPED | 64, 95, P, P
    e = abi.SsdPolicyEncodeArgs()
    assert lib.ssd_policy_head_inc_encode(C.byref(a), C.byref(e), None) == abi.SSD_ERR_UNSUPPORTED
    assert b"obs_others_last_action" in lib.ssd_last_error()


def test_pack_head_refuses_bad_others_last_action_arguments_before_any_launch():
    lib = abi.load_library()
    P = 1 << 20
    hp = abi.SsdPolicyHeadParams()
    for f in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc2_v_w", "fc2_v_b"):
        setattr(hp, f, P)
    for k in range(3):
        hp.w_i[k] = hp.w_h[k] = hp.b_i[k] = hp.b_h[k] = P
    hp.n_agents, hp.fc1_in, hp.fc2_in, hp.fc2_out = 5, 95, 64, 9
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_UNSUPPORTED     # 95 rows without the flag: as before
    hp.input_flags = abi.INPUT_EXPLICIT | SHIPPED | 64
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_INVALID         # n_actions missing
    hp.n_actions = 9
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_INVALID         # null others_rows
    hp.others_rows = P + 8
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_INVALID         # alignment
    hp.others_rows = P
    hp.fc1_in = 45 + 40                                                                     # narrower than the blocks in front of the block
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_UNSUPPORTED
    hp.n_agents, hp.fc1_in, hp.input_flags = 10, 32 + 33 + 90, abi.INPUT_EXPLICIT | 127       # dense 65
    assert lib.ssd_policy_pack_head(C.byref(hp), 2, P, None) == abi.SSD_ERR_UNSUPPORTED


def load_others_fixture(device="cpu", key=True):
    """(z, args, batch, mac) of tests/golden/rollout_others_cleanup5.npz: the base learner fixture's batch and weights, the recorded
    wider fc1 layers loaded on top."""
    from tests.learner_util import GOLDEN, build, load_fixture
    z = np.load(os.path.join(GOLDEN, "rollout_others_cleanup5.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    zb, mb = load_fixture(meta["base"])
    files = _Files({k: zb[k] for k in zb.files})
    files["w_fc1_env_w"], files["w_fc1_inc_w"] = z["fc1_env_w"], z["fc1_inc_w"]
    args, batch, mac, _ = build(files, mb, device=device, overrides=dict(meta["overrides"], fused_others_last_action=key))
    assert mac.input_shape == meta["input_shape"]
    return z, meta, args, batch, mac


class _Files(dict):
    files = property(lambda self: list(self))


def test_reference_fixture_through_the_torch_controller():
    """The recorded q_env / q_inc are the REFERENCE's (tools/gen_rollout_others_golden.py); this package's torch controller, stepped
    the same way on the CPU, reproduces them: the fixture is pinned where no GPU is needed."""
    z, meta, args, batch, mac = load_others_fixture()
    B = batch.batch_size
    mac.init_hidden(B)
    with th.no_grad():
        for t in range(meta["steps"]):
            q_env, q_inc, _ = mac.forward(batch, t)
            de = (q_env.reshape(B, args.n_agents, -1) - th.as_tensor(z["q_env"][:, t])).abs().max().item()
            di = (q_inc.reshape(B, args.n_agents, args.n_agents, -1) - th.as_tensor(z["q_inc"][:, t])).abs().max().item()
            assert de < 1e-5 and di < 1e-5, (t, de, di)
