"""CPU suite: the learner's td_lambda option (TD(lambda) targets for both heads) against the reference's own recursion, recorded in
tests/golden/learner_td_lambda.npz by tools/gen_td_lambda_golden.py (utils/rl_utils.py:4-14 build_td_lambda_targets): the helper the
tensor-op loss uses, the tensor-op learner, the numpy statement the GPU suite holds the kernel to, the identity at a lambda too small to
be seen, the refusals, and the struct member."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from homophily_marl_amd.learners.homophily_learner import lambda_returns
from tests import td_lambda_util as U
from tests.learner_util import build, load_fixture
from tests.test_learner_options import perturb_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 2.0 ** -100
Z, META = U.load_golden()
B_CASES = [c["name"] for c in META["b_cases"]]


def within(got, ref, rel):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool((np.abs(got - ref) <= rel * np.maximum(1.0, np.abs(ref))).all())


def test_fixture_holds_the_stated_cases():
    assert META["a_T"] == [1, 2, 12, 63, 64, 65, 255, 256, 257, 513] and META["a_gammas"] == [0.95, 0.995]
    assert META["a_lambdas"] == [TINY, 0.5, 0.8, 1.0] and META["b_lambdas"] == [0.5, 0.8, 1.0]
    assert {(c["base"], c["overrides"]["double_q"], c["overrides"]["consider_others_inc"]) for c in META["b_cases"]} == \
        {(b, dq, oth) for b in ("learner_cleanup5.npz", "learner_harvest5.npz") for dq in (True, False) for oth in (True, False)}
    assert all(Z[k].dtype != object for k in Z.files)
    term = Z["A/T12/terminated"][..., 0]
    assert not term[0].any() and term[1].argmax() == 4 and term[2].argmax() == 11 and term.sum() == 2
    assert Z["A/T12/mask"][1, :, 0].tolist() == [1.0] * 5 + [0.0] * 7


@pytest.mark.parametrize("T", META["a_T"])
def test_helper_reproduces_the_reference_recursion(T):
    """lambda_returns on the recorded inputs, every (gamma, lambda): the same f32 recursion in the same order, so 1e-6 relative -- and
    exact at lambda = 2^-100."""
    r, term, mask, v = (th.as_tensor(Z["A/T%d/%s" % (T, k)]) for k in ("rewards", "terminated", "mask", "target_qs"))
    for gi, gamma in enumerate(META["a_gammas"]):
        for li, lam in enumerate(META["a_lambdas"]):
            ref = Z["A/T%d/g%d_l%d/ret" % (T, gi, li)]
            got = lambda_returns(r, term, mask, v, gamma, lam).numpy()
            assert got.dtype == np.float32 and within(got, ref, 1e-6), (T, gamma, lam, float(np.abs(got - ref).max()))
            if lam == TINY:
                assert np.array_equal(got, ref), (T, gamma)
                one_step = mask.numpy() * (r.numpy() + np.float32(gamma) * v.numpy()[:, 1:] * (1 - term.numpy()))
                assert within(got, one_step, 1e-6)


def _raw_arrays(batch, qs):
    sq = lambda k: batch[k].squeeze(-1).numpy()
    arr = dict(zip(("q_env", "q_inc", "tq_env", "tq_inc"), (q.detach().numpy() for q in qs)))
    arr.update(avail=batch["avail_actions"].numpy(), actions=sq("actions"), actions_inc=sq("actions_inc"), reward=batch["reward"].numpy(),
               clean_num=batch["clean_num"].numpy(), terminated=sq("terminated"), filled=sq("filled"))
    return arr


@pytest.mark.parametrize("name", B_CASES)
def test_tensor_op_learner_matches_the_reference_returns(name):
    """Group (B): the tensor-op learner's lambda-returns of both heads and its two value losses, every recorded lambda, within the
    project's fp32 bar 1e-5 max(1, |ref|); and the numpy statement of tests/td_lambda_util.py on the same Q-values."""
    c = next(c for c in META["b_cases"] if c["name"] == name)
    z, meta = load_fixture(c["base"])
    for li, lam in enumerate(META["b_lambdas"]):
        args, batch, mac, learner = build(z, meta, overrides=dict(c["overrides"], td_lambda=lam))
        assert args.td_lambda == lam and not learner._fused(batch)
        perturb_target(learner)
        with th.no_grad():
            arr = _raw_arrays(batch, learner.unroll_pair(batch))
        logs = learner.cal_loss_and_step(batch)
        for h, got in zip(("env", "inc"), learner.last_lambda_returns):
            ref = Z["B/%s/l%d/ret_%s" % (name, li, h)]
            assert got.shape == ref.shape and within(got.numpy(), ref, 1e-5), (lam, h, float(np.abs(got.numpy() - ref).max()))
            ref_loss = float(Z["B/%s/l%d/loss_value_%s" % (name, li, h)])
            assert abs(float(logs["loss_value_" + h]) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (lam, h, float(logs["loss_value_" + h]), ref_loss)
        p = U.host_rows(arr["q_env"], arr["q_inc"], arr["tq_env"], arr["tq_inc"], arr["avail"], arr["actions"], arr["actions_inc"], arr["reward"],
                        arr["terminated"], arr["filled"], args.double_q, args.consider_others_inc, args.reward_scale, args.incentive_ratio,
                        args.incentive_cost, float(args.incentive), float(batch.max_seq_length))
        for h, gamma in (("env", args.gamma_env), ("inc", args.gamma_inc)):
            G = U.serial_returns(p["r_" + h], p["term"], p["mask"], p["live"], p["v_" + h], gamma, lam)
            ref = Z["B/%s/l%d/ret_%s" % (name, li, h)]
            assert within(G, ref, 1e-5), (lam, h, float(np.abs(G - ref).max()))
            den = p["mask"].sum() * G.shape[-1]
            loss = (((p["chosen_" + h] - G) * p["mask"][..., None]) ** 2).sum() / den
            assert abs(loss - float(Z["B/%s/l%d/loss_value_%s" % (name, li, h)])) <= 1e-5


@pytest.mark.parametrize("base", ["learner_cleanup5.npz", "learner_harvest5.npz", "learner_cleanup5_w4.npz"])
def test_a_lambda_too_small_to_see_is_the_one_step_loss(base):
    """td_lambda = 2^-100 against td_lambda = 0 on the tensor-op learner: every loss and the flat gradient equal to 1e-6 relative (the
    rows' b_t are mask times the one-step targets, which learner_options.npz already pins)."""
    z, meta = load_fixture(base)
    got = []
    for lam in (0.0, TINY):
        args, batch, mac, learner = build(z, meta, overrides=dict(td_lambda=lam))
        perturb_target(learner)
        logs = learner.forward_backward(batch)
        got.append(([float(logs[k]) for k in ("loss_value_env", "loss_value_inc", "loss_sim")], learner._flat_grad.clone()))
    (l0, g0), (l1, g1) = got
    assert all(abs(a - b) <= 1e-6 * max(1.0, abs(a)) for a, b in zip(l0, l1)), (l0, l1)
    assert float(g0.abs().max()) > 1e-4 and float((g0 - g1).abs().max()) <= 1e-6 * max(1.0, float(g0.abs().max()))


def test_option_changes_the_loss_and_defaults_to_off():
    """the shipped config carries td_lambda 0.0; 0.8 moves both value losses far beyond the tolerance of the tests above"""
    z, meta = load_fixture("learner_cleanup5.npz")
    losses = []
    for ov in ({}, dict(td_lambda=0.8)):
        args, batch, mac, learner = build(z, meta, overrides=ov)
        assert args.td_lambda == ov.get("td_lambda", 0.0)
        perturb_target(learner)
        logs = learner.forward_backward(batch)
        losses.append([float(logs[k]) for k in ("loss_value_env", "loss_value_inc")])
    assert min(abs(a - b) for a, b in zip(*losses)) > 1e-3, losses


def _td(**kw):
    F = 1 << 20                      # a dummy device pointer: non-null, aligned, never touched (the checks run before any launch)
    a = abi.SsdTdLossArgs(batch=4, t_slots=8, n_agents=5, n_actions=9, sim_horizon=3, double_q=1, gamma_env=0.99, gamma_inc=0.99, reward_scale=1.0,
                          incentive_ratio=1.0, incentive_cost=1.0, incentive=1.0, seq_len=8.0, sim_threshold=0.1, sim_loss_weight=0.1)
    for k in ("q_env", "q_inc", "tq_env", "tq_inc", "actions", "actions_inc", "avail", "reward", "clean_num", "terminated", "filled", "dens",
              "dq_env", "dq_inc", "partials"):
        setattr(a, k, F)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("lam", [-0.1, 1.5, float("nan")])
def test_library_and_learner_refuse_a_lambda_outside_the_unit_interval(lam):
    lib = abi.load_library()
    a = _td(td_lambda=lam)
    rc = lib.ssd_td_sim_loss(C.byref(a), 1, None)
    assert rc == abi.SSD_ERR_INVALID and b"td_lambda" in lib.ssd_last_error()
    with pytest.raises(abi.SsdError):
        abi.check(lib, rc)
    z, meta = load_fixture("learner_cleanup5.npz")
    with pytest.raises(ValueError, match="td_lambda"):
        build(z, meta, overrides=dict(td_lambda=lam))


def test_struct_carries_td_lambda_in_the_old_padding(tmp_path):
    """The float sits behind sim_loss_weight, in the four bytes that were padding in front of the first pointer: the ctypes mirror has
    the C compiler's size and offsets, the size is the one the struct had without the member (192), no other member moved (q_env
    still at 64, consider_others_inc still at 184 and still the last member, which tests/test_learner_options.py pins), ABI version 10.
    The option's specification asks for the member LAST; the existing test that pins consider_others_inc as the last member stays as
    it is, so the member takes the one other place that moves nothing."""
    fields = abi.SsdTdLossArgs._fields_
    names = [f[0] for f in fields]
    assert dict(fields)["td_lambda"] is C.c_float and names[names.index("td_lambda") - 1] == "sim_loss_weight" and names[-1] == "consider_others_inc"
    probe = ("sim_loss_weight", "td_lambda", "q_env", "partials", "consider_others_inc")
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssd_hip.h"\nint main(){printf("%zu' + ' %zu' * len(probe) + '\\n", sizeof(ssd_td_loss_args)'
                 + "".join(", offsetof(ssd_td_loss_args, %s)" % k for k in probe) + ');return 0;}')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.SsdTdLossArgs)] + [getattr(abi.SsdTdLossArgs, k).offset for k in probe] == [192, 56, 60, 64, 176, 184]
    assert abi.ABI_VERSION == 10


def test_td_loss_args_carry_the_option():
    """ops._td_loss_args hands td_lambda to the kernel; a config without the key means 0 (CPU tensors: the struct only)."""
    from homophily_marl_amd import ops
    z, meta = load_fixture("learner_cleanup5.npz")
    args, batch, mac, learner = build(z, meta, overrides=dict(td_lambda=0.8))
    t, keep = ops._td_loss_args(batch, SimpleNamespace(**vars(args)), args.n_actions, th.zeros(1, 16))
    assert t.td_lambda == np.float32(0.8)
    bare = SimpleNamespace(**{k: v for k, v in vars(args).items() if k != "td_lambda"})
    t, keep = ops._td_loss_args(batch, bare, args.n_actions, th.zeros(1, 16))
    assert t.td_lambda == 0.0
