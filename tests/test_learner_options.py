"""CPU suite: the loss flags of config/algs/homophily.yaml other than the shipped ones (double_q: False, consider_others_inc: True)
against numbers the reference's learner recorded (tests/golden/learner_options.npz, tools/gen_learner_options_golden.py): the
tensor-op statement of HomophilyLearner over two optimisation steps, with a target net that differs from the live net."""
import json
import os
import re

import numpy as np
import pytest
import torch as th

from tests.learner_util import GOLDEN, build, load_fixture, param_checksums

LOSS_TOL = 1e-5
LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")
DEFAULTS = dict(double_q=True, consider_others_inc=False)          # config/algs/homophily.yaml


def load_cases():
    z = np.load(os.path.join(GOLDEN, "learner_options.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


CASES = [c["name"] for c in load_cases()[1]["cases"]]


def case(name):
    """(recorded numbers of the case: key -> array, its base fixture (z, meta), its overrides)."""
    z, meta = load_cases()
    c = next(c for c in meta["cases"] if c["name"] == name)
    rec = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
    return rec, load_fixture(c["base"]), c["overrides"]


def perturb_target(learner):
    """The generator's rule: target_k = f32(f64(live_k) + 0.05 sin(0.37 arange(numel_k) + k)), k = state_dict index; applied to the
    target net through load_state_dict, which also refreshes the frozen net's cached weight images that a captured step reads (call
    it after anything that copies the live net into the target net)."""
    sd = {}
    for k, (name, v) in enumerate(learner.target_mac.agent.state_dict().items()):
        x = v.detach().double().cpu()
        d = 0.05 * th.sin(0.37 * th.arange(x.numel(), dtype=th.float64) + k).reshape(x.shape)
        sd[name] = (x + d).float()
    learner.target_mac.agent.load_state_dict(sd)


def check_step(logs, mac, rec, step, tol=LOSS_TOL):
    for k in LOG_KEYS:
        ref = float(rec["step%d_%s" % (step, k)])
        assert abs(float(logs[k]) - ref) < tol, (step, k, float(logs[k]), ref)
    sums, sqs, heads = param_checksums(mac)
    assert np.abs(heads - rec["step%d_param_head" % step]).max() < 2e-5, step
    assert np.abs(sqs - rec["step%d_param_sq" % step]).max() / np.abs(rec["step%d_param_sq" % step]).max() < 1e-5, step


def test_fixture_covers_the_option_surface():
    z, meta = load_cases()
    got = {(c["base"], c["overrides"]["double_q"], c["overrides"]["consider_others_inc"]) for c in meta["cases"]}
    assert got == {("learner_cleanup5.npz", dq, oth) for dq in (True, False) for oth in (True, False)} | \
        {("learner_harvest5.npz", True, True), ("learner_cleanup5_w4.npz", True, True)}
    assert "sin(0.37" in meta["target_perturbation"]
    assert all(z[k].dtype != object for k in z.files) and not any("/w_" in k for k in z.files)


@pytest.mark.parametrize("name", CASES)
def test_tensor_op_learner_matches_reference_options(name):
    """Two steps of the tensor-op loss (the CPU path and the yardstick of the kernel) under the case's flags: every logged value within
    1e-5 and every parameter after each step, as test_learner_parity.test_two_learner_steps_match_reference."""
    rec, (z, meta), overrides = case(name)
    args, batch, mac, learner = build(z, meta, overrides=overrides)
    assert (args.double_q, args.consider_others_inc) == (overrides["double_q"], overrides["consider_others_inc"])
    perturb_target(learner)
    for step in range(2):
        logs = learner.cal_loss_and_step(batch)
        check_step(logs, mac, rec, step)


@pytest.mark.parametrize("name", [c for c in CASES if "_dq1_oth0" not in c])
def test_fixture_pins_the_option(name):
    """Run with the default value of every option the case sets otherwise: the recorded losses must be missed by far more than the
    tolerance (the fixture would not see the option otherwise)."""
    rec, (z, meta), overrides = case(name)
    args, batch, mac, learner = build(z, meta, overrides=DEFAULTS)
    perturb_target(learner)
    miss = 0.0
    for step in range(2):
        logs = learner.cal_loss_and_step(batch)
        for k in ("loss_value_env", "loss_value_inc", "loss_sim"):
            miss = max(miss, abs(float(logs[k]) - float(rec["step%d_%s" % (step, k)])))
    assert miss > 100 * LOSS_TOL, (name, miss)


def test_abi_carries_consider_others_inc():
    from homophily_marl_amd import abi
    names = [f[0] for f in abi.SsdTdLossArgs._fields_]
    assert names[-1] == "consider_others_inc" and dict(abi.SsdTdLossArgs._fields_)["consider_others_inc"] is __import__("ctypes").c_int32
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ssd_hip.h")).read()
    body = re.search(r"typedef struct ssd_td_loss_args \{(.*?)\} ssd_td_loss_args;", hdr, re.S).group(1)
    assert body.strip().splitlines()[-1].strip() == "int32_t consider_others_inc;"
    assert abi.ABI_VERSION == int(re.search(r"#define SSD_ABI_VERSION (\d+)", hdr).group(1)) == 10


def test_td_loss_args_fill_the_option():
    """ops._td_loss_args hands the flag to the kernel (CPU tensors: the struct only, nothing is launched)."""
    from types import SimpleNamespace
    from homophily_marl_amd import ops
    z, meta = load_fixture("learner_cleanup5.npz")
    for oth in (False, True):
        args, batch, mac, learner = build(z, meta, overrides=dict(consider_others_inc=oth))
        partials = th.zeros(1, 16)
        t, keep = ops._td_loss_args(batch, SimpleNamespace(**vars(args)), args.n_actions, partials)
        assert t.consider_others_inc == int(oth) and t.double_q == 1
