"""Shared by tests/test_soft_target_host.py / _gpu.py (config key target_tau: Polyak target updates): a helper, no test
in it.

  * the recordings of tools/gen_soft_target_golden.py (tests/golden/learner_soft_target.npz) as per-arm views that tests/motion_util.py's
    bars / call_errors read like learner_target_sync.npz;
  * the rule restated in numpy f32 (three roundings), and the launch's per-workgroup partial sums restated in the order
    include/ssd_hip.h states ("Polyak target update").
"""
import numpy as np

from tests import motion_util as mu
from tests.learner_util import build, load_fixture

TAU_ARMS = {0.25: "tau0.25_", 0.05: "tau0.05_", 1.0: "tau1_"}
POWER_BARS = 10


class Arm:
    """z[<calls prefix>call<k>_*] with the sensitivities (the bars) of <bars prefix>: the arm itself, or another arm's recordings held
    to this arm's bars (the power checks)"""

    def __init__(self, z, calls, bars=None):
        self.z, self.calls, self.bars = z, calls, bars or calls

    def __getitem__(self, key):
        return self.z[(self.bars if key.startswith("sens") else self.calls) + key]


def golden():
    return load_fixture("learner_soft_target.npz")[0]


def host_learner(**over):
    """(batch, controller, learner, the logs of every cal_loss_and_step) of this package on the fixture batch, tensor ops on the host"""
    z, meta = load_fixture("learner_cleanup5.npz")
    args, batch, mac, learner = build(z, meta, overrides=over)
    return (batch, mac, learner) + (record_steps(learner, "cal_loss_and_step"),)


def record_steps(learner, name):
    seen = []
    inner = getattr(learner, name)

    def step(b):
        seen.append(inner(b))
        return seen[-1]
    setattr(learner, name, step)
    return seen


def ratios(errors, keys=("loss_value_env", "loss_value_inc")):
    return {k: errors[k][0] / errors[k][1] for k in keys}


def assert_call(zs, arm, k, logs, mac, tag=""):
    errors = mu.call_errors(Arm(zs, arm), k, logs, mac)
    print("%s%s call %d: worst %s at %.3f of its bar; losses %s" % ((tag, arm, k) + mu.worst(errors) + ({key: "%.2e" % errors[key][0] for key in mu.LOG_KEYS[:3]},)))
    for name, (err, bar) in errors.items():
        assert err < bar, (arm, k, name, err, bar)


def power(zs, arm, other, k, logs, mac):
    """the larger TD-loss distance of this call from ANOTHER arm's recording, in units of this arm's bars"""
    return max(ratios(mu.call_errors(Arm(zs, other, bars=arm), k, logs, mac)).values())


# ---- the rule and the launch, restated ------------------------------------------------------------------------------------------------
def polyak_np(t, l, tau):
    """fl(fl(t * c) + fl(l * tau)), c = fl(1 - tau): numpy rounds every f32 operation once"""
    t, l, tau = np.asarray(t, np.float32), np.asarray(l, np.float32), np.float32(tau)
    c = np.float32(1.0) - tau
    a, b = t * c, l * tau
    assert a.dtype == b.dtype == np.float32
    return a + b


def params_np(agent):
    return {k: v.detach().cpu().numpy().copy() for k, v in agent.named_parameters()}


def launch_partials(live, new, whole, workgroups):
    """[workgroups, 2] f32: the launch's partial sums over the jobs' concatenated elements (live, new: f32 [E]; whole: bool [E], the
    elements of the parameter jobs) in the header's order -- thread t of workgroup w adds its elements w P + t + 256 i in rising i,
    then the 256 accumulators fold by halves"""
    E = live.size
    P = 256 * -(-E // (256 * workgroups))
    pad = lambda x: np.concatenate([x, np.zeros(workgroups * P - E, x.dtype)]).reshape(workgroups, P // 256, 256)
    d = (live - new).astype(np.float32)
    terms = [pad(np.where(whole, d * d, np.float32(0)).astype(np.float32)), pad(np.where(whole, live * live, np.float32(0)).astype(np.float32))]
    out = np.zeros((workgroups, 2), np.float32)
    for j, x in enumerate(terms):
        acc = np.zeros((workgroups, 256), np.float32)
        for i in range(x.shape[1]):
            acc = acc + x[:, i]                    # (+0 for the elements a thread does not count: exact)
        s = 128
        while s:
            acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
            s >>= 1
        out[:, j] = acc[:, 0]
    return out


def gap_rel64(live, target):
    """target_gap_rel of two {name: array} parameter sets, in float64"""
    num = sum(float(((live[k].astype(np.float64) - target[k].astype(np.float64)) ** 2).sum()) for k in live)
    den = sum(float((live[k].astype(np.float64) ** 2).sum()) for k in live)
    return np.sqrt(num) / np.sqrt(den)
