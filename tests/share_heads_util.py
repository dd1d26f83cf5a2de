"""Shared by tests/test_share_heads_host.py / _gpu.py (config key share_heads: heads tied across agents): a helper, no
test in it.

  * the rule and the spread restated in numpy with plain loops (f32 adds in ascending agent order; float64 sums);
  * a learner of this package on the fixture batch whose tied tensors start from agent 0's slice, as the controller leaves them at
    construction (tests/learner_util.build loads the fixture's per-agent weights over that) and as tools/gen_share_heads_golden.py ties
    the reference's;
  * the recordings of tools/gen_share_heads_golden.py (tests/golden/learner_share_heads.npz) through tests/soft_target_util's views;
  * the invariant: the copies of every tied tensor, of its Adam moments and of its target copy are equal to the bit;
  * a launcher of tests/share_heads_dp_worker.py in the manner of tests/dp_util.run_ranks (which starts tests.dp_worker only).
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch as th

from tests import motion_util as mu
from tests import soft_target_util as su
from tests.learner_util import build, load_fixture

ARMS = {"both": "both_", "env": "env_", "inc": "inc_", "none": "none_"}
TAGS = {"both": ("env", "inc"), "env": ("env",), "inc": ("inc",), "none": ()}
POWER_BARS = 10
SPREAD_RTOL = 1e-9            # float64 sums of <= 41 K terms err by <= ~5e-12 relative; the margin is for another summation order
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule and the spread, restated -------------------------------------------------------------------------------------------------
def tie_np(g):
    """g f32 [n, inner] -> [n, inner]: every row the sum of the rows in ascending order, one f32 rounding per add (numpy rounds every
    f32 operation once)"""
    g = np.asarray(g, np.float32)
    acc = g[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, g.shape[0]):
            acc = acc + g[i]
    assert acc.dtype == np.float32
    return np.broadcast_to(acc, g.shape).copy()


def same_bits(a, b):
    """equal by bits, NaN payloads aside (a NaN matches any NaN)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def spread_np(x):
    """x f32 [n, inner] -> (sum_i sum_e (x_i[e] - m[e])^2, sum_i sum_e x_i[e]^2) in float64, m the mean over the rows"""
    x = np.asarray(x, np.float32).astype(np.float64)
    m = x.sum(axis=0) / x.shape[0]
    return float(((x - m) ** 2).sum()), float((x ** 2).sum())


def head_spread_np(agent, tag):
    """head_spread_<tag> of the agent's parameters as they are now, in float64"""
    num = den = 0.0
    for name, p in agent.head_parameters(tag):
        a, b = spread_np(p.detach().cpu().numpy().reshape(p.shape[1], -1))
        num, den = num + a, den + b
    return np.sqrt(num) / np.sqrt(den)


# ---- learners on the fixture ----------------------------------------------------------------------------------------------------------------
def tie_fixture(mac, learner):
    """agent 0's slice of every tied tensor over the others (what the constructor did before the fixture's weights were loaded); the
    target net follows"""
    with th.no_grad():
        for _, p in mac.agent.tied_parameters():
            p[:, 1:] = p[:, :1]
    learner.target_mac.load_state(mac)


def fixture_learner(share, device="cpu", sl=slice(None), code_obs=False, **over):
    """(batch, controller, learner, the logs of every step) on learner_cleanup5.npz at share_heads `share` (None: the key absent) and
    target_update_interval 2 (the golden's)"""
    z, meta = load_fixture("learner_cleanup5.npz")
    keys = dict(dict(target_update_interval=2), **over)
    if share is not None:
        keys["share_heads"] = share
    args, batch, mac, learner = build(z, meta, device=device, sl=sl, overrides=keys, code_obs=code_obs)
    if share is None:
        assert getattr(args, "share_heads", "none") == "none"
    tie_fixture(mac, learner)
    name = "_graph_step" if learner.use_graph else "cal_loss_and_step"
    return batch, mac, learner, su.record_steps(learner, name)


def golden():
    return load_fixture("learner_share_heads.npz")[0]


def bits_equal_across_agents(t):
    t = t.detach()
    return bool((t[:, 1:].contiguous().view(th.int32) == t[:, :1].contiguous().view(th.int32)).all())


def moments(learner, p):
    out = []
    for opt in (learner.optimiser_env, learner.optimiser_inc):
        st = opt.state.get(p)
        if st:
            out += [st["exp_avg"], st["exp_avg_sq"]]
    return out


def assert_invariant(mac, learner, tags, where):
    """per-agent tensors of a tied group: parameter, Adam moments and target copy equal across agents to the bit; of an untied group:
    the parameter and its moments are NOT (the agents see different data)"""
    target = dict(learner.target_mac.agent.named_parameters())
    for tag in ("env", "inc"):
        for name, p in mac.agent.head_parameters(tag):
            mom = moments(learner, p)
            assert len(mom) == 2, (where, name)
            if tag in tags:
                assert bits_equal_across_agents(p), (where, name)
                assert all(bits_equal_across_agents(m) for m in mom), (where, name, "Adam state")
                assert bits_equal_across_agents(target[name]), (where, name, "target")
            else:
                assert not bits_equal_across_agents(p) and not any(bits_equal_across_agents(m) for m in mom), (where, name, "untied")


def moment_sq(learner):
    """as tools/gen_share_heads_golden.moment_sq"""
    return np.array([float((opt.state[p]["exp_avg"].double() ** 2).sum()) for opt in (learner.optimiser_env, learner.optimiser_inc)
                     for p in opt.param_groups[0]["params"]])


def moment_error(zs, arm, k, learner, bars=None):
    """(relative error of Adam's first-moment checksums against <arm>'s recording, its bar: max(the two-step bar of param_sq, 8 x sens))"""
    ref = zs["%scall%d_moment_sq" % (arm, k)]
    bar = max(mu.SQ_TOL, mu.SENS_FACTOR * float(zs["%ssens%d_moment_sq_rel" % (bars or arm, k)]))
    return float(np.abs(moment_sq(learner) - ref).max() / np.abs(ref).max()), bar


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------------
def run_ranks(world, share, limit=180.0):
    """[{key: array} per rank] of one job of tests.share_heads_dp_worker on CPU tensors under ONE time limit; a rank that exits non-zero
    or the limit passing ends the job and every process of it"""
    from tests.dp_util import RankFailure, _tail, free_port
    port = free_port()
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SSD_FORCE_DIST")}
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory() as d:
        procs, logs = [], []
        try:
            for rank in range(world):
                err = open(os.path.join(d, "rank%d.err" % rank), "w")
                logs.append(err)
                procs.append(subprocess.Popen([sys.executable, "-m", "tests.share_heads_dp_worker", str(rank), str(world), str(port), share, d],
                                              cwd=ROOT, env=base, stdin=subprocess.DEVNULL, stdout=err, stderr=subprocess.STDOUT))
            failed = None
            while failed is None and any(p.poll() is None for p in procs):
                if any(p.poll() not in (None, 0) for p in procs):
                    failed = "a rank exited non-zero"
                elif time.perf_counter() - t0 > limit:
                    failed = "the job passed its limit of %g s (hung)" % limit
                else:
                    time.sleep(0.05)
            if failed is None and any(p.returncode != 0 for p in procs):
                failed = "a rank exited non-zero"
            codes = [p.poll() for p in procs]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
            for p in procs:
                p.wait()
            for f in logs:
                f.close()
        print("share_heads dp job, %d rank(s): %.1f s" % (world, time.perf_counter() - t0))
        if failed is not None:
            tails = "\n".join("---- rank %d (exit %s) ----\n%s" % (r, codes[r], _tail(os.path.join(d, "rank%d.err" % r))) for r in range(world))
            raise RankFailure("share_heads %s: %s\n%s" % (share, failed, tails), procs, codes)
        out = []
        for rank in range(world):
            with np.load(os.path.join(d, "rank%d.npz" % rank)) as z:
                out.append({k: z[k] for k in z.files})
        return out
