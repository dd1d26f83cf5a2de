"""Generate the reference trajectories under Polyak target updates FROM THE IMPORTED REFERENCE (build container only).

The construction of oracle/gen_target_sync_golden.py (its helpers are imported; learner_cleanup5.npz's batch and initial weights,
asserted bit-equal) with target_update_interval 1, driven through the reference's own learner.train(batch, 0, k) for k = 1 .. 6: the
reference calls _update_targets after EVERY call, behind both optimiser steps (its homophily_learner.py:249-257).  That method is
replaced, over the reference's own parameters, by the rule of config key target_tau:
    t_new = fl(fl(t * c) + fl(l * tau)),  c = fl(1 - tau),  all f32 -- a plain mul, mul, add.
The file holds recorded numbers only.  Arms (key prefix):
  tau0.25_ tau0.05_ tau1_   the rule at that tau,
  never_                    _update_targets a no-op: the target net stays at the initial weights,
  hard_                     the reference unpatched: a hard copy after every call.
Recorded per arm and call k as learner_target_sync.npz does:
  <arm>call<k>_<log>  the nine logs;  <arm>call<k>_param_sum / _param_sq / _param_head  checksums of every parameter after the call;
  <arm>sens<k>_<log>, <arm>sens<k>_param_head, <arm>sens<k>_param_sq_rel (the tau arms)  |delta| of the same in a second run of the
      arm whose initial weights are each moved by one f32 rounding (x (1 + 2^-23 s), s = +-1 seeded).
The tests' bar at call k is max(the two-step bar, 8 x sens<k>) (tests/motion_util.py: bars).
  power_<a>_vs_<b>          [6] per call: the larger TD-loss gap between the two arms in units of arm a's bar (the power checks).
Asserted (what the run on the reference gave):
  * tau = 1 equals the hard sync at interval 1 EXACTLY: every log and every checksum of all six calls;
  * the rule evaluated in float64 and rounded once (t_new = f32((1 - tau) t + tau l)) moves no loss of any call by more than F64_GAP;
  * tau 0.25 misses the never-updated arm by 1.56e-3 at call 2 (loss_value_inc; >= 1.2e-3 at every later call) and the hard sync
    by 7.65e-3 at call 2; tau 0.05 misses the never-updated arm by 2.7e-4 at call 2 and 6.9e-4 at call 4, and tau 0.25 by 1.3e-3 at
    call 2 (each asserted within 2 % of the figure);
  * every pair above is >= 10 bars apart at every call from 2 on: a tau that is dropped, halved or applied before the Adam step shows.
Output: tests/golden/learner_soft_target.npz
"""
import json
import os
import sys

import numpy as np
import torch as th

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import gen_learner_golden as G  # noqa: E402
from oracle import gen_target_sync_golden as S  # noqa: E402

N_CALLS = S.N_CALLS
TAUS = (0.25, 0.05, 1.0)
F64_GAP = 5.6e-9
PAIRS = (("tau0.25_", "never_"), ("tau0.25_", "hard_"), ("tau0.05_", "never_"), ("tau0.05_", "tau0.25_"))


def arm_name(tau):
    return "tau%g_" % tau


def soft_rule(learner, tau, f64=False):
    """learner._update_targets <- the Polyak rule over the reference's own parameters (f64: evaluated in float64, rounded once)"""
    tau32 = np.float32(tau)
    c, t_ = float(np.float32(1.0) - tau32), float(tau32)

    def update():
        with th.no_grad():
            for t, l in zip(learner.target_mac.parameters(), learner.mac.parameters()):
                assert t.dtype == l.dtype == th.float32 and t.shape == l.shape
                if f64:
                    t.copy_(((1.0 - float(tau32)) * t.double() + float(tau32) * l.double()).float())
                else:
                    t.copy_(t.mul(c).add(l.mul(t_)))
    learner._update_targets = update


def perturbed(init_sd):
    g = th.Generator().manual_seed(20)
    out = {}
    for k, v in init_sd.items():
        s = th.randint(0, 2, v.shape, generator=g).float() * 2 - 1
        out[k] = (th.as_tensor(v) * (1 + 2.0 ** -23 * s)).numpy()
        assert out[k].dtype == np.float32
    return out


def main(out_name="learner_soft_target.npz"):
    args, cfg, mac, learner, batch, init_sd, fresh = G.construct("cleanup", dict(num_agents=5, map="default5", episode_limit=12), 3,
                                                                 extra=dict(target_update_interval=1))
    base = np.load(os.path.join(G.GOLDEN, "learner_cleanup5.npz"))
    for k, v in G.batch_arrays(batch).items():
        assert v.dtype == base[k].dtype and np.array_equal(v, base[k]), k          # bit-equal batch: not stored again
    for k, v in init_sd.items():
        assert v.tobytes() == base["w_" + k].tobytes(), k                        # bit-equal initial weights
    pert = perturbed(init_sd)
    rows = {}
    rows["hard_"], syncs = S.trajectory(mac, learner, batch, N_CALLS)
    assert syncs == list(range(1, N_CALLS + 1)), syncs                           # the reference syncs after every call
    m, l = fresh(init_sd)
    rows["never_"], _ = S.trajectory(m, l, batch, N_CALLS, sync=False)
    sens, worst64 = {}, 0.0
    for tau in TAUS:
        for store, sd, f64 in ((rows, init_sd, False), (sens, pert, False), (None, init_sd, True)):
            m, l = fresh(sd)
            soft_rule(l, tau, f64=f64)
            got, calls = S.trajectory(m, l, batch, N_CALLS)
            assert calls == list(range(1, N_CALLS + 1))
            if store is not None:
                store[arm_name(tau)] = got
            else:
                worst64 = max(worst64, max(abs(a[0][k] - b[0][k]) for a, b in zip(got, rows[arm_name(tau)]) for k in S.LOSSES))
    print("the rule in float64 against the f32 rule: max |delta loss| over the arms and calls %.2e" % worst64)
    assert worst64 <= F64_GAP, worst64
    out = {"param_names": rows["hard_"][0][1], "n_calls": np.int64(N_CALLS), "taus": np.array(TAUS, np.float64)}
    for arm, rr in rows.items():
        for i, (logs, _, sums, sqs, heads) in enumerate(rr):
            c = i + 1
            for k, v in logs.items():
                out["%scall%d_%s" % (arm, c, k)] = np.float64(v)
            out["%scall%d_param_sum" % (arm, c)], out["%scall%d_param_sq" % (arm, c)], out["%scall%d_param_head" % (arm, c)] = sums, sqs, heads
            if arm in sens:
                logs_p, _, _, sqs_p, heads_p = sens[arm][i]
                for k, v in logs.items():
                    out["%ssens%d_%s" % (arm, c, k)] = np.float64(abs(logs_p[k] - v))
                out["%ssens%d_param_head" % (arm, c)] = np.float64(np.abs(heads_p - heads).max())
                out["%ssens%d_param_sq_rel" % (arm, c)] = np.float64(np.abs(sqs_p - sqs).max() / np.abs(sqs).max())
    # tau = 1 IS the hard sync at interval 1
    for i in range(N_CALLS):
        a, b = rows["tau1_"][i], rows["hard_"][i]
        assert a[0] == b[0], (i, a[0], b[0])
        assert all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:])), i
    # before the first update the arms are one
    assert all(rows[arm][0][0] == rows["hard_"][0][0] for arm in rows)
    gap = lambda a, b, c, k="loss_value_inc": abs(float(out["%scall%d_%s" % (a, c, k)]) - float(out["%scall%d_%s" % (b, c, k)]))
    near = lambda got, want: abs(got - want) <= 0.02 * want
    assert near(gap("tau0.25_", "never_", 2), 1.56e-3) and all(gap("tau0.25_", "never_", c) >= 1.2e-3 for c in range(3, N_CALLS + 1))
    assert near(gap("tau0.25_", "hard_", 2), 7.65e-3)
    assert near(gap("tau0.05_", "never_", 2), 2.7e-4) and near(gap("tau0.05_", "never_", 4), 6.9e-4)
    assert near(gap("tau0.05_", "tau0.25_", 2), 1.3e-3)
    for a, b in PAIRS:
        bars = []
        for c in range(1, N_CALLS + 1):
            bars.append(max(gap(a, b, c, k) / max(S.BAR_LOG, 8 * float(out["%ssens%d_%s" % (a, c, k)])) for k in S.LOSSES[:2]))
        out["power_%svs_%s" % (a, b.rstrip("_"))] = np.array(bars)
        print("%s against %s: TD-loss gap in bars per call %s" % (a, b, ["%.1f" % v for v in bars]))
        assert min(bars[1:]) >= 10, (a, b, bars)
    for arm in sens:
        print("%s sensitivity at call %d: %s  param_head %.2e  param_sq (rel) %.2e" % (
            arm, N_CALLS, {k: "%.1e" % out["%ssens%d_%s" % (arm, N_CALLS, k)] for k in S.LOSSES}, out["%ssens%d_param_head" % (arm, N_CALLS)],
            out["%ssens%d_param_sq_rel" % (arm, N_CALLS)]))
        assert max(float(out["%ssens%d_%s" % (arm, N_CALLS, k)]) for k in S.LOSSES) <= 1e-4
    out["meta"] = np.frombuffer(json.dumps(dict(env="cleanup", env_args=cfg["env_args"], batch="learner_cleanup5.npz",
                                                overrides=dict(target_update_interval=1), perturbation_seed=20, arms=sorted(rows))).encode(), np.uint8)
    OUT = os.path.join(G.GOLDEN, out_name)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KB")


if __name__ == "__main__":
    main()
