"""Generate the reference trajectory across target-network syncs FROM THE IMPORTED REFERENCE (build container only).

The construction of oracle/gen_learner_golden.py's learner_cleanup5.npz (Cleanup default5, 5 agents, episode_limit 12, seed 3) with
target_update_interval 2, driven through the reference's learner.train(batch, 0, k) for k = 1 .. N_CALLS (not cal_loss_and_step): the
reference copies the live net into the target net after calls 2, 4 and 6 (its homophily_learner.py:249-257), so calls 3 and 5
bootstrap from a freshly synced target.  The sampled batch and the initial weights are asserted bit-equal to learner_cleanup5.npz's,
so the file holds recorded results only and the tests take the batch from that fixture.

Recorded per call k (train returns nothing: cal_loss_and_step is wrapped):
  call<k>_<log>            the nine logged values,
  call<k>_param_sum / _param_sq / _param_head   checksums of every parameter after the call (as learner_cleanup5.npz's step<k>_*),
  sens<k>_<log>, sens<k>_param_head, sens<k>_param_sq_rel
                           |delta| of the same values in a second reference run whose initial parameters are each multiplied by
                           (1 + 2^-23 s), s = +-1 drawn from a seeded generator: what rounding the INPUT weights to f32 once does to
                           the reference's own six-step Adam trajectory.  (param_head: max over the entries; param_sq_rel:
                           max |delta sq| / max |sq|, the form of the two-step bar.)  The tests' bar at call k is
                           max(the two-step bar, 8 x sens<k>): 8 for this package's different summation order on top.
  nosync<k>_loss_value_env / _inc   the same reference run with _update_targets replaced by a no-op (the target net stays at the
                           initial weights): what a sync that does not reach the target net looks like.  `power_call` is the first
                           call at which it misses the synced run by more than 10 x that call's bar (asserted to exist; expected 3).

Trajectory length: N_CALLS = 6.  Had call 6's sensitivity of any loss exceeded 1e-4, the trajectory would be cut to the longest
prefix that still holds two syncs followed by a call (5); the generator asserts that this was not needed (measured: see the printout,
all loss sensitivities of call 6 are below 1e-6).
Output: tests/golden/learner_target_sync.npz
"""
import json
import os
import sys

import numpy as np
import torch as th

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import gen_learner_golden as G  # noqa: E402

N_CALLS = 6
INTERVAL = 2
LOSSES = ("loss_value_env", "loss_value_inc", "loss_sim")
BAR_LOG, BAR_HEAD, BAR_SQ = 1e-5, 2e-5, 1e-5          # tests/test_learner_parity.py: the two-step bars


def trajectory(mac, learner, batch, n_calls, sync=True):
    """n_calls of learner.train(batch, 0, k): per call the logs cal_loss_and_step returned and the parameter checksums after it"""
    seen = []
    inner = learner.cal_loss_and_step

    def step(b):
        logs = inner(b)
        seen.append({k: float(v.item()) for k, v in logs.items()})
        return logs
    learner.cal_loss_and_step = step
    syncs = []
    if sync:
        inner_sync = learner._update_targets
        learner._update_targets = lambda: (syncs.append(len(seen)), inner_sync())
    else:
        learner._update_targets = lambda: None
    rows = []
    for k in range(1, n_calls + 1):
        learner.train(batch, 0, k)
        assert len(seen) == k
        rows.append((seen[-1],) + G.checksums(mac))
    return rows, syncs


def main(out_name="learner_target_sync.npz"):
    args, cfg, mac, learner, batch, init_sd, fresh = G.construct("cleanup", dict(num_agents=5, map="default5", episode_limit=12), 3,
                                                                 extra=dict(target_update_interval=INTERVAL))
    base = np.load(os.path.join(G.GOLDEN, "learner_cleanup5.npz"))
    for k, v in G.batch_arrays(batch).items():
        assert v.dtype == base[k].dtype and np.array_equal(v, base[k]), k          # bit-equal batch: not stored again
    for k, v in init_sd.items():
        assert v.tobytes() == base["w_" + k].tobytes(), k                        # bit-equal initial weights
    rows, syncs = trajectory(mac, learner, batch, N_CALLS)
    assert syncs == [2, 4, 6][:N_CALLS // 2], syncs
    for step in range(2):                                                        # calls 1 and 2 are the fixture's two steps
        for k, v in rows[step][0].items():
            assert v == float(base["step%d_%s" % (step, k)]), (step, k)
    # sensitivity: every initial parameter times (1 + 2^-23 s)
    g = th.Generator().manual_seed(20)
    pert = {}
    for k, v in init_sd.items():
        s = th.randint(0, 2, v.shape, generator=g).float() * 2 - 1
        pert[k] = (th.as_tensor(v) * (1 + 2.0 ** -23 * s)).numpy()
        assert pert[k].dtype == np.float32
    m2, l2 = fresh(pert)
    rows_p, _ = trajectory(m2, l2, batch, N_CALLS)
    m3, l3 = fresh(init_sd)
    rows_n, _ = trajectory(m3, l3, batch, N_CALLS, sync=False)
    out = {"param_names": rows[0][1], "n_calls": np.int64(N_CALLS), "sync_after": np.array(syncs, np.int64)}
    power_call = None
    for i, ((logs, _, sums, sqs, heads), (logs_p, _, _, sqs_p, heads_p), (logs_n, _, _, _, _)) in enumerate(zip(rows, rows_p, rows_n)):
        c = i + 1
        for k, v in logs.items():
            out["call%d_%s" % (c, k)] = np.float64(v)
            out["sens%d_%s" % (c, k)] = np.float64(abs(logs_p[k] - v))
        out["call%d_param_sum" % c], out["call%d_param_sq" % c], out["call%d_param_head" % c] = sums, sqs, heads
        out["sens%d_param_head" % c] = np.float64(np.abs(heads_p - heads).max())
        out["sens%d_param_sq_rel" % c] = np.float64(np.abs(sqs_p - sqs).max() / np.abs(sqs).max())
        gaps = {}
        for k in LOSSES[:2]:
            out["nosync%d_%s" % (c, k)] = np.float64(logs_n[k])
            gaps[k] = abs(logs_n[k] - logs[k]) / max(BAR_LOG, 8 * float(out["sens%d_%s" % (c, k)]))
        if power_call is None and max(gaps.values()) > 10:
            power_call = c
        print("call %d: losses %s\n        sensitivity %s  param_head %.2e  param_sq (rel) %.2e\n        unsynced target: gap / bar %s" % (
            c, {k: "%.8f" % logs[k] for k in LOSSES}, {k: "%.1e" % out["sens%d_%s" % (c, k)] for k in logs},
            out["sens%d_param_head" % c], out["sens%d_param_sq_rel" % c], {k: "%.1f" % v for k, v in gaps.items()}))
    assert all(rows_n[i][0] == rows[i][0] for i in range(2))                      # before the first sync the arms are one
    assert max(float(out["sens%d_%s" % (N_CALLS, k)]) for k in LOSSES) <= 1e-4, "cut the trajectory (see the docstring)"
    assert power_call is not None, "the syncs change nothing measurable: raise N_CALLS"
    out["power_call"] = np.int64(power_call)
    out["meta"] = np.frombuffer(json.dumps(dict(env="cleanup", env_args=cfg["env_args"], batch="learner_cleanup5.npz",
                                                overrides=dict(target_update_interval=INTERVAL), perturbation_seed=20)).encode(), np.uint8)
    OUT = os.path.join(G.GOLDEN, out_name)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KB; power at call", power_call)


if __name__ == "__main__":
    main()
