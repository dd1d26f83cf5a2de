"""Generate the reference trajectories under heads shared across agents FROM THE IMPORTED REFERENCE (build container only).

The construction of oracle/gen_target_sync_golden.py (its helpers are imported; learner_cleanup5.npz's batch and initial weights, asserted
bit-equal; target_update_interval 2: hard syncs after calls 2, 4 and 6), driven through the reference's own learner.train(batch, 0, k)
for k = 1 .. 6.  The rule of config key share_heads is applied to the reference's own module:
  * at start agent 0's slice of every tied tensor ([1, n, in, out]; the names that carry the group's tag) is copied over the others, in
    the live and the target net;
  * every tied leaf gets a register_hook that replaces its gradient by
        g~ = fl(...fl(fl(g_0 + g_1) + g_2)... + g_n-1)     f32, ascending agent order, one rounding per add, written to all n slices
    -- the sum, not the mean -- so the reference's own clip_grad_norm_ (which then counts a tied tensor n times) and its own Adam steps
    see the tied gradient.
The file holds recorded numbers only.  Arms (key prefix):
  both_ env_ inc_     that group tied,
  none_               the reference unpatched (asserted equal to learner_target_sync.npz's recording, call by call),
  mean_               both groups tied with the MEAN of the slices in place of their sum (the losses only: a power arm),
  bothtau0.25_        both groups tied under Polyak target updates at tau 0.25 (tools/gen_soft_target_golden.soft_rule, interval 1).
Recorded per arm and call k as learner_target_sync.npz does:
  <arm>call<k>_<log>  the nine logs;  <arm>call<k>_param_sum / _param_sq / _param_head  checksums of every parameter after the call;
  <arm>sens<k>_<log>, <arm>sens<k>_param_head, <arm>sens<k>_param_sq_rel  |delta| of the same in a second run of the arm whose initial
      weights are each moved by one f32 rounding (x (1 + 2^-23 s), s = +-1 seeded) BEFORE they are tied, so the copies stay equal.
The tests' bar at call k is max(the two-step bar, 8 x sens<k>) (tests/motion_util.py: bars).
  <arm>call<k>_moment_sq, <arm>sens<k>_moment_sq_rel  the sum of squares of Adam's exp_avg per parameter (env optimiser's parameters,
      then the inc optimiser's), and its sensitivity in the form of param_sq_rel (max |delta| / max |value|).
  power_<a>_vs_<b>    [6] per call: the larger TD-loss gap between the two arms in units of arm a's bar.
  power_moment_<a>_vs_<b>   [6] the same for moment_sq, in units of max(the two-step bar of param_sq, 8 x sens).
  spread_<arm>        [6, 2] per call: head_spread_env, head_spread_inc of the reference's parameters after the call, in float64.
Asserted (what the run on the reference gave): in every tied arm the copies of every tied tensor, and of its Adam moments, are equal to
the bit after every call, and the untied group's are not; both_ and none_ are >= POWER_BARS bars apart on a TD loss at every call from
2 on.  both_ and mean_ are NOT: Adam's step does not see the scale of a gradient, so the mean moves no TD loss by more than 0.32 bars
(the gap is recorded, power_both_vs_mean); the pair is >= POWER_BARS bars apart in Adam's first moments at every call instead.
Output: tests/golden/learner_share_heads.npz
"""
import json
import os
import sys

import numpy as np
import torch as th

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import gen_learner_golden as G  # noqa: E402
from oracle import gen_target_sync_golden as S  # noqa: E402
from tools import gen_soft_target_golden as P  # noqa: E402

N_CALLS = S.N_CALLS
GROUPS = {"both_": ("env", "inc"), "env_": ("env",), "inc_": ("inc",), "none_": ()}
POWER_BARS = 10
MEAN_LOSS_BARS = 0.5
PAIRS = (("both_", "none_"), ("both_", "mean_"))


def tied_names(names, tags):
    return [k for k in names if not k.startswith("conv_to_fc") and any("_%s_" % t in k for t in tags)]


def tie_sd(sd, tags):
    """agent 0's slice of every tied tensor over the other slices"""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    for k in tied_names(out, tags):
        assert out[k].ndim == 4 and out[k].shape[0] == 1
        out[k][:, 1:] = out[k][:, :1]
    return out


def tie_hook(mean=False):
    def hook(g):
        assert g.dtype == th.float32 and g.dim() == 4 and g.shape[0] == 1
        acc = g[:, 0].clone()
        for i in range(1, g.shape[1]):
            acc = acc + g[:, i]
        if mean:
            acc = acc / g.shape[1]
        return acc.unsqueeze(1).expand_as(g).clone()
    return hook


def patch(mac, tags, mean=False):
    named = dict(mac.agent.named_parameters())
    for k in tied_names(named, tags):
        named[k].register_hook(tie_hook(mean))


def bits_equal(t):
    return bool((t[:, 1:].contiguous().view(th.int32) == t[:, :1].contiguous().view(th.int32)).all())


def check_invariant(mac, learner, tags, where):
    named = dict(mac.agent.named_parameters())
    tied = set(tied_names(named, tags))
    moments = {}
    for opt in (learner.optimiser_env, learner.optimiser_inc):
        for p, st in opt.state.items():
            moments.setdefault(id(p), []).extend([st["exp_avg"], st["exp_avg_sq"]])
    for k, p in named.items():
        if k.startswith("conv_to_fc"):
            continue
        same = bits_equal(p.detach()) and all(bits_equal(m) for m in moments.get(id(p), []))
        assert same == (k in tied), (where, k, same)
    for k, p in dict(learner.target_mac.agent.named_parameters()).items():
        if k in tied:
            assert bits_equal(p.detach()), (where, "target", k)


def spreads(mac):
    out = []
    for tag in ("env", "inc"):
        num = den = 0.0
        for k, p in mac.agent.named_parameters():
            if not k.startswith("conv_to_fc") and "_%s_" % tag in k:
                x = p.detach().double().squeeze(0)
                num += float(((x - x.mean(dim=0)) ** 2).sum())
                den += float((x ** 2).sum())
        out.append(np.sqrt(num) / np.sqrt(den))
    return out


def moment_sq(learner):
    """sum of squares of Adam's exp_avg per parameter, float64: [env optimiser's parameters | inc optimiser's], each in its own order"""
    return np.array([float((opt.state[p]["exp_avg"].double() ** 2).sum()) for opt in (learner.optimiser_env, learner.optimiser_inc)
                     for p in opt.param_groups[0]["params"]])


def run(fresh, sd, tags, batch, mean=False, tau=None):
    m, l = fresh(sd)
    patch(m, tags, mean)
    if tau is not None:
        P.soft_rule(l, tau)
    seen = []
    inner = l.cal_loss_and_step

    def step(b):
        logs = inner(b)
        seen.append({k: float(v.item()) for k, v in logs.items()})
        return logs
    l.cal_loss_and_step = step
    rows, spr = [], []
    for k in range(1, N_CALLS + 1):
        l.train(batch, 0, k)
        assert len(seen) == k
        check_invariant(m, l, tags, "call %d" % k)
        rows.append((seen[-1],) + G.checksums(m) + (moment_sq(l),))
        spr.append(spreads(m))
    return rows, np.array(spr)


def main(out_name="learner_share_heads.npz"):
    args, cfg, mac, learner, batch, init_sd, fresh = G.construct("cleanup", dict(num_agents=5, map="default5", episode_limit=12), 3,
                                                                 extra=dict(target_update_interval=S.INTERVAL))
    base = np.load(os.path.join(G.GOLDEN, "learner_cleanup5.npz"))
    for k, v in G.batch_arrays(batch).items():
        assert v.dtype == base[k].dtype and np.array_equal(v, base[k]), k          # bit-equal batch: not stored again
    for k, v in init_sd.items():
        assert v.tobytes() == base["w_" + k].tobytes(), k                        # bit-equal initial weights
    pert = P.perturbed(init_sd)
    rows, sens, spread = {}, {}, {}
    for arm, tags in GROUPS.items():
        rows[arm], spread[arm] = run(fresh, tie_sd(init_sd, tags), tags, batch)
        sens[arm], _ = run(fresh, tie_sd(pert, tags), tags, batch)
    rows["mean_"], spread["mean_"] = run(fresh, tie_sd(init_sd, GROUPS["both_"]), GROUPS["both_"], batch, mean=True)
    args.target_update_interval = 1
    try:
        rows["bothtau0.25_"], spread["bothtau0.25_"] = run(fresh, tie_sd(init_sd, GROUPS["both_"]), GROUPS["both_"], batch, tau=0.25)
        sens["bothtau0.25_"], _ = run(fresh, tie_sd(pert, GROUPS["both_"]), GROUPS["both_"], batch, tau=0.25)
    finally:
        args.target_update_interval = S.INTERVAL
    sync = np.load(os.path.join(G.GOLDEN, "learner_target_sync.npz"))
    for i in range(N_CALLS):                                                      # the unpatched arm IS learner_target_sync.npz's run
        for k, v in rows["none_"][i][0].items():
            assert v == float(sync["call%d_%s" % (i + 1, k)]), (i, k)
        assert np.array_equal(rows["none_"][i][3], sync["call%d_param_sq" % (i + 1)])
    out = {"param_names": rows["none_"][0][1], "n_calls": np.int64(N_CALLS)}
    for arm, rr in rows.items():
        out["spread_" + arm.rstrip("_")] = spread[arm]
        for i, (logs, _, sums, sqs, heads, mom) in enumerate(rr):
            c = i + 1
            out["%scall%d_moment_sq" % (arm, c)] = mom
            for k, v in logs.items():
                if arm != "mean_" or k in S.LOSSES:
                    out["%scall%d_%s" % (arm, c, k)] = np.float64(v)
            if arm == "mean_":
                continue
            out["%scall%d_param_sum" % (arm, c)], out["%scall%d_param_sq" % (arm, c)], out["%scall%d_param_head" % (arm, c)] = sums, sqs, heads
            logs_p, _, _, sqs_p, heads_p, mom_p = sens[arm][i]
            out["%ssens%d_moment_sq_rel" % (arm, c)] = np.float64(np.abs(mom_p - mom).max() / np.abs(mom).max())
            for k, v in logs.items():
                out["%ssens%d_%s" % (arm, c, k)] = np.float64(abs(logs_p[k] - v))
            out["%ssens%d_param_head" % (arm, c)] = np.float64(np.abs(heads_p - heads).max())
            out["%ssens%d_param_sq_rel" % (arm, c)] = np.float64(np.abs(sqs_p - sqs).max() / np.abs(sqs).max())
    for arm in spread:
        tags = GROUPS["both_"] if arm in ("mean_", "bothtau0.25_") else GROUPS[arm]
        for col, tag in enumerate(("env", "inc")):
            assert ((spread[arm][:, col] == 0.0) == (tag in tags)).all(), (arm, tag, spread[arm][:, col])
    gap = lambda a, b, c, k: abs(float(out["%scall%d_%s" % (a, c, k)]) - float(out["%scall%d_%s" % (b, c, k)]))
    for a, b in PAIRS:
        bars = []
        for c in range(1, N_CALLS + 1):
            bars.append(max(gap(a, b, c, k) / max(S.BAR_LOG, 8 * float(out["%ssens%d_%s" % (a, c, k)])) for k in S.LOSSES[:2]))
        out["power_%svs_%s" % (a, b.rstrip("_"))] = np.array(bars)
        print("%s against %s: TD-loss gap in bars per call %s" % (a, b, ["%.1f" % v for v in bars]))
        mom = []
        for c in range(1, N_CALLS + 1):
            x, y = out["%scall%d_moment_sq" % (a, c)], out["%scall%d_moment_sq" % (b, c)]
            mom.append(float(np.abs(x - y).max() / np.abs(x).max()) / max(S.BAR_SQ, 8 * float(out["%ssens%d_moment_sq_rel" % (a, c)])))
        out["power_moment_%svs_%s" % (a, b.rstrip("_"))] = np.array(mom)
        print("%s against %s: gap of Adam's first moments (sums of squares, relative) in bars per call %s" % (a, b, ["%.1f" % v for v in mom]))
        if b == "mean_":
            # Adam's step is invariant to the scale of a tensor's gradient (up to eps) and the clip's factor scales every tensor alike, so a
            # mean in place of the sum moves the PARAMETERS, and with them the losses, by less than a bar on this batch (recorded above:
            # at most MEAN_LOSS_BARS).  It shows where the scale lives: in Adam's moments, at every call.
            assert max(bars) <= MEAN_LOSS_BARS, bars
            assert min(mom) >= POWER_BARS, (a, b, mom)
        else:
            assert min(bars[1:]) >= POWER_BARS, (a, b, bars)
    for arm in sens:
        print("%s sensitivity at call %d: %s  param_head %.2e  param_sq (rel) %.2e;  spreads after call %d: %s" % (
            arm, N_CALLS, {k: "%.1e" % out["%ssens%d_%s" % (arm, N_CALLS, k)] for k in S.LOSSES}, out["%ssens%d_param_head" % (arm, N_CALLS)],
            out["%ssens%d_param_sq_rel" % (arm, N_CALLS)], N_CALLS, spread[arm][-1].tolist()))
        assert max(float(out["%ssens%d_%s" % (arm, N_CALLS, k)]) for k in S.LOSSES) <= 1e-4
    out["meta"] = np.frombuffer(json.dumps(dict(env="cleanup", env_args=cfg["env_args"], batch="learner_cleanup5.npz",
                                                overrides=dict(target_update_interval=S.INTERVAL), perturbation_seed=20, arms=sorted(rows))).encode(), np.uint8)
    OUT = os.path.join(G.GOLDEN, out_name)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KB")


if __name__ == "__main__":
    main()
