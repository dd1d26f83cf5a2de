"""Every epsilon-greedy pick site of the rollout held to the host restatement of the draw contract (tests/explore_util.py; the contract:
include/ssd_hip.h, "Exploration draws") by EXACT equality -- the statistical properties of the restatement itself are
tests/test_exploration_contract.py's.

CPU: what ssd_dueling_pick refuses (invalid calls only, nothing reaches a launch).
GPU: (a) ssd_dueling_pick alone over action counts, masks, epsilons, both row layouts, env_id_base, steps (2^32 + 17 draws what 17 draws),
         a ragged batch and one launch whose grid strides twice;
     (b) the matrix-core heads (k_head GEN 0 .. 3, k_inc_encode, k_inc_encode_any, k_inc_encode_gather) through FastPolicy with q_out:
         flagged rows equal the restated pick, unflagged rows the first maximum of the row's OWN q_out over the available actions
         (no tolerance: Q parity is other tests' business, this pins mask, tie-break and key);
     (c) the hip_graph runner's draw counter, from the stored actions of eager, captured and replayed episodes."""
import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from tests import explore_util as xu
from tests import policy_cases as pc

INV, UNS = abi.SSD_ERR_INVALID, abi.SSD_ERR_UNSUPPORTED
F = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched
BASE = 4096 * 7 + 3
Z_BAR = 4.0


def _z(count, R, p):
    return (count - R * p) / np.sqrt(R * p * (1 - p))


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
#                av rows A  avail eps step seed n  B  pairs actions q_out base stream
_PICK_BASELINE = [F, 15, 9, F,    F,  F,   7,   5, 3, 0,    F,      None, 0,  None]
_PICK_REFUSALS = [("null av", {0: None}, INV), ("null epsilon", {4: None}, INV), ("null step", {5: None}, INV), ("null actions", {10: None}, INV),
                  ("rows 0", {1: 0}, INV), ("n_actions 0", {2: 0}, INV), ("n_actions -1", {2: -1}, INV), ("n_agents 0", {7: 0}, INV),
                  ("batch 0", {8: 0}, INV), ("rows one short of n * B", {1: 14}, INV), ("rows one over n * B", {1: 16}, INV),
                  ("pairs with rows = n * B", {9: 1}, INV), ("rows = n * B * n without pairs", {1: 75}, INV),
                  ("pairs, rows one short of n * B * n", {9: 1, 1: 74}, INV),
                  ("n_actions 17", {2: 17}, UNS), ("n_actions 17 without a mask", {2: 17, 3: None}, UNS), ("n_actions 33 without a mask", {2: 33, 3: None}, UNS),
                  ("pairs, n_actions 32", {9: 1, 1: 75, 2: 32}, UNS)]


@pytest.mark.parametrize("label,change,expect", _PICK_REFUSALS, ids=[r[0] for r in _PICK_REFUSALS])
def test_dueling_pick_refuses(label, change, expect):
    """Single departures from a baseline of valid arguments (dummy pointers, never dereferenced; the baseline itself is never called).
    n_actions above 16: the mask is gathered into 16 bits and the pick walks one word, so the entry point refuses instead of silently
    dropping the actions from 16 on."""
    lib = abi.load_library()
    args = list(_PICK_BASELINE)
    for k, v in change.items():
        args[k] = v
    assert args != _PICK_BASELINE
    assert lib.ssd_dueling_pick(*args) == expect, label
    if expect == UNS:
        assert b"n_actions must be 1 .. 16" in lib.ssd_last_error()


# ---- GPU (a): ssd_dueling_pick ------------------------------------------------------------------------------------------------------
PICK_SEED = 0x1234ABCD
PICK_EPS = (0.0, 2.0 ** -24, 0.05, 0.3, 1.0, 1.5)
PICK_STEPS = (0, 17, 2 ** 32 + 17)
#              pairs n  B        (B = 203: ragged, rows no multiple of the 256-thread workgroup)
PICK_SHAPES = [(0, 1, 203), (0, 3, 203), (0, 10, 61), (1, 1, 203), (1, 3, 203), (1, 10, 61)]


def _masks(A):
    """NULL, all ones, the shipped holes (5, 6, 7), first off, last off, exactly one live (first / middle / last) -- without repeats"""
    one = lambda k: [int(j == k) for j in range(A)]
    cand = [None, [1] * A, [0 if 5 <= k <= 7 else 1 for k in range(A)], [0] + [1] * (A - 1), [1] * (A - 1) + [0], one(0), one(A // 2), one(A - 1)]
    out = []
    for m in cand:
        if m not in out:
            out.append(m)
    return out


def _q_bar(av, A):
    """float64 q = v + a - mean(a) of f32 rows [R, A + 1], and the f32 rounding bar per row: the sum of A advantages accumulates at most
    (A - 1) u A max|a|, i.e. (A - 1) u max|a| on the mean, the division u max|a| more; v + a_k rounds by u (|v| + max|a|), the
    subtraction of the mean by u (|v| + 2 max|a|): u ((A + 3) max|a| + 2 |v|) in all, u = 2^-24 -- below (A + 2) u (|v| + 2 max|a|)."""
    a, v = av[:, :A].astype(np.float64), av[:, A].astype(np.float64)
    q = v[:, None] + a - a.mean(axis=1, keepdims=True)
    return q, (A + 2) * 2.0 ** -24 * (np.abs(v) + 2 * np.abs(a).max(axis=1))


def _env_major(x, n, B, pairs):
    """kernel rows (i, b[, j]) -> [B, n(, n), ...]"""
    return np.swapaxes(x.reshape((n, B) + ((n,) if pairs else ()) + x.shape[1:]), 0, 1)


def _pick_inputs(A, R, rng, ties):
    av = rng.standard_normal((R, A + 1)).astype(np.float32)
    tie = np.zeros(R, dtype=bool)
    if ties:                    # small integers: exact in f32 at a power-of-two A, with many equal maxima
        tie[::4] = True
        av[tie] = rng.integers(-1, 3, (int(tie.sum()), A + 1)).astype(np.float32)
    return av, tie


def _top_gap(q, bits, A):
    ok = np.array([(bits >> k) & 1 for k in range(A)], dtype=bool)
    if ok.sum() < 2:
        return np.full(q.shape[:-1], np.inf)
    s = np.sort(np.where(ok, q, -np.inf), axis=-1)
    return s[..., -1] - s[..., -2]


def _launch_pick(lib, av, R, A, mask_t, eps_t, step_t, seed, n, B, pairs, actions, q_out, base):
    actions.fill_(-7)
    abi.check(lib, lib.ssd_dueling_pick(av.data_ptr(), R, A, None if mask_t is None else mask_t.data_ptr(), eps_t.data_ptr(), step_t.data_ptr(),
                                        seed, n, B, pairs, actions.data_ptr(), None if q_out is None else q_out.data_ptr(), base,
                                        th.cuda.current_stream().cuda_stream))


def _check_pick_launch(act, q_dev, q64, bar, gap, tie, flag, picked, bits, A, pairs, tally, label):
    """one launch against the restatement; all arrays env-major.  Returns nothing: asserts, and adds to the tally."""
    n = act.shape[-1]
    diag = np.broadcast_to(np.eye(n, dtype=bool), act.shape) if pairs else np.zeros(act.shape, dtype=bool)
    assert (act[diag] == 0).all(), label
    explored = flag & (picked >= 0) & ~diag
    assert (act[explored] == picked[explored]).all(), (label, int((act[explored] != picked[explored]).sum()))
    greedy = xu.first_max(q64, bits, A)
    rest = ~explored & ~diag
    exact = rest & tie
    assert (act[exact] == greedy[exact]).all(), (label, "ties")
    clear = rest & ~tie & (gap > 2 * bar)
    assert (act[clear] == greedy[clear]).all(), (label, int((act[clear] != greedy[clear]).sum()))
    assert ((act >= 0) & (act < A)).all(), label
    tally["rows"] += act.size
    tally["explored"] += int(explored.sum())
    tally["greedy"] += int(clear.sum()) + int(exact.sum())
    tally["skipped"] += int((rest & ~tie & ~(gap > 2 * bar)).sum())
    if q_dev is not None:
        err = np.abs(q_dev.astype(np.float64) - q64)
        worst = float((err / np.maximum(bar, 1e-300)[..., None]).max())
        assert (err <= bar[..., None]).all(), (label, worst)
        assert (q_dev[tie] == q64[tie]).all(), (label, "integer rows are exact")
        tally["q_err"] = max(tally["q_err"], worst)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 3, 8, 9, 16])
def test_dueling_pick_equals_the_restated_draws(A):
    """ssd_dueling_pick over masks x epsilons x steps x env_id_base x row layouts at one action count.  Per launch: every explore-flagged
    row equals the restated pick; the pairs diagonal is 0; q_out within (A + 2) 2^-24 (|v| + 2 max|a|) of the float64 v + a - mean(a)
    (_q_bar); every other row equals the float64 first maximum over the available actions where the float64 top-two gap exceeds twice
    that bar (normal inputs: the share of rows below the gap is asserted under 1 % per input and printed); at a power-of-two A every
    fourth row holds small integers with ties and must return the FIRST maximal available action, and q exactly."""
    lib = abi.load_library()
    rng = np.random.default_rng(1000 + A)
    pow2 = A & (A - 1) == 0
    tally = dict(rows=0, explored=0, greedy=0, skipped=0, q_err=0.0, launches=0)
    worst_skip = 0.0
    dev = dict(device="cuda")
    eps_t = {e: th.tensor(e, dtype=th.float32, **dev) for e in PICK_EPS}
    step_t = {s: th.tensor([s], dtype=th.long, **dev) for s in PICK_STEPS}
    for pairs, n, B in PICK_SHAPES:
        R = n * B * (n if pairs else 1)
        seed = PICK_SEED ^ xu.INC_SEED_XOR if pairs else PICK_SEED
        av_np, tie = _pick_inputs(A, R, rng, pow2)
        q64, bar = _q_bar(av_np, A)
        q64, bar, tie = _env_major(q64, n, B, pairs), _env_major(bar, n, B, pairs), _env_major(tie, n, B, pairs)
        av = th.from_numpy(av_np).cuda()
        actions = th.zeros((B, n, n) if pairs else (B, n), dtype=th.long, **dev)
        q_out = th.zeros(R, A, **dev)
        drawn = {}
        for base in (0, BASE):
            keys = (xu.inc_keys if pairs else xu.env_keys)(B, n, base)
            for step in PICK_STEPS:
                drawn[base, step] = xu.draws(seed, step, keys)
            assert (drawn[base, 17][0] == drawn[base, 2 ** 32 + 17][0]).all() and not (drawn[base, 17][0] == drawn[base, 0][0]).all()
        for mask in _masks(A):
            bits = xu.avail_bits(mask, A)
            mask_t = None if mask is None else th.tensor([255 if (v and k & 1) else v for k, v in enumerate(mask)], dtype=th.uint8, **dev)
            gap = _top_gap(q64, bits, A)
            below = float((~tie & ~(gap > 2 * bar)).sum()) / max(1, int((~tie).sum()))
            worst_skip = max(worst_skip, below)
            assert below <= 0.01, (pairs, n, mask, below)                     # a property of the float64 reference and the inputs alone
            for (base, step), (x0, x1) in drawn.items():
                picked = xu.pick(x1, bits, A)
                for k, eps in enumerate(PICK_EPS):
                    want_q = (k + tally["launches"]) % 2 == 0                 # q_out is nullable: every other launch goes without
                    q_out.fill_(float("nan"))
                    _launch_pick(lib, av, R, A, mask_t, eps_t[eps], step_t[step], seed, n, B, pairs, actions, q_out if want_q else None, base)
                    act = actions.cpu().numpy()
                    q_dev = _env_major(q_out.cpu().numpy(), n, B, pairs) if want_q else None
                    flag = xu.explores(x0, eps)
                    assert flag.all() if eps >= 1 else (not flag.any() if eps == 0 else True)
                    _check_pick_launch(act, q_dev, q64, bar, gap, tie, flag, picked, bits, A, pairs, tally,
                                       (A, pairs, n, B, mask, base, step, eps))
                    tally["launches"] += 1
    print("ssd_dueling_pick A = %d: %d launches, %d rows, %d explored rows equal the restated pick, %d greedy rows equal the float64 first "
          "maximum, %d near-tie rows skipped (%.2e of the rows; worst input %.2e), 0 mismatches; max q error %.3f of the bar"
          % (A, tally["launches"], tally["rows"], tally["explored"], tally["greedy"], tally["skipped"], tally["skipped"] / tally["rows"],
             worst_skip, tally["q_err"]))
    assert tally["explored"] > 0 and tally["greedy"] > 0


@pytest.mark.gpu
def test_dueling_pick_on_a_grid_that_strides_twice():
    """n = 10, pairs, B = 10 500: 1 050 000 rows on the kernel's grid of at most 4096 x 256 threads -- the last 1424 rows are second
    trips.  A = 3, no mask, epsilon 0.3, a non-zero env_id_base; same checks as above, plus the explored share within 4 sigma of 0.3."""
    lib = abi.load_library()
    A, n, B, pairs, eps, step = 3, 10, 10500, 1, 0.3, 17
    R = n * B * n
    assert R > 4096 * 256
    rng = np.random.default_rng(77)
    av_np, _ = _pick_inputs(A, R, rng, False)
    q64, bar = _q_bar(av_np, A)
    q64, bar = _env_major(q64, n, B, pairs), _env_major(bar, n, B, pairs)
    tie = np.zeros(bar.shape, dtype=bool)
    av = th.from_numpy(av_np).cuda()
    actions = th.zeros(B, n, n, dtype=th.long, device="cuda")
    q_out = th.full((R, A), float("nan"), device="cuda")
    seed = PICK_SEED ^ xu.INC_SEED_XOR
    _launch_pick(lib, av, R, A, None, th.tensor(eps, device="cuda"), th.tensor([step], dtype=th.long, device="cuda"), seed, n, B, pairs,
                 actions, q_out, BASE)
    act, q_dev = actions.cpu().numpy(), _env_major(q_out.cpu().numpy(), n, B, pairs)
    bits = xu.avail_bits(None, A)
    x0, x1 = xu.draws(seed, step, xu.inc_keys(B, n, BASE))
    flag = xu.explores(x0, eps)
    gap = _top_gap(q64, bits, A)
    tally = dict(rows=0, explored=0, greedy=0, skipped=0, q_err=0.0)
    _check_pick_launch(act, q_dev, q64, bar, gap, tie, flag, xu.pick(x1, bits, A), bits, A, pairs, tally, "strided")
    z = _z(int(flag.sum()), R, eps)
    print("strided launch: %d rows, %d explored (z = %+.2f), %d greedy, %d near-tie rows skipped (%.2e), max q error %.3f of the bar"
          % (R, tally["explored"], z, tally["greedy"], tally["skipped"], tally["skipped"] / R, tally["q_err"]))
    assert abs(z) < Z_BAR and tally["skipped"] <= 0.01 * R


#                  step   row  x0 >> 8   (found by a host search over the restatement: seed PICK_SEED, n = 1, env_id_base 0)
ON_THE_THRESHOLD = [(11712, 15, 0), (143241, 199, 0), (15987, 139, 1), (51724, 61, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("step,row,u", ON_THE_THRESHOLD)
def test_dueling_pick_compares_strictly_below_epsilon(step, row, u):
    """Draws whose 24-bit uniform is exactly 0 or 2^-24: u = 0 explores at epsilon 2^-24 and not at 0; u = 2^-24 explores at 2^-23 and not
    at 2^-24 (`<`, not `<=`).  Every row's greedy action is set one past its restated pick, so the stored action tells which was taken."""
    lib = abi.load_library()
    A, n, B = 3, 1, 203
    x0, x1 = xu.draws(PICK_SEED, step, xu.env_keys(B, n, 0))
    assert int(x0[row, 0]) >> 8 == u
    picks = xu.pick(x1, 0b111, A)
    greedy = (picks + 1) % A
    av_np = np.zeros((B, A + 1), dtype=np.float32)
    av_np[np.arange(B), greedy[:, 0]] = 1.0
    av = th.from_numpy(av_np).cuda()
    actions = th.zeros(B, n, dtype=th.long, device="cuda")
    step_t = th.tensor([step], dtype=th.long, device="cuda")
    for eps, explores in ((0.0, False), (2.0 ** -24, u == 0), (2.0 ** -23, True)):
        flag = xu.explores(x0, eps)
        assert bool(flag[row, 0]) == explores
        _launch_pick(lib, av, B, A, None, th.tensor(eps, dtype=th.float32, device="cuda"), step_t, PICK_SEED, n, B, 0, actions, None, 0)
        act = actions.cpu().numpy()
        assert (act == np.where(flag, picks, greedy)).all(), (eps, int(act[row, 0]), int(picks[row, 0]))


# ---- GPU (b): the matrix-core heads---------------------------------------------------------------------------------------------------
HEAD_SEED = 0x2545F491
HEAD_EPS = 0.3
HEAD_STEPS = (17, 18)
_BY_ID = {c.id: c for c in pc.CASES}
# one unlooped and one looping case of each head generation, both action counts among them; the table's own rows where it has one,
# else a 203-env row of the same shape family (the table's GEN 2 / 3 heads and its run-time-geometry fused launches all loop)
HEAD_CASES = [_BY_ID[k] for k in ("cleanup5-gen0-203", "harvest10-gen0-loop", "harvest5-gen1-203", "cleanup10-gen1-loop",
                                  "harvest10-gen2-loop", "cleanup10-gen3-loop")] + [
    pc._heads("cleanup5-gen2-203", "cleanup", "default5", 5, 203, pc.GEN2, False),
    pc._heads("harvest5-gen3-203", "harvest", "default10", 5, 203, pc.GEN3, False)]
FUSED_CASES = [_BY_ID[k] for k in ("cleanup5-v7-203", "harvest10-v7-loop-bt4", "harvest5-v15-96", "cleanup10-v3-any-loop",
                                   "harvest10-v3-gen2-loop", "cleanup10-v3-gen3-loop")] + [
    pc._fused("harvest5-v3-any-203", "harvest", "default10", 5, 203, 3, False, pipeline="pipeline_any_view", layouts=pc.LUT),
    pc._fused("cleanup5-v3-gen2-203", "cleanup", "default5", 5, 203, 3, False, flags=pc.GEN2, pipeline="pipeline_gathered", layouts=pc.LUT),
    pc._fused("harvest5-v3-gen3-203", "harvest", "default10", 5, 203, 3, False, flags=pc.GEN3, pipeline="pipeline_gathered", layouts=pc.LUT)]


def _declared_plan(case, N):
    """the case's declared LOOP holds on this device (else skip before any work, like tests/test_policy_instantiations.py)"""
    cus = th.cuda.get_device_properties(0).multi_processor_count
    plans = pc.plans_for(case, cus, N)
    mode = pc.MODE_FUSED if case.test == "fused" else pc.standalone_mode(case)
    assert abi.policy_head_plan(N, case.n, mode) == plans[mode]
    if (plans[mode][2] > 1) != case.loop:
        pytest.skip("%d compute units: %d envs x %d agents plan as %s" % (cus, N, case.n, plans))
    return plans[mode]


def _check_head_launch(act, q, seed, step, keys, bits, A, inc, label):
    """actions [N, n(, n)] and the launch's own q_out, env-major, against the restatement: (rows, explored rows, z of the explored share)"""
    want, flag = xu.expected_actions(seed, step, keys, HEAD_EPS, bits, A, q, zero_diagonal=inc)
    n = act.shape[-1]
    if inc:
        assert (act[..., np.arange(n), np.arange(n)] == 0).all(), label
    bad = act != want
    assert not bad.any(), (label, int(bad.sum()), int((bad & flag).sum()), np.argwhere(bad)[:4].tolist())
    z = _z(int(flag.sum()), flag.size, HEAD_EPS)
    assert abs(z) < Z_BAR, (label, z)                      # the launch explores: the case cannot pass on greedy rows alone
    return flag.size, int(flag.sum()), z


def _shipped_bits(avail, A):
    mask = avail.cpu().tolist()
    assert len(mask) == A and not any(mask[5:8]) and all(mask[:5])              # the shipped mask: holes at 5, 6, 7
    return xu.avail_bits(mask, A)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HEAD_CASES, ids=[c.id for c in HEAD_CASES])
def test_standalone_heads_pick_what_the_restatement_picks(case):
    """FastPolicy.act_env / act_inc (k_head<env> and k_head<inc> of the case's GEN) on live inputs at epsilon 0.3, steps 17 and 18:
    precision 2 with a non-zero env_id_base, the bf16 precision 1 with base 0."""
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_policy_instantiations import _live_inputs, _setup
    N = pc.resolve_n_env(case, th.cuda.get_device_properties(0).multi_processor_count)
    plan = _declared_plan(case, N)
    th.manual_seed(2)
    ctx = _setup(case, N)
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    assert A == pc.n_actions(case.kind)
    d, _ = _live_inputs(case, ctx, N)
    avail = env.avail_actions_batch[0, 0]
    bits = _shipped_bits(avail, A)
    eps = th.full((), HEAD_EPS, device="cuda")
    for prec in case.precisions:
        base = BASE if prec == 2 else 0
        fp = FastPolicy(mac, N, avail, seed=HEAD_SEED, precision=prec, env_id_base=base)
        assert fp.fused and fp.fused_enc and fp.gather == (pc.gen_of(case.flags, 1) == 3)
        for step_v in HEAD_STEPS:
            step = th.full((1,), step_v, dtype=th.long, device="cuda")
            qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
            fp.h_env.copy_(d["h0e"].transpose(0, 1)); fp.h_inc.copy_(d["h0i"].transpose(0, 1))
            a = fp.act_env(None, d["prev_a"], d["prev_r"], d["prev_i"], d["pos"], eps, step, codes=d["codes"], q_out=qe).clone()
            ai = fp.act_inc(a, d["pos"], d["orient"], d["reward"], d["clean"], d["den"], eps, step, q_out=qi).clone()
            th.cuda.synchronize()
            label = (case.id, prec, step_v)
            re = _check_head_launch(a.cpu().numpy(), qe.transpose(0, 1).cpu().numpy(), HEAD_SEED, step_v, xu.env_keys(N, n, base), bits, A,
                                    False, label + ("env",))
            ri = _check_head_launch(ai.cpu().numpy(), qi.transpose(0, 1).cpu().numpy(), HEAD_SEED ^ xu.INC_SEED_XOR, step_v,
                                    xu.inc_keys(N, n, base), 0b111, 3, True, label + ("inc",))
            print("%s N=%d plan %s precision %d step %d base %d: env %d rows, %d explored (z %+.2f); inc %d rows, %d explored (z %+.2f); "
                  "0 mismatches" % ((case.id, N, plan, prec, step_v, base) + re + ri))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=[c.id for c in FUSED_CASES])
def test_fused_launches_pick_what_the_restatement_picks(case, monkeypatch):
    """FastPolicy.act_inc_encode (k_inc_encode / _any / _gather: the inc head's pick site inside the fused launch) at every
    (precision, encoder layout) the case lists, epsilon 0.3, steps 17 and 18."""
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_policy_instantiations import _live_inputs, _setup
    monkeypatch.delenv("SSD_ENC_LAYOUT", raising=False)
    N = pc.resolve_n_env(case, th.cuda.get_device_properties(0).multi_processor_count)
    plan = _declared_plan(case, N)
    th.manual_seed(5)
    ctx = _setup(case, N, **({case.pipeline: True} if case.pipeline else {}))
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    assert A == pc.n_actions(case.kind) and env.native.V == 2 * case.view + 1
    d, g = _live_inputs(case, ctx, N, steps=4)
    eps = th.full((), HEAD_EPS, device="cuda")
    for layout in case.layouts:
        mac.args.enc_layout = layout
        for prec in case.precisions:
            base = BASE if prec == 2 else 0
            fp = FastPolicy(mac, N, env.avail_actions_batch[0, 0], seed=HEAD_SEED, precision=prec, env_id_base=base)
            assert fp.fused and fp.fused_enc and fp.inc_encode
            fp.inputs_pair.copy_(th.randn(fp.inputs_pair.shape, generator=g, device="cuda") * 0.5)
            par = {}
            if fp.prev_rec is not None:
                rec = th.randint(0, A, fp.prev_rec.shape, generator=g, device="cuda").to(th.uint8)
                rec.view(-1)[::5] = 0xFF
                fp.prev_rec.copy_(rec)
                par = dict(par=1)
            for step_v in HEAD_STEPS:
                step = th.full((1,), step_v, dtype=th.long, device="cuda")
                q = th.zeros(n, N, n, 3, device="cuda")
                fp.h_inc.copy_(d["h0i"].transpose(0, 1))
                ai = fp.act_inc_encode(d["act"], d["pos"], d["orient"], d["reward"], d["clean"], d["den"], eps, step, d["codes"], buf=0,
                                       q_out=q, **par).clone()
                th.cuda.synchronize()
                r = _check_head_launch(ai.cpu().numpy(), q.transpose(0, 1).cpu().numpy(), HEAD_SEED ^ xu.INC_SEED_XOR, step_v,
                                       xu.inc_keys(N, n, base), 0b111, 3, True, (case.id, layout, prec, step_v))
                print("%s N=%d plan %s %s precision %d step %d base %d: %d rows, %d explored (z %+.2f), 0 mismatches"
                      % ((case.id, N, plan, layout, prec, step_v, base) + r))
    env.close()


# ---- GPU (c): the runner's draw counter ------------------------------------------------------------------------------------------------
RUN_SEED = 21                               # env_args.seed: the runner seeds FastPolicy with seed * 2654435761 + 12345
RUN_ENVS = 48
RUN_EPISODES = 4                            # eager, captured, replayed, replayed with the episode-edge graphs
SHIPPED = {}


def _runner_cases():
    from tests.test_inc_encode_gathered import RUNNER_CASES
    rows = [(kind, mapname, n, view, storage, flags, "pipeline_gathered", 14) for kind, mapname, n, view, storage, flags in RUNNER_CASES]
    rows.append(("cleanup", "default5", 5, 3, "code", SHIPPED, "pipeline_any_view", 14))
    kind, mapname, n, view, storage, flags = RUNNER_CASES[0]
    rows.append((kind, mapname, n, view, storage, flags, "pipeline_gathered", 13))           # odd T: eager timesteps, no graph
    return rows


RUNNER_ROWS = _runner_cases()


def expected_step(episode, t, T):
    """The counter contract (include/ssd_hip.h; hip_graph_runner.py: plan_runner, _fast_stages): the draw counter starts at
    RunnerPlan.counter_start, is never reset, and advances once per timestep slot, the closing slot T included.  Four-launch timestep:
    starts at 0, the encoder (ssd_policy_encode_args.counter_inc) advances it BEFORE the heads of the slot read it -- slot t of episode e
    is preceded by e (T + 1) + t slots, so its heads read e (T + 1) + t + 1.  Pipelined timestep: starts at 1 (every layout this test
    runs: a window edge other than 15 / 31, or a gathered layout), the inc head advances it AFTER both heads read it (next_step_out =
    *step + 1; the env head hands its copy to the inc head) -- 1 + e (T + 1) + t again."""
    return 1 + episode * (T + 1) + t


def _run_episodes(kind, mapname, n, view, storage, flags, key, on, T):
    from homophily_marl_amd.run import setup
    from tests.test_inc_encode_gathered import _cfg
    th.manual_seed(0)
    cfg = _cfg(kind, mapname, n, RUN_ENVS, view, T=T, seed=RUN_SEED, runner="hip_graph", obs_storage=storage, steps_per_graph=2,
               epsilon_start=0.5, epsilon_finish=0.05, epsilon_anneal_time=8 * T, **dict(flags, **{key: on}))
    ctx = setup(cfg)
    r = ctx.runner
    out = []
    for ep in range(RUN_EPISODES):
        batch = r.run(test_mode=False)
        assert r.fast is not None and r.fold_store and r.pipe == on and r.fast.inc_encode == on
        assert (r._graph is not None) == (ep > 0 and T % 2 == 0)
        out.append((batch["actions"].squeeze(-1).cpu().numpy().copy(), batch["actions_inc"].squeeze(-1).cpu().numpy().copy()))
    assert T % 2 or r._bundle.begin_graph is not None                        # the last episode opened and closed as graph replays
    th.cuda.synchronize()
    info = dict(counter=int(r.rng_ctr), seed=r.fast.seed, base=r.fast.env_id_base, unit=ctx.args.schedule_unit,
                avail=r.env.avail_actions_batch[0, 0].clone(), A=ctx.args.n_actions, cfg=cfg)
    r.close_env()
    return out, info


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mapname,n,view,storage,flags,key,T", RUNNER_ROWS,
                         ids=["%s%d-v%d-%s-%s-T%d" % (c[0], c[2], c[3], c[4], c[6], c[7]) for c in RUNNER_ROWS])
def test_runner_draw_counter_follows_the_contract(kind, mapname, n, view, storage, flags, key, T):
    """hip_graph at 48 envs, steps_per_graph 2, exploring (epsilon 0.5 annealed linearly over 8 rollouts), four episodes with the
    pipelined timestep (the key set) and four with the four-launch timestep: at every explore-flagged position of every slot the stored
    action of both heads equals the restated pick at step expected_step(episode, t, T) (see its docstring for the derivation); the
    flagged share of every slot is within 4 sigma of the episode's epsilon, evaluated here from the config's schedule; consecutive slots
    flag different rows; the counter ends at counter_start + episodes (T + 1).  The same comparison one step late must fail (the check
    has power)."""
    from homophily_marl_amd.components.epsilon_schedules import DecayThenFlatSchedule
    seed_env = (RUN_SEED * 2654435761 + 12345) & xu.M32
    N = RUN_ENVS
    ek, ik = xu.env_keys(N, n, 0), xu.inc_keys(N, n, 0)
    off = ~np.broadcast_to(np.eye(n, dtype=bool), (N, n, n))
    for on in (True, False):
        episodes, info = _run_episodes(kind, mapname, n, view, storage, flags, key, on, T)
        cfg, A = info["cfg"], info["A"]
        assert info["seed"] == seed_env and info["base"] == 0 and info["unit"] == "rollouts"
        assert info["counter"] == int(on) + RUN_EPISODES * (T + 1)
        bits = xu.avail_bits(info["avail"].cpu().tolist(), A)
        sched = DecayThenFlatSchedule(cfg["epsilon_start"], cfg["epsilon_finish"], cfg["epsilon_anneal_time"], decay="linear")
        assert cfg.get("epsilon_zero") is None
        checked = late = late_hit = 0
        worst = 0.0
        prev = None
        for ep, (acts, incs) in enumerate(episodes):
            eps = sched.eval(ep * T)                     # schedule_unit "rollouts": the clock advances by episode_limit per rollout
            assert acts.shape == (N, T + 1, n) and incs.shape == (N, T + 1, n, n) and 0.05 < eps <= 0.5
            for t in range(T + 1):
                step = expected_step(ep, t, T)
                e0, e1 = xu.draws(seed_env, step, ek)
                i0, i1 = xu.draws(seed_env ^ xu.INC_SEED_XOR, step, ik)
                fe, fi = xu.explores(e0, eps), xu.explores(i0, eps)
                a, ai = acts[:, t], incs[:, t]
                assert (a[fe] == xu.pick(e1, bits, A)[fe]).all(), (on, ep, t, "env")
                assert (ai[fi & off] == xu.pick(i1, 0b111, 3)[fi & off]).all(), (on, ep, t, "inc")
                assert (ai[~off] == 0).all() and (((bits >> a) & 1) == 1).all()
                checked += int(fe.sum()) + int((fi & off).sum())
                for f in (fe, fi):
                    z = _z(int(f.sum()), f.size, eps)
                    worst = max(worst, abs(z))
                    assert abs(z) < Z_BAR, (on, ep, t, z)
                assert prev is None or not ((prev[0] == fe).all() or (prev[1] == fi).all()), (on, ep, t)
                prev = (fe, fi)
                l0, l1 = xu.draws(seed_env, step + 1, ek)                      # one step late: other rows, other picks
                lf = xu.explores(l0, eps)
                late += int(lf.sum())
                late_hit += int((a[lf] == xu.pick(l1, bits, A)[lf]).sum())
        print("%s %s=%s T=%d: %d flagged positions of %d episodes equal the restated pick at step 1 + e (T + 1) + t; worst |z| of a slot's "
              "flagged share %.2f; one step late only %d of %d match; counter ends at %d"
              % (kind, key, on, T, checked, RUN_EPISODES, worst, late_hit, late, info["counter"]))
        assert checked > 0 and late_hit < 0.9 * late
