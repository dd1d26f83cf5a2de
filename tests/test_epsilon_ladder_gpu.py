"""A rate per env in the fused rollout heads (ssd_policy_head.epsilon_rows; FastPolicy's eps_rows; config key epsilon_ladder_alpha): every
pick site of k_head / k_inc_encode / _any / _gather held to the host restatement (tests/explore_util.py) with a table of rates as its
epsilon, by EXACT equality on the launch's own Q values; then the runner's table and the stored actions of whole rollouts, and the
loop with the key off.  Cases, sizes and helpers are those of tests/test_exploration_draws.py and tests/test_policy_instantiations.py.

The table is deliberately NOT monotone (uniform values, rows ::7 at 0, rows 3::11 at 1), so that a wrong row index shows: a tile-local
row, an agent-major row, another pass's tile of a looping wave.  At N = 203, n = 5 about half of the rows are flagged under it: no
launch passes on greedy rows alone.  Every equality is followed by its power check: the same comparison against the table rolled by one
row, and against the table's mean as a scalar, must produce mismatches."""
import numpy as np
import pytest
import torch as th

from tests import explore_util as xu
from tests import policy_cases as pc
from tests.test_exploration_draws import (BASE, FUSED_CASES, HEAD_CASES, HEAD_SEED, HEAD_STEPS, RUN_ENVS, RUN_EPISODES, RUN_SEED, RUNNER_ROWS,
                                          Z_BAR, _declared_plan, _shipped_bits, expected_step)

TABLE_SEED = 0xE95


def _table(N):
    """f32 uniform on [0, 1), rows ::7 = 0 (never explore), rows 3::11 = 1 (always explore)"""
    t = np.random.default_rng(TABLE_SEED).random(N, dtype=np.float32)
    t[::7] = 0.0
    t[3::11] = 1.0
    return t


def _rows(table, inc):
    return table[:, None, None] if inc else table[:, None]


def _check_table_launch(act, q, seed, step, keys, table, bits, A, inc, label, power=True):
    """actions [N, n(, n)] and the launch's own q_out, env-major, against the restatement with the table as its epsilon: 0 mismatches;
    rows at rate 0 are never flagged and rows at rate 1 always (both sets non-empty); the comparison has power"""
    want, flag = xu.expected_actions(seed, step, keys, _rows(table, inc), bits, A, q, zero_diagonal=inc)
    bad = act != want
    assert not bad.any(), (label, int(bad.sum()), int((bad & flag).sum()), np.argwhere(bad)[:4].tolist())
    never, always = flag[table == 0.0], flag[table == 1.0]
    assert never.size > 0 and always.size > 0 and not never.any() and always.all(), label
    assert 0.3 * flag.size < flag.sum() < 0.7 * flag.size, (label, int(flag.sum()), flag.size)      # cannot pass on greedy rows alone
    if power:
        rolled, _ = xu.expected_actions(seed, step, keys, _rows(np.roll(table, 1), inc), bits, A, q, zero_diagonal=inc)
        scalar, _ = xu.expected_actions(seed, step, keys, float(table.mean()), bits, A, q, zero_diagonal=inc)
        assert (act != rolled).sum() > 0 and (act != scalar).sum() > 0, label
        return flag.size, int(flag.sum()), int((act != rolled).sum()), int((act != scalar).sum())
    return flag.size, int(flag.sum()), 0, 0


# ---- 1. the standalone heads ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", HEAD_CASES, ids=[c.id for c in HEAD_CASES])
def test_standalone_heads_explore_at_the_rows_own_rate(case):
    """FastPolicy.act_env / act_inc with eps_rows (k_head<env> and k_head<inc> of the case's GEN, unlooped or looping as the case says)
    at steps 17 and 18: precision 2 with a non-zero env_id_base, precision 1 with base 0.  The scalar eps they also get is 0.3 and is
    not what any row explores at."""
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_policy_instantiations import _live_inputs, _setup
    N = pc.resolve_n_env(case, th.cuda.get_device_properties(0).multi_processor_count)
    plan = _declared_plan(case, N)
    th.manual_seed(2)
    ctx = _setup(case, N)
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    d, _ = _live_inputs(case, ctx, N)
    avail = env.avail_actions_batch[0, 0]
    bits = _shipped_bits(avail, A)
    table = _table(N)
    rows = th.from_numpy(table).cuda()
    eps = th.full((), 0.3, device="cuda")
    for prec in case.precisions:
        base = BASE if prec == 2 else 0
        fp = FastPolicy(mac, N, avail, seed=HEAD_SEED, precision=prec, env_id_base=base)
        assert fp.fused and fp.fused_enc
        for step_v in HEAD_STEPS:
            step = th.full((1,), step_v, dtype=th.long, device="cuda")
            qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
            fp.h_env.copy_(d["h0e"].transpose(0, 1)); fp.h_inc.copy_(d["h0i"].transpose(0, 1))
            a = fp.act_env(None, d["prev_a"], d["prev_r"], d["prev_i"], d["pos"], eps, step, codes=d["codes"], q_out=qe, eps_rows=rows).clone()
            ai = fp.act_inc(a, d["pos"], d["orient"], d["reward"], d["clean"], d["den"], eps, step, q_out=qi, eps_rows=rows).clone()
            th.cuda.synchronize()
            label = (case.id, prec, step_v)
            re = _check_table_launch(a.cpu().numpy(), qe.transpose(0, 1).cpu().numpy(), HEAD_SEED, step_v, xu.env_keys(N, n, base), table, bits, A,
                                     False, label + ("env",))
            ri = _check_table_launch(ai.cpu().numpy(), qi.transpose(0, 1).cpu().numpy(), HEAD_SEED ^ xu.INC_SEED_XOR, step_v,
                                     xu.inc_keys(N, n, base), table, 0b111, 3, True, label + ("inc",))
            print("%s N=%d plan %s precision %d step %d base %d: env %d rows, %d explored, 0 mismatches (rolled table %d, scalar mean %d); "
                  "inc %d rows, %d explored, 0 mismatches (rolled %d, scalar %d)" % ((case.id, N, plan, prec, step_v, base) + re + ri))
    env.close()


# ---- 2. the fused launches --------------------------------------------------------------------------------------------------------------
def _fused_policy(case, mac, env, N, prec, layout, g, A):
    from homophily_marl_amd.fast_policy import FastPolicy
    mac.args.enc_layout = layout
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
    return fp, base, par


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=[c.id for c in FUSED_CASES])
def test_fused_launches_explore_at_the_rows_own_rate(case, monkeypatch):
    """FastPolicy.act_inc_encode with eps_rows (k_inc_encode / _any / _gather: the inc head's pick site inside the fused launch) at every
    (precision, encoder layout) the case lists, steps 17 and 18."""
    from tests.test_policy_instantiations import _live_inputs, _setup
    monkeypatch.delenv("SSD_ENC_LAYOUT", raising=False)
    N = pc.resolve_n_env(case, th.cuda.get_device_properties(0).multi_processor_count)
    plan = _declared_plan(case, N)
    th.manual_seed(5)
    ctx = _setup(case, N, **({case.pipeline: True} if case.pipeline else {}))
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    d, g = _live_inputs(case, ctx, N, steps=4)
    table = _table(N)
    rows = th.from_numpy(table).cuda()
    eps = th.full((), 0.3, device="cuda")
    for layout in case.layouts:
        for prec in case.precisions:
            fp, base, par = _fused_policy(case, mac, env, N, prec, layout, g, A)
            for step_v in HEAD_STEPS:
                step = th.full((1,), step_v, dtype=th.long, device="cuda")
                q = th.zeros(n, N, n, 3, device="cuda")
                fp.h_inc.copy_(d["h0i"].transpose(0, 1))
                ai = fp.act_inc_encode(d["act"], d["pos"], d["orient"], d["reward"], d["clean"], d["den"], eps, step, d["codes"], buf=0,
                                       q_out=q, eps_rows=rows, **par).clone()
                th.cuda.synchronize()
                r = _check_table_launch(ai.cpu().numpy(), q.transpose(0, 1).cpu().numpy(), HEAD_SEED ^ xu.INC_SEED_XOR, step_v,
                                        xu.inc_keys(N, n, base), table, 0b111, 3, True, (case.id, layout, prec, step_v))
                print("%s N=%d plan %s %s precision %d step %d base %d: %d rows, %d explored, 0 mismatches (rolled table %d, scalar mean %d)"
                      % ((case.id, N, plan, layout, prec, step_v, base) + r))
    env.close()


# ---- 3. a constant table is the scalar -----------------------------------------------------------------------------------------------
_BY_ID = {c.id: c for c in HEAD_CASES + FUSED_CASES}


@pytest.mark.gpu
def test_constant_table_picks_what_the_scalar_picks_dense_heads():
    """a table of the constant 0.3 against the scalar 0.3 (the table path and the scalar path of the same kernels), both on the device,
    each against the restatement: the dense standalone heads"""
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_policy_instantiations import _live_inputs, _setup
    case = _BY_ID["cleanup5-gen0-203"]
    N = case.N
    th.manual_seed(2)
    ctx = _setup(case, N)
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    d, _ = _live_inputs(case, ctx, N)
    avail = env.avail_actions_batch[0, 0]
    bits = _shipped_bits(avail, A)
    eps = th.full((), 0.3, device="cuda")
    const = th.full((N,), 0.3, device="cuda")
    other = th.full((), 0.9, device="cuda")                 # with a table the scalar is not read for the rows
    step = th.full((1,), 17, dtype=th.long, device="cuda")
    fp = FastPolicy(mac, N, avail, seed=HEAD_SEED, precision=2, env_id_base=BASE)
    got = []
    for e, rows in ((eps, None), (other, const)):
        qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
        fp.h_env.copy_(d["h0e"].transpose(0, 1)); fp.h_inc.copy_(d["h0i"].transpose(0, 1))
        a = fp.act_env(None, d["prev_a"], d["prev_r"], d["prev_i"], d["pos"], e, step, codes=d["codes"], q_out=qe, eps_rows=rows).clone()
        ai = fp.act_inc(a, d["pos"], d["orient"], d["reward"], d["clean"], d["den"], e, step, q_out=qi, eps_rows=rows).clone()
        th.cuda.synchronize()
        we, fe = xu.expected_actions(HEAD_SEED, 17, xu.env_keys(N, n, BASE), 0.3, bits, A, qe.transpose(0, 1).cpu().numpy())
        wi, fi = xu.expected_actions(HEAD_SEED ^ xu.INC_SEED_XOR, 17, xu.inc_keys(N, n, BASE), 0.3, 0b111, 3, qi.transpose(0, 1).cpu().numpy(),
                                     zero_diagonal=True)
        assert (a.cpu().numpy() == we).all() and (ai.cpu().numpy() == wi).all() and fe.any() and fi.any() and not fe.all()
        got.append((a, ai, qe, qi))
    for x, y in zip(*got):
        assert th.equal(x, y)
    env.close()


@pytest.mark.gpu
def test_constant_table_picks_what_the_scalar_picks_gathered_fused_launch(monkeypatch):
    """the same for the gathered fused launch (k_inc_encode_gather)"""
    from tests.test_policy_instantiations import _live_inputs, _setup
    monkeypatch.delenv("SSD_ENC_LAYOUT", raising=False)
    case = _BY_ID["cleanup5-v3-gen2-203"]
    N = case.N
    th.manual_seed(5)
    ctx = _setup(case, N, **{case.pipeline: True})
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    d, g = _live_inputs(case, ctx, N, steps=4)
    fp, base, par = _fused_policy(case, mac, env, N, 2, "lut", g, A)
    eps, other = th.full((), 0.3, device="cuda"), th.full((), 0.9, device="cuda")
    const = th.full((N,), 0.3, device="cuda")
    step = th.full((1,), 18, dtype=th.long, device="cuda")
    got = []
    for e, rows in ((eps, None), (other, const)):
        q = th.zeros(n, N, n, 3, device="cuda")
        fp.h_inc.copy_(d["h0i"].transpose(0, 1))
        ai = fp.act_inc_encode(d["act"], d["pos"], d["orient"], d["reward"], d["clean"], d["den"], e, step, d["codes"], buf=0, q_out=q,
                               eps_rows=rows, **par).clone()
        th.cuda.synchronize()
        wi, fi = xu.expected_actions(HEAD_SEED ^ xu.INC_SEED_XOR, 18, xu.inc_keys(N, n, base), 0.3, 0b111, 3, q.transpose(0, 1).cpu().numpy(),
                                     zero_diagonal=True)
        assert (ai.cpu().numpy() == wi).all() and fi.any() and not fi.all()
        got.append((ai, q))
    for x, y in zip(*got):
        assert th.equal(x, y)
    env.close()


@pytest.mark.gpu
def test_eps_rows_is_refused_by_name():
    """a wrong shape, dtype or device raises naming eps_rows; the per-layer path refuses the table; the entry point refuses a misaligned
    pointer (SSD_ERR_INVALID) before any launch"""
    import ctypes as C
    from homophily_marl_amd import abi
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_policy_mfma import _ctx
    N, n = 32, 5
    ctx = _ctx("cleanup", n, N)
    mac, env = ctx.mac, ctx.runner.env
    avail = env.avail_actions_batch[0, 0]
    fp = FastPolicy(mac, N, avail, seed=11)
    ok = th.zeros(N, device="cuda")
    assert fp._check_eps_rows(ok) == ok.data_ptr()
    for bad in (th.zeros(N + 1, device="cuda"), th.zeros(N, 1, device="cuda"), th.zeros(2 * N, device="cuda")[::2], th.zeros(N)):
        with pytest.raises(ValueError, match="eps_rows"):
            fp._check_eps_rows(bad)
    for bad in (th.zeros(N, dtype=th.float64, device="cuda"), th.zeros(N, dtype=th.float16, device="cuda"), [0.0] * N):
        with pytest.raises(TypeError, match="eps_rows"):
            fp._check_eps_rows(bad)
    with pytest.raises(ValueError, match="eps_rows"):
        FastPolicy(mac, N, avail, seed=11, fused=False)._check_eps_rows(ok)
    step, eps = th.zeros(1, dtype=th.long, device="cuda"), th.zeros((), device="cuda")
    ha = fp._head_args(True, eps, step)
    ha.actions = ha.pos_pre = ha.orient_pre = ha.reward = ha.clean_num = ha.apple_den = ha.out_actions = ok.data_ptr()
    ha.epsilon_rows = ok.data_ptr() + 2
    assert fp.lib.ssd_policy_head_inc(C.byref(ha), None) == abi.SSD_ERR_INVALID and b"epsilon_rows" in fp.lib.ssd_last_error()
    env.close()


# ---- 4. shards --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_env_shards_with_the_slices_of_one_table_reproduce_the_unsharded_launch():
    """two 64-env shards (env_id_base 0 / 64) with the two slices of one table choose exactly what one 128-env FastPolicy chooses with
    the whole table -- the table is indexed by the LOCAL env, the draw keyed by the GLOBAL one; env head and incentive head"""
    from homophily_marl_amd import abi
    from homophily_marl_amd.fast_policy import FastPolicy
    from tests.test_policy_mfma import _ctx
    th.manual_seed(1)
    N, n = 128, 5
    ctx = _ctx("cleanup", n, N)
    mac, env = ctx.mac, ctx.runner.env
    A = mac.args.n_actions
    env.reset_batch()
    o = env.observe_batch(out=env.native.obs_buffers(abi.OBS_F32, want_code=True))
    avail = env.avail_actions_batch[0, 0]
    g = th.Generator(device="cuda").manual_seed(0)
    prev_a = th.randint(-1, A, (N, n), generator=g, device="cuda")
    prev_r = th.zeros(N, n, device="cuda"); prev_i = th.zeros(N, n, n, dtype=th.long, device="cuda")
    reward, clean, den = th.zeros(N, n, device="cuda"), th.zeros(N, n, device="cuda"), th.rand(N, n, generator=g, device="cuda")
    eps, step = th.full((), 0.3, device="cuda"), th.full((1,), 5, dtype=th.long, device="cuda")
    table = _table(N)
    rows = th.from_numpy(table).cuda()
    whole = FastPolicy(mac, N, avail, seed=11)
    a_all = whole.act_env(o["obs"], prev_a, prev_r, prev_i, o["pos"], eps, step, codes=o["code"], eps_rows=rows).clone()
    i_all = whole.act_inc(a_all, o["pos"], o["orient"], reward, clean, den, eps, step, eps_rows=rows).clone()
    for k in range(2):
        sl = slice(64 * k, 64 * (k + 1))
        shard = FastPolicy(mac, 64, avail, seed=11, env_id_base=64 * k)
        part = rows[sl].contiguous()
        a_s = shard.act_env(o["obs"][sl].contiguous(), prev_a[sl].contiguous(), prev_r[sl].contiguous(), prev_i[sl].contiguous(),
                            o["pos"][sl].contiguous(), eps, step, codes=o["code"][sl], eps_rows=part)
        assert th.equal(a_s, a_all[sl]), k
        i_s = shard.act_inc(a_all[sl].contiguous(), o["pos"][sl].contiguous(), o["orient"][sl].contiguous(), reward[sl].contiguous(),
                            clean[sl].contiguous(), den[sl].contiguous(), eps, step, eps_rows=part)
        assert th.equal(i_s, i_all[sl]), k
    # the unsharded launch explores at the table's rates (and not, say, at the scalar's): flagged rows hold the restated pick
    x0, x1 = xu.draws(11, 5, xu.env_keys(N, n, 0))
    flag = xu.explores(x0, table[:, None])
    bits = xu.avail_bits(avail.cpu().tolist(), A)
    assert (a_all.cpu().numpy()[flag] == xu.pick(x1, bits, A)[flag]).all() and 0.3 * flag.size < flag.sum() < 0.7 * flag.size
    env.close()


# ---- 5. the runner ----------------------------------------------------------------------------------------------------------------------
LADDER_ALPHA = 7.0


def _run_ladder_episodes(kind, mapname, n, view, storage, flags, key, on, T):
    """RUN_EPISODES training episodes of hip_graph under the ladder, the runner's table read back after every begin_episode; then the
    opening of a test-mode episode"""
    from homophily_marl_amd.run import setup
    from tests.test_inc_encode_gathered import _cfg
    th.manual_seed(0)
    cfg = _cfg(kind, mapname, n, RUN_ENVS, view, T=T, seed=RUN_SEED, runner="hip_graph", obs_storage=storage, steps_per_graph=2,
               epsilon_start=0.5, epsilon_finish=0.05, epsilon_anneal_time=8 * T, epsilon_ladder_alpha=LADDER_ALPHA, **dict(flags, **{key: on}))
    ctx = setup(cfg)
    r = ctx.runner
    out = []
    for ep in range(RUN_EPISODES):
        r.begin_episode(test_mode=False)
        table = r.eps_rows.cpu().numpy().copy()
        scalar = float(r.eps)
        while not r.step_once():
            pass
        batch = r.finish_episode()
        assert r.fast is not None and r.fast.fused and r.fold_store and r.pipe == on
        assert (r._graph is not None) == (ep > 0 and T % 2 == 0)
        out.append((batch["actions"].squeeze(-1).cpu().numpy().copy(), batch["actions_inc"].squeeze(-1).cpu().numpy().copy(), table, scalar))
    assert T % 2 or r._bundle.begin_graph is not None
    r.begin_episode(test_mode=True)
    th.cuda.synchronize()
    test_table = r.eps_rows.cpu().numpy().copy()
    info = dict(seed=r.fast.seed, avail=r.env.avail_actions_batch[0, 0].clone(), A=ctx.args.n_actions, cfg=cfg,
                expo=r.expo.cpu().numpy().copy(), test_table=test_table, test_scalar=float(r.eps))
    r.close_env()
    return out, info


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mapname,n,view,storage,flags,key,T", RUNNER_ROWS,
                         ids=["%s%d-v%d-%s-%s-T%d" % (c[0], c[2], c[3], c[4], c[6], c[7]) for c in RUNNER_ROWS])
def test_runner_explores_along_the_ladder(kind, mapname, n, view, storage, flags, key, T):
    """hip_graph at 48 envs, steps_per_graph 2, epsilon 0.5 -> 0.05 over 8 rollouts, epsilon_ladder_alpha 7; four episodes (eager,
    captured, replayed, with the episode-edge graphs) with the pipelined and with the four-launch timestep.  The runner's table after
    every begin_episode is within 3e-7 (relative) of float64(f32 eps) ** exponent and all zeros in a test-mode episode; with the table
    as the restatement's epsilon, every flagged position of every slot holds the restated pick at expected_step(ep, t, T) in both
    heads; per quarter of the envs, pooled over slots, heads and episodes, the flagged count is within |z| < 4 of the sum of the
    rates (the first episode expects 272 / 79 / 23 / 6.6 env-head flags in the four quarters, hence the pooling).  Power: in the
    greediest quarter the positions the SCALAR 0.5 would flag but the ladder does not hold the pick in fewer than half of the cases."""
    from homophily_marl_amd.components.epsilon_schedules import DecayThenFlatSchedule, ladder_exponents
    seed_env = (RUN_SEED * 2654435761 + 12345) & xu.M32
    N = RUN_ENVS
    ek, ik = xu.env_keys(N, n, 0), xu.inc_keys(N, n, 0)
    off = ~np.broadcast_to(np.eye(n, dtype=bool), (N, n, n))
    quarter = np.arange(N) // (N // 4)
    for on in (True, False):
        episodes, info = _run_ladder_episodes(kind, mapname, n, view, storage, flags, key, on, T)
        cfg, A = info["cfg"], info["A"]
        assert info["seed"] == seed_env
        expo = ladder_exponents(LADDER_ALPHA, 0, N, N)
        assert np.array_equal(info["expo"], expo)
        assert (info["test_table"] == 0.0).all() and info["test_scalar"] == 0.0
        bits = xu.avail_bits(info["avail"].cpu().tolist(), A)
        sched = DecayThenFlatSchedule(cfg["epsilon_start"], cfg["epsilon_finish"], cfg["epsilon_anneal_time"], decay="linear")
        count, mean, var = np.zeros(4), np.zeros(4), np.zeros(4)
        checked = scalar_only = scalar_hit = 0
        worst_rel = 0.0
        for ep, (acts, incs, table, scalar) in enumerate(episodes):
            eps = np.float32(sched.eval(ep * T))
            assert scalar == float(eps) and table.dtype == np.float32 and table.shape == (N,)
            want = np.float64(eps) ** expo.astype(np.float64)
            rel = np.abs(table.astype(np.float64) - want) / want
            worst_rel = max(worst_rel, float(rel.max()))
            print("%s %s=%s T=%d episode %d: eps %.6f, table %.3e .. %.3e, worst relative error against the float64 formula %.3e"
                  % (kind, key, on, T, ep, float(eps), float(table.min()), float(table.max()), float(rel.max())))
            assert rel.max() <= 3e-7, (on, ep, float(rel.max()))
            assert (np.diff(table) < 0).all()                 # (env 0: eps to within the bound above -- the device's pow(x, 1) may round)
            for t in range(T + 1):
                step = expected_step(ep, t, T)
                e0, e1 = xu.draws(seed_env, step, ek)
                i0, i1 = xu.draws(seed_env ^ xu.INC_SEED_XOR, step, ik)
                fe, fi = xu.explores(e0, table[:, None]), xu.explores(i0, table[:, None, None]) & off
                a, ai = acts[:, t], incs[:, t]
                assert (a[fe] == xu.pick(e1, bits, A)[fe]).all(), (on, ep, t, "env")
                assert (ai[fi] == xu.pick(i1, 0b111, 3)[fi]).all(), (on, ep, t, "inc")
                assert (ai[~off] == 0).all()
                checked += int(fe.sum()) + int(fi.sum())
                p = table.astype(np.float64)
                for qd in range(4):
                    rows = quarter == qd
                    count[qd] += fe[rows].sum() + fi[rows].sum()
                    mean[qd] += (n + n * (n - 1)) * p[rows].sum()
                    var[qd] += (n + n * (n - 1)) * (p[rows] * (1 - p[rows])).sum()
                # power: what the scalar would flag and the ladder does not, in the greediest quarter
                only = xu.explores(e0, 0.5) & ~fe & (quarter == 3)[:, None]
                scalar_only += int(only.sum())
                scalar_hit += int((a[only] == xu.pick(e1, bits, A)[only]).sum())
        z = (count - mean) / np.sqrt(var)
        print("%s %s=%s T=%d: %d flagged positions equal the restated pick; flagged per quarter %s, expected %s, z %s; worst table error "
              "%.3e; greediest quarter: %d of %d scalar-only positions hold the pick"
              % (kind, key, on, T, checked, count.astype(int).tolist(), np.round(mean, 1).tolist(), np.round(z, 2).tolist(), worst_rel,
                 scalar_hit, scalar_only))
        assert (np.abs(z) < Z_BAR).all(), (on, z.tolist())
        assert checked > 0 and scalar_only > 0 and scalar_hit < 0.5 * scalar_only


# ---- 6. the default path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_key_zero_is_the_loop_without_the_key():
    """epsilon_ladder_alpha absent against 0: no table, epsilon_rows stays NULL, and the stored bytes, the sampled ids of every call and
    the learner's parameters after four iterations are equal bit for bit"""
    from homophily_marl_amd import ops
    from homophily_marl_amd.run import train_iteration
    from tests.test_rollout_priority_gpu import _ctx
    runs = []
    for drop, over in ((("epsilon_ladder_alpha",), {}), ((), dict(epsilon_ladder_alpha=0))):
        ctx = _ctx(drop=drop, n_env=32, t_ep=12, obs_storage="code", **over)
        try:
            ids = []
            inner = ctx.learner.train

            def train(sample, t_env, episode, ids=ids, inner=inner):
                ids.append(sample.priority[1].cpu().tolist())
                inner(sample, t_env, episode)
            ctx.learner.train = train
            ep = 0
            for _ in range(4):
                ep = train_iteration(ctx, ep)
            th.cuda.synchronize()
            assert ctx.args.epsilon_ladder_alpha == 0.0 and ctx.runner.eps_rows is None and ctx.runner.expo is None
            assert ctx.runner.fast._head_args(False, ctx.runner.eps, ctx.runner.rng_ctr, eps_rows=ctx.runner.eps_rows).epsilon_rows is None
            runs.append((ids, {k: v.cpu().clone() for k, v in ctx.buffer.data.transition_data.items()},
                         [p.detach().cpu().clone() for p in ctx.mac.parameters()], ctx.buffer._sample_calls))
        finally:
            ops.set_strict(False)
            ctx.runner.close_env()
    (ids_a, data_a, par_a, calls_a), (ids_b, data_b, par_b, calls_b) = runs
    assert len(ids_a) == 8 and ids_a == ids_b and calls_a == calls_b
    assert set(data_a) == set(data_b)
    for k in data_a:
        assert th.equal(data_a[k], data_b[k]), k
    assert all(th.equal(a, b) for a, b in zip(par_a, par_b)) and len(par_a) > 0


@pytest.mark.gpu
def test_ladder_statistics_are_logged_next_to_epsilon():
    """with the key on, a log event of the training rollouts carries epsilon_ladder_min = eps ** (1 + alpha) and
    ladder_greedy_return_mean = the mean collective return of the ceil(N / 8) highest-id envs, read with the other runner sums"""
    from homophily_marl_amd.run import setup
    from tests.test_inc_encode_gathered import _cfg
    N, T = 20, 6
    th.manual_seed(0)
    cfg = _cfg("cleanup", "default5", 5, N, 7, T=T, seed=RUN_SEED, runner="hip_graph", obs_storage="code", runner_stats=True,
               runner_log_interval=2 * T, epsilon_start=0.5, epsilon_finish=0.05, epsilon_anneal_time=8 * T, epsilon_ladder_alpha=LADDER_ALPHA)
    ctx = setup(cfg)
    r = ctx.runner
    sums = []
    for _ in range(3):      # the first rollout logs at once (the runner's log clock starts far in the past), then every second one
        r.run(test_mode=False)
        sums.append(float(r.env.native.out["collective_return"][-3:].double().sum()))       # ceil(20 / 8) = 3
    th.cuda.synchronize()
    stats = ctx.logger.stats
    assert len(stats["ladder_greedy_return_mean"]) == 2 and len(stats["return_mean"]) == 2 and len(stats["epsilon"]) == 2
    for k, want in enumerate((sums[0] / 3, (sums[1] + sums[2]) / (2 * 3))):
        eps = stats["epsilon"][k][1]
        assert 0.05 < eps <= 0.5 and abs(stats["epsilon_ladder_min"][k][1] - eps ** (1.0 + LADDER_ALPHA)) <= 1e-15
        assert abs(stats["ladder_greedy_return_mean"][k][1] - want) <= 1e-9 * max(1.0, abs(want)), (k, stats["ladder_greedy_return_mean"], sums)
    assert float(r._stat_buf(False).abs().sum()) == 0.0 and r._stat_buf(False).numel() == 8
    r.close_env()
