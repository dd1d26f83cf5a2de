"""Every instantiation of the rollout head, encoder and pack kernels under test (k_head, k_inc_encode, k_inc_encode_any,
k_inc_encode_gather: templates over precision, action count, GEN, inc, LOOP, window edge, BT, layout; k_encode*, k_pack_*).

CPU: a ledger.  tests/policy_cases.py restates the host dispatch in Python; every compiled kernel must be the kernel some GPU case holds
to a reference, or stand in UNREACHABLE with its reason.  A kernel added without a case fails here.  Plus the refusal of
ssd_policy_head_plan's third argument outside 0 .. 2.
GPU: the restated plan against ssd_policy_head_plan, then
  (a) the standalone heads against the torch controller: assemble_inputs in f32 as the controller builds them (its encoder and tail
      kernel are f32 only), forward_env / forward_inc on a float64 copy of the agent.  Bars: TOL_Q = 1e-5 on q and h, 2e-6 on the input
      rows, equal greedy actions where the reference's top two are more than 4 TOL_Q apart, more than 0.99 of the rows clear of ties;
      precision 1: 1e-6 < max |q1 - q2| < 5e-2 against the precision-2 heads and not bit-equal (the bf16 variant's existing bar);
  (b) every looped case again as two shards on unlooped grids (env_id_base set): q, h, input rows and actions bit-equal at
      epsilon 0 and 0.3 -- exploration is keyed by the global env id, so a row's result does not depend on the grid;
  (c) the fused launches bit for bit against the inc head + the encoder as two launches, at every (precision, layout) the case lists,
      with the encoder's features within 2e-6 of the torch encoder at precision 2 and within 2e-2 max(1, |ref|) at precision 1 (the
      encoder tests' bars; the Toeplitz rollout kernels have no other test);
  (d) the learner's training forward (k_encode with ACT) at the (V, BT, precision) the older test of ops.encode_codes leaves out."""
import copy
import ctypes as C
import os
import sys

import pytest
import torch as th
import torch.nn.functional as F

from homophily_marl_amd import abi
from tests import policy_cases as pc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL_Q = 1e-5          # DESIGN section 2 "Bars"


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))


def _isa():
    import asm_hazards
    return asm_hazards.isa_of("ssd_policy_mfma.hip")


def ledger(kernels, cases, act_cases):
    """(kernels neither held by a case nor argued unreachable, UNREACHABLE entries that are held or not compiled, fused cases whose
    two-launch side no heads case holds, looped heads whose unlooped twin no case holds)"""
    held = pc.existing_held()
    for c in cases:
        held |= pc.case_kernels(c)[0]
    for V, R, prec in act_cases:
        held |= pc.encode_act_kernels(V, R, prec)
    heads_held = {k for k in held if k.startswith("k_head<")}
    loose = sorted(c.id for c in cases if c.test == "fused" and not pc.two_launch_side(c) <= heads_held)
    return (sorted(kernels - held - set(pc.UNREACHABLE)), sorted(k for k in pc.UNREACHABLE if k in held or k not in kernels), loose,
            pc.twinless(held))


def test_every_policy_kernel_is_held_by_a_case_or_argued_unreachable():
    kernels = pc.compiled_kernels(_isa())
    for k in ("k_head<1,2,9,0,true>", "k_inc_encode_gather<1,8,3,true>", "k_encode<15,2,false,5>", "k_encode_lut_any<1>", "k_pack_head<2>"):
        assert k in kernels, (k, sorted(kernels)[:5])                                  # the metadata was read and demangled
    missing, stale, loose, twinless = ledger(kernels, pc.CASES, pc.ENCODE_ACT_CASES)
    assert not missing, "compiled kernels that no GPU case holds to a reference: %s" % missing
    assert not stale, "UNREACHABLE entries that a case reaches, or that are not compiled: %s" % stale
    assert not loose, "fused cases whose standalone inc head no heads case holds to the reference: %s" % loose
    assert not twinless, "looped heads whose unlooped twin no case holds to the reference: %s" % twinless
    # without the tables the kernels they brought under test are missing again
    moved = ledger(kernels, [], [])[0]
    for k in ("k_head<1,1,8,0,true>", "k_inc_encode<1,8,31,true,5,false>", "k_encode<15,1,false,4>", "k_encode<15,2,true,5>", "k_pack_encoder<31,1>"):
        assert k in moved, (k, moved)
    # a kernel nobody planned for, of either family
    assert ledger(kernels | {"k_head<1,2,7,0,false>", "k_encode<15,2,false,6>"}, pc.CASES, pc.ENCODE_ACT_CASES)[0] == ["k_encode<15,2,false,6>", "k_head<1,2,7,0,false>"]
    # a looped case alone does not hold its kernel: the twin must be held as well
    alone = pc.twinless({"k_head<0,1,8,2,true>", "k_head<0,2,9,1,true>", "k_head<1,2,9,0,true>", "k_head<1,2,9,0,false>"})
    assert alone == ["k_head<0,1,8,2,true>"]


def test_unreachable_kernels_are_unreachable_by_arithmetic():
    """k_inc_encode<*, *, 15, false, 5, *>: no team size puts more than 32768 rows on an unlooped 7-wave head grid of 256 workgroups."""
    assert pc._unlooped_bt5_at_15_needs_cus() == 293 > pc.LEDGER_CUS
    for n in range(1, pc.MAX_AGENTS + 1):
        for N in range(pc.ENC_BT4_MAX_ROWS // n + 1, pc.ENC_BT4_MAX_ROWS // n + 4000, 7):
            assert pc.enc_bt(15, N * n) == 5 and pc.head_plan(N, n, pc.MODE_FUSED, pc.LEDGER_CUS)[2] > 1, (n, N)
    for c in pc.CASES + pc.existing_cases():
        assert not pc.case_kernels(c)[0] & set(pc.UNREACHABLE), c.id


def test_the_restated_plan_at_the_sizes_the_design_names():
    assert pc.looping_size(10, pc.MODE_DENSE, 256) == 3210 and pc.looping_size(10, pc.MODE_GATHER, 256) == 2810
    assert pc.looping_size(10, pc.MODE_FUSED, 256) == 2810 and pc.bt5_size(10, 256) * 10 > 32768 >= pc.looping_size(10, pc.MODE_FUSED, 256) * 10
    assert pc.head_plan(3000, 10, pc.MODE_GATHER, 256) == (25, 7, 2) and pc.head_plan(3000, 10, pc.MODE_DENSE, 256) == (24, 8, 1)
    assert pc.demangled_key("_ZN3ssd6k_headILi1ELi2ELi9ELi0ELb1EEEvjiPfS1_PKlPKfPKhS5_NS_5HeadKENS_8HeadColdE") == "k_head<1,2,9,0,true>"
    for c in pc.CASES:
        N = pc.resolve_n_env(c, 256)
        mode = pc.MODE_FUSED if c.test == "fused" else pc.standalone_mode(c)
        assert (pc.head_plan(N, c.n, mode, 256)[2] > 1) == c.loop, c.id


def test_head_plan_refuses_a_mode_outside_0_to_2():
    lib = abi.load_library()
    a, b, c = C.c_int32(-5), C.c_int32(-5), C.c_int32(-5)
    for mode in (-1, 3, 7):
        assert lib.ssd_policy_head_plan(64, 5, mode, C.byref(a), C.byref(b), C.byref(c)) == abi.SSD_ERR_INVALID
        assert b"0 (standalone dense heads), 1 (fused with the encoder) or 2 (standalone gathered heads)" in lib.ssd_last_error()
        assert (a.value, b.value, c.value) == (-5, -5, -5)
    with pytest.raises(abi.SsdError):
        abi.policy_head_plan(64, 5, 3)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _cus():
    return th.cuda.get_device_properties(0).multi_processor_count


def _setup(case, N, **keys):
    from homophily_marl_amd.run import load_config, setup
    over = dict(runner="hip_vec", batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False, store_state=False,
                env_args=dict(num_agents=case.n, map=case.map, episode_limit=20, seed=case.seed, view_size=case.view),
                use_cuda=True, save_model=False, runner_stats=False)
    over.update(case.flags)
    over.update(keys)
    return setup(load_config(case.kind, overrides=over))


def _check_plans(case, N):
    """the restated plan equals the library's for all three modes; the case's declared LOOP holds on this device, and the two shards of
    a looped heads case fit unlooped grids (else skip, before any work)"""
    cus = _cus()
    plans = pc.plans_for(case, cus, N)
    for mode, plan in plans.items():
        assert abi.policy_head_plan(N, case.n, mode) == plan, (mode, plan)
    mode = pc.MODE_FUSED if case.test == "fused" else pc.standalone_mode(case)
    if (plans[mode][2] > 1) != case.loop:
        pytest.skip("%d compute units: %d envs x %d agents plan as %s" % (cus, N, case.n, plans))
    if case.test == "heads" and case.loop:
        halves = [abi.policy_head_plan(part, case.n, mode) for part in pc.shard_sizes(N)]
        assert halves == [pc.head_plan(part, case.n, mode, cus) for part in pc.shard_sizes(N)]
        if max(h[2] for h in halves) > 1:
            pytest.skip("%d compute units: the halves of %d envs still loop (%s)" % (cus, N, halves))
    return plans


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2800, 2801, 3000, 3200, 3201])
def test_head_plan_of_the_gathered_heads_is_their_launch_grid(N):
    """mode 2 = launch_policy_head's cut for GEN 2 / 3 (7 compute waves), mode 0 the dense heads' (8), from the device's CU count."""
    n, cus, tiles = 10, _cus(), (N + 15) // 16
    got = {mode: abi.policy_head_plan(N, n, mode) for mode in (0, 1, 2)}
    assert got == {mode: pc.head_plan(N, n, mode, cus) for mode in (0, 1, 2)}
    assert abi.policy_head_plan(N, n, True) == got[1] and abi.policy_head_plan(N, n, False) == got[0] == abi.policy_head_plan(N, n)
    for mode, waves in ((0, 8), (1, 7), (2, 7)):
        wg, w, walks = got[mode]
        fit = n * ((tiles + waves - 1) // waves) <= cus
        assert w == waves and wg * w * walks >= tiles and (walks == 1) == fit and n * wg <= max(cus, n), (mode, got[mode])
    if N == 3000 and n * ((tiles + 6) // 7) > cus >= n * ((tiles + 7) // 8):       # (256 CUs: 270 > 256 >= 240)
        assert got[2][1] == 7 and got[2][2] > 1 and got[0][1:] == (8, 1)


def _live_inputs(case, ctx, N, steps=5):
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    env.reset_batch()
    g = th.Generator(device="cuda").manual_seed(case.seed)
    ok = th.nonzero(env.avail_actions_batch[0, 0]).squeeze(-1).to(th.int32)
    for _ in range(steps):
        env.step_batch(ok[th.randint(0, ok.numel(), (N, n), generator=g, device="cuda")].contiguous(), observe=False)
    o = env.observe_batch(out=env.native.obs_buffers(abi.OBS_F32, want_code=True))
    d = dict(obs=o["obs"].clone(), pos=o["pos"].clone(), orient=o["orient"].clone(), codes=o["code"].clone())
    d["prev_a"] = th.randint(-1, A, (N, n), generator=g, device="cuda")
    d["prev_r"] = th.randint(-1, 2, (N, n), generator=g, device="cuda").float()
    d["prev_i"] = th.randint(0, 3, (N, n, n), generator=g, device="cuda")
    d["h0e"] = th.randn(N, n, 64, generator=g, device="cuda") * 0.3
    d["h0i"] = th.randn(N, n, 64, generator=g, device="cuda") * 0.3
    d["reward"] = th.randint(-1, 2, (N, n), generator=g, device="cuda").float()
    d["clean"] = th.randint(0, 3, (N, n), generator=g, device="cuda").float()
    d["den"] = th.rand(N, n, generator=g, device="cuda")
    d["act"] = th.randint(0, A, (N, n), generator=g, device="cuda")
    return d, g


ROW_KEYS = ("obs", "pos", "orient", "codes", "prev_a", "prev_r", "prev_i", "h0e", "h0i", "reward", "clean", "den", "act")


def _run_heads(mac, avail, d, rows, prec, eps_value, base=0):
    """both standalone heads on the env rows `rows` (a slice) as a launch of their own: (q_env, h_env, input rows, actions, q_inc,
    h_inc, incentive actions), env-major"""
    from homophily_marl_amd.fast_policy import FastPolicy
    x = {k: d[k][rows].contiguous() for k in ROW_KEYS}
    N, n, A = x["pos"].shape[0], mac.n_agents, mac.args.n_actions
    fp = FastPolicy(mac, N, avail, seed=7, precision=prec, env_id_base=base)
    assert fp.fused and fp.fused_enc
    qe, qi = th.zeros(n, N, A, device="cuda"), th.zeros(n, N, n, 3, device="cuda")
    fp.h_env.copy_(x["h0e"].transpose(0, 1)); fp.h_inc.copy_(x["h0i"].transpose(0, 1))
    eps, step = th.full((), eps_value, device="cuda"), th.full((1,), 17, dtype=th.long, device="cuda")
    a = fp.act_env(None, x["prev_a"], x["prev_r"], x["prev_i"], x["pos"], eps, step, codes=x["codes"], q_out=qe).clone()
    ai = fp.act_inc(x["act"], x["pos"], x["orient"], x["reward"], x["clean"], x["den"], eps, step, q_out=qi).clone()
    th.cuda.synchronize()
    return (qe.transpose(0, 1).clone(), fp.h_env.transpose(0, 1).clone(), fp.inputs.transpose(0, 1).clone(), a, qi.transpose(0, 1).clone(),
            fp.h_inc.transpose(0, 1).clone(), ai), fp


HEAD_CASES = [c for c in pc.CASES if c.test == "heads"]
FUSED_CASES = [c for c in pc.CASES if c.test == "fused"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", HEAD_CASES, ids=[c.id for c in HEAD_CASES])
def test_standalone_heads_match_the_float64_controller_and_their_unlooped_twins(case):
    """(a) and (b) of the module docstring for one row of policy_cases.CASES; each case prints its max |diff| against the float64
    heads before it asserts."""
    cus = _cus()
    N = pc.resolve_n_env(case, cus)
    plans = _check_plans(case, N)
    th.manual_seed(2)
    ctx = _setup(case, N)
    mac, env = ctx.mac, ctx.runner.env
    n, A = case.n, mac.args.n_actions
    assert A == pc.n_actions(case.kind)
    gen_env, gen_inc = pc.gen_of(case.flags, 0), pc.gen_of(case.flags, 1)
    assert mac.shipped_flags == (not case.flags) and (gen_env != 1 or not mac.shipped_flags)      # GEN 1: a dense set other than the shipped one
    d, g = _live_inputs(case, ctx, N)
    avail = env.avail_actions_batch[0, 0]
    with th.no_grad():
        inputs = mac.assemble_inputs(mac.encode_obs(d["obs"]), d["prev_a"], d["prev_r"], d["prev_i"], d["pos"], False)
        assert inputs.shape[1] == mac.input_shape
        ag64 = copy.deepcopy(mac.agent).double()
        x64 = inputs.double()
        q_env, h_env, _ = ag64.forward_env(x64, d["h0e"].double().unsqueeze(2))
        masked = q_env.masked_fill(avail.view(1, 1, -1) == 0, -float("inf"))
        ref_act = masked.argmax(-1)
        top2 = masked.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 4 * TOL_Q
        d["act"] = ref_act
        q_inc, h_inc, _ = ag64.forward_inc(x64, d["h0i"].double().unsqueeze(2), F.one_hot(ref_act, A), (d["pos"] / mac.pos_scale).double(),
                                           d["orient"].double(), d["reward"].double().unsqueeze(-1), d["clean"].double().unsqueeze(-1),
                                           d["den"].double().unsqueeze(-1))
        t2 = q_inc.topk(2, dim=-1).values
        clear_i = (t2[..., 0] - t2[..., 1]) > 4 * TOL_Q
        off = ~th.eye(n, device="cuda", dtype=th.bool).expand(N, n, n)
        ref_inc = q_inc.argmax(-1)
    assert clear.float().mean() > 0.99                                                # a property of the reference and the inputs alone
    if gen_inc == 3:
        from tests.test_heads_onehot_gather import _dense_columns
        dense = _dense_columns(mac)
    elif gen_inc == 2:
        from tests.test_heads_others_last_action import _dense_columns
        dense = _dense_columns(mac)
    else:
        dense = th.arange(mac.input_shape, device="cuda")
    whole = slice(0, N)
    res = {}
    for prec in case.precisions:
        res[prec], fp = _run_heads(mac, avail, d, whole, prec, 0.0)
        assert fp.gather == (gen_inc == 3) and fp.others == bool(case.flags.get("obs_others_last_action"))
    qe, he, rows, a, qi, hi, ai = res[2]
    rows = rows.reshape(N * n, -1)
    d_rows = (rows[:, :dense.numel()] - inputs[:, dense]).abs().max().item()
    assert d_rows < 2e-6 and (rows[:, dense.numel():] == 0).all(), d_rows
    diff = [(qe - q_env).abs().max().item(), (he - h_env.squeeze(2)).abs().max().item(), (qi - q_inc).abs().max().item(),
            (hi - h_inc.squeeze(2)).abs().max().item()]
    print("%s N=%d plan %s: max |diff| vs float64 heads: q_env %.2e h_env %.2e q_inc %.2e h_inc %.2e rows %.2e; clear %.4f / %.4f"
          % ((case.id, N, plans[pc.standalone_mode(case)]) + tuple(diff) + (d_rows, clear.float().mean().item(), clear_i[off].float().mean().item())))
    assert max(diff) < TOL_Q, diff
    assert (a == ref_act)[clear].all()
    assert (ai == ref_inc)[clear_i & off].all() and (ai.diagonal(dim1=1, dim2=2) == 0).all()
    if 1 in case.precisions:
        b_env, b_inc = (res[1][0] - qe).abs().max().item(), (res[1][4] - qi).abs().max().item()
        print("%s bf16 vs f32-equivalent: q_env %.3e q_inc %.3e" % (case.id, b_env, b_inc))
        assert 1e-6 < b_env < 5e-2 and 1e-6 < b_inc < 5e-2
        assert not th.equal(res[1][0], qe) and not th.equal(res[1][4], qi)
    if plans[pc.standalone_mode(case)][2] > 1:      # (b) the same rows on two unlooped grids
        first, second = pc.shard_sizes(N)                 # (_check_plans: both fit unlooped grids)
        names = ("q_env", "h_env", "input rows", "actions", "q_inc", "h_inc", "actions_inc")
        for prec in case.precisions:
            for eps_value in (0.0, 0.3):
                looped = res[prec] if eps_value == 0.0 else _run_heads(mac, avail, d, whole, prec, eps_value)[0]
                if eps_value:
                    assert not th.equal(looped[3], res[prec][3]) and not th.equal(looped[6], res[prec][6])      # it explores
                for sl, base in ((slice(0, first), 0), (slice(first, N), first)):
                    shard = _run_heads(mac, avail, d, sl, prec, eps_value, base=base)[0]
                    for name, x, y in zip(names, shard, looped):
                        assert th.equal(x, y[sl]), (prec, eps_value, base, name, (x.float() - y[sl].float()).abs().max().item())
    env.close()


def _torch_features(mac, obs, chunk=4096):
    with th.no_grad():
        return th.cat([mac.encode_obs(obs[i:i + chunk]) for i in range(0, obs.shape[0], chunk)])      # [N * n, 32], env-major rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=[c.id for c in FUSED_CASES])
def test_fused_launch_equals_the_two_launches_in_every_variant(case, monkeypatch):
    """ssd_policy_head_inc_encode against ssd_policy_head_inc + ssd_policy_encode, bit for bit, per (precision, encoder layout)."""
    from homophily_marl_amd.fast_policy import FastPolicy
    monkeypatch.delenv("SSD_ENC_LAYOUT", raising=False)
    cus = _cus()
    N = pc.resolve_n_env(case, cus)
    plans = _check_plans(case, N)
    alone = plans[pc.standalone_mode(case)]
    if case.N == "loop1" and pc.standalone_mode(case) == pc.MODE_DENSE:
        # the window where the 7-wave fused head loops and the 8-wave standalone head does not: the case holds both plans, and they differ
        if alone[2] != 1:
            pytest.skip("%d compute units: no n_env where only the fused head loops (%s)" % (cus, plans))
        assert plans[pc.MODE_FUSED][2] > 1 and plans[pc.MODE_FUSED][1] == 7 and alone[1] == 8 and plans[pc.MODE_FUSED] != alone
    th.manual_seed(5)
    ctx = _setup(case, N, **({case.pipeline: True} if case.pipeline else {}))
    mac, env = ctx.mac, ctx.runner.env
    n, A, V = case.n, mac.args.n_actions, 2 * case.view + 1
    assert A == pc.n_actions(case.kind) and env.native.V == V
    gen = pc.gen_of(case.flags, 1)
    d, g = _live_inputs(case, ctx, N, steps=4)
    feat_ref = _torch_features(mac, d["obs"]).reshape(N, n, 32).transpose(0, 1)
    eps, step = th.full((), 0.3, device="cuda"), th.full((1,), 17, dtype=th.long, device="cuda")
    nxt = th.zeros(1, dtype=th.long, device="cuda")
    rows = N * n
    for layout in case.layouts:
        mac.args.enc_layout = layout
        for prec in case.precisions:
            fp = FastPolicy(mac, N, env.avail_actions_batch[0, 0], seed=11, precision=prec)
            assert fp.fused and fp.fused_enc and fp.inc_encode and fp.V == V and fp.bands == abi.encode_bands(V)
            assert fp.enc_layout == (abi.ENCODE_LAYOUT_LUT if layout == "lut" else abi.ENCODE_LAYOUT_TOEPLITZ)
            assert (fp.gather, fp.others and not fp.gather) == (gen == 3, gen == 2)
            key = pc.fused_key(prec, A, V, gen, plans[pc.MODE_FUSED][2] > 1, rows, layout == "lut")
            assert key in pc.expected_kernels(case, dict(plans, N=N))[0]
            fp.inputs_pair.copy_(th.randn(fp.inputs_pair.shape, generator=g, device="cuda") * 0.5)
            inputs0 = fp.inputs_pair.clone()
            par = {}
            if fp.prev_rec is not None:
                rec = th.randint(0, A, fp.prev_rec.shape, generator=g, device="cuda").to(th.uint8)
                rec.view(-1)[::5] = 0xFF
                fp.prev_rec.copy_(rec)
                par = dict(par=1)
            res = []
            for fused_launch in (False, True):
                fp.inputs_pair.copy_(inputs0); fp.h_inc.copy_(d["h0i"].transpose(0, 1)); nxt.zero_()
                if fp.feat_part is not None:
                    fp.feat_part.fill_(-7.0)
                q = th.zeros(n, N, n, 3, device="cuda")
                args = (d["act"], d["pos"], d["orient"], d["reward"], d["clean"], d["den"], eps, step)
                if fused_launch:
                    a = fp.act_inc_encode(*args, d["codes"], buf=0, q_out=q, file=dict(next_step_out=nxt.data_ptr()), **par).clone()
                else:
                    a = fp.act_inc(*args, q_out=q, buf=0, file=dict(next_step_out=nxt.data_ptr()), **par).clone()
                    fp.encode(None, codes=d["codes"], buf=1)
                th.cuda.synchronize()
                assert int(nxt) == 18
                res.append((a, q, fp.h_inc.clone(), fp.inputs_pair.clone(), None if fp.feat_part is None else fp.feat_part.clone()))
            for name, x, y in zip(("actions_inc", "q_out", "h_inc", "inputs_pair", "feat_part"), *res):
                assert (x is None and y is None) or th.equal(x, y), (key, name)
            assert not th.equal(res[1][2], d["h0i"].transpose(0, 1)) and bool(res[1][1].abs().sum() > 0)
            assert th.equal(res[1][3][0], inputs0[0])                      # the inc head's buffer is read-only in this launch
            if fp.feat_part is None:
                feat = res[1][3][1][..., :32]
                assert th.equal(res[1][3][1][..., 32:], inputs0[1][..., 32:])
            else:
                assert th.equal(res[1][3][1], inputs0[1]) and bool((res[1][4] != -7.0).any(dim=-1).all())     # every band row written
                feat = F.leaky_relu(fp.p["lb"] + res[1][4].sum(0)).reshape(n, N, 32)
            d_feat = (feat - feat_ref).abs().max().item()
            print("%s %s: encoder half max |diff| vs torch f32 %.2e" % (case.id, key, d_feat))
            # the encoder tests' bars: 2e-6, and for the bf16 variant test_rollout_encoder_at_other_views_matches_the_torch_encoder's
            assert d_feat < (2e-6 if prec == 2 else 2e-2 * max(1.0, feat_ref.abs().max().item())), (key, d_feat)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("V,R,prec", pc.ENCODE_ACT_CASES)
def test_learner_forward_encoder_matches_the_float64_encoder(V, R, prec):
    """(d) ops.encode_codes with gradients (k_encode<V, PREC, ACT = true, BT> on the Toeplitz images): the features and the emitted
    LeakyReLU(conv) against Conv2d + LeakyReLU + Flatten + Linear + LeakyReLU in float64 (the convolution as nine tap products).  Bars:
    1e-5 at precision 2 (test_encode_codes_op_forward_and_backward_match_torch_autograd); the bf16 variant within 2e-2 max(1, |ref|)
    (the encoder tests' bar for precision 1) and more than 1e-5 off (it really runs: test_bf16_learner_variant_is_close_...)."""
    from homophily_marl_amd import ops
    O = V - 2
    assert pc.encode_act_kernels(V, R, prec) == {"k_encode<%d,%d,true,%d>" % (V, prec, 4 if (V == 15 and R <= 32768) else 5), "k_pack_encoder<%d,%d>" % (V, prec)}
    g = th.Generator(device="cuda").manual_seed(V * 1000 + R)
    codes = th.randint(0, 4, (R, V, V), generator=g, device="cuda", dtype=th.uint8)
    th.manual_seed(V + R)
    conv, lin = th.nn.Conv2d(3, 6, 3, 1).cuda(), th.nn.Linear(6 * O * O, 32).cuda()
    try:
        ops.set_learner_precision(prec)
        feat = ops.encode_codes(codes, conv.weight, conv.bias, lin.weight, lin.bias)
        act = feat.grad_fn.saved_tensors[1]
        th.cuda.synchronize()
    finally:
        ops.set_learner_precision(2)
    assert act.shape == (R, 6, O, O)
    with th.no_grad():
        planes = ops.expand_codes(codes).double()
        cw = conv.weight.double()
        a_ref = conv.bias.double().view(1, 6, 1, 1).expand(R, 6, O, O).clone()
        for dy in range(3):
            for dx in range(3):
                a_ref += th.einsum("oc,rcyx->royx", cw[:, :, dy, dx], planes[:, :, dy:dy + O, dx:dx + O])
        a_ref = F.leaky_relu(a_ref)
        f_ref = F.leaky_relu(a_ref.flatten(1) @ lin.weight.double().t() + lin.bias.double())
        d_act, d_feat = (act.double() - a_ref).abs().max().item(), (feat.double() - f_ref).abs().max().item()
        m_act, m_feat = a_ref.abs().max().item(), f_ref.abs().max().item()
    print("k_encode<%d,%d,true,%d> R=%d: max |diff| vs float64: features %.2e (|ref| max %.2f) act %.2e (|ref| max %.2f)"
          % (V, prec, pc.enc_bt(V, R), R, d_feat, m_feat, d_act, m_act))
    if prec == 2:
        assert d_feat < 1e-5 and d_act < 1e-5
    else:
        assert 1e-5 < d_feat < 2e-2 * max(1.0, m_feat) and 1e-5 < d_act < 2e-2 * max(1.0, m_act)
