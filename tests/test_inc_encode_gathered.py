"""The pipelined three-launch rollout timestep for the gathered head layouts (fused_others_last_action: k_head GEN 2; fused_onehot_gather:
GEN 3), config key pipeline_gathered: k_inc_encode_gather = the gathering inc head of timestep t and the run-time-geometry class-LUT
encoder of t + 1 as one launch (ssd_policy_head_inc_encode with ssd_policy_head.pipeline_gather set), at every odd window edge 3 .. 63,
15 and 31 included.

CPU: the kernel-argument layout the compiler emitted for the new kernels (the heads read the gather pointers by offset), the argument
refusals of the entry point under the new field that return before any launch, and the truth table of plan_rollout's inc_encode.
GPU: the fused launch against the two standalone launches bit for bit (both layouts, ragged tiles, one to three bands, both action
counts, both precisions, the looped grid; V = 15 / 31: the run-time-geometry encoder half against the compile-time kernels the standalone
launch takes there), the pipelined hip_graph runner against the four-launch runner field by field, replayed on the CPU oracle, and the
reference's Q-values (bar 1e-5, DESIGN section 2 "Bars") through act_env / act_inc_encode."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from tests.policy_cases import dummy_encode_args as _enc, dummy_head as _head
from tests.policy_cases import host_plan as _host_policy      # plan_rollout over a stand-in controller: a rollout flag word with a gather bit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ODD_EDGES = list(range(3, 64, 2))
SHIPPED = 1 | 2 | 4 | 8 | 32
OTHERS, GATHER = abi.INPUT_OTHERS_LAST_ACTION, abi.INPUT_GATHER_ONEHOT
TOL_Q = 1e-5


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_kernel_arguments_of_the_gathered_launch_sit_where_the_heads_read_them():
    """k_inc_encode_gather: the arguments of k_inc_encode_any byte for byte -- six 4-byte and four 8-byte leading scalars (the 14
    preloaded dwords), HeadK at 56, HeadCold directly behind it (gather_slots<1>() and refetch_head_args read by offset), EncK, then
    the run-time V as a 4-byte last argument.  One instantiation per (precision, action count, GEN): the looped head half serves any
    grid, so 8 and no more."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_hazards
    from tests.test_isa_hazards import _kernel_args
    isa = asm_hazards.isa_of("ssd_policy_mfma.hip")
    fused = _kernel_args(isa, "_ZN3ssd19k_inc_encode_gatherI")
    assert len(fused) == 8, sorted(fused)
    any_edge = _kernel_args(isa, "_ZN3ssd16k_inc_encode_anyI")
    layouts = {tuple(args) for args in any_edge.values()}
    assert len(any_edge) == 8 and len(layouts) == 1
    text = open(isa).read()
    for name, args in fused.items():
        (ko, ks), (co, cs), (eo, es), (vo, vs) = args[-4:]
        assert ko == 56 and co == ko + ks, (name, args)
        assert vs == 4 and vo >= eo + es, (name, args)
        assert [s for _, s in args[:-4]] == [4] * 6 + [8] * 4, (name, args)
        assert tuple(args) == next(iter(layouts)), (name, args)                           # EncK and V sized and ordered as in k_inc_encode_any
        block = text[text.index(".amdhsa_kernel " + name):]
        block = block[:block.index(".end_amdhsa_kernel")]
        assert ".amdhsa_user_sgpr_kernarg_preload_length 14" in block, name


HEAD_FLAGS = [SHIPPED | OTHERS, SHIPPED | GATHER, SHIPPED | OTHERS | GATHER]


@pytest.mark.parametrize("flags", HEAD_FLAGS)
def test_gathered_launch_refuses_bad_arguments_before_any_launch(flags):
    """Every row returns from the argument checks: the addresses are dummies, so a launch would fault."""
    lib = abi.load_library()
    fn = lib.ssd_policy_head_inc_encode
    UNS, INV = abi.SSD_ERR_UNSUPPORTED, abi.SSD_ERR_INVALID
    P = 1 << 20
    # the field on a head without a gather bit: such a head leaves it zero
    assert fn(C.byref(_head(SHIPPED)), C.byref(_enc(15)), None) == UNS and b"every other input set leaves it zero" in lib.ssd_last_error()
    h = _head(SHIPPED)
    h.input_flags = 0                                                           # the shipped set as "no flag word"
    assert fn(C.byref(h), C.byref(_enc(15)), None) == UNS
    for V in (15, 21, 31):
        assert fn(C.byref(_head(flags)), C.byref(_enc(V, abi.ENCODE_LAYOUT_TOEPLITZ)), None) == UNS, V
    assert b"SSD_ENCODE_LAYOUT_LUT" in lib.ssd_last_error()
    for V in (1, 2, 16, 64, 65):
        assert fn(C.byref(_head(flags)), C.byref(_enc(V)), None) == UNS, V
        assert b"view_edge must be odd, 3 .. 63" in lib.ssd_last_error()
    table = "onehot_rows" if flags & GATHER else "others_rows"
    h = _head(flags)
    setattr(h, table, None)
    assert fn(C.byref(h), C.byref(_enc(15)), None) == INV                       # the table is missing
    h = _head(flags)
    setattr(h, table, P + 4)
    assert fn(C.byref(h), C.byref(_enc(15)), None) == INV                       # ... misaligned
    h = _head(flags)
    h.prev_record = None
    assert fn(C.byref(h), C.byref(_enc(15)), None) == INV                       # the record is missing
    h = _head(flags)
    h.prev_record_out = P + 4096
    assert fn(C.byref(h), C.byref(_enc(15)), None) == INV                       # the env head's output
    e = _enc(15)
    e.precision = 1
    assert fn(C.byref(_head(flags)), C.byref(e), None) == INV and b"one precision" in lib.ssd_last_error()
    h, e = _head(flags), _enc(13)
    e.out = h.inputs
    assert fn(C.byref(h), C.byref(e), None) == INV and b"other inputs buffer" in lib.ssd_last_error()
    for field in ("act", "slot_t_copy", "counter_inc"):
        e = _enc(15)
        e.slot_t = P + 64
        setattr(e, field, P + 128)
        assert fn(C.byref(_head(flags)), C.byref(e), None) == INV, field
    h, e = _head(flags), _enc(15)
    h.t_index, h.t_slots, h.next_t_out = P + 256, 4, P + 64
    e.slot_t = P + 64
    assert fn(C.byref(h), C.byref(e), None) == INV and b"scalar the inc head writes" in lib.ssd_last_error()
    h = _head(flags, A=7)
    assert fn(C.byref(h), C.byref(_enc(15)), None) == UNS and b"n_actions 9" in lib.ssd_last_error()
    assert fn(None, C.byref(_enc(15)), None) == INV and fn(C.byref(_head(flags)), None, None) == INV
    # without the field the entry point still refuses both bits
    assert fn(C.byref(_head(flags, pipe=0)), C.byref(_enc(15)), None) == UNS
    assert (b"SSD_INPUT_GATHER_ONEHOT" if flags & GATHER else b"obs_others_last_action") in lib.ssd_last_error()


@pytest.mark.parametrize("flags", HEAD_FLAGS)
def test_inc_encode_truth_table_of_the_gathered_layouts(flags, monkeypatch):
    """key off: False at every edge (15 / 31 and pipeline_any_view included); key on under the class-LUT layout: True at every odd
    edge 3 .. 63, whatever pipeline_any_view says; key on with enc_layout toeplitz: False."""
    monkeypatch.delenv("SSD_ENC_LAYOUT", raising=False)
    for V in ODD_EDGES:
        fp = _host_policy(V, flags)
        assert fp.fused and fp.fused_enc and fp.needs_prev_rec and (fp.gather or fp.others)
        assert not fp.inc_encode, V
        assert not _host_policy(V, flags, pipeline_gathered=False, pipeline_any_view=True).inc_encode, V
        assert _host_policy(V, flags, pipeline_gathered=True).inc_encode, V
        assert _host_policy(V, flags, pipeline_gathered=True, pipeline_any_view=False).inc_encode, V
    for V in (11, 15, 31):
        assert not _host_policy(V, flags, pipeline_gathered=True, enc_layout="toeplitz").inc_encode, V
    assert not _host_policy(16, flags, pipeline_gathered=True).inc_encode and not _host_policy(65, flags, pipeline_gathered=True).inc_encode
    from homophily_marl_amd.run import load_config
    assert load_config("cleanup")["pipeline_gathered"] is False


def test_the_key_leaves_the_dense_layouts_alone(monkeypatch):
    """pipeline_gathered says nothing about a controller without a gather bit: 15 / 31 pipelined, the rest by pipeline_any_view."""
    monkeypatch.delenv("SSD_ENC_LAYOUT", raising=False)
    for V in (7, 15, 31):
        assert _host_policy(V, SHIPPED, pipeline_gathered=True).inc_encode == (V in (15, 31))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
GEN2 = dict(obs_others_last_action=True, fused_others_last_action=True)
GEN3_OTHERS = dict(obs_others_last_action=True, fused_onehot_gather=True)
GEN3_DISTANCE = dict(obs_distance=True, fused_onehot_gather=True)
GEN3_ALL = dict(obs_distance=True, obs_others_last_action=True, fused_onehot_gather=True)


def _cfg(kind, mapname, n, N, view, T=20, seed=3, runner="hip_vec", **over):
    from homophily_marl_amd.run import load_config
    return load_config(kind, overrides=dict(dict(
        runner=runner, batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False, store_state=False,
        env_args=dict(num_agents=n, map=mapname, episode_limit=T, seed=seed, view_size=view), use_cuda=True, save_model=False,
        runner_stats=False), **over))


#               kind       map          n   view  N     prec  flags          what the row covers
LAUNCH_CASES = [("cleanup", "default5", 5, 7, 16, 2, GEN2),                 # V = 15 (compile-time encoder kernel in the standalone launch)
                ("cleanup", "default5", 5, 7, 203, 2, GEN2),                # ragged last head tile, ragged last 80-row encoder group
                ("cleanup", "default5", 5, 3, 203, 1, GEN2),                # the bf16 variant
                ("cleanup", "default5", 5, 7, 203, 2, GEN3_OTHERS),         # gathered one-hots with the others' block
                ("cleanup", "default10", 6, 10, 203, 2, GEN3_DISTANCE),     # no others' block; V = 21: two bands (10 + 9 rows)
                ("harvest", "default10", 5, 15, 203, 2, GEN2),              # A = 8; V = 31: three bands (compile-time kernel standalone)
                ("cleanup", "default10", 10, 3, 4112, 2, GEN3_ALL)]         # a grid larger than the chip: the waves walk several tiles


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mapname,n,view,N,precision,flags", LAUNCH_CASES,
                         ids=["%s%d-v%d-N%d-p%d-%s" % (c[0], c[2], c[3], c[4], c[5], "+".join(sorted(c[6]))) for c in LAUNCH_CASES])
def test_gathered_inc_encode_launch_equals_the_two_launches(kind, mapname, n, view, N, precision, flags):
    """With pipeline_gathered, FastPolicy.act_inc_encode (k_inc_encode_gather) must produce bit for bit what act_inc and encode
    produce as two launches: incentive actions, q_out, h_inc, both input buffers and the band sums; next_step_out advances; the inc
    head's buffer and both previous-action record buffers are unchanged.  The records are random actions with every fifth byte 0xFF
    (no previous action), and the launch reads the buffer of parity 1."""
    from homophily_marl_amd.fast_policy import FastPolicy
    from homophily_marl_amd.run import setup
    V = 2 * view + 1
    th.manual_seed(5)
    assert (abi.policy_head_plan(N, n, True)[2] > 1) == (N == 4112)
    ctx = setup(_cfg(kind, mapname, n, N, view, pipeline_gathered=True, **flags))
    mac, env = ctx.mac, ctx.runner.env
    A = mac.args.n_actions
    assert A == (8 if kind == "harvest" else 9) and env.native.V == V
    env.reset_batch()
    g = th.Generator(device="cuda").manual_seed(1)
    ok_actions = th.nonzero(env.avail_actions_batch[0, 0]).squeeze(-1).to(th.int32)
    for _ in range(4):
        env.step_batch(ok_actions[th.randint(0, ok_actions.numel(), (N, n), generator=g, device="cuda")].contiguous(), observe=False)
    o = env.observe_batch(out=env.native.obs_buffers(abi.OBS_F32, want_code=True))
    pos, orient, codes = o["pos"].clone(), o["orient"].clone(), o["code"].clone()
    fp = FastPolicy(mac, N, env.avail_actions_batch[0, 0], seed=11, precision=precision)
    assert fp.fused and fp.fused_enc and fp.inc_encode and fp.V == V and fp.bands == abi.encode_bands(V)
    assert fp.gather == ("fused_onehot_gather" in flags) and fp.others == ("obs_others_last_action" in flags)
    assert (fp.feat_part is None) == (fp.bands == 1)
    fp.inputs_pair.copy_(th.randn(fp.inputs_pair.shape, generator=g, device="cuda") * 0.5)
    inputs0 = fp.inputs_pair.clone()
    rec = th.randint(0, A, fp.prev_rec.shape, generator=g, device="cuda").to(th.uint8)
    rec.view(-1)[::5] = 0xFF
    fp.prev_rec.copy_(rec)
    assert not th.equal(rec[0], rec[1])
    h0 = th.randn(fp.h_inc.shape, generator=g, device="cuda") * 0.3
    act = th.randint(0, A, (N, n), generator=g, device="cuda")
    reward = th.randint(-1, 2, (N, n), generator=g, device="cuda").float()
    clean = th.randint(0, 3, (N, n), generator=g, device="cuda").float()
    den = th.rand(N, n, generator=g, device="cuda")
    eps, step = th.full((), 0.3, device="cuda"), th.full((1,), 17, dtype=th.long, device="cuda")
    nxt = th.zeros(1, dtype=th.long, device="cuda")
    res = []
    for fused_launch in (False, True):
        fp.inputs_pair.copy_(inputs0); fp.h_inc.copy_(h0); nxt.zero_()
        if fp.feat_part is not None:
            fp.feat_part.fill_(-7.0)
        q = th.zeros(n, N, n, 3, device="cuda")
        if fused_launch:
            a = fp.act_inc_encode(act, pos, orient, reward, clean, den, eps, step, codes, buf=0, q_out=q, par=1,
                                  file=dict(next_step_out=nxt.data_ptr())).clone()
        else:
            a = fp.act_inc(act, pos, orient, reward, clean, den, eps, step, q_out=q, buf=0, par=1, file=dict(next_step_out=nxt.data_ptr())).clone()
            fp.encode(None, codes=codes, buf=1)
        th.cuda.synchronize()
        assert int(nxt) == 18
        assert th.equal(fp.prev_rec, rec)
        res.append((a, q, fp.h_inc.clone(), fp.inputs_pair.clone(), None if fp.feat_part is None else fp.feat_part.clone()))
    for name, x, y in zip(("actions_inc", "q_out", "h_inc", "inputs_pair", "feat_part"), *res):
        assert (x is None and y is None) or th.equal(x, y), name
    assert not th.equal(res[1][2], h0) and bool(res[1][1].abs().sum() > 0)
    assert th.equal(res[1][3][0], inputs0[0])                      # the inc head's buffer is read-only in this launch
    if fp.feat_part is None:
        assert not th.equal(res[1][3][1][..., :32], inputs0[1][..., :32]) and th.equal(res[1][3][1][..., 32:], inputs0[1][..., 32:])
    else:
        assert th.equal(res[1][3][1], inputs0[1]) and bool((res[1][4] != -7.0).any(dim=-1).all())     # every band row written
    # the records are read: the other parity's buffer gives other values
    q1 = th.zeros(n, N, n, 3, device="cuda")
    fp.inputs_pair.copy_(inputs0); fp.h_inc.copy_(h0)
    fp.act_inc_encode(act, pos, orient, reward, clean, den, eps, step, codes, buf=0, q_out=q1, par=0)
    th.cuda.synchronize()
    assert not th.equal(q1, res[1][1])
    env.close()


FIELDS = ("obs", "actions", "actions_inc", "reward", "clean_num", "apple_den", "agent_pos", "agent_orientation", "terminated")
RUNNER_CASES = [("cleanup", "default5", 5, 7, "code", GEN2), ("cleanup", "default5", 5, 7, "f32", GEN2),
                ("cleanup", "default5", 5, 3, "code", GEN3_OTHERS), ("cleanup", "default10", 6, 7, "code", GEN3_DISTANCE),
                ("harvest", "default10", 5, 15, "code", GEN2)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mapname,n,view,storage,flags", RUNNER_CASES,
                         ids=["%s%d-v%d-%s-%s" % (c[0], c[2], c[3], c[4], "+".join(sorted(c[5]))) for c in RUNNER_CASES])
def test_pipelined_runner_of_the_gathered_layouts_equals_the_four_launch_runner(kind, mapname, n, view, storage, flags):
    """hip_graph with pipeline_gathered (three launches per timestep, the encoder one timestep ahead, the previous-action records
    alternating with the parity of t) against the same job without the key (four launches): three training episodes each (eager,
    captured, replayed) from the same seeds store identical batches -- the exploration draws are keyed by (seed, step, global env id,
    agent) and the draw counter starts so that both runners read the same steps.  The pipelined runner's batches replay on the CPU
    oracle; then one train_iteration with strict device ops and finite losses."""
    from homophily_marl_amd import ops
    from homophily_marl_amd.run import setup, train_iteration
    from oracle.oracle_py import OracleEnv
    N, T = 48, 14
    ofmt = abi.OBS_CODE if storage == "code" else abi.OBS_F32

    def episodes(key):
        th.manual_seed(0)
        ctx = setup(_cfg(kind, mapname, n, N, view, T=T, seed=21, runner="hip_graph", obs_storage=storage, steps_per_graph=2,
                         strict_device_ops=True, pipeline_gathered=key, **flags))
        r = ctx.runner
        assert r.env.native.V == 2 * view + 1
        out = []
        for ep in range(3):                                  # eager, captured, replayed
            batch = r.run(test_mode=False)
            assert r.fast is not None and r.fast.fused_enc and r.direct_obs and r.fold_store and r.fast.prev_rec is not None
            assert r.fast.gather == ("fused_onehot_gather" in flags) and r.fast.others == ("obs_others_last_action" in flags)
            assert r.fast.inc_encode == key and r.pipe == key
            assert ep == 0 or r._graph is not None
            assert int(batch["filled"].sum()) == N * (T + 1)
            out.append({k: batch[k].clone() for k in FIELDS})
        return ctx, out

    try:
        ctx, piped = episodes(True)
        ctx4, four = episodes(False)
        ctx4.runner.close_env()
        for ep, (a, b) in enumerate(zip(piped, four)):
            for k in FIELDS:
                assert th.equal(a[k], b[k]), (ep, k)
        assert len({int(p["actions"].sum()) for p in piped}) > 1                 # exploring episodes: not three copies of one
        orc = OracleEnv(kind, map=mapname, num_agents=n, n_env=N, view_size=view, episode_limit=T, rng_mode=abi.RNG_COUNTER, seed=21)
        for ep, batch in enumerate(piped):
            orc.reset()
            acts = batch["actions"].squeeze(-1).cpu().numpy()
            for t in range(T):
                ob = orc.observe(ofmt)
                assert (batch["obs"][:, t].cpu().numpy() == ob["obs"]).all(), (ep, t)
                assert (batch["agent_pos"][:, t].cpu().numpy() == ob["pos"]).all(), (ep, t)
                o = orc.step(acts[:, t])
                for k in ("reward", "clean_num", "apple_den"):
                    assert (batch[k][:, t].cpu().numpy() == o[k]).all(), (ep, t, k)
            assert (batch["obs"][:, T].cpu().numpy() == orc.observe(ofmt)["obs"]).all()
        orc.close()
        logged = {}
        log_stat = ctx.learner.logger.log_stat
        ctx.learner.logger.log_stat = lambda k, v, t, *a, **kw: (logged.__setitem__(k, float(v)), log_stat(k, v, t, *a, **kw))
        train_iteration(ctx, 0)
        assert ctx.runner.pipe
        assert all(k in logged for k in ("loss_value_env", "loss_value_inc", "loss_sim")), sorted(logged)
        assert all(np.isfinite(v) for v in logged.values()), logged
        ctx.runner.close_env()
    finally:
        ops.set_strict(False)


def _drive_fixture(z, meta, args, batch, mac):
    """act_env / act_inc_encode step by step over a recorded batch, the way a pipelined rollout issues them: the features of step t + 1
    come from the launch that evaluates the inc head of step t, the input rows and the records alternate with the parity of t.  The
    record of a step is set from the batch's previous actions (the reference's, not the picks of the head before)."""
    from homophily_marl_amd.fast_policy import FastPolicy
    mac.args.pipeline_gathered = True
    B, n, A = batch.batch_size, args.n_agents, args.n_actions
    avail = batch["avail_actions"][0, 0, 0].to(th.uint8)
    fp = FastPolicy(mac, B, avail, seed=1)
    assert fp.fused and fp.fused_enc and fp.inc_encode and fp.prev_rec is not None and fp.bands == 1
    q_env_ref, q_inc_ref = th.as_tensor(z["q_env"]).cuda(), th.as_tensor(z["q_inc"]).cuda()
    eps, step = th.zeros((), device="cuda"), th.zeros(1, dtype=th.long, device="cuda")
    qe, qi = th.zeros(n, B, A, device="cuda"), th.zeros(n, B, n, 3, device="cuda")
    acts, rew, ainc = batch["actions"].squeeze(-1), batch["reward"], batch["actions_inc"].squeeze(-1)
    slots = batch["obs"].shape[1]
    worst_e = worst_i = 0.0
    n_clear = 0
    fp.encode(batch["obs"][:, 0].contiguous(), buf=0)
    for t in range(meta["steps"]):
        prev_a = acts[:, t - 1].contiguous() if t else th.full((B, n), -1, dtype=th.long, device="cuda")
        prev_r = rew[:, t - 1].contiguous() if t else th.zeros(B, n, device="cuda")
        prev_i = ainc[:, t - 1].contiguous() if t else th.zeros(B, n, n, dtype=th.long, device="cuda")
        pos, orient = batch["agent_pos"][:, t].contiguous(), batch["agent_orientation"][:, t].contiguous()
        fp.set_prev_actions(prev_a, t)
        a_env = fp.head_env(prev_a, prev_r, prev_i, pos, eps, step, q_out=qe, buf=t & 1, par=t)
        worst_e = max(worst_e, (qe.transpose(0, 1) - q_env_ref[:, t]).abs().max().item())
        masked = q_env_ref[:, t].masked_fill(batch["avail_actions"][:, t] == 0, -float("inf"))
        top2 = masked.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-6
        assert (a_env == masked.argmax(-1))[clear].all(), t
        n_clear += int(clear.sum())
        nxt = FastPolicy.codes_from_obs(batch["obs"][:, min(t + 1, slots - 1)].contiguous())
        fp.act_inc_encode(acts[:, t].contiguous(), pos, orient, rew[:, t].contiguous(), batch["clean_num"][:, t].contiguous(),
                          batch["apple_den"][:, t].contiguous(), eps, step, nxt, buf=t & 1, q_out=qi, par=t, mask_alphabet=False)
        worst_i = max(worst_i, (qi.transpose(0, 1) - q_inc_ref[:, t]).abs().max().item())
    print("max |q - reference| over %d steps: env %.2e inc %.2e; %d clear greedy rows" % (meta["steps"], worst_e, worst_i, n_clear))
    assert worst_e < TOL_Q and worst_i < TOL_Q
    assert n_clear > 0.9 * B * meta["steps"] * n


@pytest.mark.gpu
def test_pipelined_gather_heads_reproduce_the_reference_q_values_others():
    """tests/golden/rollout_others_cleanup5.npz (the REFERENCE controller with obs_others_last_action) through k_head<env> GEN 2 and
    k_inc_encode_gather GEN 2: q_env and q_inc within 1e-5 at every step."""
    from tests.test_others_last_action_host import load_others_fixture
    z, meta, args, batch, mac = load_others_fixture(device="cuda:0")
    assert mac.rollout_input_flags & OTHERS and not mac.rollout_input_flags & GATHER
    _drive_fixture(z, meta, args, batch, mac)


@pytest.mark.gpu
def test_pipelined_gather_heads_reproduce_the_reference_q_values_all_seven():
    """tests/golden/rollout_wide_cleanup10.npz (the REFERENCE controller with all seven flags at Cleanup-10) through the GEN 3 kernels."""
    from tests.test_onehot_gather_host import load_wide_fixture
    z, meta, args, batch, mac = load_wide_fixture(device="cuda:0")
    assert mac.rollout_input_flags == 127 | GATHER
    _drive_fixture(z, meta, args, batch, mac)
