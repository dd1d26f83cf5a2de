"""The pipelined three-launch rollout timestep at every odd window edge V = 3 .. 63 (view_size 1 .. 31), config key
pipeline_any_view: k_inc_encode_any = the inc head of timestep t and the run-time-geometry class-LUT encoder of t + 1 as one launch.

CPU: the kernel-argument layout the compiler emitted for the new kernels (the heads read part of their arguments by offset), the
argument refusals of ssd_policy_head_inc_encode that return before any launch, and the truth table of plan_rollout's inc_encode.
GPU: the fused launch against the two standalone launches bit for bit (one to six bands, ragged tiles, both action counts, both
precisions, the looped head), and the pipelined hip_graph runner against the four-launch runner field by field, replayed on the CPU
oracle."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi
from tests.policy_cases import dummy_encode_args as _enc, dummy_head as _head, env_map as _map, v_max as _v_max
from tests.policy_cases import host_plan as _host_policy      # plan_rollout over a stand-in controller: the shipped input set

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ODD_EDGES = list(range(3, 64, 2))


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_kernel_arguments_of_the_any_edge_launch_sit_where_the_heads_read_them():
    """k_inc_encode_any: HeadK at offset LEAD (behind the 14 preloaded dwords), HeadCold directly behind it, EncK, then the run-time
    V as a 4-byte last argument -- the layout of k_inc_encode with V appended, so the heads' cold-argument offsets and
    refetch_head_args read the right bytes.  One instantiation per (precision, action count, looped) and no more."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_hazards
    from tests.test_isa_hazards import _kernel_args
    src = open(os.path.join(ROOT, "homophily_marl_amd", "csrc", "ssd_policy_mfma.hip")).read()
    lead = eval(re.search(r"constexpr int LEAD = ([0-9*+ ]+);", src).group(1))
    assert lead == 14 * 4
    isa = asm_hazards.isa_of("ssd_policy_mfma.hip")
    fused = _kernel_args(isa, "_ZN3ssd16k_inc_encode_anyI")
    assert len(fused) == 8, sorted(fused)
    shipped = _kernel_args(isa, "_ZN3ssd12k_inc_encodeI")
    sizes = {tuple(s for _, s in args[-3:]) for args in shipped.values()}            # (HeadK, HeadCold, EncK) of the shipped launch
    assert len(sizes) == 1
    text = open(isa).read()
    for name, args in fused.items():
        (ko, ks), (co, cs), (eo, es), (vo, vs) = args[-4:]
        assert ko == lead and co == ko + ks, (name, args)
        assert (ks, cs, es) == next(iter(sizes)) and eo >= co + cs, (name, args)
        assert vs == 4 and vo >= eo + es, (name, args)
        assert [s for _, s in args[:-4]] == [4] * 6 + [8] * 4, (name, args)              # the leading scalars of k_inc_encode
        block = text[text.index(".amdhsa_kernel " + name):]
        block = block[:block.index(".end_amdhsa_kernel")]
        assert ".amdhsa_user_sgpr_kernarg_preload_length 14" in block, name


@pytest.mark.parametrize("V", [1, 2, 16, 20, 64, 65])
def test_fused_launch_refuses_even_and_out_of_range_edges_before_any_launch(V):
    """Even edges and edges outside 3 .. 63: SSD_ERR_UNSUPPORTED with the odd-edge message from the argument check (dummy addresses:
    a launch would fault)."""
    lib = abi.load_library()
    h, e = _head(), _enc(V, abi.ENCODE_LAYOUT_LUT)
    assert lib.ssd_policy_head_inc_encode(C.byref(h), C.byref(e), None) == abi.SSD_ERR_UNSUPPORTED
    assert b"view_edge must be odd, 3 .. 63" in lib.ssd_last_error()


def test_fused_launch_refuses_the_toeplitz_layout_at_other_edges_before_any_launch():
    lib = abi.load_library()
    h, e = _head(), _enc(21, abi.ENCODE_LAYOUT_TOEPLITZ)
    assert lib.ssd_policy_head_inc_encode(C.byref(h), C.byref(e), None) == abi.SSD_ERR_UNSUPPORTED
    assert b"Toeplitz" in lib.ssd_last_error()
    # the refusals that do not depend on the edge hold at the new edges too
    e = _enc(21, abi.ENCODE_LAYOUT_LUT)
    e.counter_inc = 1 << 20
    assert lib.ssd_policy_head_inc_encode(C.byref(h), C.byref(e), None) == abi.SSD_ERR_INVALID
    e = _enc(21, abi.ENCODE_LAYOUT_LUT)
    e.precision = 1
    assert lib.ssd_policy_head_inc_encode(C.byref(h), C.byref(e), None) == abi.SSD_ERR_INVALID and b"one precision" in lib.ssd_last_error()
    e = _enc(13, abi.ENCODE_LAYOUT_LUT)
    e.out = h.inputs
    assert lib.ssd_policy_head_inc_encode(C.byref(h), C.byref(e), None) == abi.SSD_ERR_INVALID and b"other inputs buffer" in lib.ssd_last_error()


def test_inc_encode_truth_table(monkeypatch):
    """key off: V in (15, 31); key on under the class-LUT layout: every supported edge; key on with enc_layout toeplitz: the shipped
    edges only (V = 11: False)."""
    monkeypatch.delenv("SSD_ENC_LAYOUT", raising=False)
    for V in ODD_EDGES:
        assert _host_policy(V).fused_enc
        assert _host_policy(V).inc_encode == (V in (15, 31)), V
        assert _host_policy(V, pipeline_any_view=False).inc_encode == (V in (15, 31)), V
        assert _host_policy(V, pipeline_any_view=True).inc_encode, V
    assert not _host_policy(11, pipeline_any_view=True, enc_layout="toeplitz").inc_encode
    assert _host_policy(15, pipeline_any_view=True, enc_layout="toeplitz").inc_encode
    assert not _host_policy(16, pipeline_any_view=True).inc_encode and not _host_policy(65, pipeline_any_view=True).inc_encode
    from homophily_marl_amd.run import load_config
    assert load_config("cleanup")["pipeline_any_view"] is False


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _ctx(kind, n, N, view, **over):
    from homophily_marl_amd.run import load_config, setup
    cfg = load_config(kind, overrides=dict(dict(runner="hip_vec", batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False,
                                                store_state=False,
                                                env_args=dict(num_agents=n, map=_map(kind, n), episode_limit=20, seed=3, view_size=view),
                                                use_cuda=True, save_model=False, runner_stats=False, pipeline_any_view=True), **over))
    return setup(cfg)


LAUNCH_VIEWS = [1, 3, 6, 8, 10, "max"]
LAUNCH_CASES = [(kind, 5, view, N, 2) for kind in ("cleanup", "harvest") for view in LAUNCH_VIEWS for N in (16, 203)] + \
               [(kind, 5, view, 203, 1) for kind in ("cleanup", "harvest") for view in (3, 10)] + [("cleanup", 10, 3, 4112, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,view,N,precision", LAUNCH_CASES)
def test_any_view_inc_encode_launch_equals_the_two_launches(kind, n, view, N, precision):
    """With pipeline_any_view, FastPolicy.act_inc_encode (k_inc_encode_any) must produce bit for bit what act_inc and encode produce
    as two launches: incentive actions, q_out, h_inc, both input buffers and the band sums; the inc head's buffer is unchanged and
    next_step_out advances.  N = 203: a ragged last 16-row head tile and a ragged last 80-row encoder group; views with 1, 2 (10 + 9
    rows) and more bands; Cleanup-10 x 4112: the looped head half.  A listed view above the largest the env accepts is covered by the
    `max` case; `max` returns at once where it coincides with a listed view."""
    from homophily_marl_amd.fast_policy import FastPolicy
    vmax = _v_max(kind, _map(kind, n), n)
    listed = [v for v in LAUNCH_VIEWS if v != "max"]
    if view == "max":
        if vmax in listed:
            return
        view = vmax
    elif view > vmax:
        return
    V = 2 * view + 1
    th.manual_seed(5)
    looped = n == 10
    assert (abi.policy_head_plan(N, n, True)[2] > 1) == looped
    ctx = _ctx(kind, n, N, view)
    mac, env = ctx.mac, ctx.runner.env
    A = mac.args.n_actions
    assert A == (8 if kind == "harvest" else 9)
    env.reset_batch()
    g = th.Generator(device="cuda").manual_seed(1)
    ok_actions = th.nonzero(env.avail_actions_batch[0, 0]).squeeze(-1).to(th.int32)
    for _ in range(4):
        env.step_batch(ok_actions[th.randint(0, ok_actions.numel(), (N, n), generator=g, device="cuda")].contiguous(), observe=False)
    o = env.observe_batch(out=env.native.obs_buffers(abi.OBS_F32, want_code=True))
    pos, orient, codes = o["pos"].clone(), o["orient"].clone(), o["code"].clone()
    fp = FastPolicy(mac, N, env.avail_actions_batch[0, 0], seed=11, precision=precision)
    assert fp.fused and fp.fused_enc and fp.inc_encode and fp.V == V and fp.bands == abi.encode_bands(V)
    assert (fp.feat_part is None) == (fp.bands == 1)
    fp.inputs_pair.copy_(th.randn(fp.inputs_pair.shape, generator=g, device="cuda") * 0.5)
    inputs0 = fp.inputs_pair.clone()
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
            a = fp.act_inc_encode(act, pos, orient, reward, clean, den, eps, step, codes, buf=0, q_out=q,
                                  file=dict(next_step_out=nxt.data_ptr())).clone()
        else:
            a = fp.act_inc(act, pos, orient, reward, clean, den, eps, step, q_out=q, buf=0, file=dict(next_step_out=nxt.data_ptr())).clone()
            fp.encode(None, codes=codes, buf=1)
        th.cuda.synchronize()
        assert int(nxt) == 18
        res.append((a, q, fp.h_inc.clone(), fp.inputs_pair.clone(), None if fp.feat_part is None else fp.feat_part.clone()))
    for name, x, y in zip(("actions_inc", "q_out", "h_inc", "inputs_pair", "feat_part"), *res):
        assert (x is None and y is None) or th.equal(x, y), name
    assert not th.equal(res[1][2], h0) and bool(res[1][1].abs().sum() > 0)
    assert th.equal(res[1][3][0], inputs0[0])                      # the inc head's buffer is read-only in this launch
    if fp.feat_part is None:
        assert not th.equal(res[1][3][1][..., :32], inputs0[1][..., :32]) and th.equal(res[1][3][1][..., 32:], inputs0[1][..., 32:])
    else:
        assert th.equal(res[1][3][1], inputs0[1]) and bool((res[1][4] != -7.0).any(dim=-1).all())     # every band row written
    env.close()


FIELDS = ("obs", "actions", "actions_inc", "reward", "clean_num", "apple_den", "agent_pos", "agent_orientation", "terminated")
RUNNER_CASES = [("cleanup", 3, "code"), ("cleanup", 3, "f32"), ("cleanup", 5, "code"), ("cleanup", 5, "f32"), ("cleanup", 10, "code"),
                ("cleanup", 10, "f32"), ("harvest", 10, "code")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,view,storage", RUNNER_CASES)
def test_pipelined_runner_at_other_views_equals_the_four_launch_runner(kind, view, storage):
    """hip_graph with pipeline_any_view (three launches per timestep, the encoder one timestep ahead, band sums folded by the next env
    head) against the same job without the key (four launches): three training episodes each (eager, captured, replayed) from the
    same seeds store identical batches -- the exploration draws are keyed by (seed, step, global env id, agent).  The pipelined
    runner's batches replay on the CPU oracle; then one train_iteration with strict device ops and finite losses."""
    from homophily_marl_amd import ops
    from homophily_marl_amd.run import load_config, setup, train_iteration
    from oracle.oracle_py import OracleEnv
    N, T, n = 48, 14, 5
    mp = _map(kind, n)
    view = min(view, _v_max(kind, mp, n))
    ofmt = abi.OBS_CODE if storage == "code" else abi.OBS_F32

    def episodes(key):
        th.manual_seed(0)
        cfg = load_config(kind, overrides=dict(
            runner="hip_graph", batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False, store_state=False,
            env_args=dict(num_agents=n, map=mp, episode_limit=T, seed=21, view_size=view), use_cuda=True, save_model=False,
            runner_stats=False, obs_storage=storage, steps_per_graph=2, strict_device_ops=True, pipeline_any_view=key))
        ctx = setup(cfg)
        r = ctx.runner
        assert r.env.native.V == 2 * view + 1 and r.env.native.V not in (15, 31)
        out = []
        for ep in range(3):                                  # eager, captured, replayed
            batch = r.run(test_mode=False)
            assert r.fast is not None and r.fast.fused_enc and r.direct_obs and r.fold_store
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
        orc = OracleEnv(kind, map=mp, num_agents=n, n_env=N, view_size=view, episode_limit=T, rng_mode=abi.RNG_COUNTER, seed=21)
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
