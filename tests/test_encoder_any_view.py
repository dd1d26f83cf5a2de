"""The class-code encoder and the device learner at every window edge V = 3 .. 63 (view_size 1 .. 31), not only the shipped 15 / 31:
the header's geometry against abi.py and the entry points' argument checks (CPU), then on the GPU the learner op (ops.encode_codes
forward + backward), the rollout encoder (FastPolicy.encode), the hip_graph runner with both storages and a strict device train
step, and the captured train step against the tensor-op learner on the CPU."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

from homophily_marl_amd import abi
from tests.policy_cases import v_max as _v_max

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ODD_EDGES = list(range(3, 64, 2))
LOG_KEYS = ("loss_value_env", "loss_value_inc", "loss_sim", "value_give_mean", "value_receive_mean", "q_env_taken_mean", "q_inc_taken_mean",
            "incentives_to_cleanup_per", "incentives_to_harvest_per")


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_geometry_macros_match_abi_at_every_edge(tmp_path):
    """SSD_ENCODE_BAND_ROWS / _BANDS / _LUT_KSTEPS / _LUT_LIN_BYTES as a C compiler evaluates them == abi.py, for every odd edge; the
    shipped values at 15 / 31 are unchanged and no edge has more bands than the env head folds."""
    c = tmp_path / "g.c"
    c.write_text('#include <stdio.h>\n#include "ssd_hip.h"\nint main(){for(int V=3;V<=63;V+=2)printf("%d %d %d %d %d %d\\n",V,'
                 'SSD_ENCODE_BAND_ROWS(V),SSD_ENCODE_BANDS(V),SSD_ENCODE_LUT_KSTEPS(V),SSD_ENCODE_LUT_LIN_BYTES(V,1),SSD_ENCODE_LUT_LIN_BYTES(V,2));'
                 'printf("%d %d %d\\n",SSD_ENCODE_EDGE_MIN,SSD_ENCODE_EDGE_MAX,SSD_ENCODE_BANDS_MAX);return 0;}')
    exe = tmp_path / "g"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    rows = [[int(x) for x in ln.split()] for ln in lines[:len(ODD_EDGES)]]
    assert [int(x) for x in lines[len(ODD_EDGES)].split()] == [abi.ENCODE_EDGE_MIN, abi.ENCODE_EDGE_MAX, abi.ENCODE_BANDS_MAX]
    for V, r, nb, ks, l1, l2 in rows:
        O = V - 2
        assert (r, nb, ks) == (abi.encode_band_rows(V), abi.encode_bands(V), abi.encode_lut_ksteps(V)), V
        assert (abi.ENCODE_LUT_TABLE_BYTES, l1) == abi.encode_frag_bytes(V, 1, abi.ENCODE_LAYOUT_LUT)
        assert (abi.ENCODE_LUT_TABLE_BYTES, l2) == abi.encode_frag_bytes(V, 2, abi.ENCODE_LAYOUT_LUT)
        assert 1 <= nb <= 6 and (nb - 1) * r < O <= nb * r, V
        assert ks == sum((min(r, O - k * r) * O + 3) // 4 for k in range(nb)), V
    assert (abi.encode_bands(15), abi.encode_lut_ksteps(15), abi.encode_bands(31), abi.encode_lut_ksteps(31)) == (1, 43, 3, 73 + 73 + 66)
    assert [abi.encode_edge_supported(V) for V in (1, 2, 3, 15, 16, 31, 63, 64, 65)] == [False, False, True, True, False, True, True, False, False]


@pytest.mark.parametrize("V", [2, 16, 65])
def test_encoder_entry_points_refuse_unsupported_edges(V):
    """Even edges and edges outside 3 .. 63 are refused by the argument checks with a message, before any launch (no device needed:
    the pointers are never dereferenced)."""
    lib = abi.load_library()
    fake = 1 << 20                                          # aligned, non-null, never touched
    ea = abi.SsdPolicyEncodeArgs()
    ea.codes, ea.code_bytes, ea.env_stride, ea.agent_stride = fake, 1 << 20, V * V, V * V
    ea.rows, ea.view_edge, ea.n_agents, ea.precision, ea.layout = 16, V, 1, 2, abi.ENCODE_LAYOUT_LUT
    ea.conv_frags, ea.lin_frags, ea.conv_b, ea.lin_b, ea.out, ea.out_stride = fake, fake, fake, fake, fake, 32
    calls = (lambda: lib.ssd_policy_encode(C.byref(ea), None),
             lambda: lib.ssd_policy_pack_encoder_lut(fake, fake, fake, V, 2, fake, fake, None),
             lambda: lib.ssd_conv_wgrad_codes(fake, fake, fake, 16, V, None))
    for call in calls:
        with pytest.raises(abi.SsdError, match="view_edge must be odd, 3 .. 63"):
            abi.check(lib, call())


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _ctx(kind, n, N, view, **over):
    from homophily_marl_amd.run import load_config, setup
    cfg = load_config(kind, overrides=dict(dict(runner="hip_vec", batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False,
                                                store_state=False,
                                                env_args=dict(num_agents=n, map="default10" if kind == "harvest" else "default5",
                                                              episode_limit=20, seed=3, view_size=view),
                                                use_cuda=True, save_model=False, runner_stats=False), **over))
    return setup(cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("V", ODD_EDGES)
def test_encode_codes_op_at_every_edge_matches_torch_autograd(V):
    """ops.encode_codes (forward: the class-LUT encoder kernel, which also emits LeakyReLU(conv) at these edges; backward from those
    activations + ssd_conv_wgrad_codes) against torch autograd through Conv2d + LeakyReLU + Flatten + Linear + LeakyReLU on the
    expanded planes: features within 1e-5, each parameter gradient within 1e-5 of its scale; ragged R; and the no-grad form.  The
    reference runs in float64 on the CPU: MIOpen's own f32 weight gradient of this Conv2d is 3e-2 off at V = 59, R = 203 (measured on
    MI355X against float64; the kernels here are within 4e-6 there)."""
    from homophily_marl_amd import ops
    O = V - 2
    for R in (1, 17, 203):
        g = th.Generator(device="cuda").manual_seed(V * 1000 + R)
        codes = th.randint(0, 4, (R, V, V), generator=g, device="cuda", dtype=th.uint8)
        th.manual_seed(V + R)
        conv = th.nn.Conv2d(3, 6, 3, 1).cuda()
        lin = th.nn.Linear(6 * O * O, 32).cuda()
        wout = th.randn(R, 32, generator=g, device="cuda")
        feat = ops.encode_codes(codes, conv.weight, conv.bias, lin.weight, lin.bias)
        (feat * wout).sum().backward()
        got = [p.grad.cpu().double() for p in (conv.weight, conv.bias, lin.weight, lin.bias)]
        ps = [p.detach().cpu().double().requires_grad_() for p in (conv.weight, conv.bias, lin.weight, lin.bias)]
        ref = F.leaky_relu(F.linear(F.leaky_relu(F.conv2d(ops.expand_codes(codes).cpu().double(), ps[0], ps[1])).flatten(1), ps[2], ps[3]))
        (ref * wout.cpu().double()).sum().backward()
        assert (feat.cpu().double() - ref).abs().max() < 1e-5, (V, R, (feat.cpu().double() - ref).abs().max().item())
        for a, p_, name in zip(got, ps, ("conv_w", "conv_b", "lin_w", "lin_b")):
            assert (a - p_.grad).abs().max() < 1e-5 * max(1.0, p_.grad.abs().max().item()), (V, R, name, (a - p_.grad).abs().max().item())
        with th.no_grad():
            f0 = ops.encode_codes(codes, conv.weight, conv.bias, lin.weight, lin.bias)
            assert (f0.cpu().double() - ref).abs().max() < 1e-5, (V, R)


ROLLOUT_VIEWS = [1, 2, 3, 5, 10, 16, 20, "max"]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [203, 4096])
@pytest.mark.parametrize("kind", ["cleanup", "harvest"])
@pytest.mark.parametrize("view", ROLLOUT_VIEWS)
def test_rollout_encoder_at_other_views_matches_the_torch_encoder(view, kind, N):
    """FastPolicy.encode (fused class-LUT encoder) against mac.encode_obs at views other than 7 / 15: class codes in the dense side
    buffer, the same windows as channel masks, an episode storage read at a device time slot, codes derived from f32 planes; 5 agents.
    A view above the largest the env accepts is asserted refused by ssd_create instead."""
    from homophily_marl_amd.fast_policy import FastPolicy
    from homophily_marl_amd.envs.native import NativeEnv
    n, mapname = 5, "default10" if kind == "harvest" else "default5"
    vmax = _v_max(kind, mapname, n)
    view = vmax if view == "max" else view
    if view > vmax:
        with pytest.raises(abi.SsdError):
            NativeEnv(kind, device=0, map=mapname, num_agents=n, n_env=1, view_size=view)
        return
    th.manual_seed(2)
    ctx = _ctx(kind, n, N, view)
    mac, V = ctx.mac, 2 * view + 1
    fp = FastPolicy(mac, N, ctx.runner.env.avail_actions_batch[0, 0], seed=1)
    assert fp.fused_enc and fp.bands == abi.encode_bands(V) and fp.inc_encode == (V in (15, 31))
    g = th.Generator(device="cuda").manual_seed(5)
    u = th.rand(N, n, V, V, generator=g, device="cuda")
    codes = (u > 0.55).to(th.uint8) + (u > 0.7).to(th.uint8) + (u > 0.85).to(th.uint8)      # classes 0..3
    obs = mac.expand_codes(codes)
    with th.no_grad():
        ref = mac.encode_obs(obs).reshape(N, n, 32).transpose(0, 1)

    def features():
        if fp.bands == 1:
            return fp.inputs[..., :32].clone()
        return F.leaky_relu(fp.p["lb"] + fp.feat_part.sum(0)).reshape(n, N, 32)

    dense = F.pad(codes.reshape(N, n, V * V), (0, abi.code_agent_stride(V) - V * V)).contiguous()
    fp.encode(None, codes=dense, mask_alphabet=False)
    d = [(features() - ref).abs().max().item()]
    masks = th.tensor([0, 2, 1, 4], dtype=th.uint8, device="cuda")[dense.long()]
    fp.inputs.zero_()
    fp.encode(None, codes=masks)
    d.append((features() - ref).abs().max().item())
    fp.inputs.zero_()
    storage = th.zeros(N, 4, n, V, V, dtype=th.uint8, device="cuda")
    storage[:, 2] = codes
    t = th.full((1,), 1, dtype=th.long, device="cuda")
    tc, ctr = th.zeros(1, dtype=th.long, device="cuda"), th.zeros(1, dtype=th.long, device="cuda")
    fp.encode(None, codes=storage[:, 1:], slot_t=t, t_copy=tc, counter_inc=ctr)     # (a view: the rows end inside the storage)
    d.append((features() - ref).abs().max().item())
    fp.inputs.zero_()
    fp.encode(obs)
    d.append((features() - ref).abs().max().item())
    print("view", view, "V", V, "bands", fp.bands, "max |diff|", d, "ref max", ref.abs().max().item())
    assert max(d) < 2e-6 and int(tc) == 1 and int(ctr) == 1
    if N == 203:            # the labelled bf16 variant (precision 1): single bf16 products
        fp1 = FastPolicy(mac, N, ctx.runner.env.avail_actions_batch[0, 0], seed=1, precision=1)
        fp1.encode(None, codes=dense, mask_alphabet=False)
        f1 = fp1.inputs[..., :32] if fp1.bands == 1 else F.leaky_relu(fp1.p["lb"] + fp1.feat_part.sum(0)).reshape(n, N, 32)
        assert (f1 - ref).abs().max().item() < 2e-2 * max(1.0, ref.abs().max().item())
    ctx.runner.close_env()


RUNNER_CASES = [("cleanup", 3, "code"), ("cleanup", 3, "f32"), ("cleanup", 5, "code"), ("cleanup", 5, "f32"), ("cleanup", 10, "code"),
                ("cleanup", 10, "f32"), ("harvest", 10, "code"), ("harvest", 10, "f32")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,view,storage", RUNNER_CASES)
def test_graph_runner_keeps_the_fused_policy_at_other_views(kind, view, storage):
    """hip_graph at views other than 7 / 15 keeps FastPolicy with the fused encoder under both storages (the pipelined
    inc-head + encoder launch is instantiated for 15 / 31 only: pipe is False and the standalone launches run with direct_obs /
    fold_store).  The stored batch replays exactly on the CPU oracle; greedy env actions equal the argmax of the torch controller's Q
    on the stored batch where the top two are not tied; then one train_iteration with strict_device_ops and finite losses."""
    from homophily_marl_amd import ops
    from homophily_marl_amd.run import load_config, setup, train_iteration
    from oracle.oracle_py import OracleEnv
    N, T, n = 48, 14, 5
    mp = "default10" if kind == "harvest" else "default5"
    view = min(view, _v_max(kind, mp, n))
    th.manual_seed(0)
    cfg = load_config(kind, overrides=dict(
        runner="hip_graph", batch_size_run=N, batch_size=8, buffer_size=N, buffer_cpu_only=False, store_state=False,
        env_args=dict(num_agents=n, map=mp, episode_limit=T, seed=21, view_size=view), use_cuda=True, save_model=False, runner_stats=False,
        obs_storage=storage, steps_per_graph=2, strict_device_ops=True))
    try:
        ctx = setup(cfg)
        r = ctx.runner
        ofmt = abi.OBS_CODE if storage == "code" else abi.OBS_F32
        assert r.env.native.V == 2 * view + 1 and r.env.native.V not in (15, 31)
        orc = OracleEnv(kind, map=mp, num_agents=n, n_env=N, view_size=view, episode_limit=T, rng_mode=abi.RNG_COUNTER, seed=21)
        for ep in range(3):                                  # eager, captured, replayed
            batch = r.run(test_mode=False)
            assert r.fast is not None and r.fast.fused_enc and r.direct_obs and r.fold_store and not r.fast.inc_encode and not r.pipe
            assert ep == 0 or r._graph is not None
            orc.reset()
            acts = batch["actions"].squeeze(-1).cpu().numpy()
            for t in range(T):
                ob = orc.observe(ofmt)
                assert (batch["obs"][:, t].cpu().numpy() == ob["obs"]).all(), (ep, t)
                assert (batch["agent_pos"][:, t].cpu().numpy() == ob["pos"]).all()
                o = orc.step(acts[:, t])
                for k in ("reward", "clean_num", "apple_den"):
                    assert (batch[k][:, t].cpu().numpy() == o[k]).all(), (ep, t, k)
            assert (batch["obs"][:, T].cpu().numpy() == orc.observe(ofmt)["obs"]).all()
            assert int(batch["filled"].sum()) == N * (T + 1)
        orc.close()
        # greedy actions against the torch controller's Q on the stored batch
        batch = r.run(test_mode=True)
        with th.no_grad():
            q_env, _ = ctx.mac.unroll(batch)
        q = q_env[:, :T].masked_fill(batch["avail_actions"][:, :T] == 0, -1e30)
        top2 = q.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-4
        acts = batch["actions"][:, :T].squeeze(-1)
        assert float(clear.float().mean()) > 0.9
        assert bool((q.argmax(-1) == acts)[clear].all()), int((q.argmax(-1) != acts)[clear].sum())
        logged = {}
        log_stat = ctx.learner.logger.log_stat
        ctx.learner.logger.log_stat = lambda k, v, t, *a, **kw: (logged.__setitem__(k, float(v)), log_stat(k, v, t, *a, **kw))
        train_iteration(ctx, 0)
        assert all(k in logged for k in ("loss_value_env", "loss_value_inc", "loss_sim")), sorted(logged)
        assert all(np.isfinite(v) for v in logged.values()), logged
        r.close_env()
    finally:
        ops.set_strict(False)


def _learner_pair(view, B=4, T=12, n=5, seed=3):
    """A random class-code batch at `view` (cleanup default5): a device learner on the codes (captured train step) and a CPU
    learner (tensor-op statement) on the expanded planes, both from the same weights."""
    from homophily_marl_amd import ops
    from homophily_marl_amd.components.episode_buffer import EpisodeBatch
    from homophily_marl_amd.components.transforms import OneHot
    from homophily_marl_amd.controllers import REGISTRY as mac_REGISTRY
    from homophily_marl_amd.learners import REGISTRY as le_REGISTRY
    from homophily_marl_amd.run import load_config
    V, A = 2 * view + 1, 9
    g = th.Generator().manual_seed(seed)
    avail = (th.rand(B, T + 1, n, A, generator=g) < 0.7).int()
    avail[..., 4] = 1
    cls = th.randint(0, 4, (B, T + 1, n, V, V), generator=g).to(th.uint8)
    term = th.zeros(B, T + 1, 1, dtype=th.uint8)
    term[:, T - 1] = 1
    data = dict(actions=th.multinomial(avail.reshape(-1, A).float(), 1).reshape(B, T + 1, n, 1), avail_actions=avail,
                actions_inc=(th.randint(0, 3, (B, T + 1, n, n), generator=g) * (1 - th.eye(n, dtype=th.long))).unsqueeze(-1), terminated=term,
                reward=th.randint(-1, 3, (B, T + 1, n), generator=g).float() * (th.rand(B, T + 1, n, generator=g) < 0.3),
                clean_num=th.randint(0, 3, (B, T + 1, n), generator=g).float() * (th.rand(B, T + 1, n, generator=g) < 0.3),
                apple_den=th.rand(B, T + 1, n, generator=g), agent_pos=th.randint(1, 17, (B, T + 1, n, 2), generator=g).float(),
                agent_orientation=th.tensor([-1.0, 0.0]).expand(B, T + 1, n, 2).contiguous())
    logger = SimpleNamespace(log_stat=lambda *a, **k: None, console_logger=None)
    out = []
    for dev in ("cuda:0", "cpu"):
        cfg = load_config("cleanup", overrides=dict(env_args=dict(num_agents=n, map="default5", episode_limit=T, view_size=view),
                                                    use_cuda=dev != "cpu", batch_size=B, train_graph=dev != "cpu"))
        args = SimpleNamespace(**cfg)
        args.device, args.n_agents, args.n_actions = dev, n, A
        args.obs_shape, args.obs_dims, args.state_dims = (3, V, V), (V, V), (25, 18)
        code = dev != "cpu"
        scheme = {"obs": {"vshape": (V, V), "group": "agents", "dtype": th.uint8} if code else {"vshape": (3, V, V), "group": "agents"},
                  "actions": {"vshape": (1,), "group": "agents", "dtype": th.long},
                  "avail_actions": {"vshape": (A,), "group": "agents", "dtype": th.int}, "reward": {"vshape": (n,)},
                  "terminated": {"vshape": (1,), "dtype": th.uint8}, "clean_num": {"vshape": (n,)}, "apple_den": {"vshape": (n,)},
                  "agent_pos": {"vshape": (n, 2)}, "agent_orientation": {"vshape": (n, 2)},
                  "actions_inc": {"vshape": (n, 1), "group": "agents", "dtype": th.long}}
        batch = EpisodeBatch(scheme, {"agents": n}, B, T + 1, preprocess={"actions": ("actions_onehot", [OneHot(out_dim=A)])}, device=dev)
        batch.update(dict(data, obs=cls if code else ops.expand_codes(cls)))
        th.manual_seed(seed)
        mac = mac_REGISTRY[args.mac](batch.scheme, {"agents": n}, args)
        if out:
            mac.agent.load_state_dict({k: v.cpu() for k, v in out[0][1].agent.state_dict().items()})
        learner = le_REGISTRY[args.learner](mac, batch.scheme, logger, args)
        if dev != "cpu":
            mac.cuda(); learner.cuda()
        learner.target_mac.load_state(mac)
        out.append((batch, mac, learner))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("view", [2, 10])
def test_captured_train_step_at_other_views_matches_the_cpu_learner(view):
    """On the same class-code batch and weights: the device learner (encoder through ops.encode_codes, every operator on the HIP
    kernels, the step captured as hipGraphs and replayed) against the tensor-op learner on the CPU on the expanded planes: every
    logged value and the whole parameter gradient of the step within 1e-5 of scale."""
    from homophily_marl_amd import ops
    th.backends.cuda.matmul.allow_tf32 = False
    (bg, mg, lg), (bc, mc, lc) = _learner_pair(view)
    sd0 = {k: v.clone() for k, v in mg.agent.state_dict().items()}
    ops.set_strict(True)
    try:
        for _ in range(3):                                   # two eager calls, the capture at the third
            lg.train(bg, 0, 0)
        assert lg._graph is not None
        mg.agent.load_state_dict(sd0); lg.target_mac.load_state(mg)
        for opt in (lg.optimiser_env, lg.optimiser_inc):
            for st in opt.state.values():
                st["step"].zero_(); st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
        lg.train(bg, 0, 0)                                   # a replay
        logs_g = lg._static_logs
        grad_g = th.cat([p.grad.reshape(-1) for p in lg.params]).cpu()
    finally:
        ops.set_strict(False)
    logs_c = lc.cal_loss_and_step(bc)
    grad_c = th.cat([p.grad.reshape(-1) for p in lc.params])
    for k in LOG_KEYS:
        a, b = float(logs_g[k]), float(logs_c[k])
        assert abs(a - b) < 1e-5 * max(1.0, abs(b)), (k, a, b)
    assert float(grad_c.abs().max()) > 1e-4
    assert float((grad_g - grad_c).abs().max()) < 1e-5 * max(1.0, float(grad_c.abs().max())), (float((grad_g - grad_c).abs().max()),
                                                                                               float(grad_c.abs().max()))
    for (kg, vg), (kc, vc) in zip(mg.agent.state_dict().items(), mc.agent.state_dict().items()):     # the step itself
        assert kg == kc and float((vg.cpu() - vc).abs().max()) < 2e-5, kg
