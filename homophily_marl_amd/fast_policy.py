"""FastPolicy: rollout-time (no-grad) evaluation of the homophily controller for N vectorised envs.

Computes what HomophilyMAC.select_actions_env / select_actions_inc compute (homophily_controller.py:30-65 on top of
homophily_agent.py:154-208) with agent-major activations [n, N, 64] and the weights re-packed once per episode:
  * fused path (default; csrc/ssd_policy_mfma.hip): k_encode (conv + Linear encoder as banded GEMMs on the 16-bit matrix cores,
    reading the u8 class codes the env kernel emits) and ONE launch per head -- k_head<env> (input tail + fc1 + GRU + dueling +
    epsilon-greedy) and k_head<inc> (the same plus the per-pair term) -- which also file their results in the episode storage.
    `precision` 2 (default): every f32 product as three f16 MFMA products of two-term splits (f32-equivalent, the reference's dtype);
    1: single bf16 products (BASELINE.json's "bf16 Q-net" variant; rollout inference only, the learner stays fp32);
  * per-layer path (fused=False, or window sizes / palettes without a fused encoder): every per-agent layer as one batched GEMM
    (hipBLASLt) between the small kernels of csrc/ssd_policy.hip; the incentive head's pairwise layer [h_i | other_j] @ W is
    split into h_i @ W_h + other_j @ W_o, so the [n, N * n, H + E] concatenation is never materialised.
Both implement the shipped _build_inputs flag set (config/default.yaml:45-51).  obs_others_last_action (fused heads, opt-in through
the controller's rollout_input_flags): the block's n * n_actions columns are n one-hot vectors, so the heads add the matching rows of
fc1 (others_rows, snapshot by the pack launch) instead of multiplying by them; the previous actions of all agents travel in a pair of
per-env byte records selected by the timestep's parity (prev_rec: the env head of t reads [t & 1] and writes the other, the inc head of
t reads [t & 1]) -- no launch reads what a sibling workgroup writes.  fused_onehot_gather (rollout_input_flags holds
abi.INPUT_GATHER_ONEHOT): every one-hot block is gathered that way -- the own last action, the agent id, the inc head's one-hot action,
the others' block if flagged -- from one table per head (onehot_<head>); the image keeps 32 + sign r + sign inc + distances + pos, which
fits at any team size.  The own previous action is then read from prev_rec as well.
Which of these a controller takes -- fused heads or per-layer, gathered blocks, encoder layout, fused encoder, the pipelined launch -- is
decided in one place, plan_rollout (pure: the runners and the host tests call it without a device); FastPolicy takes its values from there.
Action RNG: the package's counter generator (not torch's Philox) keyed by the GLOBAL env id (env_id_base + local env), so env
shards draw what the unsharded job draws; exploration draws are not parity-pinned against torch.
"""
import ctypes as C
import os
from dataclasses import dataclass

import torch as th
import torch.nn.functional as F

from . import abi, ops


@dataclass(frozen=True)
class RolloutPlan:
    """Which rollout kernels a controller takes (plan_rollout): every choice FastPolicy and the runners make from the controller alone."""
    supported: bool         # the rollout kernels build this controller's input layout (on the fused heads or the per-layer path)
    fused: bool             # one launch per head (csrc/ssd_policy_mfma.hip); else the per-layer composition
    flags: object           # the controller's rollout flag word (None: a set the kernels do not take)
    others: bool            # the others' last-action block is gathered (INPUT_OTHERS_LAST_ACTION)
    gather: bool            # every one-hot block is gathered (INPUT_GATHER_ONEHOT)
    inp_dense: int          # columns of the 64-column image / of `inputs`
    V: int                  # window edge
    enc_layout: int         # abi.ENCODE_LAYOUT_LUT / _TOEPLITZ
    fused_enc: bool         # the fused encoder reads class codes
    inc_encode: bool        # act_inc_encode exists: the pipelined rollout's third launch
    bands: int              # bands the fused encoder cuts the output rows into
    needs_prev_rec: bool    # the heads read the previous actions of all agents from the record pair (FastPolicy.prev_rec)


def plan_rollout(mac, fused=True, environ=os.environ):
    """The RolloutPlan of controller `mac` (fused: the caller allows the fused heads).  Pure: no device, no library, no allocation.
    supported: the shipped flag set on either path, any other combination of the _build_inputs flags (homophily_controller.py:137-184)
    on the fused heads as long as the DENSE inputs (+ the inc head's one-hot action) fit the 64-column weight image.
    obs_others_last_action is not dense -- the heads gather fc1's rows for it -- and is taken when the controller opts in
    (rollout_input_flags holds bit 64; else its flag word is None).  Under abi.INPUT_GATHER_ONEHOT (config key fused_onehot_gather) no
    one-hot block is dense and every flag set fits (32 + sign r + sign inc + distances + pos <= 46 at n <= abi.MAX_AGENTS)."""
    a = mac.args
    n, H, A = mac.n_agents, a.rnn_hidden_dim, a.n_actions
    flags = getattr(mac, "rollout_input_flags", mac.input_flags)
    others = flags is not None and bool(flags & abi.INPUT_OTHERS_LAST_ACTION)
    gather = flags is not None and bool(flags & abi.INPUT_GATHER_ONEHOT)
    inp_dense = mac.input_shape - (n * A if others else 0)
    if gather:     # every one-hot block is gathered: the inc head's action too (nothing follows the dense columns)
        inp_dense -= (A if flags & abi.INPUT_LAST_ACTION else 0) + (n if flags & abi.INPUT_AGENT_ID else 0)
    V = int(a.obs_dims[0])
    # fused: one launch per head (csrc/ssd_policy_mfma.hip), inputs padded to 64 columns; otherwise the per-layer composition
    # (batched hipBLASLt GEMMs + the small kernels of csrc/ssd_policy.hip), which assembles the shipped input layout only
    fused = bool(fused) and H == 64 and inp_dense + (0 if gather else A) <= 64 and A + 7 <= 16 and flags is not None
    supported = bool(mac.shipped_flags) or (fused and (not gather or n <= abi.MAX_AGENTS))
    # encoder images: the class-LUT layout (conv as a table sum, no conv MFMAs: include/ssd_hip.h SSD_ENCODE_LAYOUT_LUT) unless
    # enc_layout / SSD_ENC_LAYOUT asks for round 3's Toeplitz fragments (kept as the cross-check and for the training forward)
    lay = getattr(a, "enc_layout", None) or environ.get("SSD_ENC_LAYOUT", "lut")
    enc_layout = abi.ENCODE_LAYOUT_TOEPLITZ if str(lay).lower() in ("toeplitz", "0") else abi.ENCODE_LAYOUT_LUT
    lut = enc_layout == abi.ENCODE_LAYOUT_LUT
    # the fused encoder: the class-LUT layout for every odd window edge 3 .. 63 (view_size 1 .. 31), the Toeplitz layout for
    # 15 x 15 and 31 x 31 windows (view_size 7 / 15: the shipped configurations)
    shipped = V in (15, 31)
    fused_enc = fused and abi.encode_edge_supported(V) and tuple(a.obs_dims) == (V, V) and (shipped or lut)
    # act_inc_encode (inc head of t + encoder of t + 1 as one launch: the pipelined rollout): 15 / 31 always; every other edge
    # with the opt-in key pipeline_any_view under the class-LUT layout (k_inc_encode_any), else the standalone encoder and
    # inc-head launches.  The gathered layouts (others / gather): with the opt-in key pipeline_gathered under the class-LUT layout
    # at every supported edge (k_inc_encode_gather), else the four standalone launches
    if others or gather:
        inc_encode = fused_enc and bool(getattr(a, "pipeline_gathered", False)) and lut
    else:
        inc_encode = fused_enc and (shipped or (bool(getattr(a, "pipeline_any_view", False)) and lut))
    return RolloutPlan(supported=supported, fused=fused, flags=flags, others=others, gather=gather, inp_dense=inp_dense, V=V,
                       enc_layout=enc_layout, fused_enc=fused_enc, inc_encode=inc_encode, bands=abi.encode_bands(V) if fused_enc else 1,
                       needs_prev_rec=others or gather)


class FastPolicy:
    def __init__(self, mac, n_env, avail_mask_u8, seed=0, fused=True, precision=2, env_id_base=0):
        self.mac, self.agent, self.a = mac, mac.agent, mac.args
        a = self.a
        assert a.rgb_input and a.conv_out == 6 and a.obs_dim_net == 32 and a.conv_kernel == 3 and a.conv_stride == 1
        assert precision in (1, 2)
        self.plan = plan = plan_rollout(mac, fused)
        assert plan.supported, "FastPolicy: this _build_inputs flag set needs the fused heads (FastPolicy.supports)"
        self.fused, self.flags, self.others, self.gather, self.inp_dense = plan.fused, plan.flags, plan.others, plan.gather, plan.inp_dense
        self.V, self.enc_layout, self.fused_enc, self.inc_encode, self.bands = plan.V, plan.enc_layout, plan.fused_enc, plan.inc_encode, plan.bands
        self.lib = abi.load_library()
        self.N, self.n, self.H, self.A = n_env, mac.n_agents, a.rnn_hidden_dim, a.n_actions
        self.dev = next(self.agent.parameters()).device
        self.inp = mac.input_shape
        self.precision, self.env_id_base = int(precision), int(env_id_base) & 0xFFFFFFFF
        n, N, H = self.n, self.N, self.H
        f32 = dict(dtype=th.float32, device=self.dev)
        # bf16 MFMA products an f32-equivalent product costs (bench.py's roofline accounting); conv: the planes are exact, 2
        self.n_products = dict(encode_conv=2, encode_lin=3, head_env=3, head_inc=3) if precision == 2 else \
            dict(encode_conv=1, encode_lin=1, head_env=1, head_inc=1)
        if self.fused_enc and self.enc_layout == abi.ENCODE_LAYOUT_LUT:
            self.n_products["encode_conv"] = 0      # the conv is a table sum on the vector unit: no matrix-core products

        # [feat | tail (| 0)], agent-major; a PAIR of buffers: the pipelined rollout (act_inc_encode) encodes timestep t + 1 into
        # the other buffer while the inc head still reads the rows of t.  Everything else uses buffer 0 (`inputs`).
        self.inputs_pair = th.zeros(2, n, N, 64 if self.fused else self.inp, **f32)
        self.inputs = self.inputs_pair[0]
        self.feat_part = th.zeros(self.bands, n * N, 32, **f32) if self.bands > 1 else None
        self.h_env = th.zeros(n, N, H, **f32)
        self.h_inc = th.zeros(n, N, H, **f32)
        self.actions = th.zeros(N, n, dtype=th.long, device=self.dev)
        self.actions_inc = th.zeros(N, n, n, dtype=th.long, device=self.dev)
        self.avail = avail_mask_u8.to(device=self.dev, dtype=th.uint8).contiguous()
        self._avail_bits = 0x80000000 | sum(1 << k for k, v in enumerate(avail_mask_u8.detach().cpu().reshape(-1).tolist()[:31]) if v)   # ssd_policy_head.avail_bits
        self.seed = seed & 0xFFFFFFFF
        self.arange_n = th.arange(n, device=self.dev).unsqueeze(1)
        # every agent's previous env action, one byte per agent (0xFF = none), 16 bytes per env, as a pair selected by the timestep's parity
        self.prev_rec = th.full((2, N, abi.PREV_RECORD_BYTES), 0xFF, dtype=th.uint8, device=self.dev) if plan.needs_prev_rec else None
        self.pack()

    def _stream(self):
        return th.cuda.current_stream(self.dev).cuda_stream

    @th.no_grad()
    def pack(self):
        """Snapshot the (possibly just trained) weights into kernel-ready packs; values are written in place so that a captured
        graph keeps seeing the same addresses.  Fused path: the fragment images of the encoder and one image per agent and head,
        built on the device by ssd_policy_pack_encoder / ssd_policy_pack_head (3 launches); per-layer path: GEMM-ready operands.
        The launches are themselves replayed as one hipGraph from the third call on (parameters and packs live at fixed addresses;
        the optimisers update in place)."""
        self._pack_calls = getattr(self, "_pack_calls", 0) + 1
        g = getattr(self, "_pack_graph", None)
        if g is not None:
            g.replay()
            return
        if self._pack_calls == 3 and self.dev.type == "cuda" and not th.cuda.is_current_stream_capturing():
            th.cuda.synchronize()
            g = th.cuda.CUDAGraph()
            with ops.capture(g, capture_error_mode="thread_local"):
                self._pack_eager()
            self._pack_graph = g
            g.replay()
            return
        self._pack_eager()

    @th.no_grad()
    def _pack_eager(self):
        ag, H, A = self.agent, self.H, self.A
        w, b = ag._w, ag._b
        lin = ag.conv_to_fc[3].weight
        packs = dict(cw=ag.conv_to_fc[0].weight, cb=ag.conv_to_fc[0].bias, lb=ag.conv_to_fc[3].bias)
        if not self.fused_enc:
            packs["lw_t"] = lin.t()
        if not self.fused:
            packs.update(
                w1e=w("fc1_env_w"), b1e=b("fc1_env_b"),
                w2e=th.cat([w("fc2_env_w"), w("fc2_env_v_w")], dim=2), b2e=th.cat([b("fc2_env_b"), b("fc2_env_v_b")], dim=2),
                w1i_x=w("fc1_inc_w")[:, :self.inp], w1i_a=w("fc1_inc_w")[:, self.inp:], b1i=b("fc1_inc_b"))
            packs["wie"], packs["whe"], packs["bie"], packs["bhe"] = ag._gru_weights("env")
            packs["wii"], packs["whi"], packs["bii"], packs["bhi"] = ag._gru_weights("inc")
            w2i = th.cat([w("fc2_inc_w"), w("fc2_inc_v_w")], dim=2)                       # [n, H + E, 4]
            packs["w2i_h"] = w2i[:, :H]
            packs["w2i_o"] = w2i[:, H:].permute(1, 0, 2).reshape(w2i.shape[1] - H, -1)    # [E, n(i) * 4]
            packs["b2i"] = th.cat([b("fc2_inc_b"), b("fc2_inc_v_b")], dim=2).unsqueeze(2)  # [n, 1, 1, 4]
        if not hasattr(self, "p"):
            self.p = {k: v.detach().clone().contiguous() for k, v in packs.items()}
            u8 = dict(dtype=th.uint8, device=self.dev)
            if self.fused:
                for head in ("env", "inc"):
                    self.p["img_" + head] = th.zeros(self.n, abi.policy_image_bytes(self.precision), **u8)
                    if self.gather:     # fc1's rows of every one-hot block (ssd_policy_head.onehot_rows; written by the pack launch)
                        self.p["onehot_" + head] = th.zeros(self.n, abi.onehot_rows(self.n, self.A, self.flags), 64, dtype=th.float32, device=self.dev)
                    elif self.others:   # fc1's rows of the others' last-action block, f32 as they are (written by the pack launch)
                        self.p["rows_" + head] = th.zeros(self.n, self.n * self.A, 64, dtype=th.float32, device=self.dev)
            if self.fused_enc:
                cbytes, lbytes = abi.encode_frag_bytes(self.V, self.precision, self.enc_layout)
                self.p["conv_frags"], self.p["lin_frags"] = th.zeros(cbytes, **u8), th.zeros(lbytes, **u8)
        else:
            for k, v in packs.items():
                self.p[k].copy_(v)
        st = self._stream()
        if self.fused:
            for head in ("env", "inc"):
                hp = self._head_params(head)
                if self.gather:
                    hp.input_flags, hp.n_actions = abi.INPUT_EXPLICIT | int(self.flags), self.A
                    hp.onehot_rows = self.p["onehot_" + head].data_ptr()
                elif self.others:
                    hp.input_flags, hp.n_actions = abi.INPUT_EXPLICIT | int(self.flags), self.A
                    hp.others_rows = self.p["rows_" + head].data_ptr()
                abi.check(self.lib, self.lib.ssd_policy_pack_head(C.byref(hp), self.precision, self.p["img_" + head].data_ptr(), st))
        if self.fused_enc:
            pack = self.lib.ssd_policy_pack_encoder_lut if self.enc_layout == abi.ENCODE_LAYOUT_LUT else self.lib.ssd_policy_pack_encoder
            abi.check(self.lib, pack(ag.conv_to_fc[0].weight.data_ptr(), ag.conv_to_fc[0].bias.data_ptr(), lin.data_ptr(), self.V, self.precision,
                                     self.p["conv_frags"].data_ptr(), self.p["lin_frags"].data_ptr(), st))

    @staticmethod
    def supports(mac, fused=True):
        """Whether the rollout kernels build this controller's input layout (plan_rollout)."""
        return plan_rollout(mac, fused).supported

    def _head_params(self, head):
        """ssd_policy_head_params of one head: pointers to the reference-shaped parameters (homophily_agent.py:37-125)."""
        ag = self.agent
        g = lambda name: getattr(ag, name)
        for t in (g("fc1_%s_w" % head), g("fc2_%s_w" % head)):
            assert t.is_contiguous() and t.dtype == th.float32
        hp = abi.SsdPolicyHeadParams()
        hp.fc1_w, hp.fc1_b = g("fc1_%s_w" % head).data_ptr(), g("fc1_%s_b" % head).data_ptr()
        for k, gate in enumerate("rzn"):
            hp.w_i[k], hp.w_h[k] = g("rnn_%s_i%s_w" % (head, gate)).data_ptr(), g("rnn_%s_h%s_w" % (head, gate)).data_ptr()
            hp.b_i[k], hp.b_h[k] = g("rnn_%s_i%s_b" % (head, gate)).data_ptr(), g("rnn_%s_h%s_b" % (head, gate)).data_ptr()
        hp.fc2_w, hp.fc2_b = g("fc2_%s_w" % head).data_ptr(), g("fc2_%s_b" % head).data_ptr()
        hp.fc2_v_w, hp.fc2_v_b = g("fc2_%s_v_w" % head).data_ptr(), g("fc2_%s_v_b" % head).data_ptr()
        hp.n_agents, hp.fc1_in = self.n, g("fc1_%s_w" % head).shape[2]
        hp.fc2_in, hp.fc2_out = g("fc2_%s_w" % head).shape[2], g("fc2_%s_w" % head).shape[3]
        return hp

    def _check_eps_rows(self, eps_rows):
        """eps_rows (ssd_policy_head.epsilon_rows): a rate per env of this policy, f32 [n_env], contiguous, on the policy's device"""
        if not self.fused:
            raise ValueError("eps_rows: a rate per env is read by the fused heads only (the per-layer path keeps the scalar eps)")
        if not isinstance(eps_rows, th.Tensor) or eps_rows.dtype != th.float32:
            raise TypeError("eps_rows must be a float32 tensor, got %s" % (getattr(eps_rows, "dtype", type(eps_rows)),))
        if tuple(eps_rows.shape) != (self.N,) or not eps_rows.is_contiguous():
            raise ValueError("eps_rows must be contiguous with shape [n_env] = [%d], got %s" % (self.N, tuple(eps_rows.shape)))
        if eps_rows.device != self.dev:
            raise ValueError("eps_rows must be on the policy's device %s, got %s" % (self.dev, eps_rows.device))
        return eps_rows.data_ptr()

    def _head_args(self, inc, eps, step, q_out=None, buf=0, par=0, eps_rows=None):
        a = abi.SsdPolicyHead()
        if eps_rows is not None:
            a.epsilon_rows = self._check_eps_rows(eps_rows)
        a.n_env, a.n_agents, a.n_actions, a.input_shape = self.N, self.n, self.A, self.inp
        a.pos_scale = float(self.mac.pos_scale)
        a.seed = (self.seed ^ 0x5bd1e995) if inc else self.seed
        a.inputs = self.inputs_pair[buf].data_ptr()
        a.h = (self.h_inc if inc else self.h_env).data_ptr()
        a.weights = self.p["img_inc" if inc else "img_env"].data_ptr()
        a.epsilon, a.step = eps.data_ptr(), step.data_ptr()
        a.q_out = None if q_out is None else q_out.data_ptr()
        a.precision, a.env_id_base = self.precision, self.env_id_base
        a.input_flags = abi.INPUT_EXPLICIT | int(self.flags)
        if self.gather:
            a.onehot_rows = self.p["onehot_inc" if inc else "onehot_env"].data_ptr()
        elif self.others:
            a.others_rows = self.p["rows_inc" if inc else "rows_env"].data_ptr()
        if self.prev_rec is not None:
            a.prev_record = self.prev_rec[par & 1].data_ptr()
            if not inc:
                a.prev_record_out = self.prev_rec[(par & 1) ^ 1].data_ptr()
        return a

    def reset(self):
        self.h_env.zero_(); self.h_inc.zero_()
        if self.prev_rec is not None:
            self.prev_rec.fill_(0xFF)

    def set_prev_actions(self, prev_actions, par=0):
        """obs_others_last_action: write previous actions i64 [N, n] (-1 = none) into the record buffer of parity `par` -- for callers
        that hold the actions themselves (tests, a resumed episode); inside a rollout the env head carries the records."""
        self.prev_rec[par & 1, :, :self.n] = prev_actions.to(th.int8).view(th.uint8)

    # ---- env head -----------------------------------------------------------------------------------------------
    @th.no_grad()
    def act_env(self, obs, prev_actions, prev_reward, prev_inc, pos, eps, step, codes=None, slot_t=None, store_obs=None, store_t=None,
                q_out=None, orient=None, actions_i32=None, pos_copy=None, orient_copy=None, t_copy=None, counter_inc=None, file=None,
                mask_alphabet=None, eps_rows=None):
        """encode() followed by head_env(); returns actions i64 [N, n] (static buffer).  See the two methods for the arguments."""
        if eps_rows is not None:
            self._check_eps_rows(eps_rows)         # (refused before the encoder is launched)
        self.encode(obs, codes=codes, slot_t=slot_t, store_obs=store_obs, store_t=store_t, t_copy=t_copy, counter_inc=counter_inc,
                    mask_alphabet=mask_alphabet)
        return self.head_env(prev_actions, prev_reward, prev_inc, pos, eps, step, q_out=q_out, orient=orient, actions_i32=actions_i32,
                             pos_copy=pos_copy, orient_copy=orient_copy, file=file, eps_rows=eps_rows)

    @staticmethod
    def codes_from_obs(obs):
        """u8 class codes [N, n, stride] (SSD_OBS_CODE alphabet; stride = V * V rounded up to 16) of a simplified-palette observation
        f32 [N, n, 3, V, V]: waste = R -> 2, apple = G -> 1, wall / agent = B -> 3 (cleanup.py:93-105).  For callers that hold no
        code buffer (tests); the runner takes the codes the env kernel emits (ssd_obs_out.obs_code)."""
        N, n, _, V, _ = obs.shape
        c = ((obs[:, :, 0] > 0) * 2 + (obs[:, :, 1] > 0) * 1 + (obs[:, :, 2] > 0) * 3).to(th.uint8).reshape(N, n, V * V)
        return F.pad(c, (0, abi.code_agent_stride(V) - V * V)).contiguous()

    def _encode_args(self, obs, codes, slot_t, mask_alphabet, buf=0, slot_add=0, t_copy=None, counter_inc=None):
        """ssd_policy_encode_args of the fused encoder (see encode) writing inputs_pair[buf] / the band sums; returns (args, codes)."""
        p, n, N, V = self.p, self.n, self.N, self.V
        if codes is None:
            codes, mask_alphabet = self.codes_from_obs(obs), False
        if mask_alphabet is None:
            mask_alphabet = codes.dim() == 3
        assert codes.dtype == th.uint8 and codes.shape[0] == N
        ea = abi.SsdPolicyEncodeArgs()
        ea.codes = codes.data_ptr()
        ea.code_bytes = codes.untyped_storage().nbytes() - codes.storage_offset()
        if codes.dim() == 5:        # an episode storage [N, T+1, n, V, V], time slot *slot_t (+ slot_add)
            assert slot_t is not None and codes[0, 0].is_contiguous()
            ea.env_stride, ea.slot_stride, ea.agent_stride = codes.stride(0), codes.stride(1), V * V
        else:                       # the dense side buffer [N, n, stride]
            assert codes.dim() == 3 and codes[0].is_contiguous()
            ea.env_stride, ea.slot_stride, ea.agent_stride = codes.stride(0), 0, codes.stride(1)
        ea.slot_t = None if slot_t is None else slot_t.data_ptr()
        ea.slot_add = int(slot_add) if slot_t is not None else 0
        ea.rows, ea.view_edge, ea.n_agents, ea.agent_major, ea.precision = N * n, V, n, 1, self.precision
        ea.alphabet = abi.CODE_CHANNEL_MASK if mask_alphabet else abi.CODE_CLASS
        ea.conv_frags, ea.lin_frags = p["conv_frags"].data_ptr(), p["lin_frags"].data_ptr()
        ea.conv_b, ea.lin_b = p["cb"].data_ptr(), p["lb"].data_ptr()
        ea.layout = self.enc_layout
        if self.bands > 1:
            ea.part = self.feat_part.data_ptr()
        else:
            ea.out, ea.out_stride = self.inputs_pair[buf].data_ptr(), self.inputs_pair.shape[-1]
        ea.slot_t_copy = None if t_copy is None else t_copy.data_ptr()
        ea.counter_inc = None if counter_inc is None else counter_inc.data_ptr()
        return ea, codes

    @th.no_grad()
    def encode(self, obs, codes=None, slot_t=None, store_obs=None, store_t=None, t_copy=None, counter_inc=None, mask_alphabet=None, buf=0):
        """rgb_preprocess (homophily_agent.py:20-27,213-214) of the current observation into columns 0..31 of `inputs` (31 x 31
        windows: into the per-band partial sums that head_env finishes).
        Fused encoder: reads one byte per window cell -- `codes` [N, n, stride] = the env's obs_code side buffer (channel masks;
        mask_alphabet defaults to True for this layout) or an episode storage of class codes u8 [N, T+1, n, V, V] read at the
        device time index slot_t (SSD_OBS_CODE classes); with codes = None, class codes are derived from obs f32 [N, n, 3, V, V].
        Per-layer path: obs f32.  store_obs / store_t: copy obs into store_obs[:, t] (callers whose env does not write the storage
        itself).  t_copy receives *slot_t; counter_inc is incremented (device scalars for the kernels that follow)."""
        p, lib, n, N = self.p, self.lib, self.n, self.N
        st = self._stream()
        if self.fused_enc:
            ea, codes = self._encode_args(obs, codes, slot_t, mask_alphabet, buf=buf, t_copy=t_copy, counter_inc=counter_inc)
            abi.check(lib, lib.ssd_policy_encode(C.byref(ea), st))
            self._keep_codes = codes
            if store_obs is not None and obs is not None:
                store_obs.index_copy_(1, store_t, obs.unsqueeze(1))
            return
        assert buf == 0
        V = obs.shape[-1]
        so = (None if store_obs is None else store_obs.data_ptr(), 0 if store_obs is None else store_obs.stride(0),
              None if store_t is None else store_t.data_ptr())
        K = 6 * (V - 2) * (V - 2)
        if getattr(self, "_conv", None) is None or self._conv.shape[1] != K:
            self._conv = th.empty(n * N, K, dtype=th.float32, device=self.dev)           # agent-major rows
        abi.check(lib, lib.ssd_conv_leaky(obs.data_ptr(), N * n, V, 6, p["cw"].data_ptr(), p["cb"].data_ptr(), self._conv.data_ptr(), n, 1,
                                          so[0], so[1], so[2], st))
        feat = self.inputs.view(n * N, self.inputs.shape[-1])[:, :32]                    # Linear + LeakyReLU straight into the input matrix
        th.addmm(p["lb"], self._conv, p["lw_t"], out=feat)
        F.leaky_relu_(feat)

    @th.no_grad()
    def head_env(self, prev_actions, prev_reward, prev_inc, pos, eps, step, q_out=None, orient=None, actions_i32=None, pos_copy=None,
                 orient_copy=None, file=None, buf=0, par=None, eps_rows=None):
        """input tail + fc1 + GRU + dueling + epsilon-greedy of the env head on the features encode() left in `inputs`.
        eps_rows (optional, all three fused head launches): f32 [n_env] on the device, contiguous -- env b explores at eps_rows[b]
        instead of the scalar eps (ssd_policy_head.epsilon_rows); the per-layer path refuses it.
        obs_others_last_action: `par` = the timestep's parity -- the head reads prev_rec[par] and writes its picks to prev_rec[par ^ 1]
        (the rollout); par = None: a stand-alone call, the record is first set from `prev_actions` (set_prev_actions) and parity 0 used."""
        p, lib, n, N, H = self.p, self.lib, self.n, self.N, self.H
        st = self._stream()
        if eps_rows is not None:
            self._check_eps_rows(eps_rows)
        if self.fused:
            if self.prev_rec is not None and par is None:
                self.set_prev_actions(prev_actions, 0)
            ha = self._head_args(False, eps, step, q_out, buf, par or 0, eps_rows=eps_rows)
            ha.avail = self.avail.data_ptr()
            ha.avail_bits = self._avail_bits       # the mask itself (a constant of the env class): the kernel issues no loads for it
            ha.prev_actions, ha.prev_reward, ha.prev_actions_inc, ha.pos = (prev_actions.data_ptr(), prev_reward.data_ptr(),
                                                                          prev_inc.data_ptr(), pos.data_ptr())
            ha.out_actions = self.actions.data_ptr()
            if actions_i32 is not None:
                ha.out_actions_i32 = actions_i32.data_ptr()
            if pos_copy is not None:
                ha.orient, ha.pos_copy, ha.orient_copy = orient.data_ptr(), pos_copy.data_ptr(), orient_copy.data_ptr()
            if self.fused_enc and self.bands > 1:      # the encoder left per-band partial sums: the head finishes the features
                ha.feat_part, ha.feat_bands, ha.lin_b = self.feat_part.data_ptr(), self.bands, p["lb"].data_ptr()
            for k, v in (file or {}).items():
                setattr(ha, k, v)
            abi.check(lib, lib.ssd_policy_head_env(C.byref(ha), st))
            return self.actions
        abi.check(lib, lib.ssd_build_inputs(N, n, self.A, 2, prev_actions.data_ptr(), prev_reward.data_ptr(), prev_inc.data_ptr(),
                                            pos.data_ptr(), float(self.mac.pos_scale), self.inputs.data_ptr(), self.inp, 32, st))
        x = F.leaky_relu(th.baddbmm(p["b1e"], self.inputs, p["w1e"]))
        gi = th.baddbmm(p["bie"], x, p["wie"])
        gh = th.baddbmm(p["bhe"], self.h_env, p["whe"])
        abi.check(lib, lib.ssd_gru_gates(gi.data_ptr(), gh.data_ptr(), self.h_env.data_ptr(), n * N, H, st))
        av = th.baddbmm(p["b2e"], self.h_env, p["w2e"])                                # [n, N, A + 1]
        abi.check(lib, lib.ssd_dueling_pick(av.data_ptr(), n * N, self.A, self.avail.data_ptr(), eps.data_ptr(), step.data_ptr(),
                                            self.seed, n, N, 0, self.actions.data_ptr(), None if q_out is None else q_out.data_ptr(),
                                            self.env_id_base, st))
        self._keep = (x, gi, gh, av)
        return self.actions

    # ---- incentive head ---------------------------------------------------------------------------------------------
    @th.no_grad()
    def _inc_args(self, actions, pos, orient, reward, clean_num, apple_den, eps, step, q_out=None, file=None, buf=0, par=None, eps_rows=None):
        ha = self._head_args(True, eps, step, q_out, buf, par or 0, eps_rows=eps_rows)
        ha.actions, ha.pos_pre, ha.orient_pre = actions.data_ptr(), pos.data_ptr(), orient.data_ptr()
        ha.reward, ha.clean_num, ha.apple_den = reward.data_ptr(), clean_num.data_ptr(), apple_den.data_ptr()
        ha.out_actions = self.actions_inc.data_ptr()
        for k, v in (file or {}).items():
            setattr(ha, k, v)
        return ha

    @th.no_grad()
    def act_inc_encode(self, actions, pos, orient, reward, clean_num, apple_den, eps, step, codes, slot_t=None, slot_add=0, buf=0,
                       q_out=None, file=None, mask_alphabet=None, par=None, eps_rows=None):
        """act_inc of timestep t on inputs_pair[buf] AND encode of timestep t + 1 into inputs_pair[buf ^ 1] (several bands: into
        the band sums) as ONE launch (ssd_policy_head_inc_encode; the gathered layouts: with ssd_policy_head.pipeline_gather set): the
        pipelined rollout's third launch of a timestep.  `codes` / slot_t / slot_add as in encode(): the observation the env step of t
        just produced (storage slot *slot_t + slot_add).  `par` as in act_inc (the gathered layouts read prev_rec[par])."""
        assert self.fused and self.inc_encode
        ha = self._inc_args(actions, pos, orient, reward, clean_num, apple_den, eps, step, q_out=q_out, file=file, buf=buf, par=par, eps_rows=eps_rows)
        ea, codes = self._encode_args(None, codes, slot_t, mask_alphabet, buf=buf ^ 1, slot_add=slot_add)
        ha.pipeline_gather = int(self.others or self.gather)         # the gathered layouts ask for their own fused launch
        abi.check(self.lib, self.lib.ssd_policy_head_inc_encode(C.byref(ha), C.byref(ea), self._stream()))
        self._keep_codes = codes
        return self.actions_inc

    @th.no_grad()
    def act_inc(self, actions, pos, orient, reward, clean_num, apple_den, eps, step, q_out=None, file=None, buf=0, par=None, eps_rows=None):
        """actions i64 [N, n] (the env actions just taken); pos / orient: the PRE-step pose [N, n, 2]; reward, clean_num,
        apple_den [N, n] of this step.  Returns actions_inc i64 [N, n, n] with a zero diagonal (static buffer).
        obs_others_last_action: reads prev_rec[par] (the same buffer the env head of this timestep read; None = 0)."""
        p, lib, n, N, H = self.p, self.lib, self.n, self.N, self.H
        st = self._stream()
        if eps_rows is not None:
            self._check_eps_rows(eps_rows)
        if self.fused:
            ha = self._inc_args(actions, pos, orient, reward, clean_num, apple_den, eps, step, q_out=q_out, file=file, buf=buf, par=par, eps_rows=eps_rows)
            abi.check(lib, lib.ssd_policy_head_inc(C.byref(ha), st))
            return self.actions_inc
        assert buf == 0
        x = th.baddbmm(p["b1i"], self.inputs, p["w1i_x"]) + p["w1i_a"][self.arange_n, actions.t()]    # one-hot(a) @ W_a = row gather
        x = F.leaky_relu(x)
        gi = th.baddbmm(p["bii"], x, p["wii"])
        gh = th.baddbmm(p["bhi"], self.h_inc, p["whi"])
        abi.check(lib, lib.ssd_gru_gates(gi.data_ptr(), gh.data_ptr(), self.h_inc.data_ptr(), n * N, H, st))
        hpart = th.bmm(self.h_inc, p["w2i_h"])                                          # [n(i), N, 4]
        other = th.cat([F.one_hot(actions, self.A).float(), pos / self.mac.pos_scale, orient, reward.unsqueeze(-1),
                        clean_num.unsqueeze(-1), apple_den.unsqueeze(-1)], dim=-1)       # [N, n(j), E]
        opart = (other.reshape(N * n, -1) @ p["w2i_o"]).reshape(N, n, n, 4).permute(2, 0, 1, 3)   # [n(i), N, n(j), 4]
        av = (hpart.unsqueeze(2) + opart + p["b2i"]).contiguous()                        # [n(i), N, n(j), 4]
        abi.check(lib, lib.ssd_dueling_pick(av.data_ptr(), n * N * n, self.a.n_inc_actions, None, eps.data_ptr(), step.data_ptr(),
                                            self.seed ^ 0x5bd1e995, n, N, 1, self.actions_inc.data_ptr(), None if q_out is None else q_out.data_ptr(),
                                            self.env_id_base, st))
        self._keep2 = (x, gi, gh, av)
        return self.actions_inc

    # ---- reference-shaped Q access (tests) ---------------------------------------------------------------------------
    @th.no_grad()
    def q_values(self, av):
        a = av[..., :-1]
        return av[..., -1:] + a - a.mean(dim=-1, keepdim=True)
