"""What the learner-side entry points of libssd_hip.so refuse (CPU suite: the library loads without a device and every argument check
runs before any launch, as tests/test_encoder_any_view.py::test_encoder_entry_points_refuse_unsupported_edges already relies on).

For every learner export a baseline of valid arguments (dummy, never dereferenced device pointers) and a table of single departures
from it, each with the status the header promises.  ONLY invalid calls are made: the baseline itself is never called, nothing here may
reach a launch.  The export list is checked against abi.HIP_SIGNATURES, so a new export without a row in one of the three categories
(a refusal table here, NOT_LEARNER, ELSEWHERE) fails."""
import ctypes as C
import os

import numpy as np
import pytest

from homophily_marl_amd import abi

INV, UNS = abi.SSD_ERR_INVALID, abi.SSD_ERR_UNSUPPORTED
F = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched
I32_MAX = 2 ** 31 - 1

# exports that are not the learner's kernels (env, rollout, packing, process state): categorised, so a NEW name must be put somewhere
NOT_LEARNER = {
    "ssd_abi_version", "ssd_last_error", "ssd_create", "ssd_destroy", "ssd_reset", "ssd_step", "ssd_observe", "ssd_export_state",
    "ssd_import_state", "ssd_get_info", "ssd_step_observe", "ssd_encoder", "ssd_policy_head_env", "ssd_policy_head_inc",
    "ssd_build_inputs_width", "ssd_bmm_reserve_scratch", "ssd_learner_precision", "ssd_policy_head_plan", "ssd_policy_head_inc_encode",
    "ssd_policy_pack_encoder_lut", "ssd_policy_pack_encoder", "ssd_numeric_status", "ssd_policy_pack_head", "ssd_conv_leaky",
    "ssd_store_step_launch", "ssd_dueling_pick", "ssd_poll_error", "ssd_set_render", "ssd_render",
}

# exports whose refusal tables live in their feature's host test: export -> test module (under tests/)
ELSEWHERE = {
    "ssd_behaviour_stats": "test_behaviour_host",
    "ssd_sample_windows": "test_train_window_host", "ssd_gather_windows": "test_train_window_host",
    "ssd_priority_sample": "test_priority_host", "ssd_priority_update": "test_priority_host",
    "ssd_rollout_priority": "test_rollout_priority_host",
    "ssd_store_hidden": "test_stored_state_host", "ssd_gru_seq_fwd_h0": "test_stored_state_host", "ssd_gru_seq_bwd_h0": "test_stored_state_host",
}

CASES = []          # (export, label, callable(lib) -> status, expected status)
_keep = []          # host tables the calls read: kept alive


def table(name, base, rows):
    """rows: (label, {argument index: value}, expected)"""
    for label, change, expect in rows:
        args = list(base)
        for k, v in change.items():
            args[k] = v
        CASES.append((name, label, (lambda lib, n=name, a=tuple(args): getattr(lib, n)(*a)), expect))


def nulls(idx, expect=INV):
    return [("null argument %d" % k, {k: None}, expect) for k in idx]


def zeros(idx, expect=INV):
    return [("argument %d = 0" % k, {k: 0}, expect) for k in idx]


# ---- input assembly -----------------------------------------------------------------------------------------------------------------
_bi = [4, 5, 9, 0, F, F, F, F, 1.0, F, 64, 0, None]
table("ssd_build_inputs", _bi, zeros([0, 1, 2]) + nulls([4, 5, 6, 7, 9]) + [
    ("out_stride one short", {10: 9 + 5 + 3}, INV), ("out_offset < 0", {11: -1}, INV),
    ("batch * n_agents overflows int32", {0: 1 << 30, 1: 4}, INV), ("row width overflows int32", {1: 1 << 16, 2: 1 << 16, 10: I32_MAX}, INV)])
_bf = [4, 5, 9, 0, 0, F, F, F, F, 1.0, F, 128, 0, None]
table("ssd_build_inputs_flags", _bf, zeros([0, 1, 2]) + nulls([5, 6, 7, 8, 10]) + [
    ("unknown flag bit", {4: 0x100}, UNS), ("out_stride one short", {4: abi.INPUT_EXPLICIT | 127, 11: 9 + 5 + 2 + 45 + 5 + 2 - 1}, INV),
    ("out_offset < 0", {12: -1}, INV), ("batch * n_agents overflows int32", {0: 1 << 30, 1: 4}, INV),
    ("row width overflows int32", {1: 1 << 16, 2: 1 << 16, 11: I32_MAX}, INV)])
_uo = [F, F, F, F, F, F, 30.0, 4, 7, 5, 9, F, F, None]
table("ssd_unroll_other", _uo, nulls([0, 1, 2, 3, 4, 5, 11, 12]) + zeros([7, 8, 9, 10]) + [
    ("pos_scale 0", {6: 0.0}, INV), ("B * T * n overflows int32", {7: 1 << 16, 8: 1 << 16, 9: 2}, INV),
    ("B * T * n = limit + 1 (the last workgroup's thread index must fit)", {7: I32_MAX - 255, 8: 1, 9: 1}, INV)])
_it = [4, 7, 5, F, F, 1.0, 1.0, 1.0, 7.0, F, F, F, F, F, F, None]
table("ssd_incentive_transfer", _it, zeros([0, 2]) + [("T = 1", {1: 1}, INV)] + nulls([3, 4, 9, 10, 11, 12, 13, 14]))

# ---- reductions, copies ----------------------------------------------------------------------------------------------------------------
table("ssd_column_sums", [F, F, 2, 100, 7, None, None], nulls([0, 1]) + zeros([2, 3, 4]) + [
    ("groups over the grid limit", {2: 65536}, INV), ("row chunks over the grid limit", {3: 65535 * abi.COLSUM_CHUNK + 1}, INV)])
for _n, _lim in (("ssd_dueling_q_fwd", 16), ("ssd_dueling_q_bwd", 16)):
    table(_n, [F, F, F, 5, 7, 4, 1, 9, None], nulls([0, 1, 2]) + zeros([3, 4, 5, 6, 7]) + [("K = limit + 1", {7: _lim + 1}, INV)])
table("ssd_dueling_head_fwd", [F, F, 5, 7, 4, 1, 9, None], nulls([0, 1]) + zeros([2, 3, 4, 5, 6]) + [("K = limit + 1", {6: 16}, INV)])
table("ssd_dueling_head_bwd", [F, F, None, 5, 7, 4, 1, 9, None], nulls([0, 1]) + zeros([3, 4, 5, 6, 7]) + [("K = limit + 1", {7: 16}, INV)])


def _gather(src=F, dst=F, row_bytes=8, n=1):
    t = (abi.SsdRowGather * n)(*[abi.SsdRowGather(src, dst, row_bytes)] * n)
    _keep.append(t)
    return C.addressof(t)


table("ssd_gather_rows", [_gather(), 1, F, 4, None], nulls([0, 2]) + zeros([1, 3]) + [
    ("count = limit + 1", {0: _gather(n=abi.COPY_BLOCKS_MAX + 1), 1: abi.COPY_BLOCKS_MAX + 1}, INV), ("n_ids over the grid limit", {3: 65536}, INV),
    ("field src null", {0: _gather(src=None)}, INV), ("field dst null", {0: _gather(dst=None)}, INV), ("row_bytes 0", {0: _gather(row_bytes=0)}, INV)])
table("ssd_sample_ids", [7, 0, 2000, 16, F, None], nulls([4]) + zeros([3]) + [
    ("count = limit + 1", {3: abi.SAMPLE_IDS_MAX + 1}, INV), ("population < count", {2: 15}, INV)])


def _copy(src=F, dst=F, rows=3, cols=4, ss=5, ds=6, n=1):
    t = (abi.SsdBlockCopy * n)(*[abi.SsdBlockCopy(src, dst, rows, cols, ss, ds)] * n)
    _keep.append(t)
    return C.addressof(t)


table("ssd_copy_blocks", [_copy(), 1, None], nulls([0]) + zeros([1]) + [
    ("count = limit + 1", {0: _copy(n=abi.COPY_BLOCKS_MAX + 1), 1: abi.COPY_BLOCKS_MAX + 1}, INV),
    ("src null", {0: _copy(src=None)}, INV), ("dst null", {0: _copy(dst=None)}, INV), ("rows 0", {0: _copy(rows=0)}, INV),
    ("cols 0", {0: _copy(cols=0, ss=1, ds=1)}, INV), ("src_stride < cols", {0: _copy(ss=3)}, INV), ("dst_stride < cols", {0: _copy(ds=3)}, INV),
    ("rows * cols overflows int32", {0: _copy(rows=46341, cols=46341, ss=46341, ds=46341)}, INV),
    ("rows * cols = limit + 1 (the last grid stride must fit)", {0: _copy(rows=1, cols=I32_MAX - 64 * 256 + 1, ss=I32_MAX, ds=I32_MAX)}, INV)])


def _fill(dst=F, nbytes=8, n=1):
    t = (abi.SsdBlockFill * n)(*[abi.SsdBlockFill(dst, nbytes, 0, 0)] * n)
    _keep.append(t)
    return C.addressof(t)


table("ssd_fill_blocks", [_fill(), 1, None], nulls([0]) + zeros([1]) + [
    ("count = limit + 1", {0: _fill(n=abi.FILL_BLOCKS_MAX + 1), 1: abi.FILL_BLOCKS_MAX + 1}, INV), ("dst null", {0: _fill(dst=None)}, INV),
    ("0 bytes", {0: _fill(nbytes=0)}, INV), ("bytes not a multiple of 4", {0: _fill(nbytes=6)}, INV), ("dst misaligned", {0: _fill(dst=F + 2)}, INV)])
table("ssd_runner_stats", [F, F, F, 64, 320, F, None], nulls([0, 1, 2, 5]) + zeros([3, 4]))


# ---- optimiser tail, loss ------------------------------------------------------------------------------------------------------------
def _adam(**kw):
    a = abi.SsdClipAdamArgs(flat_grad=F, total=1000, jobs=F, n_jobs=3, partials=F, lr_inc=1e-3, lr_env=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip=10.0)
    for k, v in kw.items():
        setattr(a, k, v)
    _keep.append(a)
    return C.byref(a)


table("ssd_clip_adam_step", [_adam(), None], nulls([0]) + [(k + " = " + repr(v), {0: _adam(**{k: v})}, INV) for k, v in (
    ("flat_grad", None), ("jobs", None), ("partials", None), ("total", 0), ("total", 1 << 31), ("n_jobs", 0), ("n_jobs", abi.ADAM_MAX_JOBS + 1),
    ("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("eps", 0.0), ("clip", 0.0))])


def _td(**kw):
    a = abi.SsdTdLossArgs(batch=4, t_slots=8, n_agents=5, n_actions=9, sim_horizon=3, double_q=1, gamma_env=0.99, gamma_inc=0.99, reward_scale=1.0,
                          incentive_ratio=1.0, incentive_cost=1.0, incentive=1.0, seq_len=8.0, sim_threshold=0.1, sim_loss_weight=0.1)
    for k in ("q_env", "q_inc", "tq_env", "tq_inc", "actions", "actions_inc", "avail", "reward", "clean_num", "terminated", "filled", "dens",
              "dq_env", "dq_inc", "partials"):
        setattr(a, k, F)
    for k, v in kw.items():
        setattr(a, k, v)
    _keep.append(a)
    return C.byref(a)


_td_rows = [(k + " = " + repr(v), {0: _td(**{k: v})}, INV) for k, v in (
    ("batch", 0), ("t_slots", 1), ("n_agents", 1), ("n_agents", abi.MAX_AGENTS + 1), ("n_actions", 0), ("sim_horizon", 0), ("seq_len", 0.0),
    ("reward_scale", 0.0), ("reward", None), ("clean_num", None), ("terminated", None), ("filled", None), ("partials", None))]
_td_rows += [("B * T * n overflows int32", {0: _td(batch=1 << 28, t_slots=2, n_agents=10)}, INV),
             ("B * T * n = limit + 1 (the last workgroup's thread index must fit)", {0: _td(batch=(I32_MAX - 255) // 4 + 1, t_slots=2, n_agents=2)}, INV)]
table("ssd_td_sim_loss", [_td(), 0, None], nulls([0]) + _td_rows)
table("ssd_td_sim_loss", [_td(), 1, None], [("mode 1: " + k + " null", {0: _td(**{k: None})}, INV) for k in (
    "q_env", "q_inc", "tq_env", "tq_inc", "actions", "actions_inc", "avail", "dens", "dq_env", "dq_inc")])

# ---- GRU ------------------------------------------------------------------------------------------------------------------------------
table("ssd_gru_gates", [F, F, F, 10, 64, None], nulls([0, 1, 2]) + zeros([3, 4]))
table("ssd_gru_gates_fwd", [F, F, F, F, F, 10, 64, None], nulls([0, 1, 2, 3, 4]) + zeros([5, 6]))
table("ssd_gru_gates_bwd", [F] * 7 + [10, 64, None], nulls(range(7)) + zeros([7, 8]))
table("ssd_gru_seq_fwd", [F] * 6 + [7, 3, 16, None], nulls([0, 1, 2, 3]) + zeros([6, 7, 8]) + [
    ("rzn without ghn", {5: None}, INV), ("ghn without rzn", {4: None}, INV), ("B % 16", {8: 17}, INV), ("B % 16 (8)", {8: 8}, INV)] +
    [("argument %d misaligned" % k, {k: F + 4}, INV) for k in range(6)])
table("ssd_gru_seq_bwd", [F] * 9 + [7, 3, 16, None], nulls(range(9)) + zeros([9, 10, 11]) + [("B % 16", {11: 24}, INV)] +
      [("argument %d misaligned" % k, {k: F + 8}, INV) for k in range(7)])


def _ptrs(*p):
    t = (C.c_void_p * 4)(*p)
    _keep.append(t)
    return C.addressof(t)


_P2, _P4 = _ptrs(F, F), _ptrs(F, F, F, F)
table("ssd_gru_seq_fwd_parts", [_P2, 2, _P2, _P2, 2, F, F, F, 7, 4, 16, None], nulls([0, 2, 3, 5]) + zeros([1, 4, 8, 9, 10]) + [
    ("n_parts = limit + 1", {1: 5, 9: 20}, INV), ("n_wparts = limit + 1", {4: 5, 9: 20}, INV), ("G % n_parts", {9: 3, 4: 1}, INV),
    ("G % n_wparts", {9: 3, 1: 1}, INV), ("rzn without ghn", {7: None}, INV), ("B % 16", {10: 20}, INV),
    ("a gi part null", {0: _ptrs(F, None)}, INV), ("a gi part misaligned", {0: _ptrs(F, F + 4)}, INV), ("a wh part null", {2: _ptrs(F, None)}, INV),
    ("a wh part misaligned", {2: _ptrs(F + 4, F)}, INV), ("a bh part null", {3: _ptrs(None, F)}, INV), ("a bh part misaligned", {3: _ptrs(F, F + 12)}, INV),
    ("hs misaligned", {5: F + 4}, INV), ("rzn misaligned", {6: F + 4}, INV), ("ghn misaligned", {7: F + 4}, INV)])
table("ssd_gru_seq_bwd_parts", [_P4, F, F, F, _P2, 2, _P4, 4, F, F, F, 7, 8, 4, 16, None], nulls([0, 1, 2, 3, 4, 6, 8, 9, 10]) + zeros([5, 7, 11, 12, 13, 14]) + [
    ("n_parts = limit + 1", {7: 5, 12: 20}, INV), ("n_wparts = limit + 1", {5: 5, 12: 20}, INV), ("G % n_parts", {12: 6, 13: 6}, INV),
    ("G_grad > G", {13: 10}, INV), ("G_grad not whole parts", {13: 3}, INV), ("B % 16", {14: 40}, INV),
    ("a dhs part with a gradient null", {0: _ptrs(F, None, F, F)}, INV), ("a dhs part misaligned", {0: _ptrs(F + 4, F, F, F)}, INV),
    ("a wh part null", {4: _ptrs(None, F)}, INV), ("a wh part misaligned", {4: _ptrs(F, F + 8)}, INV),
    ("a d_gi part with a gradient null", {6: _ptrs(F, None, F, F)}, INV), ("a d_gi part misaligned", {6: _ptrs(F, F + 4, F, F)}, INV),
    ("hs misaligned", {1: F + 4}, INV), ("rzn misaligned", {2: F + 4}, INV), ("ghn misaligned", {3: F + 4}, INV), ("dgh misaligned", {8: F + 4}, INV)])

# ---- affine layers ----------------------------------------------------------------------------------------------------------------------
_big = [("in * out = 2^30", {6: 1 << 15, 7: 1 << 15}, UNS), ("rows * in = 2^30", {5: 1 << 20, 6: 1 << 10}, UNS)]
table("ssd_bias_bmm_fwd", [F, F, F, F, 5, 100, 64, 9, None], nulls([0, 1, 2, 3]) + zeros([4, 5, 6, 7]) + _big)
table("ssd_bias_bmm_leaky_fwd", [F, F, F, F, 5, 100, 64, 9, None], nulls([0, 1, 2, 3]) + zeros([4, 5, 6, 7]) + _big)
table("ssd_bias_bmm_bwd", [F, F, F, F, F, F, None, 5, 100, 64, 9, None], nulls([0]) + zeros([7, 8, 9, 10]) + [
    ("dx without w", {2: None}, INV), ("dw / db without x", {1: None}, INV), ("db alone without x", {1: None, 3: None, 4: None}, INV),
    ("slope_of without dx", {3: None, 6: F}, INV), ("in * out = 2^30", {9: 1 << 15, 10: 1 << 15}, UNS), ("rows * in = 2^30", {8: 1 << 20, 9: 1 << 10}, UNS),
    ("rows * out = 2^30 (past the row-chunk threshold)", {8: 1 << 20, 9: 1, 10: 1 << 10}, UNS), ("rows = 2^30, one column", {8: 1 << 30, 9: 1, 10: 1}, UNS)])
table("ssd_bias_bmm_leaky_bwd", [F, F, F, F, F, F, F, None, 5, 100, 64, 9, None], nulls([0, 1]) + zeros([8, 9, 10, 11]) + [
    ("dx without w", {3: None}, INV), ("dw / db without x", {2: None}, INV), ("slope_of without dx", {4: None, 7: F}, INV),
    ("in * out = 2^30", {10: 1 << 15, 11: 1 << 15}, UNS), ("rows * out = 2^30", {9: 1 << 20, 11: 1 << 10}, UNS)])
_b2 = [("in1 % 16", {7: 24}, INV), ("x1_div 0", {10: 0}, INV), ("x1_div < 0", {10: -1}, INV), ("rows % x1_div", {6: 101}, INV),
       ("in * out = 2^30", {7: 1 << 15, 9: 1 << 15}, UNS), ("rows * in = 2^30", {6: 5 << 18, 7: 1 << 10}, UNS)]
table("ssd_bias_bmm2_fwd", [F, F, F, F, F, 5, 100, 64, 16, 4, 5, 1, None], nulls([0, 1, 2, 3, 4]) + zeros([5, 6, 7, 8, 9]) + _b2)
table("ssd_bias_bmm2_bwd_w", [F, F, F, F, F, 5, 100, 64, 16, 4, 5, 1, None], nulls([0, 1, 2]) + zeros([5, 6, 7, 8, 9]) + _b2 + [
    ("neither dw nor db", {3: None, 4: None}, INV), ("rows * x1_div > 2^32 (the row / x1_div multiplier is exact below)", {6: 1 << 17, 10: 1 << 16}, UNS)])
table("ssd_bias_bmm_bwd_x", [F, F, F, 5, 100, 64, 4, 80 * 4, None], nulls([0, 1, 2]) + zeros([3, 4, 5, 6]) + [
    ("w_set < in * out", {7: 64 * 4 - 1}, INV), ("rows * in = 2^30", {4: 1 << 20, 5: 1 << 10, 7: 1 << 12}, UNS)])
table("ssd_set_learner_precision", [2], [("precision 0", {0: 0}, INV), ("precision 3", {0: 3}, INV)])

# ---- encoder (learner call form) --------------------------------------------------------------------------------------------------------
table("ssd_conv_wgrad_codes", [F, F, F, 16, 15, None], nulls([0, 1, 2]) + zeros([3]) + [("view_edge %d" % V, {4: V}, UNS) for V in (1, 2, 16, 64, 65)])


def _enc(V=15, **kw):
    bands = abi.encode_bands(V)
    a = abi.SsdPolicyEncodeArgs(codes=F, code_bytes=1 << 20, env_stride=5 * abi.code_agent_stride(V), slot_stride=0, agent_stride=abi.code_agent_stride(V),
                                rows=20, view_edge=V, n_agents=5, agent_major=1, precision=2, conv_frags=F, lin_frags=F, conv_b=F, lin_b=F,
                                out=F if bands == 1 else None, out_stride=32 if bands == 1 else 0, part=None if bands == 1 else F,
                                alphabet=abi.CODE_CLASS, act=F, layout=abi.ENCODE_LAYOUT_TOEPLITZ if V in (15, 31) else abi.ENCODE_LAYOUT_LUT)
    for k, v in kw.items():
        setattr(a, k, v)
    _keep.append(a)
    return C.byref(a)


table("ssd_policy_encode", [_enc(), None], nulls([0]) + [(k + " = " + repr(v), {0: _enc(**{k: v})}, e) for k, v, e in (
    ("codes", None, INV), ("conv_frags", None, INV), ("lin_frags", None, INV), ("conv_b", None, INV), ("lin_b", None, INV), ("rows", 0, INV),
    ("n_agents", 0, INV), ("rows", 21, INV), ("view_edge", 16, UNS), ("view_edge", 65, UNS), ("precision", 3, INV), ("alphabet", 2, INV),
    ("layout", 2, INV), ("layout", abi.ENCODE_LAYOUT_LUT, INV), ("out", None, INV), ("part", F, INV), ("out_stride", 31, INV),
    ("conv_frags", F + 4, INV), ("lin_frags", F + 8, INV), ("agent_stride", 224, INV), ("env_stride", 4 * 240, INV), ("slot_stride", -1, INV),
    ("slot_stride", 64, INV), ("code_bytes", 3 * 5 * 240 + 4 * 240 + 224, INV), ("slot_add", 1, INV), ("slot_t_copy", F, INV))] + [
    ("V = 31 (3 bands): part misaligned", {0: _enc(31, part=F + 4)}, INV), ("V = 31: out given", {0: _enc(31, out=F)}, INV),
    ("V = 31: part null", {0: _enc(31, part=None)}, INV), ("V = 17: Toeplitz layout", {0: _enc(17, layout=abi.ENCODE_LAYOUT_TOEPLITZ)}, UNS)])

LEARNER = sorted({c[0] for c in CASES} | {"ssd_conv_wgrad_partial_rows"})


def test_every_export_is_categorised():
    """abi.HIP_SIGNATURES = the learner exports with a refusal table here + the named others + the exports whose tables a feature's
    host test holds: a new export must be put in exactly one of the three."""
    names = set(abi.HIP_SIGNATURES)
    assert not (set(LEARNER) & NOT_LEARNER) and not (set(ELSEWHERE) & NOT_LEARNER) and not (set(ELSEWHERE) & set(LEARNER))
    other = NOT_LEARNER | set(ELSEWHERE)
    assert names - other == set(LEARNER), sorted(names - other - set(LEARNER)) + sorted(set(LEARNER) - names)
    assert other <= names, sorted(other - names)
    for name, module in ELSEWHERE.items():
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), module + ".py")
        assert os.path.isfile(path), (name, module)
        assert '"%s"' % name in open(path).read(), (name, module)


@pytest.mark.parametrize("case", CASES, ids=["%s-%s" % (c[0], c[1].replace(" ", "_")) for c in CASES])
def test_invalid_call_is_refused_with_a_message(case):
    name, label, call, expect = case
    lib = abi.load_library()
    rc = call(lib)
    assert rc == expect, (name, label, rc, lib.ssd_last_error())
    assert lib.ssd_last_error(), (name, label)
    with pytest.raises(abi.SsdError):
        abi.check(lib, rc)


def test_conv_wgrad_partial_rows_is_a_pure_size_function():
    """no status: 0 rows for a count below 1, else whole workgroups of 4 waves x 4 windows"""
    lib = abi.load_library()
    assert [lib.ssd_conv_wgrad_partial_rows(r) for r in (-1, 0, 1, 4, 5, 16, 17, 203)] == [0, 0, 4, 4, 4, 4, 8, 52]
