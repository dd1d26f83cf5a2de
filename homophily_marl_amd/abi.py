"""ctypes mirror of include/ssd_hip.h and the loader of the in-tree HIP library.

The native library is REQUIRED: there is no CPU fallback on the product path.  `load_library()` raises if
`libssd_hip.so` is missing or does not export every symbol the header declares.

Top to bottom: constants, struct classes, the export table, the size / layout helpers, the loader.  A new export is one line of
HIP_SIGNATURES under its header section; a new struct is a class named after its typedef (ssd_td_loss_args -> SsdTdLossArgs).
tests/test_abi_symbols.py holds the table to the header's declarations and every struct to the header's layout.
"""
import ctypes as C
import os

# ---- constants ---------------------------------------------------------------------------------------------------------------
ABI_VERSION = 10
MAX_AGENTS = 10
MAX_CELLS = 1024
MAX_SITES = 256

ENV_CLEANUP, ENV_HARVEST = 0, 1
RNG_TAPE, RNG_COUNTER = 0, 1
OBS_F32, OBS_BF16, OBS_U8, OBS_CODE = 0, 1, 2, 3
COLOR_SIMPLIFIED, COLOR_FULL = 0, 1
CODE_CLASS, CODE_CHANNEL_MASK = 0, 1
# ssd_policy_head.input_flags (include/ssd_hip.h, SSD_INPUT_*): the _build_inputs blocks in the reference's order
INPUT_LAST_ACTION, INPUT_AGENT_ID, INPUT_REWARD, INPUT_INC_REWARD, INPUT_DISTANCE, INPUT_AGENT_POS = 1, 2, 4, 8, 16, 32
INPUT_OTHERS_LAST_ACTION = 64     # ssd_build_inputs_flags builds the columns; the fused heads gather fc1's rows (ssd_policy_head.others_rows)
INPUT_GATHER_ONEHOT = 0x100       # a layout, not a block: the fused heads gather fc1's rows for EVERY one-hot block (ssd_policy_head.onehot_rows)
PREV_RECORD_BYTES = 16            # ssd_policy_head.prev_record: one byte per agent, 16 bytes per env
INPUT_EXPLICIT = 0x80000000   # marks a given flag word: the empty set is INPUT_EXPLICIT alone, 0 means the shipped set
STREAM_UNIFORM, STREAM_MOVE, STREAM_WASTE, STREAM_SPAWN_ROT = 0, 1, 2, 3

SSD_OK, SSD_ERR_INVALID, SSD_ERR_DEVICE, SSD_ERR_NOMEM, SSD_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
ERRBIT_F16_RANGE = 32
ERR_BAD_RENDER = 64

COPY_BLOCKS_MAX = 32
FILL_BLOCKS_MAX = 16
ADAM_MAX_JOBS = 64
POLYAK_MAX_JOBS, POLYAK_WORKGROUPS = 128, 256
SAMPLE_IDS_MAX = 1024
COLSUM_CHUNK = 64
TD_LOSS_PARTIALS = 16
POLICY_HEAD_FRAGS, POLICY_HEAD_TAIL_FLOATS = 58, 464 + 64
POLICY_TAIL_PIECES = 3

ENCODE_EDGE_MIN, ENCODE_EDGE_MAX, ENCODE_BANDS_MAX = 3, 63, 6
ENCODE_LAYOUT_TOEPLITZ, ENCODE_LAYOUT_LUT = 0, 1
ENCODE_LUT_TABLE_BYTES = 3 * 64 * 6 * 4

BEHAVIOUR_MAX_GROUPS = 256
BEHAVIOUR_WAVES = 16         # envs a workgroup of k_behaviour_partials walks at a time (a wave each)
BEHAVIOUR_ROLES = ("idle", "cleaner", "harvester", "mixed")

PRIORITY_ONE = 65536
PRIORITY_MAX = 1 << 24
PRIORITY_POP_MAX = 1 << 20
PRIORITY_SEGMENTS_MAX = 256       # windows per episode of a per-window priority table (per_unit "window")


# ---- struct classes (include/ssd_hip.h, in its order) ------------------------------------------------------------------------
class SsdConfig(C.Structure):
    _fields_ = [
        ("env_kind", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("ascii_map", C.c_char_p),
        ("n_agents", C.c_int32), ("n_env", C.c_int32), ("view_size", C.c_int32), ("episode_limit", C.c_int32),
        ("random_spawn_point", C.c_int32), ("spawn_rotation", C.c_int32), ("obs_color", C.c_int32),
        ("rng_mode", C.c_int32), ("device", C.c_int32), ("env_id_base", C.c_uint32), ("seed", C.c_uint64),
        ("threshold_depletion", C.c_double), ("threshold_restoration", C.c_double),
        ("waste_spawn_prob", C.c_double), ("apple_respawn_prob", C.c_double),
        ("harvest_spawn_prob", C.c_double * 4),
    ]


class SsdTape(C.Structure):
    _fields_ = [
        ("move_order", C.c_void_p), ("uniforms", C.c_void_p), ("uniforms_stride", C.c_int32),
        ("waste_order", C.c_void_p), ("spawn_rot", C.c_void_p), ("spawn_order", C.c_void_p),
    ]


class SsdStepOut(C.Structure):
    _fields_ = [
        ("reward", C.c_void_p), ("clean_num", C.c_void_p), ("apple_den", C.c_void_p), ("terminated", C.c_void_p),
        ("collective_return", C.c_void_p), ("equality", C.c_void_p), ("n_draws", C.c_void_p),
    ]


class SsdObsOut(C.Structure):
    _fields_ = [
        ("obs", C.c_void_p), ("obs_format", C.c_int32), ("state", C.c_void_p), ("pos", C.c_void_p),
        ("orient", C.c_void_p), ("obs_env_stride", C.c_int64), ("obs_slot_stride", C.c_int64),
        ("obs_t_slots", C.c_int32), ("obs_code", C.c_void_p),
    ]


class SsdState(C.Structure):
    _fields_ = [
        ("grid", C.c_void_p), ("pos", C.c_void_p), ("orient", C.c_void_p), ("ep_reward", C.c_void_p),
        ("ep_step", C.c_void_p), ("epoch", C.c_void_p),
    ]


class SsdInfo(C.Structure):
    _fields_ = [
        ("n_actions", C.c_int32), ("n_apple_sites", C.c_int32), ("n_waste_sites", C.c_int32),
        ("n_spawn_points", C.c_int32), ("max_uniforms", C.c_int32), ("obs_edge", C.c_int32),
    ]


class SsdRowGather(C.Structure):
    """one field of ssd_gather_rows"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64)]


class SsdBlockCopy(C.Structure):
    """one strided 2-D f32 block copy of ssd_copy_blocks"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("src_stride", C.c_int32),
                ("dst_stride", C.c_int32)]


class SsdBlockFill(C.Structure):
    """one 32-bit pattern fill of ssd_fill_blocks"""
    _fields_ = [("dst", C.c_void_p), ("bytes", C.c_int64), ("value", C.c_uint32), ("reserved", C.c_uint32)]


class SsdBehaviourArgs(C.Structure):
    _fields_ = [("n_env", C.c_int32), ("t_slots", C.c_int32), ("n_agents", C.c_int32), ("n_actions", C.c_int32),
                ("actions", C.c_void_p), ("actions_inc", C.c_void_p), ("reward", C.c_void_p), ("clean_num", C.c_void_p),
                ("workspace", C.c_void_p), ("acc", C.c_void_p)]


class SsdWindowField(C.Structure):
    """one field of ssd_gather_windows"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("slot_bytes", C.c_int64), ("filled", C.c_int32), ("reserved", C.c_int32)]


class SsdPrioritySampleArgs(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("call", C.c_uint32), ("population", C.c_int32), ("count", C.c_int32), ("n_starts", C.c_int32),
                ("beta", C.c_float), ("table", C.c_void_p), ("ids", C.c_void_p), ("t0", C.c_void_p), ("weights", C.c_void_p), ("log", C.c_void_p),
                ("n_segments", C.c_int32), ("seg_stride", C.c_int32), ("last_start", C.c_int32), ("entries", C.c_void_p)]


class SsdPriorityUpdateArgs(C.Structure):
    _fields_ = [("batch", C.c_int32), ("t_slots", C.c_int32), ("n_agents", C.c_int32), ("n_actions", C.c_int32), ("table_len", C.c_int32),
                ("alpha", C.c_float), ("eta", C.c_float), ("eps", C.c_float),
                ("partials", C.c_void_p), ("ids", C.c_void_p), ("weights", C.c_void_p), ("dq_env", C.c_void_p), ("dq_inc", C.c_void_p),
                ("q_new", C.c_void_p), ("table", C.c_void_p)]


class SsdRolloutPriorityArgs(C.Structure):
    _fields_ = [("t_index", C.c_void_p), ("n_env", C.c_int32), ("n_agents", C.c_int32), ("n_actions", C.c_int32), ("t_slots", C.c_int32),
                ("avail_bits", C.c_uint32), ("reserved", C.c_int32), ("q_env", C.c_void_p), ("q_inc", C.c_void_p),
                ("q_env_agent_stride", C.c_int64), ("q_env_env_stride", C.c_int64), ("q_inc_agent_stride", C.c_int64), ("q_inc_env_stride", C.c_int64),
                ("actions", C.c_void_p), ("actions_inc", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p), ("filled", C.c_void_p),
                ("gamma_env", C.c_float), ("gamma_inc", C.c_float), ("reward_scale", C.c_float), ("incentive_ratio", C.c_float),
                ("incentive_cost", C.c_float), ("incentive", C.c_float), ("seq_len", C.c_float), ("alpha", C.c_float), ("eta", C.c_float),
                ("eps", C.c_float), ("carry", C.c_void_p), ("acc", C.c_void_p), ("q_init", C.c_void_p),
                ("n_segments", C.c_int32), ("win_len", C.c_int32), ("seg_stride", C.c_int32), ("burn_in", C.c_int32)]


class SsdAdamJob(C.Structure):
    """one parameter tensor of ssd_clip_adam_step"""
    _fields_ = [("param", C.c_void_p), ("offset", C.c_int64), ("numel", C.c_int32), ("segment", C.c_int32),
                ("exp_avg", C.c_void_p * 2), ("exp_avg_sq", C.c_void_p * 2), ("step", C.c_void_p * 2)]


class SsdPolyakJob(C.Structure):
    """one 2-D block of the Polyak target update of ssd_clip_adam_step (a target parameter, or a parameter's slice of a concatenated copy)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("dst_row_stride", C.c_int64)]


class SsdClipAdamArgs(C.Structure):
    _fields_ = [("flat_grad", C.c_void_p), ("total", C.c_int64), ("jobs", C.c_void_p),
                ("n_jobs", C.c_int32), ("partials", C.c_void_p), ("lr_inc", C.c_float), ("lr_env", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("clip", C.c_float),
                ("polyak_jobs", C.c_void_p), ("n_polyak", C.c_int32), ("target_tau", C.c_float), ("polyak_partials", C.c_void_p)]


def polyak_job_table(blocks):
    """(SsdPolyakJob * len(blocks)) of (src, dst, rows, cols, dst_row_stride) tuples (addresses, elements).  What the entry point cannot
    check of a table in device memory is checked here: the count, non-null 4-byte aligned addresses, rows, cols >= 1, rows * cols < 2^31,
    dst_row_stride >= cols."""
    if not 1 <= len(blocks) <= POLYAK_MAX_JOBS:
        raise ValueError("a Polyak job table holds 1 .. %d jobs, got %d" % (POLYAK_MAX_JOBS, len(blocks)))
    jobs = (SsdPolyakJob * len(blocks))()
    for j, (src, dst, rows, cols, stride) in zip(jobs, blocks):
        if not src or not dst or src % 4 or dst % 4 or rows < 1 or cols < 1 or rows * cols >= 2 ** 31 or stride < cols:
            raise ValueError("Polyak job (src 0x%x, dst 0x%x, rows %d, cols %d, dst_row_stride %d): addresses must be non-null and 4-byte aligned, "
                             "rows, cols >= 1, rows * cols < 2^31, dst_row_stride >= cols" % (src or 0, dst or 0, rows, cols, stride))
        j.src, j.dst, j.rows, j.cols, j.dst_row_stride = src, dst, rows, cols, stride
    return jobs


def tie_job_table(triples):
    """(c_int64 * (3 n)) of n (first, copies, inner) triples: the job table of include/ssd_hip_tie.h as the entry points read it on
    the host (first: an element offset into the flat gradient buffer for ssd_tie_agent_grads, an address for ssd_agent_spread).  The
    device copy is the caller's: th.tensor(list(table), dtype=th.int64, device=...)."""
    flat = [int(v) for t in triples for v in t]
    if len(flat) != 3 * len(triples):
        raise ValueError("a tie job is a (first, copies, inner) triple")
    return (C.c_int64 * len(flat))(*flat)


class SsdTdLossArgs(C.Structure):
    _fields_ = [("batch", C.c_int32), ("t_slots", C.c_int32), ("n_agents", C.c_int32), ("n_actions", C.c_int32), ("sim_horizon", C.c_int32),
                ("double_q", C.c_int32),
                ("gamma_env", C.c_float), ("gamma_inc", C.c_float), ("reward_scale", C.c_float), ("incentive_ratio", C.c_float),
                ("incentive_cost", C.c_float), ("incentive", C.c_float), ("seq_len", C.c_float), ("sim_threshold", C.c_float),
                ("sim_loss_weight", C.c_float), ("td_lambda", C.c_float),
                ("q_env", C.c_void_p), ("q_inc", C.c_void_p), ("tq_env", C.c_void_p), ("tq_inc", C.c_void_p),
                ("actions", C.c_void_p), ("actions_inc", C.c_void_p), ("avail", C.c_void_p), ("reward", C.c_void_p), ("clean_num", C.c_void_p),
                ("terminated", C.c_void_p), ("filled", C.c_void_p), ("dens", C.c_void_p),
                ("dq_env", C.c_void_p), ("dq_inc", C.c_void_p), ("partials", C.c_void_p), ("consider_others_inc", C.c_int32)]


class SsdStoreStep(C.Structure):
    _fields_ = [("t_index", C.c_void_p), ("n_env", C.c_int32), ("n_agents", C.c_int32), ("n_actions", C.c_int32), ("t_slots", C.c_int32),
                ("pos", C.c_void_p), ("orient", C.c_void_p), ("reward", C.c_void_p), ("clean_num", C.c_void_p), ("apple_den", C.c_void_p),
                ("terminated", C.c_void_p), ("actions", C.c_void_p), ("actions_inc", C.c_void_p),
                ("dst_pos", C.c_void_p), ("dst_orient", C.c_void_p), ("dst_reward", C.c_void_p), ("dst_clean_num", C.c_void_p),
                ("dst_apple_den", C.c_void_p), ("dst_actions_onehot", C.c_void_p), ("dst_terminated", C.c_void_p),
                ("dst_actions", C.c_void_p), ("dst_actions_inc", C.c_void_p),
                ("prev_actions", C.c_void_p), ("prev_reward", C.c_void_p), ("prev_actions_inc", C.c_void_p), ("ep_return", C.c_void_p),
                ("next_t_out", C.c_void_p), ("counter_inc", C.c_void_p)]


class SsdStoreHiddenArgs(C.Structure):
    _fields_ = [("t_index", C.c_void_p), ("n_env", C.c_int32), ("n_agents", C.c_int32), ("t_slots", C.c_int32), ("reserved", C.c_int32),
                ("h_env", C.c_void_p), ("h_inc", C.c_void_p), ("src_agent_stride", C.c_int64), ("src_env_stride", C.c_int64), ("dst", C.c_void_p)]


class SsdPolicyHead(C.Structure):
    """fused controller step, one launch per head"""
    _fields_ = [("n_env", C.c_int32), ("n_agents", C.c_int32), ("n_actions", C.c_int32), ("input_shape", C.c_int32),
                ("pos_scale", C.c_float), ("seed", C.c_uint32),
                ("inputs", C.c_void_p), ("h", C.c_void_p), ("weights", C.c_void_p), ("avail", C.c_void_p), ("epsilon", C.c_void_p),
                ("step", C.c_void_p), ("prev_actions", C.c_void_p), ("prev_reward", C.c_void_p), ("prev_actions_inc", C.c_void_p),
                ("pos", C.c_void_p), ("actions", C.c_void_p), ("pos_pre", C.c_void_p), ("orient_pre", C.c_void_p),
                ("reward", C.c_void_p), ("clean_num", C.c_void_p), ("apple_den", C.c_void_p), ("out_actions", C.c_void_p),
                ("q_out", C.c_void_p), ("orient", C.c_void_p), ("out_actions_i32", C.c_void_p), ("pos_copy", C.c_void_p),
                ("orient_copy", C.c_void_p),
                ("t_index", C.c_void_p), ("t_slots", C.c_int32),
                ("dst_pos", C.c_void_p), ("dst_orient", C.c_void_p), ("dst_actions_onehot", C.c_void_p), ("dst_reward", C.c_void_p),
                ("dst_clean_num", C.c_void_p), ("dst_apple_den", C.c_void_p), ("dst_terminated", C.c_void_p), ("terminated", C.c_void_p),
                ("dst_actions", C.c_void_p), ("dst_actions_inc", C.c_void_p), ("prev_actions_out", C.c_void_p),
                ("prev_actions_inc_out", C.c_void_p), ("prev_reward_out", C.c_void_p), ("ep_return", C.c_void_p), ("next_t_out", C.c_void_p),
                ("precision", C.c_int32), ("env_id_base", C.c_uint32), ("feat_part", C.c_void_p), ("feat_bands", C.c_int32),
                ("lin_b", C.c_void_p), ("input_flags", C.c_uint32),
                ("next_step_out", C.c_void_p), ("t_copy_out", C.c_void_p), ("step_copy_out", C.c_void_p),
                ("recv_inc", C.c_void_p), ("recv_inc_out", C.c_void_p), ("avail_bits", C.c_uint32),
                ("others_rows", C.c_void_p), ("prev_record", C.c_void_p), ("prev_record_out", C.c_void_p), ("onehot_rows", C.c_void_p),
                ("pipeline_gather", C.c_int32), ("epsilon_rows", C.c_void_p)]


class SsdPolicyHeadParams(C.Structure):
    """the reference-shaped f32 parameters of one head"""
    _fields_ = [("fc1_w", C.c_void_p), ("fc1_b", C.c_void_p), ("w_i", C.c_void_p * 3), ("w_h", C.c_void_p * 3), ("b_i", C.c_void_p * 3),
                ("b_h", C.c_void_p * 3), ("fc2_w", C.c_void_p), ("fc2_b", C.c_void_p), ("fc2_v_w", C.c_void_p), ("fc2_v_b", C.c_void_p),
                ("n_agents", C.c_int32), ("fc1_in", C.c_int32), ("fc2_in", C.c_int32), ("fc2_out", C.c_int32),
                ("input_flags", C.c_uint32), ("n_actions", C.c_int32), ("others_rows", C.c_void_p), ("onehot_rows", C.c_void_p)]


class SsdPolicyEncodeArgs(C.Structure):
    _fields_ = [("codes", C.c_void_p), ("code_bytes", C.c_int64), ("env_stride", C.c_int64), ("slot_stride", C.c_int64),
                ("agent_stride", C.c_int64), ("slot_t", C.c_void_p),
                ("rows", C.c_int32), ("view_edge", C.c_int32), ("n_agents", C.c_int32), ("agent_major", C.c_int32), ("precision", C.c_int32),
                ("conv_frags", C.c_void_p), ("lin_frags", C.c_void_p), ("conv_b", C.c_void_p), ("lin_b", C.c_void_p),
                ("out", C.c_void_p), ("out_stride", C.c_int32), ("part", C.c_void_p), ("slot_t_copy", C.c_void_p), ("counter_inc", C.c_void_p),
                ("alphabet", C.c_int32), ("act", C.c_void_p), ("slot_add", C.c_int32), ("layout", C.c_int32)]


# ---- the export table: name -> (restype, argtypes) ---------------------------------------------------------------------------
# the exports that the CPU checker (prefix ssd_cpu_, no stream argument) shares with the library
def _sigs(prefix, with_stream):
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    st = [vp] if with_stream else []
    P = C.POINTER
    return {
        prefix + "abi_version": (C.c_int, []),
        prefix + "last_error": (C.c_char_p, []),
        prefix + "create": (C.c_int, [P(SsdConfig), P(vp)]),
        prefix + "destroy": (C.c_int, [vp]),
        prefix + "reset": (C.c_int, [vp, vp, P(SsdTape), P(SsdStepOut)] + st),
        prefix + "step": (C.c_int, [vp, vp, P(SsdTape), P(SsdStepOut)] + st),
        prefix + "observe": (C.c_int, [vp, P(SsdObsOut)] + st),
        prefix + "export_state": (C.c_int, [vp, P(SsdState)] + st),
        prefix + "import_state": (C.c_int, [vp, P(SsdState)] + st),
        prefix + "get_info": (C.c_int, [vp, P(SsdInfo)]),
        prefix + "build_inputs": (C.c_int, [i32, i32, i32, i32, vp, vp, vp, vp, f32, vp, i32, i32] + st),
        prefix + "incentive_transfer": (C.c_int, [i32, i32, i32, vp, vp, f32, f32, f32, f32,
                                                  vp, vp, vp, vp, vp, vp] + st),
    }


CPU_SIGNATURES = _sigs("ssd_cpu_", False)

vp, i32, i64, u32, u64, f32, P = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.POINTER
# every export of libssd_hip.so, grouped like include/ssd_hip.h; every one returns int
HIP_SIGNATURES = {name: (C.c_int, args) for name, args in {
    # environment: fused step, error word, render mode (device-only: no CPU counterpart)
    "ssd_step_observe": [vp, vp, P(SsdTape), P(SsdStepOut), P(SsdObsOut), vp],
    "ssd_poll_error": [vp, P(i32)],
    "ssd_set_render": [vp, i32],
    "ssd_render": [vp, vp, i32, vp, vp, i64, vp],
    # learner pieces outside the GEMMs, replay gathers, fills and rollout statistics
    "ssd_unroll_other": [vp] * 6 + [f32] + [i32] * 4 + [vp] * 3,
    "ssd_column_sums": [vp, vp, i32, i32, i32, vp, vp],
    "ssd_dueling_q_fwd": [vp] * 3 + [i32] * 5 + [vp],
    "ssd_dueling_q_bwd": [vp] * 3 + [i32] * 5 + [vp],
    "ssd_gather_rows": [vp, i32, vp, i32, vp],
    "ssd_sample_ids": [u64, u32, i32, i32, vp, vp],
    "ssd_copy_blocks": [vp, i32, vp],
    "ssd_fill_blocks": [vp, i32, vp],
    "ssd_runner_stats": [vp, vp, vp, i32, i32, vp, vp],
    "ssd_behaviour_stats": [P(SsdBehaviourArgs), vp],
    # sampled time windows
    "ssd_sample_windows": [u64, u32, i32, i32, i32, vp, vp, vp],
    "ssd_gather_windows": [vp, i32, vp, vp, i32, i32, i32, i32, vp],
    # prioritised replay
    "ssd_priority_sample": [P(SsdPrioritySampleArgs), vp],
    "ssd_priority_update": [P(SsdPriorityUpdateArgs), vp],
    "ssd_rollout_priority": [P(SsdRolloutPriorityArgs), vp],
    # optimiser tail and fused loss
    "ssd_clip_adam_step": [P(SsdClipAdamArgs), vp],
    "ssd_td_sim_loss": [P(SsdTdLossArgs), i32, vp],
    # rollout-time controller pieces that are not GEMMs
    "ssd_encoder": [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, i64, vp, vp],
    "ssd_conv_leaky": [vp, i32, i32, i32, vp, vp, vp, i32, i32, vp, i64, vp, vp],
    "ssd_store_step_launch": [P(SsdStoreStep), vp],
    "ssd_store_hidden": [P(SsdStoreHiddenArgs), vp],
    "ssd_gru_gates": [vp, vp, vp, i32, i32, vp],
    "ssd_gru_gates_fwd": [vp] * 5 + [i32, i32, vp],
    "ssd_gru_gates_bwd": [vp] * 7 + [i32, i32, vp],
    "ssd_dueling_pick": [vp, i32, i32, vp, vp, vp, u32, i32, i32, i32, vp, vp, u32, vp],
    # the learner's recurrence over all T timesteps
    "ssd_gru_seq_fwd": [vp] * 6 + [i32] * 3 + [vp],
    "ssd_gru_seq_bwd": [vp] * 9 + [i32] * 3 + [vp],
    "ssd_gru_seq_fwd_parts": [vp, i32, vp, vp, i32] + [vp] * 3 + [i32] * 3 + [vp],
    "ssd_gru_seq_bwd_parts": [vp] * 5 + [i32, vp, i32] + [vp] * 3 + [i32] * 4 + [vp],
    "ssd_gru_seq_fwd_h0": [vp, i32, vp, vp, i32, vp, i64, i64] + [vp] * 3 + [i32] * 3 + [vp],
    "ssd_gru_seq_bwd_h0": [vp] * 5 + [i32, vp, i32] + [vp] * 3 + [i32] * 4 + [vp],
    # the learner's per-agent affine layers and dueling heads
    "ssd_bias_bmm_fwd": [vp] * 4 + [i32] * 4 + [vp],
    "ssd_bias_bmm_leaky_fwd": [vp] * 4 + [i32] * 4 + [vp],
    "ssd_bias_bmm_leaky_bwd": [vp] * 8 + [i32] * 4 + [vp],
    "ssd_bias_bmm_bwd": [vp] * 7 + [i32] * 4 + [vp],
    "ssd_bias_bmm2_fwd": [vp] * 5 + [i32] * 7 + [vp],
    "ssd_bias_bmm2_bwd_w": [vp] * 5 + [i32] * 7 + [vp],
    "ssd_bias_bmm_bwd_x": [vp] * 3 + [i32] * 4 + [i64, vp],
    "ssd_dueling_head_fwd": [vp] * 2 + [i32] * 5 + [vp],
    "ssd_dueling_head_bwd": [vp] * 3 + [i32] * 5 + [vp],
    "ssd_bmm_reserve_scratch": [vp],
    "ssd_set_learner_precision": [i32],
    "ssd_learner_precision": [],
    "ssd_conv_wgrad_partial_rows": [i32],
    "ssd_conv_wgrad_codes": [vp, vp, vp, i32, i32, vp],
    # fused rollout-time controller step
    "ssd_build_inputs_width": [i32, i32, u32],
    "ssd_build_inputs_flags": [i32, i32, i32, i32, u32, vp, vp, vp, vp, f32, vp, i32, i32, vp],
    "ssd_policy_head_env": [P(SsdPolicyHead), vp],
    "ssd_policy_head_inc": [P(SsdPolicyHead), vp],
    "ssd_policy_head_plan": [i32] * 3 + [P(i32)] * 3,
    "ssd_policy_pack_head": [P(SsdPolicyHeadParams), i32, vp, vp],
    "ssd_policy_encode": [P(SsdPolicyEncodeArgs), vp],
    "ssd_policy_head_inc_encode": [P(SsdPolicyHead), P(SsdPolicyEncodeArgs), vp],
    "ssd_policy_pack_encoder_lut": [vp, vp, vp, i32, i32, vp, vp, vp],
    "ssd_policy_pack_encoder": [vp, vp, vp, i32, i32, vp, vp, vp],
    "ssd_numeric_status": [P(i32)],
}.items()}
# library, lifecycle, step / observe, state, inputs and incentives: shared with the CPU checker
HIP_SIGNATURES.update(_sigs("ssd_", True))
# the exports of include/ssd_hip_train.h (the train step's shared launches of the live and the target net, fc1's row assembly); every
# one returns int.  tests/test_train_pairs_host.py holds this table to that header and every entry to a refusal table.
TRAIN_SIGNATURES = {name: (C.c_int, args) for name, args in {
    "ssd_bias_bmm_pair_fwd": [vp] * 5 + [i32] + [vp] * 5 + [i32] * 8 + [vp],
    "ssd_dueling_head_pair_fwd": [vp, vp, i32, vp, vp, i32] + [i32] * 4 + [vp],
    "ssd_fc1_rows_fwd": [vp] * 8 + [i32] * 6 + [vp],
    "ssd_fc1_rows_bwd": [vp] * 3 + [i32] * 7 + [vp],
}.items()}
# the export of include/ssd_hip_reward.h (the reward model over a finished rollout); returns int.  tests/test_social_reward_host.py
# holds this table to that header and the entry to a refusal table.
REWARD_IA, REWARD_PROSOCIAL = 1, 2
REWARD_SIGNATURES = {name: (C.c_int, args) for name, args in {
    "ssd_social_reward": [i32] + [vp] * 3 + [i32] * 7 + [f32] * 3 + [vp],
}.items()}
# the exports of include/ssd_hip_tie.h (heads shared across agents: config key share_heads); return int.  Job tables are plain int64
# triples (tie_job_table), given as a host and a device copy.  tests/test_share_heads_host.py holds this table to that header and both
# entries to a refusal table.
TIE_SIGNATURES = {name: (C.c_int, args) for name, args in {
    "ssd_tie_agent_grads": [vp, i64, vp, vp, i32, vp],
    "ssd_agent_spread": [vp, vp, i32, vp, vp],
}.items()}
# the export of include/ssd_hip_mix.h (the VDN mixer of the env head: config key mixer); returns int.  It takes the SsdTdLossArgs that
# ssd_td_sim_loss has just been handed.  tests/test_team_mixer_host.py holds this table to that header and the entry to a refusal table.
MIX_SIGNATURES = {name: (C.c_int, args) for name, args in {
    "ssd_team_td": [vp, vp],
}.items()}


# ---- size / layout helpers ---------------------------------------------------------------------------------------------------
def onehot_rows(n_agents, n_actions, flags):
    """include/ssd_hip.h SSD_ONEHOT_ROWS: rows per owner of the INPUT_GATHER_ONEHOT table (id row | last action | inc action | others)."""
    return 1 + 2 * n_actions + (n_agents * n_actions if flags & INPUT_OTHERS_LAST_ACTION else 0)


def policy_image_bytes(precision):
    """SSD_POLICY_IMAGE_BYTES: 14 K-steps of 4 * precision pieces + the resident chunk (fc2, tail, padding), 1 KiB pieces."""
    return (56 * precision + 8) * 1024


def policy_tail_piece(precision):
    """first 1 KiB piece of the f32 tail (biases, pair part of fc2) inside a head image"""
    return 56 * precision + 2 * precision


def policy_frag_piece(precision, F, term):
    """1 KiB piece of fragment F (the numbering of csrc: 2 ot + s fc1; 8 + 2 ot + s GRU input side, 12 tiles; 32 + 2 ot + s hidden
    side; 56 + s fc2) and split term `term` inside a head image (include/ssd_hip.h: consumption order)."""
    if F < 8:
        c, ot = F & 1, F >> 1
    elif F < 56:
        G = (F - 8) % 24
        c, ot = (8 if F >= 32 else 2) + 2 * (G >> 3) + (G & 1), (G & 7) >> 1
    else:
        return 56 * precision + 2 * term + (F - 56)
    return 4 * precision * c + 4 * term + ot


def policy_head_plan(n_env, n_agents, fused_with_encoder=False):
    """(workgroups per agent, compute waves per workgroup, tiles the busiest wave walks) of a head launch on the current device
    (ssd_policy_head_plan); tiles > 1 = the looped kernel instantiations.  fused_with_encoder: 0 / False = the standalone dense heads,
    1 / True = the inc head inside the fused launch, 2 = the standalone gathered heads (others' last action / one-hot gather)."""
    lib = load_library()
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(lib, lib.ssd_policy_head_plan(n_env, n_agents, int(fused_with_encoder), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def encode_edge_supported(V):
    """Whether the class-LUT encoder (ssd_policy_encode, ssd_policy_pack_encoder_lut, ssd_conv_wgrad_codes) takes window edge V:
    every odd edge 3 .. 63 (view_size 1 .. 31)."""
    return ENCODE_EDGE_MIN <= V <= ENCODE_EDGE_MAX and V % 2 == 1


def encode_band_rows(V):
    """SSD_ENCODE_BAND_ROWS: output rows per band (O = V - 2 rows; one band up to O = 13, else ceil(O / 10) bands, at most 6)"""
    O = V - 2
    nb = 1 if O <= 13 else min(ENCODE_BANDS_MAX, (O + 9) // 10)
    return (O + nb - 1) // nb


def encode_bands(V):
    """SSD_ENCODE_BANDS: bands the encoder cuts the output rows into (each writes a partial Linear sum when > 1)"""
    return (V - 2 + encode_band_rows(V) - 1) // encode_band_rows(V)


def encode_lut_ksteps(V):
    """SSD_ENCODE_LUT_KSTEPS: K-steps of the Linear image in the class-LUT layout (4 output positions each, numbered through the bands)"""
    O, R, nb = V - 2, encode_band_rows(V), encode_bands(V)
    return (nb - 1) * ((R * O + 3) // 4) + ((O - (nb - 1) * R) * O + 3) // 4


def encode_frag_bytes(V, precision, layout=ENCODE_LAYOUT_TOEPLITZ):
    """(conv image, Linear image) sizes in bytes (include/ssd_hip.h SSD_ENCODE_*): Toeplitz fragments, or the class-LUT table + the
    position-major Linear image."""
    if layout == ENCODE_LAYOUT_LUT:
        return ENCODE_LUT_TABLE_BYTES, encode_lut_ksteps(V) * 2 * precision * 1024
    units = 29 * 2 * 3 if V == 31 else 13 * 3
    return precision * 9 * 1024, units * 2 * precision * 1024


def code_agent_stride(V):
    return (V * V + 15) & ~15


def behaviour_len(n, A):
    """SSD_BEHAVIOUR_LEN"""
    return 12 * n + n * A + 3 * n * n + 3


def behaviour_layout(n, A):
    """name -> (offset, shape) of the blocks of ssd_behaviour_stats' accumulator (include/ssd_hip.h), in order."""
    blocks = (("reward_sum", (n,)), ("clean_sum", (n,)), ("clean_steps", (n,)), ("harvest_steps", (n,)), ("harvest_time", (n,)),
              ("action_count", (n, A)), ("inc_count", (n, n, 3)), ("recv_on_clean", (n,)), ("recv_on_reward", (n,)), ("role_count", (n, 4)),
              ("cleaners_hist", (n + 1,)), ("n_episodes", (1,)), ("n_steps", (1,)))
    out, off = {}, 0
    for name, shape in blocks:
        out[name] = (off, shape)
        size = 1
        for s in shape:
            size *= s
        off += size
    assert off == behaviour_len(n, A)
    return out


def behaviour_blocks(vec, n, A):
    """the accumulator (any 1-D sequence of behaviour_len(n, A) numbers) as name -> f64 array of the block's shape"""
    import numpy as np
    vec = np.asarray(vec, dtype=np.float64).reshape(-1)
    assert vec.size == behaviour_len(n, A), (vec.size, n, A)
    return {k: vec[o:o + int(np.prod(s))].reshape(s).copy() for k, (o, s) in behaviour_layout(n, A).items()}


def behaviour_summary(vec, n, A):
    """The logged scalars of a behaviour accumulator (one pure function: the runner's _log, run.py and the tools share it).
    rollout_* are the learner's four log values (homophily_learner.py:234-238) over EVERY step of the rollouts instead of the 16
    sampled episodes, on the raw rewards (reward_scale is not applied)."""
    b = behaviour_blocks(vec, n, A)
    n_ep, n_steps = max(1.0, float(b["n_episodes"][0])), max(1.0, float(b["n_steps"][0]))
    inc, roles = b["inc_count"], b["role_count"].sum(axis=0)
    pairs = max(1, n * (n - 1)) * n_steps
    clean = b["clean_sum"]
    out = {"cleaners_per_env_mean": float((b["cleaners_hist"] * range(n + 1)).sum() / n_ep)}
    for k, name in enumerate(BEHAVIOUR_ROLES):
        out["role_%s_frac" % name] = float(roles[k] / (n * n_ep))
    out["inc_pos_rate"] = float(inc[..., 1].sum() / pairs)
    out["inc_neg_rate"] = float(inc[..., 2].sum() / pairs)
    out["rollout_incentives_to_cleanup_per"] = float(b["recv_on_clean"].sum() / (b["clean_steps"].sum() + 1e-6))
    out["rollout_incentives_to_harvest_per"] = float(b["recv_on_reward"].sum() / (b["reward_sum"].sum() + 1e-6))
    out["rollout_value_give_mean"] = float((inc[..., 1].sum() + inc[..., 2].sum()) / (n * n_steps))
    out["rollout_value_receive_mean"] = float((inc[..., 1].sum() - inc[..., 2].sum()) / (n * n_steps))
    out["harvest_time_mean"] = float(b["harvest_time"].sum() / max(1.0, b["harvest_steps"].sum()))
    out["clean_share_max"] = float(clean.max() / clean.sum()) if clean.sum() > 0 else 0.0
    return out


# ---- the loader --------------------------------------------------------------------------------------------------------------
_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# SSD_HIP_LIB_PATH: diagnostics only (tools/stamps.py loads a -DSSD_STAMPS build of the same sources)
HIP_LIB_PATH = os.environ.get("SSD_HIP_LIB_PATH", os.path.join(_PKG_DIR, "libssd_hip.so"))
_lib = None


def bind(lib, signatures):
    missing = []
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise ImportError("native library is missing symbols: " + ", ".join(missing))
    return lib


def load_library():
    """Load homophily_marl_amd/libssd_hip.so (built by __graft_entry__.build()).  Fails loudly when absent."""
    global _lib
    if _lib is None:
        # torch first: the PyTorch-ROCm wheel bundles its own libamdhip64.so (soname libamdhip64.so.7).  Loaded
        # first, it satisfies this library's NEEDED entry, so both share ONE HIP runtime (device pointers and
        # streams are only meaningful within one runtime).  Loaded second, /opt/rocm's copy would already be in
        # the process and torch would bring a second runtime.
        import torch  # noqa: F401
        if not os.path.exists(HIP_LIB_PATH):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % HIP_LIB_PATH)
        lib = C.CDLL(HIP_LIB_PATH)
        bind(lib, HIP_SIGNATURES)
        bind(lib, TRAIN_SIGNATURES)
        bind(lib, REWARD_SIGNATURES)
        bind(lib, TIE_SIGNATURES)
        bind(lib, MIX_SIGNATURES)
        ver = lib.ssd_abi_version()
        if ver != ABI_VERSION:
            raise ImportError("libssd_hip.so ABI version %d != %d" % (ver, ABI_VERSION))
        _lib = lib
    return _lib


class SsdError(RuntimeError):
    pass


def check(lib, rc, err_fn="ssd_last_error"):
    if rc != 0:
        msg = getattr(lib, err_fn)()
        raise SsdError("ssd error %d: %s" % (rc, msg.decode() if msg else "?"))
