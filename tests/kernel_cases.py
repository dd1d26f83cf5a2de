"""Which kernel of csrc/ssd_env.hip, ssd_learner.hip, ssd_bmm.hip, ssd_gru_seq.hip and ssd_policy.hip a GPU case launches: a pure-Python
restatement of the host dispatch of each family (written from the launch function, whose lines it cites), and `held()`: the kernels that
the GPU cases of the suite hold to an independent reference -- the CPU oracle, the reference's recordings, a float64 or integer
restatement, the law of the draws, the torch controller.  The sibling of tests/policy_cases.py, which keeps the same ledger for
csrc/ssd_policy_mfma.hip; tests/test_kernel_ledger_host.py asserts that every compiled kernel is held or stands in UNREACHABLE.

`held()` maps the tests' OWN parameter lists (imported from their modules, never copied) through the restated dispatch.  A family
whose kernels have a single form is held by a named test (SINGLE): the ledger checks that the test exists, is marked gpu and that its
module names the export that launches the kernel.  A case that only compares kernel with kernel holds nothing.

Keys are the template argument lists as a demangler prints them, without spaces:
    k_env<MODE,NT,TAPE,OV,REC>   k_bias_bmm_fwd<XV,BF>   k_bias_bmm_bwd<OV,ACT,BF>   k_conv_wgrad<V>   k_gru_seq_fwd[_h0]<TRAIN,BF>
    k_gru_seq_bwd[_h0]<BF>   k_sample_draw<SLOTS>   k_dueling_q<BWD>   k_td_sim_loss<MODE>   k_conv_leaky<C,VT>   k_encoder<C,F,RPW>"""
import functools
import importlib
import os
import re
import sys

from homophily_marl_amd import abi
from tests.policy_cases import _params, compiled_kernels, demangled_key      # noqa: F401  (demangled_key: the ledger's self-check)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SOURCES = ("ssd_env.hip", "ssd_learner.hip", "ssd_bmm.hip", "ssd_gru_seq.hip", "ssd_policy.hip")


@functools.lru_cache(maxsize=None)
def compiled(src):
    """the keys of every kernel of one source: the .name entries of its code-object metadata (names only, no instruction is looked at)"""
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_hazards
    return frozenset(compiled_kernels(asm_hazards.isa_of(src), prefixes=("k_",)))


def _csrc(source):
    return open(os.path.join(ROOT, "homophily_marl_amd", "csrc", source)).read()


def _csrc_int(source, pattern):
    found = re.findall(pattern, _csrc(source))
    assert found and len(set(found)) == 1, (source, pattern, found)
    return int(found[0])


def _b(x):
    return "true" if x else "false"


# ---- ssd_env.hip: launch_env (:1258-1309) ----------------------------------------------------------------------------------------------
RESET, STEP, STEP_OBS, OBS = 0, 1, 2, 3                 # ssd_device.h:20
OV_ANY, OV_CODE, OV_F32 = 0, 1, 2                        # ssd_env.hip:805
ENV_FORMATS = (None, abi.OBS_F32, abi.OBS_BF16, abi.OBS_U8, abi.OBS_CODE)      # None: no `obs` output asked for
NT_SIZES = (5, 10, 3)                                    # the team sizes with a compile-time instantiation


def _env(mode, nt, tape, ov=OV_ANY, rec=False):
    return "k_env<%d,%d,%s,%d,%s>" % (mode, nt, _b(tape), ov, _b(rec))


def env_kernel(mode, n, tape, render, fmt, want_state, want_code, full_colour):
    """render: ssd_set_render is on (the launch is handed the beam record for the two stepping modes only, ssd_abi.hip:311,327);
    fmt: the observation format, None without an `obs` output; want_state / want_code: the state planes / the class-code side buffer"""
    if render and mode in (STEP, STEP_OBS):                                     # :1268-1279  (SSD_LAUNCH_REC)
        return _env(mode, 0, True, rec=True) if tape else _env(mode, 5 if n == 5 else 0, False, rec=True)
    by_n = lambda m: _env(m, 0, True) if tape else _env(m, n if n in NT_SIZES else 0, False)      # :1281-1286  (SSD_LAUNCH_N)
    if mode == RESET:                                                           # :1288
        return _env(RESET, 0, tape)
    if mode == STEP:                                                            # :1289
        return by_n(STEP)
    if mode == STEP_OBS:                                                        # :1290-1300
        plain = not tape and not full_colour and fmt is not None and not want_state and n in (5, 10)
        ov = OV_ANY if not plain else OV_CODE if fmt == abi.OBS_CODE else OV_F32 if (fmt == abi.OBS_F32 and not want_code) else OV_ANY
        return _env(STEP_OBS, n, False, ov) if ov != OV_ANY else by_n(STEP_OBS)
    return _env(OBS, n if n in NT_SIZES else 0, False)                          # :1301-1304  (observations draw nothing: no tape form)


def env_domain():
    """every argument set of env_kernel: mode x n 1 .. 10 x tape x render x format x state x code x colour"""
    for mode in (RESET, STEP, STEP_OBS, OBS):
        for n in range(1, 11):
            for tape in (False, True):
                for render in (False, True):
                    for fmt in ENV_FORMATS:
                        for state in (False, True):
                            for code in (False, True):
                                for full in (False, True):
                                    yield mode, n, tape, render, fmt, state, code, full


def _lockstep(n, fmts, full=False, tape=False, render=False, step_alone=False, observe_state=False, observe=False, imports=False, fused=True):
    """the kernels of one device-against-reference run: reset, step_observe at every format of `fmts` (fused), step alone, observe
    with / without the state planes, import_state, and the export_state every state comparison makes"""
    ks = {env_kernel(RESET, n, tape, render, None, False, False, full), "k_export"}
    if fused:
        ks |= {env_kernel(STEP_OBS, n, tape, render, f, False, False, full) for f in fmts}
    if step_alone:
        ks.add(env_kernel(STEP, n, tape, render, None, False, False, full))
    if observe_state:
        ks.add(env_kernel(OBS, n, tape, render, fmts[0], True, False, full))
    if observe:
        ks.add(env_kernel(OBS, n, tape, render, fmts[0], False, False, full))
    if imports:
        ks.add("k_import")
    return ks


def _golden_meta(pattern):
    import glob
    import json
    import numpy as np
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", pattern))):
        out.append((os.path.basename(path), json.loads(bytes(np.load(path)["meta"]).decode())))
    return out


def _full(meta):
    return (meta.get("extra_args") or {}).get("obs_color", "simplified") == "full"


def env_held(new_cases=True):
    """the env kernels that a GPU case holds to the oracle, the reference's recordings or the law of the draws"""
    from tests import beam_util, env_law_util, env_state_util, golden_util, test_env_domain as D, test_hip_parity as HP
    F, F_FULL = D.FORMATS, D.FORMATS[1:]
    held = set()
    # tests/test_env_domain.py (run_vs_oracle: reset, step_observe at every format, one observe with the state planes per episode)
    for _, n in D.SWEEP:            # the palettes of views 0, 1, 3, 7 (indices 0 .. 3: they do not depend on v_max) + the simplified one of v_max
        for full in {(i + n) % 3 == 2 for i in range(4)} | {False}:
            held |= _lockstep(n, F_FULL if full else F, full, observe_state=True)
    for _, n, _ in D.MANY:
        held |= _lockstep(n, F, observe_state=True)
    for _, _, n, _ in D.CUSTOM.values():
        held |= _lockstep(n, F, observe_state=True) | _lockstep(n, F_FULL, True, observe_state=True)
    for n, _ in D.RENDER_VIEWS:
        held |= _lockstep(n, F, render=True, observe_state=True)
    # tests/test_env_states_gpu.py (env_state_util.run_case: every step is a step_observe, the format rotating; imports per builder)
    for c in env_state_util.CASES.values():
        assert c.T // c.episodes >= len(F)
        held |= _lockstep(c.n, F, imports=c.builder is not None)
    # tests/test_env_beams_gpu.py (beam_util.run_case: step_observe and step + observe alternate, states imported, frames under render)
    for name, c in beam_util.CASES.items():
        assert c.T >= 16                                                      # fmts[(t + t // 4) % 4]: both call shapes meet every format
        held |= _lockstep(c.n, F, step_alone=True, observe=True, imports=True)
        if name in beam_util.RENDER_CASES:
            held |= _lockstep(c.n, F, render=True, step_alone=True, observe=True, imports=True) | {"k_render"}
        if name == beam_util.FULL_COLOUR_CASE:
            held |= _lockstep(c.n, F_FULL, True, step_alone=True, observe=True, imports=True)
    # tests/test_env_law_gpu.py (the device's own exported states against the law: step alone, or step_observe with class codes)
    for _, _, n, _, code, _ in env_law_util.SWEEPS.values():
        held |= _lockstep(n, (abi.OBS_CODE,), fused=code, step_alone=not code, imports=True)
    # tests/test_hip_parity.py: the reference's trajectories in TAPE mode (step alone; observe in four formats), COUNTER mode against the oracle
    for _, meta in _golden_meta("traj_*.npz"):
        held |= _lockstep(meta["num_agents"], (abi.OBS_U8,), _full(meta), tape=True, fused=False, step_alone=True, observe_state=True, observe=True, imports=True)
    for cfg in HP.CONFIGS.values():
        for full in (False, True):
            held |= _lockstep(cfg["num_agents"], (abi.OBS_F32,), full, step_alone=True, observe_state=True, imports=True)
    for _, n, _, _ in HP.OTHER_TEAMS:
        held |= _lockstep(n, (abi.OBS_CODE, abi.OBS_F32, abi.OBS_U8))
    # tests/test_render_gpu.py::test_frames_match_the_reference (TAPE, render mode: step alone; reset frames under env_mask)
    for _, meta in _golden_meta("render_*.npz"):
        held |= _lockstep(meta["num_agents"], (abi.OBS_U8,), _full(meta), tape=True, render=True, fused=False, step_alone=True, imports=True)
        held |= {"k_render", "k_beam_clear"}
    if new_cases:
        # the TAPE instantiations of step_observe: test_hip_parity.test_golden_trajectory_through_step_observe and
        # test_render_gpu.test_frames_match_the_reference_through_step_observe
        metas = dict(_golden_meta("traj_*.npz") + _golden_meta("render_*.npz"))
        for name in golden_util.FUSED_TAPE_TRAJ:
            held |= _lockstep(metas[name]["num_agents"], D.FORMATS if not _full(metas[name]) else F_FULL, _full(metas[name]), tape=True, imports=True)
        for name in golden_util.FUSED_TAPE_RENDER:
            held |= _lockstep(metas[name]["num_agents"], D.FORMATS if not _full(metas[name]) else F_FULL, _full(metas[name]), tape=True, render=True, imports=True)
    return held


# ---- ssd_bmm.hip -------------------------------------------------------------------------------------------------------------------------
def bmm_fwd(I, precision, I2=None):
    """launch_bias_bmm_fwd (:426-440): 16-byte row loads for rows of whole quads; launch_bias_bmm2_fwd (:443-462): the same for the
    second source (in1 is a multiple of 16).  The leaky form is a run-time flag of the same kernels."""
    xv = (I & 3) == 0 if I2 is None else (I2 & 3) == 0
    return "k_bias_bmm_fwd<%s,%s>" % (_b(xv), _b(precision == 1))


def bmm_bwd(O, leaky, precision):
    """launch_bias_bmm_bwd (:493-502)"""
    return "k_bias_bmm_bwd<%s,%s,%s>" % (_b((O & 3) == 0), _b(leaky), _b(precision == 1))


def bmm_row_chunked(n, R, I, O):
    """the rule at :486-491 for a launch that asks for dw or db (with the per-stream scratch allocated): long row axes whose tiles would
    leave the chip mostly idle are cut into row chunks, and k_bmm_dw_reduce adds the partial tiles"""
    waves, part, scratch = (_csrc_int("ssd_bmm.hip", p) for p in (r"constexpr int BMM_BWD_WAVES = (\d+);", r"constexpr int BMM_PART = (\d+);",
                                                                  r"constexpr size_t BMM_SCRATCH_BYTES = 1 << (\d+);"))
    dwb = ((I + 15) // 16) * ((O + 15) // 16)
    if not ((R + 3) // 4 >= 64 * waves and dwb * n <= 128):
        return False
    c = min(256 // (dwb * n), 8)
    return c > 1 and n * dwb * c * part * 4 <= 1 << scratch


def conv_wgrad(V):
    """launch_conv_wgrad (:678-684)"""
    return "k_conv_wgrad<%d>" % V if V in (15, 31) else "k_conv_wgrad_any"


def bmm_held(new_cases=True):
    from tests import test_learner_kernel_bounds as KB
    held = set()
    for n, R, I, O in KB._bmm_shapes():                  # test_bias_bmm_forward_and_backward_in_the_arena: f32 and bf16, plain and leaky
        for prec in (2, 1):
            held |= {bmm_fwd(I, prec), bmm_bwd(O, False, prec), bmm_bwd(O, True, prec)}
        if bmm_row_chunked(n, R, I, O):
            held.add("k_bmm_dw_reduce")
    for n, R, I1, I2, O, div, shared in KB._bmm2_shapes():      # test_two_source_layer_in_the_arena
        for prec in (2, 1):
            held |= {bmm_fwd(I1 + I2, prec, I2), bmm_bwd(O, False, prec)}
    for R, V in KB.CONV_WGRAD_CASES:                     # test_conv_wgrad_codes_in_the_arena
        held.add(conv_wgrad(V))
    return held


# ---- ssd_gru_seq.hip ---------------------------------------------------------------------------------------------------------------------
def gru_fwd(train, precision, h0):
    """launch_gru_seq_fwd (:155-177): train = the saved gates are asked for"""
    return "k_gru_seq_fwd%s<%s,%s>" % ("_h0" if h0 else "", _b(train), _b(precision == 1))


def gru_bwd(precision, h0):
    """launch_gru_seq_bwd (:201-205)"""
    return "k_gru_seq_bwd%s<%s>" % ("_h0" if h0 else "", _b(precision == 1))


# (module, test, the forms it holds to the stepwise float64 unroll or to the reference's numbers): (train, precision, h0, backward too)
GRU_USES = [
    # ops.gru_sequence(h0=...) with gradients, then under no_grad (bit-equal to the first, which is held to the unroll)
    ("test_stored_state_gpu", "test_kernels_from_a_given_state_match_the_stepwise_unroll", [(True, 2, True, True), (False, 2, True, False)]),
    # the same under ssd_set_learner_precision(1), at the bf16 bar (the no_grad form: this pull request)
    ("test_stored_state_gpu", "test_bf16_instantiations_at_the_bf16_bar", [(True, 1, True, True), (False, 1, True, False)]),
    # learner_dtype bf16 against the reference's Q-values and losses: unroll under no_grad, then two train steps
    ("test_hip_learner_path", "test_bf16_learner_variant_is_close_to_the_reference_and_labelled", [(False, 1, False, False), (True, 1, False, True)]),
]
GRU_NEW = {gru_fwd(False, 1, True)}                      # what this pull request's addition to test_bf16_instantiations_at_the_bf16_bar brought in


def gru_held(new_cases=True):
    from tests import test_learner_kernel_bounds as KB
    held = set()
    for T, G, B, train in KB.GRU_SEQ_CASES:              # test_gru_sequence_in_the_arena: values at f32 only (bf16: bounds alone, holds nothing)
        held.add(gru_fwd(bool(train), 2, False))
        if train:
            held.add(gru_bwd(2, False))
    for module, test, forms in GRU_USES:
        _gpu_test(module, test)
        for train, prec, h0, bwd in forms:
            held.add(gru_fwd(train, prec, h0))
            if bwd:
                held.add(gru_bwd(prec, h0))
    return held if new_cases else held - GRU_NEW


# ---- ssd_learner.hip ---------------------------------------------------------------------------------------------------------------------
def sample_draw(count):
    """launch_sample_draw (:846-852): 64 picks per register slot"""
    slots = 1 if count <= 64 else 2 if count <= 128 else 4 if count <= 256 else abi.SAMPLE_IDS_MAX // 64
    return "k_sample_draw<%d>" % slots


def dueling_q(backward):
    """launch_dueling_q (:748-749): the backward form is the one handed dq"""
    return "k_dueling_q<%s>" % _b(backward)


def td_loss(mode, lam):
    """launch_td_sim_loss (:1732-1734)"""
    return "k_td_lambda_loss" if (mode and lam > 0) else "k_td_sim_loss<%d>" % (1 if mode else 0)


def priority_sample(n_segments):
    """launch_priority_sample (:1176-1177)"""
    return "k_priority_sample_seq" if n_segments else "k_priority_sample"


def rollout_priority(n_segments):
    """launch_rollout_priority (:1440-1441)"""
    return "k_rollout_priority_seq" if n_segments else "k_rollout_priority"


def _gpu_test(module, test):
    """the test function, which must exist and carry the gpu mark (its own or its module's)"""
    mod = importlib.import_module("tests." + module)
    fn = getattr(mod, test)
    marks = [m.name for m in getattr(fn, "pytestmark", [])]
    pm = getattr(mod, "pytestmark", [])
    marks += [m.name for m in (pm if isinstance(pm, (list, tuple)) else [pm])]
    assert "gpu" in marks, (module, test)
    return fn


# kernels with a single form: kernel -> (module, test that compares what it wrote with a reference, the export that launches it)
SINGLE = {
    "ssd_env.hip": {
        "k_export": ("test_env_domain", "test_team_sizes_and_views", "export_state"),
        "k_import": ("test_env_states_gpu", "test_states_past_a_reset_rollout", "run_case"),
        "k_render": ("test_render_gpu", "test_frames_match_the_reference", "get_frames"),
        "k_beam_clear": ("test_render_gpu", "test_frames_match_the_reference", "env_mask"),
    },
    "ssd_learner.hip": {
        "k_behaviour_partials": ("test_behaviour_gpu", "test_export_equals_the_reference_exactly", "behaviour"),
        "k_behaviour_finish": ("test_behaviour_gpu", "test_export_equals_the_reference_exactly", "behaviour"),
        "k_build_inputs": ("test_learner_kernel_bounds", "test_build_inputs_in_the_arena", "ssd_build_inputs"),
        "k_build_inputs_flags": ("test_learner_kernel_bounds", "test_build_inputs_in_the_arena", "ssd_build_inputs_flags"),
        "k_gradsq_partials": ("test_learner_kernel_bounds", "test_clip_adam_step_in_the_arena", "ssd_clip_adam_step"),
        "k_clip_adam": ("test_learner_kernel_bounds", "test_clip_adam_step_in_the_arena", "ssd_clip_adam_step"),
        "k_polyak": ("test_soft_target_gpu", "test_polyak_launch_in_the_arena", "ssd_clip_adam_step"),
        "k_column_sums": ("test_learner_kernel_bounds", "test_column_sums_in_the_arena", "ssd_column_sums"),
        "k_copy_blocks": ("test_learner_kernel_bounds", "test_copy_blocks_in_the_arena", "ssd_copy_blocks"),
        "k_fill_blocks": ("test_learner_kernel_bounds", "test_fill_blocks_in_the_arena", "ssd_fill_blocks"),
        "k_gather_rows": ("test_learner_kernel_bounds", "test_gather_rows_in_the_arena", "ssd_gather_rows"),
        "k_gather_windows": ("test_train_window_gpu", "test_gather_windows_in_the_arena", "ssd_gather_windows"),
        "k_incentive_transfer": ("test_learner_kernel_bounds", "test_incentive_transfer_in_the_arena", "ssd_incentive_transfer"),
        "k_unroll_other": ("test_learner_kernel_bounds", "test_unroll_other_in_the_arena", "ssd_unroll_other"),
        "k_runner_stats": ("test_learner_kernel_bounds", "test_runner_stats_in_the_arena", "ssd_runner_stats"),
        "k_priority_rows": ("test_priority_gpu", "test_update_in_the_arena", "ssd_priority_update"),
        "k_priority_apply": ("test_priority_gpu", "test_update_in_the_arena", "ssd_priority_update"),
    },
    "ssd_bmm.hip": {},
    "ssd_gru_seq.hip": {},
    "ssd_policy.hip": {
        "k_gru_gates": ("test_learner_kernel_bounds", "test_gru_gate_kernels_in_the_arena", "ssd_gru_gates"),
        "k_gru_fwd_train": ("test_learner_kernel_bounds", "test_gru_gate_kernels_in_the_arena", "ssd_gru_gates_fwd"),
        "k_gru_bwd": ("test_learner_kernel_bounds", "test_gru_gate_kernels_in_the_arena", "ssd_gru_gates_bwd"),
        "k_dueling_pick": ("test_exploration_draws", "test_dueling_pick_equals_the_restated_draws", "ssd_dueling_pick"),
        "k_store_step": ("test_hip_learner_path", "test_fast_graph_runner_stores_a_consistent_batch", "fold_store"),      # fold = 0: the store-step kernel files the fields
        "k_store_hidden": ("test_stored_state_gpu", "test_store_hidden_writes_its_slot_and_nothing_else", "store_hidden"),
    },
}


def single_held(src):
    """the single-form kernels of a source whose named test exists, is a GPU test and names the export (or the helper) in its module"""
    held = set()
    for kernel, (module, test, word) in SINGLE[src].items():
        _gpu_test(module, test)
        assert word in open(os.path.join(ROOT, "tests", module + ".py")).read(), (kernel, module, word)
        held.add(kernel)
    return held


def learner_held(new_cases=True):
    from tests import test_learner_kernel_bounds as KB, test_td_lambda_gpu as TL, test_train_window_gpu as TW
    held = single_held("ssd_learner.hip")
    for count, _ in KB.SAMPLE_IDS_CASES:                 # test_sample_ids_in_the_arena (the ids of a second implementation on the host)
        held.add(sample_draw(count))
    for _, count, _ in TW.SHAPES + TW.MORE_SHAPES:       # test_device_draws_are_the_restatement
        held.add(sample_draw(count))
    assert KB._dueling_shapes(16)                        # test_dueling_q_in_the_arena: ssd_dueling_q_fwd and _bwd per shape
    held |= {dueling_q(False), dueling_q(True)}
    assert _params(KB.test_td_sim_loss_in_the_arena)     # modes 0 and 1 per shape, one-step targets (td_lambda 0)
    held |= {td_loss(0, 0.0), td_loss(1, 0.0)}
    for lam in dict(_params(TL.test_lambda_kernel_in_the_arena))["lam"]:
        if TL.ARENA_CASES:
            held.add(td_loss(1, lam))
    _gpu_test("test_priority_gpu", "test_device_draws_are_the_restatement")                          # no segments
    _gpu_test("test_window_priority_gpu", "test_draw_over_entries_is_the_flat_draw_bit_for_bit")     # segments = (S, s, last)
    held |= {priority_sample(0), priority_sample(3)}
    _gpu_test("test_rollout_priority_gpu", "test_kernel_is_the_restatement_on_exact_td_inputs")
    _gpu_test("test_window_priority_gpu", "test_window_kernel_is_the_restatement_on_exact_td_inputs")
    held |= {rollout_priority(0), rollout_priority(3)}
    return held


# ---- ssd_policy.hip ----------------------------------------------------------------------------------------------------------------------
def conv_leaky(V):
    """launch_conv_leaky (:299-305)"""
    return "k_conv_leaky<6,%d>" % (V if V in (15, 31) else 0)


def encoder():
    """launch_encoder (:290-298): one instantiation"""
    return "k_encoder<6,32,1>"


# tests/test_kernel_ledger_gpu.py: ssd_conv_leaky and ssd_encoder against float64, every operand in the arena
CONV_LEAKY_EDGES = (3, 5, 15, 17, 31, 33, 63)
CONV_LEAKY_ROWS = ((1, 1), (10, 5), (21, 3))             # (rows, n_agents)
ENCODER_EDGES = (3, 5, 15, 17, 29, 31)
ENCODER_ROWS = ((1, 1), (5, 5), (203, 7))                # against 4 rows per workgroup
ENCODER_LDS_MAX_EDGE, CONV_LEAKY_LDS_MAX_EDGE = 36, 73   # the last window edges whose staging fits 64 KiB of LDS


def policy_held(new_cases=True):
    from tests import test_policy_mfma as PM
    held = single_held("ssd_policy.hip")
    (_, rows), = _params(PM.test_fast_policy_matches_torch_controller)
    for fused, N, kind, n, view in rows:                 # fused = False: the per-layer path against the torch controller
        if not fused:
            held.add(conv_leaky(2 * view + 1))
    if new_cases:
        held |= {conv_leaky(V) for V in CONV_LEAKY_EDGES}
        if ENCODER_EDGES:
            held.add(encoder())
    return held


# ---- the ledger --------------------------------------------------------------------------------------------------------------------------
HELD = {"ssd_env.hip": lambda new_cases=True: env_held(new_cases) | single_held("ssd_env.hip"), "ssd_learner.hip": learner_held,
        "ssd_bmm.hip": bmm_held, "ssd_gru_seq.hip": gru_held, "ssd_policy.hip": policy_held}


@functools.lru_cache(maxsize=None)
def held(src, new_cases=True):
    return frozenset(HELD[src](new_cases))


# source -> {kernel: why no configuration reaches it}; each entry is backed by an assertion over the restated dispatch in the host test
UNREACHABLE = {src: {} for src in SOURCES}


def ledger(src, kernels=None, new_cases=True):
    """(kernels neither held nor argued unreachable, UNREACHABLE entries of this source that are held or not compiled)"""
    kernels = compiled(src) if kernels is None else kernels
    h = held(src, new_cases)
    return sorted(set(kernels) - h - set(UNREACHABLE[src])), sorted(k for k in UNREACHABLE[src] if k in h or k not in kernels)
