"""CPU: the ledger of the env, learner and per-layer kernels (csrc/ssd_env.hip, ssd_learner.hip, ssd_bmm.hip, ssd_gru_seq.hip,
ssd_policy.hip), the sibling of the policy ledger of tests/test_policy_instantiations.py.

tests/kernel_cases.py restates the host dispatch of every kernel family in Python and maps the GPU cases' own parameter lists through
it; here every compiled kernel (read by name from the code-object metadata) must be one that a GPU case holds to an independent
reference, or stand in UNREACHABLE with its reason.  A kernel added without a case fails on the CPU.  Each restatement is kept honest
by a set equality: swept over its whole domain it returns every compiled kernel of its family and nothing else.

Plus the refusal tables of ssd_encoder and ssd_conv_leaky (no launch: dummy pointers, invalid calls only), with the LDS limits of
both pinned at the first refused window edge."""
import pytest

from homophily_marl_amd import abi
from tests import kernel_cases as kc

INV, UNS = abi.SSD_ERR_INVALID, abi.SSD_ERR_UNSUPPORTED
F = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched

# per source: names that must be read from the metadata, the kernels this pull request's cases brought under test, a made-up name
KNOWN = {
    "ssd_env.hip": (("k_env<2,5,false,1,false>", "k_env<1,0,true,0,true>", "k_export", "k_beam_clear"),
                    ("k_env<2,0,true,0,false>", "k_env<2,0,true,0,true>"), "k_env<1,4,false,0,false>"),
    "ssd_learner.hip": (("k_sample_draw<16>", "k_dueling_q<true>", "k_td_sim_loss<0>", "k_priority_sample_seq", "k_polyak"), (), "k_sample_draw<8>"),
    "ssd_bmm.hip": (("k_bias_bmm_bwd<false,true,true>", "k_bias_bmm_fwd<true,false>", "k_conv_wgrad<31>", "k_conv_wgrad_any", "k_bmm_dw_reduce"), (),
                    "k_conv_wgrad<63>"),
    "ssd_gru_seq.hip": (("k_gru_seq_fwd<true,false>", "k_gru_seq_bwd_h0<true>"), ("k_gru_seq_fwd_h0<false,true>",), "k_gru_seq_bwd<2>"),
    "ssd_policy.hip": (("k_encoder<6,32,1>", "k_conv_leaky<6,0>", "k_store_hidden"), ("k_conv_leaky<6,0>", "k_conv_leaky<6,31>", "k_encoder<6,32,1>"),
                       "k_conv_leaky<6,63>"),
}
COUNTS = {"ssd_env.hip": 30, "ssd_learner.hip": 30, "ssd_bmm.hip": 16, "ssd_gru_seq.hip": 12, "ssd_policy.hip": 10}


@pytest.mark.parametrize("src", kc.SOURCES)
def test_every_kernel_is_held_by_a_case_or_argued_unreachable(src):
    kernels = kc.compiled(src)
    known, brought, made_up = KNOWN[src]
    for k in known:
        assert k in kernels, (k, sorted(kernels)[:5])                           # the metadata was read and demangled
    missing, stale = kc.ledger(src)
    assert not missing, "compiled kernels of %s that no GPU case holds to a reference: %s" % (src, missing)
    assert not stale, "UNREACHABLE entries that a case reaches, or that are not compiled: %s" % stale
    assert len(kernels) == COUNTS[src], sorted(kernels)
    assert set(kc.SINGLE[src]) <= kernels, sorted(set(kc.SINGLE[src]) - kernels)      # no named holder of a kernel that is gone
    # without the new case tables the kernels they brought under test are missing again -- and only those
    assert kc.ledger(src, new_cases=False)[0] == sorted(brought)
    # a kernel nobody planned for
    assert made_up not in kernels and kc.ledger(src, kernels | {made_up})[0] == [made_up]


def test_unreachable_entries_are_backed_and_compiled():
    """UNREACHABLE is expected to be empty: every one of the 98 kernels is reached by a GPU case.  An entry needs an assertion over the
    restated dispatch next to it (UNREACHABLE_CHECKS below) and must name a compiled kernel that no case holds."""
    every = set().union(*(kc.compiled(s) for s in kc.SOURCES))
    assert len(every) == sum(COUNTS.values()) == 98
    argued = {k for src in kc.SOURCES for k in kc.UNREACHABLE[src]}
    assert set(kc.UNREACHABLE) == set(kc.SOURCES) and argued == set(UNREACHABLE_CHECKS) and argued <= every
    for check in UNREACHABLE_CHECKS.values():
        check()
    assert kc.demangled_key("_ZN3ssd5k_envILi2ELi5ELb0ELi1ELb0EEEvPK15HIP_vector_typeIjLj4EE") == "k_env<2,5,false,1,false>"


UNREACHABLE_CHECKS = {}


# ---- the restatements against the compiled kernels: set equalities -------------------------------------------------------------------------
def test_env_dispatch_over_its_whole_domain_is_the_compiled_set():
    """mode x n 1 .. 10 x tape x render x format x state x code x colour: only compiled kernels, and every compiled k_env"""
    compiled = {k for k in kc.compiled("ssd_env.hip") if k.startswith("k_env<")}
    reached = {kc.env_kernel(*args) for args in kc.env_domain()}
    assert reached == compiled, "returned but not compiled: %s; compiled but never returned: %s" % (sorted(reached - compiled), sorted(compiled - reached))
    assert len(compiled) == 26
    assert compiled | set(kc.SINGLE["ssd_env.hip"]) == kc.compiled("ssd_env.hip")
    # the rules the restatement carries, at the points where they switch
    f32, code = abi.OBS_F32, abi.OBS_CODE
    assert kc.env_kernel(kc.STEP_OBS, 5, False, False, code, False, False, False) == "k_env<2,5,false,1,false>"
    assert kc.env_kernel(kc.STEP_OBS, 10, False, False, f32, False, False, False) == "k_env<2,10,false,2,false>"
    assert kc.env_kernel(kc.STEP_OBS, 10, False, False, f32, False, True, False) == "k_env<2,10,false,0,false>"        # with the code side buffer
    assert kc.env_kernel(kc.STEP_OBS, 5, False, False, f32, True, False, False) == "k_env<2,5,false,0,false>"          # with the state planes
    assert kc.env_kernel(kc.STEP_OBS, 5, False, False, f32, False, False, True) == "k_env<2,5,false,0,false>"          # full colour
    assert kc.env_kernel(kc.STEP_OBS, 3, False, False, code, False, False, False) == "k_env<2,3,false,0,false>"        # plain needs n = 5 / 10
    assert kc.env_kernel(kc.STEP_OBS, 10, False, True, code, False, False, False) == "k_env<2,0,false,0,true>"         # render: 5 or run-time
    assert kc.env_kernel(kc.OBS, 3, True, True, code, True, False, False) == "k_env<3,3,false,0,false>"                # observe: no tape, no record
    assert kc.env_kernel(kc.RESET, 5, True, True, None, False, False, False) == "k_env<0,0,true,0,false>"


def test_bmm_gru_learner_and_policy_restatements_are_the_compiled_sets():
    reached = {kc.bmm_fwd(I, p) for I in range(1, 9) for p in (1, 2)} | {kc.bmm_fwd(16 + I2, p, I2) for I2 in range(1, 9) for p in (1, 2)}
    reached |= {kc.bmm_bwd(O, leaky, p) for O in range(1, 9) for leaky in (False, True) for p in (1, 2)}
    reached |= {kc.conv_wgrad(V) for V in range(3, 64)}
    chunked = {kc.bmm_row_chunked(n, R, I, O) for n in (1, 5) for R in (255, 4093, 4094, 8080) for I, O in ((16, 16), (80, 3), (73, 192))}
    assert chunked == {False, True}
    assert kc.bmm_row_chunked(1, 4093, 16, 16) and not kc.bmm_row_chunked(1, 4092, 16, 16) and not kc.bmm_row_chunked(10, 8080, 73, 192)
    assert reached | {"k_bmm_dw_reduce"} == kc.compiled("ssd_bmm.hip"), sorted(reached ^ kc.compiled("ssd_bmm.hip"))
    reached = {kc.gru_fwd(t, p, h) for t in (False, True) for p in (1, 2) for h in (False, True)} | {kc.gru_bwd(p, h) for p in (1, 2) for h in (False, True)}
    assert reached == kc.compiled("ssd_gru_seq.hip"), sorted(reached ^ kc.compiled("ssd_gru_seq.hip"))
    reached = {kc.sample_draw(c) for c in range(1, abi.SAMPLE_IDS_MAX + 1)} | {kc.dueling_q(b) for b in (False, True)}
    reached |= {kc.td_loss(m, lam) for m in (0, 1) for lam in (0.0, 0.5)} | {kc.priority_sample(s) for s in (0, 4)} | {kc.rollout_priority(s) for s in (0, 4)}
    assert [kc.sample_draw(c) for c in (64, 65, 128, 129, 256, 257)] == ["k_sample_draw<%d>" % s for s in (1, 2, 2, 4, 4, 16)]
    assert kc.td_loss(0, 0.5) == "k_td_sim_loss<0>"                                 # the lambda kernel serves the loss mode only
    assert reached | set(kc.SINGLE["ssd_learner.hip"]) == kc.compiled("ssd_learner.hip"), sorted((reached | set(kc.SINGLE["ssd_learner.hip"])) ^ kc.compiled("ssd_learner.hip"))
    reached = {kc.conv_leaky(V) for V in range(3, kc.CONV_LEAKY_LDS_MAX_EDGE + 1)} | {kc.encoder()}
    assert reached | set(kc.SINGLE["ssd_policy.hip"]) == kc.compiled("ssd_policy.hip")


def test_the_new_cases_stand_where_the_ledger_says():
    """the window edges reach the three k_conv_leaky instantiations, the rows a partly filled workgroup of k_encoder (4 rows each),
    and the largest edges stay inside the LDS refusals"""
    assert {kc.conv_leaky(V) for V in kc.CONV_LEAKY_EDGES} == {"k_conv_leaky<6,0>", "k_conv_leaky<6,15>", "k_conv_leaky<6,31>"}
    assert {r % 4 for r, _ in kc.ENCODER_ROWS} >= {1, 3} and all(r % n == 0 for r, n in kc.ENCODER_ROWS + kc.CONV_LEAKY_ROWS)
    assert 31 in kc.ENCODER_EDGES and max(kc.ENCODER_EDGES) <= kc.ENCODER_LDS_MAX_EDGE and max(kc.CONV_LEAKY_EDGES) <= kc.CONV_LEAKY_LDS_MAX_EDGE


# ---- refusals of ssd_encoder and ssd_conv_leaky (ONLY invalid calls: the baselines themselves are never called) ----------------------------
LDS = b"exceeds the 64 KiB a launch may ask for"
# obs, rows, view_edge, conv_out, feat_out, conv_w, conv_b, lin_w, lin_b, out, out_stride, n_agents, agent_major, store_obs, store_env_stride, store_t, stream
ENCODER = [F, 20, 15, 6, 32, F, F, F, F, F, 32, 5, 1, None, 0, None, None]
STORE_WITHOUT_T = {13: F}        # an accepted window edge with this fault is refused for the storage: the LDS check let it pass
ENCODER_ROWS = [("null argument %d" % k, {k: None}, INV, b"") for k in (0, 5, 6, 7, 8, 9)] + [
    ("rows 0", {1: 0}, INV, b""), ("view_edge 2", {2: 2}, INV, b""), ("conv_out 5", {3: 5}, UNS, b"conv_out 6"), ("feat_out 31", {4: 31}, UNS, b"obs_dim_net 32"),
    ("rows % n_agents, agent-major", {1: 21}, INV, b"multiple of n_agents"), ("n_agents 0, agent-major", {11: 0}, INV, b"multiple of n_agents"),
    ("rows % n_agents, storage", {1: 21, 12: 0, 13: F, 15: F}, INV, b"multiple of n_agents"), ("store_obs without store_t", STORE_WITHOUT_T, INV, b"store_obs needs store_t"),
    # the LDS limit: 4 windows of 3 V^2 + 4 floats; 36 is the last edge that fits 64 KiB, and 31 (a shipped size) is accepted
    ("view_edge 37: first over the LDS limit", {2: 37}, INV, LDS), ("view_edge 37 and a storage fault", {**STORE_WITHOUT_T, 2: 37}, INV, LDS),
    ("view_edge 63", {2: 63}, INV, LDS), ("view_edge 2^15 (no overflow in the byte count)", {2: 1 << 15}, INV, LDS),
    ("view_edge 36 passes the LDS check", {**STORE_WITHOUT_T, 2: 36}, INV, b"store_obs needs store_t"),
    ("view_edge 31 passes the LDS check", {**STORE_WITHOUT_T, 2: 31}, INV, b"store_obs needs store_t")]
# obs, rows, view_edge, conv_out, conv_w, conv_b, out, n_agents, agent_major, store_obs, store_env_stride, store_t, stream
CONV_LEAKY = [F, 20, 15, 6, F, F, F, 5, 1, None, 0, None, None]
STORE_WITHOUT_T_CL = {9: F}
CONV_LEAKY_ROWS = [("null argument %d" % k, {k: None}, INV, b"") for k in (0, 4, 5, 6)] + [
    ("rows 0", {1: 0}, INV, b""), ("view_edge 2", {2: 2}, INV, b""), ("n_agents 0", {7: 0}, INV, b""), ("rows % n_agents", {1: 21}, INV, b""),
    ("conv_out 5", {3: 5}, UNS, b"conv_out 6"), ("store_obs without store_t", STORE_WITHOUT_T_CL, INV, b"store_obs needs store_t"),
    # the LDS limit: one window of 3 V^2 floats + 168 of weights; 73 is the last edge that fits 64 KiB
    ("view_edge 74: first over the LDS limit", {2: 74}, INV, LDS), ("view_edge 74 and a storage fault", {**STORE_WITHOUT_T_CL, 2: 74}, INV, LDS),
    ("view_edge 2^15 (no overflow in the byte count)", {2: 1 << 15}, INV, LDS),
    ("view_edge 73 passes the LDS check", {**STORE_WITHOUT_T_CL, 2: 73}, INV, b"store_obs needs store_t"),
    ("view_edge 63 passes the LDS check", {**STORE_WITHOUT_T_CL, 2: 63}, INV, b"store_obs needs store_t")]
REFUSALS = [("ssd_encoder", ENCODER) + r for r in ENCODER_ROWS] + [("ssd_conv_leaky", CONV_LEAKY) + r for r in CONV_LEAKY_ROWS]


@pytest.mark.parametrize("name,base,label,change,expect,message", REFUSALS, ids=["%s-%s" % (r[0], r[2].replace(" ", "_")) for r in REFUSALS])
def test_invalid_call_is_refused_with_a_message(name, base, label, change, expect, message):
    lib = abi.load_library()
    args = list(base)
    for k, v in change.items():
        args[k] = v
    rc = getattr(lib, name)(*args)
    assert rc == expect, (name, label, rc, lib.ssd_last_error())
    assert lib.ssd_last_error() and message in lib.ssd_last_error(), (name, label, lib.ssd_last_error())
    with pytest.raises(abi.SsdError):
        abi.check(lib, rc)


def test_the_lds_limits_are_the_launches_own_byte_counts():
    """the edges the refusal tables pin, from the byte counts the launches ask for: 4 (3 V^2 + 4) and 3 V^2 + 168 floats against 64 KiB"""
    enc = lambda V: 4 * (3 * V * V + 4) * 4
    conv = lambda V: (3 * V * V + 6 * 27 + 6) * 4
    assert enc(kc.ENCODER_LDS_MAX_EDGE) <= 65536 < enc(kc.ENCODER_LDS_MAX_EDGE + 1) and enc(31) == 46192
    assert conv(kc.CONV_LEAKY_LDS_MAX_EDGE) <= 65536 < conv(kc.CONV_LEAKY_LDS_MAX_EDGE + 1)
    src = kc._csrc("ssd_policy.hip")
    assert "encoder_lds_bytes(V)" in src and "conv_leaky_lds_bytes(V)" in src             # the launches take the shared expressions
    abi_src = kc._csrc("ssd_abi.hip")
    assert "encoder_lds_bytes(view_edge) > kDefaultLdsLimit" in abi_src and "conv_leaky_lds_bytes(view_edge) > kDefaultLdsLimit" in abi_src
