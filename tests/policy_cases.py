"""Which instantiation of the rollout head, encoder and pack kernels (csrc/ssd_policy_mfma.hip: k_head, k_inc_encode, k_inc_encode_any,
k_inc_encode_gather, k_encode*, k_pack_*) a test case launches: a pure-Python restatement of the host dispatch, the table of GPU cases of
tests/test_policy_instantiations.py, and adapters that read the case lists of the older test files (imported, not copied).

Keys are the kernels' template argument lists as a demangler prints them, without spaces:
    k_head<INC,PREC,AT,GEN,LOOP>   k_inc_encode<PREC,AT,V,LOOP,BT,LUT>   k_inc_encode_any<PREC,AT,LOOP>   k_inc_encode_gather<PREC,AT,GEN,LOOP>
    k_encode<V,PREC,ACT,BT>   k_encode_lut<V,PREC,BT>   k_encode_lut_any<PREC>   k_pack_head[_others|_onehot]<PREC>   k_pack_encoder[_lut]<V,PREC>
    k_pack_encoder_lut_any<PREC>
The ledger (test_every_policy_kernel_is_held_by_a_case_or_argued_unreachable) covers LEDGER_PREFIXES.  An encoder or pack kernel counts
as held where the case compares what it produced with a reference: the features (or the q-values computed from them) against the
torch encoder / controller.  A case that only compares kernel with kernel (the older two-launch tests) holds none of them."""
import functools
import re
from collections import namedtuple

LEDGER_CUS = 256                              # the CPU test plans for an MI355X; the GPU tests plan for the device they run on
LEDGER_PREFIXES = ("k_head", "k_inc_encode", "k_encode", "k_pack_")      # k_inc_encode_any / _gather, k_encode_lut / _lut_any included
HEAD_WAVES, HEAD_WAVES_GATHER, FUSED_HEAD_WAVES = 8, 7, 7
MAX_AGENTS = 10
ENC_BT4_MAX_ROWS = 32768                      # enc_bt: a 15 x 15 launch of at most this many rows takes BT = 4, every other launch BT = 5
RAGGED_ROWS = 10                              # rows in the last tile of a derived n_env: half-full quads of lanes on both sides
MODE_DENSE, MODE_FUSED, MODE_GATHER = 0, 1, 2  # the third argument of ssd_policy_head_plan


# ---- the launch plan (head_bpa / plan_head / plan_head_standalone / policy_head_plan) -------------------------------------------------
def head_bpa(tiles, waves, agents, cus):
    bpa = (tiles + waves - 1) // waves
    if agents * bpa <= cus:
        return bpa
    return max(1, cus // agents)


def plan_head(N, n, waves, cus, always_looped=False):
    """(workgroups per agent, compute waves, looped); every kernel today has the same wave count with and without the back edge"""
    tiles = (N + 15) // 16
    bpa = head_bpa(tiles, waves, n, cus)
    return bpa, waves, bool(always_looped or bpa * waves < tiles)


def plan_standalone(N, n, gen, cus):
    return plan_head(N, n, HEAD_WAVES_GATHER if gen >= 2 else HEAD_WAVES, cus, always_looped=gen == 1)


def head_plan(N, n, mode, cus):
    """what ssd_policy_head_plan reports: (workgroups per agent, compute waves, tiles the busiest wave walks)"""
    bpa, waves, _ = plan_head(N, n, FUSED_HEAD_WAVES, cus) if mode == MODE_FUSED else plan_standalone(N, n, 2 if mode == MODE_GATHER else 0, cus)
    tiles = (N + 15) // 16
    return bpa, waves, (tiles + bpa * waves - 1) // (bpa * waves)


def looping_size(n, mode, cus):
    """the smallest n_env whose plan loops and whose last 16-row tile is ragged with RAGGED_ROWS rows in it (256 CUs, n = 10: 3210 for
    the 8-wave heads, 2810 for the 7-wave)"""
    N = RAGGED_ROWS
    while head_plan(N, n, mode, cus)[2] == 1:
        N += 16
    return N


def bt5_size(n, cus):
    """the smallest ragged n_env whose 15 x 15 encoder launch takes BT = 5 and whose fused head loops"""
    N = RAGGED_ROWS
    while N * n <= ENC_BT4_MAX_ROWS or head_plan(N, n, MODE_FUSED, cus)[2] == 1:
        N += 16
    return N


# ---- cases -------------------------------------------------------------------------------------------------------------------------
# test: "heads" = the standalone heads against the torch controller (and, looped, against their unlooped twins on two shards);
#       "fused" = the one-launch inc head + encoder against the two launches.
# N: a number, or "loop0" / "loop1" / "loop2" = looping_size of that plan mode on the device, "bt5" = bt5_size.
# flags: the config keys of the input set; pipeline: the config key that asks for the fused launch (None: 15 / 31 need none).
# precisions / layouts: every combination runs inside the one test case (one env, one reference).  loop: what the case declares about
# tiles_per_wave > 1 of ITS kernel under test (heads: the standalone plan of its GEN; fused: the fused plan).  feat: the case compares the
# encoder's features (or q-values computed from them) with the torch encoder / controller, so it holds its encoder and pack kernels too.
Case = namedtuple("Case", "id test kind map n N view precisions flags pipeline layouts loop seed feat", defaults=(True,))
SHIPPED = {}
GEN1_ALL_SIX = dict(obs_distance=True)                                            # n = 5: 55 columns + the inc head's action = 64
GEN1_DIST_ONLY = dict(obs_last_action=False, obs_agent_id=False, obs_reward=False, obs_inc_reward=False, obs_agent_pos=False, obs_distance=True)
GEN2 = dict(obs_others_last_action=True, fused_others_last_action=True)
GEN3 = dict(obs_distance=True, obs_others_last_action=True, fused_onehot_gather=True)
BOTH, LUT, P21 = ("lut", "toeplitz"), ("lut",), (2, 1)


def _heads(id, kind, map, n, N, flags, loop, precisions=P21, seed=3):
    return Case(id, "heads", kind, map, n, N, 7, precisions, flags, None, LUT, loop, seed)


def _fused(id, kind, map, n, N, view, loop, flags=SHIPPED, pipeline=None, layouts=BOTH, precisions=P21, seed=3):
    return Case(id, "fused", kind, map, n, N, view, precisions, flags, pipeline, layouts, loop, seed)


CASES = [
    # (a) / (b): GEN 0 -- A = 9 precision 1 looped, A = 8 looped at both precisions, the unlooped precision-1 heads of both action counts
    _heads("cleanup10-gen0-loop", "cleanup", "default10", 10, "loop0", SHIPPED, True),
    _heads("harvest10-gen0-loop", "harvest", "default10", 10, "loop0", SHIPPED, True),
    _heads("harvest5-gen0-203", "harvest", "default10", 5, 203, SHIPPED, False),
    _heads("cleanup5-gen0-203", "cleanup", "default5", 5, 203, SHIPPED, False),
    # GEN 1 (generic tail, env head, looped-only kernel; the inc head of such a set is GEN 0): precision 1 at either action count,
    # on a grid that walks one tile per wave and on one that loops
    _heads("cleanup5-gen1-203", "cleanup", "default5", 5, 203, GEN1_ALL_SIX, False),
    _heads("harvest5-gen1-203", "harvest", "default10", 5, 203, GEN1_ALL_SIX, False),
    _heads("cleanup10-gen1-loop", "cleanup", "default10", 10, "loop0", GEN1_DIST_ONLY, True),
    _heads("harvest10-gen1-loop", "harvest", "default10", 10, "loop0", GEN1_DIST_ONLY, True),
    # GEN 2 / GEN 3: A = 8 looped (and A = 9 at the 7-wave looping size, which the 4112-env cases pass by)
    _heads("harvest10-gen2-loop", "harvest", "default10", 10, "loop2", GEN2, True),
    _heads("harvest10-gen3-loop", "harvest", "default10", 10, "loop2", GEN3, True),
    _heads("cleanup10-gen2-loop", "cleanup", "default10", 10, "loop2", GEN2, True),
    _heads("cleanup10-gen3-loop", "cleanup", "default10", 10, "loop2", GEN3, True),
    # (c) k_inc_encode, V = 15: unlooped BT 4, looped BT 4 (at most 32768 rows), looped BT 5; both layouts, precisions, action counts
    _fused("cleanup5-v7-203", "cleanup", "default5", 5, 203, 7, False),
    _fused("harvest5-v7-203", "harvest", "default10", 5, 203, 7, False),
    _fused("cleanup10-v7-loop-bt4", "cleanup", "default10", 10, "loop1", 7, True),
    _fused("harvest10-v7-loop-bt4", "harvest", "default10", 10, "loop1", 7, True),
    _fused("cleanup10-v7-loop-bt5", "cleanup", "default10", 10, "bt5", 7, True),
    _fused("harvest10-v7-loop-bt5", "harvest", "default10", 10, "bt5", 7, True),
    # V = 31 (three bands, BT 5 only)
    _fused("cleanup5-v15-96", "cleanup", "default5", 5, 96, 15, False),
    _fused("harvest5-v15-96", "harvest", "default10", 5, 96, 15, False),
    _fused("cleanup10-v15-loop", "cleanup", "default10", 10, "loop1", 15, True),
    _fused("harvest10-v15-loop", "harvest", "default10", 10, "loop1", 15, True),
    # k_inc_encode_any: the looped head half with A = 8 and with precision 1
    _fused("cleanup10-v3-any-loop", "cleanup", "default10", 10, "loop1", 3, True, pipeline="pipeline_any_view", layouts=LUT),
    _fused("harvest10-v3-any-loop", "harvest", "default10", 10, "loop1", 3, True, pipeline="pipeline_any_view", layouts=LUT),
    # k_inc_encode_gather (looped-only kernels): A = 8 and precision 1 of both GENs, on a grid that really loops
    _fused("cleanup10-v3-gen2-loop", "cleanup", "default10", 10, "loop1", 3, True, flags=GEN2, pipeline="pipeline_gathered", layouts=LUT),
    _fused("cleanup10-v3-gen3-loop", "cleanup", "default10", 10, "loop1", 3, True, flags=GEN3, pipeline="pipeline_gathered", layouts=LUT),
    _fused("harvest10-v3-gen2-loop", "harvest", "default10", 10, "loop1", 3, True, flags=GEN2, pipeline="pipeline_gathered", layouts=LUT),
    _fused("harvest10-v3-gen3-loop", "harvest", "default10", 10, "loop1", 3, True, flags=GEN3, pipeline="pipeline_gathered", layouts=LUT),
]


def n_actions(kind):
    return 8 if kind == "harvest" else 9


SHIPPED_WORD = 1 | 2 | 4 | 8 | 32             # the shipped _build_inputs flag set as a flag word


def host_plan(V, flags=SHIPPED_WORD, **keys):
    """plan_rollout (fast_policy.py) over a stand-in controller of 5 agents and 9 actions with window edge V, the shipped input set plus
    the gather bits of the rollout flag word `flags` (64: the others' last actions, 0x100: gathered one-hots) and the config keys `keys`:
    the host tests read the plan's fields without a device."""
    from types import SimpleNamespace
    from homophily_marl_amd.fast_policy import plan_rollout
    n, A, others = 5, 9, bool(flags & 64)
    args = SimpleNamespace(rnn_hidden_dim=64, n_actions=A, obs_dims=(V, V), **keys)
    mac = SimpleNamespace(args=args, n_agents=n, input_shape=32 + A + n + 4 + (n * A if others else 0),
                          input_flags=None if others else SHIPPED_WORD, rollout_input_flags=flags, shipped_flags=not others)
    return plan_rollout(mac)


# ---- dummy arguments of the host refusal tests, and what the GPU tests of the run-time window edges ask of the env -------------------
def dummy_head(flags=None, n=5, A=9, pipe=1):
    """A head's arguments with dummy addresses (non-null, 16-byte aligned, never read): every refusal under test returns from the
    argument checks, a launch would fault.  flags None: the shipped input set without a flag word, every pointer of the dense heads
    set.  Else the explicit flag word `flags` with the gather pointers its bits ask for and `pipe` as pipeline_gather (which asks
    ssd_policy_head_inc_encode for the gathered fused launch); the previous-step pointers the gathered heads do not read stay null."""
    from homophily_marl_amd import abi
    a = abi.SsdPolicyHead()
    P = 1 << 20
    others, gather = abi.INPUT_OTHERS_LAST_ACTION, abi.INPUT_GATHER_ONEHOT
    a.n_env, a.n_agents, a.n_actions, a.pos_scale = 16, n, A, 1.0
    a.input_shape = 32 + A + n + 4 + (n * A if flags is not None and flags & others else 0)
    fields = ("inputs", "h", "weights", "epsilon", "step", "out_actions", "actions", "pos_pre", "orient_pre", "reward", "clean_num", "apple_den")
    if flags is None:
        fields += ("prev_actions", "prev_reward", "prev_actions_inc", "pos")
    else:
        a.input_flags, a.pipeline_gather = abi.INPUT_EXPLICIT | flags, pipe
        if flags & gather:
            a.onehot_rows, a.prev_record = P, P
        elif flags & others:
            a.others_rows, a.prev_record = P, P
    for f in fields:
        setattr(a, f, P)
    return a


def dummy_encode_args(V, layout=None, n=5):
    """The encoder arguments of 16 * n rows at window edge V with dummy addresses (layout None: the class-LUT images)"""
    from homophily_marl_amd import abi
    P = 1 << 20
    ea = abi.SsdPolicyEncodeArgs()
    ea.codes, ea.code_bytes, ea.env_stride, ea.agent_stride = P, 1 << 24, n * V * V, V * V
    ea.rows, ea.view_edge, ea.n_agents, ea.precision, ea.layout = 16 * n, V, n, 2, abi.ENCODE_LAYOUT_LUT if layout is None else layout
    ea.conv_frags, ea.lin_frags, ea.conv_b, ea.lin_b = P, P, P, P
    if 3 <= V <= 63 and V & 1 and abi.encode_bands(V) > 1:
        ea.part = P + (1 << 16)
    else:
        ea.out, ea.out_stride = P + (1 << 16), 64
    return ea


def env_map(kind, n):
    return "default10" if (kind == "harvest" or n == 10) else "default5"


@functools.lru_cache(maxsize=None)
def v_max(kind, mapname, n):
    """The largest view ssd_create accepts for this map and team size (found by creating)."""
    from homophily_marl_amd import abi
    from homophily_marl_amd.envs.native import NativeEnv
    for v in range(31, -1, -1):
        try:
            e = NativeEnv(kind, device=0, map=mapname, num_agents=n, n_env=1, view_size=v)
        except abi.SsdError:
            continue
        e.close()
        return v
    raise AssertionError("no view accepted")


def gen_of(flags, inc):
    """launch_policy_head: GEN 3 = SSD_INPUT_GATHER_ONEHOT, GEN 2 = the others' block gathered, GEN 1 = an env head whose dense flag
    set is not the shipped one, GEN 0 = everything else (the inc head of a GEN 1 set included)"""
    others = bool(flags.get("obs_others_last_action"))
    onehot_blocks = flags.get("obs_last_action", True) or flags.get("obs_agent_id", True) or others
    if flags.get("fused_onehot_gather") and onehot_blocks:
        return 3
    if others and flags.get("fused_others_last_action"):
        return 2
    assert not others, "obs_others_last_action without a gather key does not take the fused heads"
    shipped = all(flags.get(k, True) for k in ("obs_last_action", "obs_agent_id", "obs_reward", "obs_inc_reward", "obs_agent_pos")) \
        and not flags.get("obs_distance", False)
    return 0 if (inc or shipped) else 1


def resolve_n_env(case, cus):
    if isinstance(case.N, int):
        return case.N
    if case.N == "bt5":
        return bt5_size(case.n, cus)
    return looping_size(case.n, int(case.N[-1]), cus)


def standalone_mode(case):
    return MODE_GATHER if gen_of(case.flags, 1) >= 2 else MODE_DENSE


def plans_for(case, cus, N=None):
    """{plan mode: (workgroups per agent, waves, tiles per wave)} of the case on a device of `cus` compute units"""
    N = resolve_n_env(case, cus) if N is None else N
    return {m: head_plan(N, case.n, m, cus) for m in (MODE_DENSE, MODE_FUSED, MODE_GATHER)}


def _b(x):
    return "true" if x else "false"


def head_key(inc, prec, A, gen, looped):
    """head_kernel: GEN 1 exists for the env head and looped only, and serves any grid"""
    assert not (gen == 1 and inc)
    return "k_head<%d,%d,%d,%d,%s>" % (inc, prec, A, gen, _b(looped or gen == 1))


def enc_bt(V, rows):
    return 4 if (V == 15 and rows <= ENC_BT4_MAX_ROWS) else 5


def encode_key(V, prec, rows, lut):
    """launch_policy_encode without the training side output"""
    if lut and V not in (15, 31):
        return "k_encode_lut_any<%d>" % prec
    if lut:
        return "k_encode_lut<%d,%d,%d>" % (V, prec, enc_bt(V, rows))
    return "k_encode<%d,%d,false,%d>" % (V, prec, enc_bt(V, rows))


def pack_encoder_key(V, prec, lut):
    if not lut:
        return "k_pack_encoder<%d,%d>" % (V, prec)
    return "k_pack_encoder_lut<%d,%d>" % (V, prec) if V in (15, 31) else "k_pack_encoder_lut_any<%d>" % prec


def pack_keys(V, prec, gen, lut):
    head = {0: "k_pack_head", 1: "k_pack_head", 2: "k_pack_head_others", 3: "k_pack_head_onehot"}[gen]
    return {"%s<%d>" % (head, prec), pack_encoder_key(V, prec, lut)}


def encode_act_kernels(V, R, prec):
    """the learner's training forward (ops.encode_codes with gradients, V = 15 / 31): launch_policy_encode with `act` on the Toeplitz images"""
    assert V in (15, 31)
    return {"k_encode<%d,%d,true,%d>" % (V, prec, enc_bt(V, R)), pack_encoder_key(V, prec, False)}


def fused_key(prec, A, V, gen, looped, rows, lut):
    """launch_policy_inc_encode / launch_policy_inc_encode_gather"""
    if gen >= 2:
        assert lut
        return "k_inc_encode_gather<%d,%d,%d,true>" % (prec, A, gen)
    if V not in (15, 31):
        assert lut
        return "k_inc_encode_any<%d,%d,%s>" % (prec, A, _b(looped))
    return "k_inc_encode<%d,%d,%d,%s,%d,%s>" % (prec, A, V, _b(looped), enc_bt(V, rows), _b(lut))


def shard_sizes(N):
    """(b): the rows of a looped case as two shards, the first a whole number of 16-row tiles"""
    first = (N // 2 + 15) // 16 * 16
    return first, N - first


def expected_kernels(case, plans):
    """(held, launched): the LEDGER_PREFIXES kernels the case holds to its reference (heads: the torch controller, the precision-2
    heads for precision 1, the unlooped twin for a looped kernel; fused: the two launches, and the torch encoder for the encoder half),
    and every kernel it launches on the way.
    plans: plans_for(case, cus) plus the resolved n_env under "N" -- the dispatch depends on the device through them alone."""
    A, V, rows = n_actions(case.kind), 2 * case.view + 1, plans["N"] * case.n
    held, launched = set(), set()
    gen_env, gen_inc = gen_of(case.flags, 0), gen_of(case.flags, 1)
    mode = standalone_mode(case)
    looped_alone = plans[mode][2] > 1
    for prec in case.precisions:
        for layout in case.layouts:
            lut = layout == "lut"
            packs, enc = pack_keys(V, prec, gen_inc if gen_inc >= 2 else 0, lut), encode_key(V, prec, rows, lut)
            launched |= packs | {enc}
            if case.feat:       # heads: q and the input rows come out of both images; fused: the features out of the encoder's
                held |= (packs if case.test == "heads" else {pack_encoder_key(V, prec, lut)}) | {enc}
            if case.test == "heads":
                keys = {head_key(0, prec, A, gen_env, looped_alone), head_key(1, prec, A, gen_inc, looped_alone)}
                held |= keys
                launched |= keys
                if looped_alone:        # the two shards: the unlooped twins (GEN 1: the same looped-only kernel on a one-tile grid)
                    launched |= {head_key(0, prec, A, gen_env, False), head_key(1, prec, A, gen_inc, False)}
            else:
                key = fused_key(prec, A, V, gen_inc, plans[MODE_FUSED][2] > 1, rows, lut)
                held.add(key)
                launched |= {key, head_key(1, prec, A, gen_inc, looped_alone)}
    return held, launched


def case_kernels(case, cus=LEDGER_CUS):
    plans = dict(plans_for(case, cus), N=resolve_n_env(case, cus))
    return expected_kernels(case, plans)


def two_launch_side(case, cus=LEDGER_CUS):
    """the standalone inc heads a fused case compares with: they must be held by a heads case"""
    N = resolve_n_env(case, cus)
    looped = head_plan(N, case.n, standalone_mode(case), cus)[2] > 1
    return {head_key(1, prec, n_actions(case.kind), gen_of(case.flags, 1), looped) for prec in case.precisions}


# ---- the cases of the older files, read from their own lists -----------------------------------------------------------------------------
def _params(fn):
    """the argument tuples of a function's pytest.mark.parametrize marks, [(names, [values, ...]), ...]"""
    return [(m.args[0], list(m.args[1])) for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]


def existing_cases():
    """Case tuples for the parametrisations of test_policy_mfma.py, test_heads_*.py and test_inc_encode_*.py that hold head or fused
    kernels to a reference (n_env as listed: those files size their cases for 256 compute units)."""
    from tests import test_heads_onehot_gather as oh, test_heads_others_last_action as ot, test_inc_encode_any_view as av
    from tests import test_inc_encode_gathered as ga, test_policy_mfma as pm
    out = []
    map_of = lambda kind, n: "default10" if (kind == "harvest" or n == 10) else "default5"
    (_, rows), = _params(pm.test_fast_policy_matches_torch_controller)
    for fused, N, kind, n, view in rows:
        if fused:
            out.append(Case("mfma-heads", "heads", kind, map_of(kind, n), n, N, view, (2,), SHIPPED, None, LUT, None, 3))
    marks = dict(_params(pm.test_fused_heads_build_every_input_flag_set_that_fits))
    for name in marks["flags"]:
        for kind, N in marks["kind,N"]:
            out.append(Case("mfma-flags", "heads", kind, map_of(kind, 5), 5, N, 7, (2,), pm.FLAG_SETS[name], None, LUT, None, 3))
    for kind, n, N, name in ot.SHAPES:
        out.append(Case("others", "heads", kind, map_of(kind, n), n, N, 7, P21, ot.FLAG_SETS[name], None, LUT, None, 3))
    for kind, map_, n, N, name in oh.SHAPES:
        out.append(Case("onehot", "heads", kind, map_, n, N, 7, P21, oh.FLAG_SETS[name], None, LUT, None, 3))
    (_, rows), = _params(pm.test_inc_encode_launch_equals_the_two_launches)
    for kind, n, view, N in rows:
        out.append(Case("mfma-fused", "fused", kind, map_of(kind, n), n, N, view, (2,), SHIPPED, None, LUT, None, 3, False))
    for kind, n, view, N, prec in av.LAUNCH_CASES:
        if view != "max":                         # the largest view a map takes is found by creating an env: not on the CPU
            out.append(Case("any-view", "fused", kind, env_map(kind, n), n, N, view, (prec,), SHIPPED, "pipeline_any_view", LUT, None, 3, False))
    for kind, map_, n, view, N, prec, flags in ga.LAUNCH_CASES:
        out.append(Case("gathered", "fused", kind, map_, n, N, view, (prec,), flags, "pipeline_gathered", LUT, None, 3, False))
    return out


def existing_encoder_held():
    """the encoder and pack kernels that the older encoder tests hold to the torch encoder, from their own parametrisations:
    test_encoder_matches_the_torch_encoder (FastPolicy.encode, class-LUT layout, precision 2, 2e-6), test_rollout_encoder_at_other_views_
    matches_the_torch_encoder (the run-time-geometry kernel; precision 1 at 203 envs; views 1 .. 3 fit every map), and
    test_encode_codes_op_forward_and_backward_match_torch_autograd (the learner's training forward, precision 2, 1e-5)."""
    from tests import test_encoder_any_view as ev, test_policy_mfma as pm
    held = set()
    (_, rows), = _params(pm.test_encoder_matches_the_torch_encoder)
    for kind, n, view, N in rows:
        held |= {encode_key(2 * view + 1, 2, N * n, True), pack_encoder_key(2 * view + 1, 2, True)}
    marks = dict(_params(ev.test_rollout_encoder_at_other_views_matches_the_torch_encoder))
    for view in marks["view"]:
        if view != "max" and view <= 3:
            for N in marks["N"]:
                for prec in (2, 1) if N == 203 else (2,):
                    held |= {encode_key(2 * view + 1, prec, N * 5, True), pack_encoder_key(2 * view + 1, prec, True)}
    (_, rows), = _params(pm.test_encode_codes_op_forward_and_backward_match_torch_autograd)
    for V, R in rows:
        held |= encode_act_kernels(V, R, 2)
    return held


def existing_held(cus=LEDGER_CUS):
    """the kernels those cases hold.  Their looped cases compare kernel with kernel only where the standalone twin is itself held, and
    precision 1 is held to precision 2 by the bf16 bar; test_bf16_variant_is_close_to_fp32_and_labelled adds the unlooped env head
    (with the precision-1 images and encoder under it)."""
    held = {head_key(0, 1, 9, 0, False), encode_key(15, 1, 1024 * 5, True)} | pack_keys(15, 1, 0, True) | existing_encoder_held()
    for c in existing_cases():
        held |= case_kernels(c, cus)[0]
    return held


def twinless(held):
    """looped standalone heads in `held` whose unlooped twin is not: a looped kernel is pinned to its twin by the two-shard comparison,
    and the twin to the reference (GEN 1 is its own twin: one looped-only kernel serves every grid)"""
    out = []
    for k in held:
        if k.startswith("k_head<"):
            inc, prec, A, gen, loop = k[len("k_head<"):-1].split(",")
            if loop == "true" and gen != "1" and head_key(int(inc), int(prec), int(A), int(gen), False) not in held:
                out.append(k)
    return sorted(out)


# ---- the compiled kernels -----------------------------------------------------------------------------------------------------------
def demangled_key(symbol):
    """_ZN3ssd6k_headILi1ELi2ELi9ELi0ELb1EEEv... -> k_head<1,2,9,0,true>; None for a symbol outside namespace ssd"""
    m = re.match(r"_ZN3ssd(\d+)", symbol)
    if not m:
        return None
    name = symbol[m.end():m.end() + int(m.group(1))]
    rest = symbol[m.end() + int(m.group(1)):]
    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    if not t:
        return name
    args = [("true" if v == "1" else "false") if k == "b" else v for k, v in re.findall(r"L([ib])(\d+)E", t.group(1))]
    return "%s<%s>" % (name, ",".join(args))


def compiled_kernels(isa_path, prefixes=LEDGER_PREFIXES):
    """the keys of every kernel in the code-object metadata (.name entries, names only) whose function name starts with a prefix"""
    text = open(isa_path).read()
    meta = text[text.index("amdhsa.kernels"):]
    keys = set()
    for sym in re.findall(r"^\s+\.name:\s+(\S+)\s*$", meta, flags=re.M):
        key = demangled_key(sym)
        if key and key.startswith(tuple(prefixes)):
            keys.add(key)
    return keys


# ---- the learner's training forward (k_encode<V, PREC, ACT = true, BT>) -------------------------------------------------------------------
# (window edge, rows, precision) of test_learner_forward_encoder_matches_the_float64_encoder: what the older test of ops.encode_codes leaves
# out -- BT = 5 at V = 15 (more than 32768 rows; ragged: 43 rows in the last 80-row group) and precision 1 at every (V, BT)
ENCODE_ACT_CASES = [(15, ENC_BT4_MAX_ROWS + 43, 2), (15, 203, 1), (15, ENC_BT4_MAX_ROWS + 43, 1), (31, 85, 1)]


# ---- kernels no configuration reaches on the devices this project targets ---------------------------------------------------------------
def _unlooped_bt5_at_15_needs_cus():
    """k_inc_encode<*, *, 15, false, 5, *>: BT = 5 at V = 15 needs n_env * n > 32768; the unlooped fused head needs n * ceil(tiles / 7)
    workgroups to fit the chip.  The smallest such grid over every team size (the count grows with n_env)."""
    need = []
    for n in range(1, MAX_AGENTS + 1):
        N = ENC_BT4_MAX_ROWS // n + 1
        tiles = (N + 15) // 16
        need.append(n * ((tiles + FUSED_HEAD_WAVES - 1) // FUSED_HEAD_WAVES))
    return min(need)


UNREACHABLE = {
    "k_inc_encode<%d,%d,15,false,5,%s>" % (prec, A, lut):
        "BT = 5 at V = 15 needs more than 32768 rows, whose unlooped 7-wave head grid needs at least %d compute units (MI355X: 256)" % _unlooped_bt5_at_15_needs_cus()
    for prec in (2, 1) for A in (9, 8) for lut in ("false", "true")
}
