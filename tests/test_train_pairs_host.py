"""CPU: what the paired forward exports of the train step refuse ("ssd_bias_bmm_pair_fwd", "ssd_dueling_head_pair_fwd": the layer, and the
dueling combination, of the learner's live and target net in one launch), and the row assembly in front of fc1 ("ssd_fc1_rows_fwd",
"ssd_fc1_rows_bwd") -- the exports of include/ssd_hip_train.h, abi.TRAIN_SIGNATURES.  Dummy pointers, ONLY invalid calls: every argument check runs
before any launch, the baselines themselves are never called (the form of the refusal tables of tests/test_kernel_ledger_host.py)."""
import os
import re

import pytest

from homophily_marl_amd import abi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

INV, UNS = abi.SSD_ERR_INVALID, abi.SSD_ERR_UNSUPPORTED
F = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched

# x_a, x2_a, w_a, b_a, y_a, n_a, x_b, x2_b, w_b, b_b, y_b, n_b, rows, in1, in2, out, x1_div, x2_shared, leaky, stream
ONE = [F, None, F, F, F, 5, F, None, F, F, F, 5, 100, 64, 0, 192, 1, 0, 0, None]          # one source per row (fc1, the GRU projections)
TWO = [F, F, F, F, F, 5, F, F, F, F, F, 5, 100, 64, 16, 4, 5, 1, 0, None]                 # two-source rows (the incentive head's layer)
PAIR_ROWS = [("ssd_bias_bmm_pair_fwd", base, "%s: %s" % (tag, label), change, expect, message) for tag, base, rows in (
    ("one source", ONE, [("null argument %d" % k, {k: None}, INV, b"null operand") for k in (0, 2, 3, 4, 6, 8, 9, 10)] + [
        ("n_a 0", {5: 0}, INV, b"set count"), ("n_b 0: a second group without a set count", {11: 0}, INV, b"set count"), ("n_b < 0", {11: -1}, INV, b"set count"),
        ("rows 0", {12: 0}, INV, b""), ("in1 0", {13: 0}, INV, b""), ("in2 < 0", {14: -1}, INV, b""), ("out 0", {15: 0}, INV, b""),
        ("a second source of group a without in2", {1: F}, INV, b"second source"), ("a second source of group b without in2", {7: F}, INV, b"second source"),
        ("65536 weight sets", {5: 65535, 11: 1}, UNS, b"65535"), ("in * out = 2^30", {13: 1 << 15, 15: 1 << 15}, UNS, b"2^30"),
        ("rows * in = 2^30", {12: 1 << 20, 13: 1 << 10}, UNS, b"2^30")]),
    ("two sources", TWO, [("null argument %d" % k, {k: None}, INV, b"") for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)] + [
        ("n_a 0", {5: 0}, INV, b"set count"), ("n_b 0: a second group without a set count", {11: 0}, INV, b"set count"),
        ("in2 without the second source of group b", {7: None}, INV, b"second source"), ("x1_div 0", {16: 0}, INV, b"x1_div"), ("x1_div < 0", {16: -1}, INV, b"x1_div"),
        ("rows % x1_div", {12: 101}, INV, b"x1_div"),
        # 16-byte row loads (in2 a multiple of 4) pick the source per 16-column chunk: in1 must then be whole chunks
        ("in1 % 16 with in2 % 4 == 0", {13: 50, 14: 12}, INV, b"multiple of 16"), ("rows * in = 2^30", {12: 5 << 18, 13: 1 << 10, 14: 1 << 10}, UNS, b"2^30")]))
    for label, change, expect, message in rows]

# y_a, q_a, n_a, y_b, q_b, n_b, T, B, inner, K, stream
DUEL = [F, F, 5, F, F, 5, 7, 4, 1, 9, None]
DUEL_ROWS = [("ssd_dueling_head_pair_fwd", DUEL, label, change, expect, message) for label, change, expect, message in
             [("null argument %d" % k, {k: None}, INV, b"null operand") for k in (0, 1, 3, 4)] + [
                 ("n_a 0", {2: 0}, INV, b"set count"), ("n_b 0: a second group without a set count", {5: 0}, INV, b"set count"),
                 ("T 0", {6: 0}, INV, b""), ("B 0", {7: 0}, INV, b""), ("inner 0", {8: 0}, INV, b""), ("K 0", {9: 0}, INV, b""), ("K = limit + 1", {9: 16}, INV, b"")]]
# feat_a, feat_b, tail, act, x_env_a, x_inc_a, x_env_b, x_inc_b, B, T, n, feat_w, tail_w, act_w, stream
ROWS_FWD = [F, F, F, F, F, F, F, F, 2, 5, 5, 32, 18, 9, None]
# d_x_env, d_x_inc, d_feat, B, T, n, feat_w, tail_w, act_w, d_feat_stride, stream
ROWS_BWD = [F, F, F, 2, 5, 5, 32, 18, 9, 50, None]
FC1_ROWS = [("ssd_fc1_rows_fwd", ROWS_FWD, label, change, expect, message) for label, change, expect, message in
            [("null argument %d" % k, {k: None}, INV, b"first net") for k in (0, 3, 4, 5)] + [
                ("second net: features without outputs", {6: None, 7: None}, INV, b"come together"), ("second net: one output missing", {7: None}, INV, b"come together"),
                ("second net: outputs without features", {1: None}, INV, b"come together"), ("tail_w without tail", {2: None}, INV, b"tail_w"),
                ("tail without tail_w", {12: 0}, INV, b"tail_w"), ("B 0", {8: 0}, INV, b""), ("T 0", {9: 0}, INV, b""), ("n 0", {10: 0}, INV, b""),
                ("feat_w 0", {11: 0}, INV, b""), ("tail_w < 0", {12: -1}, INV, b""), ("act_w 0", {13: 0}, INV, b""),
                ("2^40 elements", {8: 1 << 20, 9: 1 << 10, 10: 1 << 5, 11: 1 << 5}, UNS, b"2^40")]] + [
           ("ssd_fc1_rows_bwd", ROWS_BWD, label, change, expect, message) for label, change, expect, message in
           [("null argument %d" % k, {k: None}, INV, b"null operand") for k in (0, 1, 2)] + [
               ("B 0", {3: 0}, INV, b""), ("T 0", {4: 0}, INV, b""), ("n 0", {5: 0}, INV, b""), ("feat_w 0", {6: 0}, INV, b""), ("tail_w < 0", {7: -1}, INV, b""),
               ("act_w 0", {8: 0}, INV, b""), ("d_feat_stride below feat_w", {9: 31}, INV, b"d_feat_stride"), ("2^40 elements", {3: 1 << 20, 4: 1 << 10, 5: 1 << 5, 6: 1 << 5}, UNS, b"2^40")]]
REFUSALS = PAIR_ROWS + DUEL_ROWS + FC1_ROWS


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


def _declared():
    """the functions include/ssd_hip_train.h declares (comments stripped), as tests/test_abi_symbols.py reads ssd_hip.h"""
    src = open(os.path.join(ROOT, "include", "ssd_hip_train.h")).read()
    return sorted(set(re.findall(r"\b(ssd_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))


def test_header_table_library_and_refusal_tables_name_the_same_exports():
    """what tests/test_abi_symbols.py and tests/test_learner_abi_refusals.py hold for include/ssd_hip.h and abi.HIP_SIGNATURES, for the
    train step's header and table: the header's declarations are the table, the library exports and binds each as the table says, no
    name is in both tables, and every export has a refusal table above"""
    import ctypes
    names = set(abi.TRAIN_SIGNATURES)
    assert _declared() == sorted(names) and not names & set(abi.HIP_SIGNATURES)
    assert {r[0] for r in REFUSALS} == names
    raw, bound = ctypes.CDLL(abi.HIP_LIB_PATH), abi.load_library()
    for name, (res, argtypes) in abi.TRAIN_SIGNATURES.items():
        assert hasattr(raw, name), name
        assert getattr(bound, name).argtypes == argtypes and getattr(bound, name).restype is res, name
    sig = lambda k: len(abi.TRAIN_SIGNATURES[k][1])
    assert sig("ssd_fc1_rows_fwd") == len(ROWS_FWD) and sig("ssd_fc1_rows_bwd") == len(ROWS_BWD)
    assert sig("ssd_bias_bmm_pair_fwd") == len(ONE) == len(TWO) and sig("ssd_dueling_head_pair_fwd") == len(DUEL)
    assert bound.ssd_abi_version() == abi.ABI_VERSION == 10


def test_the_header_compiles_as_c(tmp_path):
    import subprocess
    c = tmp_path / "t.c"
    c.write_text('#include "ssd_hip_train.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])
