"""CPU suite: heads shared across agents (config key share_heads; DESIGN sections 4.2 and 7) -- the rule against its numpy restatement,
the two exports' header / table / refusals (dummy pointers, ONLY invalid calls and n_jobs = 0: nothing is launched), the refusals of
run.setup and load_models, the invariant over six train calls of the tensor-op learner, the REFERENCE's own train() with the rule
hooked onto its tied leaves (tests/golden/learner_share_heads.npz, tools/gen_share_heads_golden.py), the logged spreads, two gloo ranks.
Device half: tests/test_share_heads_gpu.py; shared: tests/share_heads_util.py."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

from homophily_marl_amd import abi, run
from homophily_marl_amd.learners import homophily_learner as HL
from tests import motion_util as mu
from tests import share_heads_util as U
from tests import soft_target_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = abi.SSD_ERR_INVALID
F = 1 << 20                      # a dummy device pointer: non-null, 16-byte aligned, never touched


# ---- 1. the rule -------------------------------------------------------------------------------------------------------------------------
def _values(rng, n, inner):
    """normal finite numbers of mixed magnitude with +-0, +-inf and NaN sprinkled in"""
    g = (rng.standard_normal((n, inner)) * 10.0 ** rng.integers(-6, 6, (n, inner))).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    hit = rng.random((n, inner)) < 0.1
    g[hit] = special[rng.integers(0, 5, int(hit.sum()))]
    return g


@pytest.mark.parametrize("n", [2, 3, 10])
def test_rule_equals_its_plain_loop_restatement_to_the_bit(n):
    rng = np.random.default_rng(n)
    for shape in ((1, 1), (7, 5), (59, 64)):
        g = _values(rng, n, shape[0] * shape[1])
        t = th.from_numpy(g.copy()).reshape(1, n, *shape)
        out = HL.tie_agent_grads(t)
        assert out is t                                                       # in place: the gradient is a view of the flat buffer
        want = U.tie_np(g)
        assert U.same_bits(t.numpy().reshape(n, -1), want), (n, shape)
        assert all(U.same_bits(want[i], want[0]) for i in range(n))
    # the order is the stated one: 2^24 + 1 + 1 in f32 is 2^24 from the left and 2^24 + 2 from the right
    g = np.array([[2.0 ** 24], [1.0], [1.0]], np.float32)
    assert HL.tie_agent_grads(th.from_numpy(g.copy()).reshape(1, 3, 1, 1)).reshape(-1).tolist() == [2.0 ** 24] * 3 == U.tie_np(g).reshape(-1).tolist()
    # the sum, not the mean
    assert HL.tie_agent_grads(th.ones(1, 5, 2, 2)).unique().tolist() == [5.0]


def test_spread_rows_are_the_float64_restatement_and_zero_for_equal_copies():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 33)).astype(np.float32)
    rows = HL.spread_rows([th.from_numpy(x).reshape(1, 5, 3, 11), th.from_numpy(x[:1].repeat(5, 0).copy()).reshape(1, 5, 3, 11)])
    want = U.spread_np(x)
    assert rows.dtype == th.float64 and np.allclose(rows[0].numpy(), want, rtol=U.SPREAD_RTOL, atol=0)
    assert float(rows[1, 0]) == 0.0 and float(rows[1, 1]) > 0
    assert HL.spread_rel(rows[1:]) == 0.0 and abs(HL.spread_rel(rows[:1]) - np.sqrt(want[0] / want[1])) <= 1e-12


# ---- 2. the exports: header, table, refusals -----------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssd_hip_tie.h")).read(), flags=re.S)


def test_header_table_and_library_name_the_same_exports():
    names = set(abi.TIE_SIGNATURES)
    assert sorted(set(re.findall(r"\b(ssd_[a-z_0-9]+)\s*\(", _header()))) == sorted(names) == ["ssd_agent_spread", "ssd_tie_agent_grads"]
    assert not names & (set(abi.HIP_SIGNATURES) | set(abi.TRAIN_SIGNATURES) | set(abi.REWARD_SIGNATURES))
    raw, bound = C.CDLL(abi.HIP_LIB_PATH), abi.load_library()
    for name, (res, argtypes) in abi.TIE_SIGNATURES.items():
        assert hasattr(raw, name), name
        assert getattr(bound, name).argtypes == argtypes and getattr(bound, name).restype is res, name
    assert bound.ssd_abi_version() == abi.ABI_VERSION == 10


def test_the_header_compiles_as_c(tmp_path):
    import subprocess
    c = tmp_path / "t.c"
    c.write_text('#include "ssd_hip_tie.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])


def _table(triples):
    return abi.tie_job_table(triples)


OK_TIE = [(6, 5, 7), (50, 2, 3)]                                       # in a buffer of 100 elements
MAXJ, MAXA = abi.ADAM_MAX_JOBS, abi.MAX_AGENTS
TIE_ROWS = [
    ("null flat", dict(flat=None), b"null"), ("null host table", dict(host=None), b"null"), ("null device table", dict(dev=None), b"null"),
    ("n_jobs -1", dict(n=-1), b"n_jobs"), ("n_jobs limit + 1", dict(jobs=[(3 * k, 2, 1) for k in range(MAXJ + 1)], total=1000), b"n_jobs"),
    ("copies 1", dict(jobs=[(6, 1, 7)]), b"copies"), ("copies 11", dict(jobs=[(6, MAXA + 1, 7)]), b"copies"), ("copies 0", dict(jobs=[(6, 0, 7)]), b"copies"),
    ("inner 0", dict(jobs=[(6, 5, 0)]), b"inner"), ("inner negative", dict(jobs=[(6, 5, -4)]), b"inner"),
    ("extent one past total", dict(jobs=[(6, 5, 7), (95, 2, 3)]), b"past total"), ("offset past total", dict(jobs=[(101, 2, 1)]), b"past total"),
    ("negative offset", dict(jobs=[(-2, 2, 1)]), b"past total"), ("extent that overflows", dict(jobs=[(6, 10, 2 ** 62)]), b"past total"),
    ("overlap by one element", dict(jobs=[(6, 5, 7), (40, 2, 3)]), b"overlap"), ("descending jobs", dict(jobs=[(50, 2, 3), (6, 5, 7)]), b"overlap"),
    ("the same job twice", dict(jobs=[(6, 5, 7), (6, 5, 7)]), b"overlap"),
    ("flat at 2 bytes", dict(flat=F + 2), b"4-byte"), ("flat at 1 byte", dict(flat=F + 1), b"4-byte"),
    ("total 0", dict(total=0), b"total"), ("total 2^31", dict(total=2 ** 31), b"total")]


def _tie(flat=F, total=100, jobs=OK_TIE, host=True, dev=F + 4096, n=None):
    lib = abi.load_library()
    table = _table(jobs)
    return lib.ssd_tie_agent_grads(flat, total, table if host is True else host, dev, len(jobs) if n is None else n, None), lib.ssd_last_error()


@pytest.mark.parametrize("label,over,text", TIE_ROWS, ids=[r[0] for r in TIE_ROWS])
def test_tie_entry_point_refuses_before_any_launch(label, over, text):
    rc, msg = _tie(**over)
    assert rc == INV and b"ssd_tie_agent_grads" in msg and text in msg, (label, rc, msg)


def test_no_jobs_is_ok_without_a_launch():
    """n_jobs = 0 returns before a pointer is looked at (the dummy pointers here could not be launched on), from both exports"""
    lib = abi.load_library()
    assert lib.ssd_tie_agent_grads(None, 0, None, None, 0, None) == abi.SSD_OK
    assert lib.ssd_tie_agent_grads(F, 100, None, None, 0, None) == abi.SSD_OK
    assert lib.ssd_agent_spread(None, None, 0, None, None) == abi.SSD_OK


SPREAD_ROWS = [
    ("null host table", dict(host=None), b"null"), ("null device table", dict(dev=None), b"null"), ("null out", dict(out=None), b"null"),
    ("n_jobs -1", dict(n=-1), b"n_jobs"), ("n_jobs limit + 1", dict(jobs=[(F, 2, 1)] * (MAXJ + 1)), b"n_jobs"),
    ("address 0", dict(jobs=[(0, 5, 7)]), b"address"), ("address at 2 bytes", dict(jobs=[(F, 5, 7), (F + 4098, 5, 7)]), b"address"),
    ("copies 1", dict(jobs=[(F, 1, 7)]), b"copies"), ("copies 11", dict(jobs=[(F, MAXA + 1, 7)]), b"copies"),
    ("inner 0", dict(jobs=[(F, 5, 0)]), b"inner"), ("inner past 2^31 / copies", dict(jobs=[(F, 5, 2 ** 31 // 5 + 1)]), b"inner"),
    ("out at 4 bytes, not 8", dict(out=F + 8196), b"8-byte")]


@pytest.mark.parametrize("label,over,text", SPREAD_ROWS, ids=[r[0] for r in SPREAD_ROWS])
def test_spread_entry_point_refuses_before_any_launch(label, over, text):
    kw = dict(dict(jobs=[(F, 5, 7), (F + 4096, 2, 3)], host=True, dev=F + 8192, out=F + 16384, n=None), **over)
    lib = abi.load_library()
    table = _table(kw["jobs"])
    rc = lib.ssd_agent_spread(table if kw["host"] is True else kw["host"], kw["dev"], len(kw["jobs"]) if kw["n"] is None else kw["n"], kw["out"], None)
    msg = lib.ssd_last_error()
    assert rc == INV and b"ssd_agent_spread" in msg and text in msg, (label, rc, msg)


def test_job_table_builder_takes_triples_only():
    t = abi.tie_job_table([(1, 2, 3), (4, 5, 6)])
    assert list(t) == [1, 2, 3, 4, 5, 6] and C.sizeof(t) == 48
    with pytest.raises(ValueError, match="triple"):
        abi.tie_job_table([(1, 2)])


# ---- 2b. run.setup and load_models -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["all", "Both", "", True, 1, ("env",)])
def test_setup_refuses_an_unknown_value(bad):
    cfg = run.load_config("cleanup", overrides=dict(share_heads=bad, use_cuda=False, env_args=dict(num_agents=5, map="default5", episode_limit=12)))
    with pytest.raises(ValueError, match="share_heads"):
        run.setup(cfg)
    with pytest.raises(ValueError, match="share_heads"):
        run._check_share_heads(SimpleNamespace(share_heads=bad, n_agents=5))


@pytest.mark.parametrize("share", ["env", "inc", "both"])
def test_setup_refuses_one_agent(share):
    with pytest.raises(ValueError, match="n_agents"):
        run._check_share_heads(SimpleNamespace(share_heads=share, n_agents=1))
    import inspect
    src = inspect.getsource(run.setup)                                        # ... and setup asks once n_agents is known, before the controller
    assert src.index("args.n_agents, args.n_actions = ") < src.rindex("_check_share_heads(args)") < src.index("mac_REGISTRY[args.mac]")


def test_setup_accepts_the_four_values_and_the_key_absent():
    for v, tags in (("none", ()), ("env", ("env",)), ("inc", ("inc",)), ("both", ("env", "inc"))):
        a = SimpleNamespace(share_heads=v, n_agents=2)
        assert run._check_share_heads(a) == tags and a.share_heads == v
    for a in (SimpleNamespace(n_agents=1), SimpleNamespace(share_heads=None, n_agents=1), SimpleNamespace(share_heads="none", n_agents=1)):
        assert run._check_share_heads(a) == () and a.share_heads == "none"
    assert run.load_config("cleanup")["share_heads"] == "none"


def test_the_controller_starts_every_tied_tensor_from_agent_zero_and_draws_as_before():
    """construction at "both" against "none" from the same seed: agent 0's slices and the encoder equal, every other slice a copy of
    agent 0's, and the generator left where the untied construction leaves it"""
    from tests.learner_util import build, load_fixture
    z, meta = load_fixture("learner_cleanup5.npz")
    z = _Z({k: z[k] for k in z.files if not k.startswith("w_")})              # no stored weights: the controller's own initialisation
    made = {}
    for share in ("none", "both", "env"):
        th.manual_seed(11)
        _, _, mac, learner = build(z, meta, overrides=dict(share_heads=share))
        made[share] = (dict(mac.agent.named_parameters()), th.rand(1).item(), learner)
    for share in ("both", "env"):
        got, after, learner = made[share]
        assert after == made["none"][1]
        tied = dict(learner.mac.agent.tied_parameters())
        assert len(tied) == 18 * len(U.TAGS[share]) and not any(k.startswith("conv_to_fc") for k in tied)
        for k, p in got.items():
            ref = made["none"][0][k]
            if k in tied:
                assert th.equal(p[:, 0], ref[:, 0]) and U.bits_equal_across_agents(p) and not U.bits_equal_across_agents(ref), k
            else:
                assert th.equal(p, ref), k
        assert all(th.equal(a, b) for a, b in zip(learner.target_mac.parameters(), learner.mac.parameters()))


class _Z:
    """an npz-like view of a dict (learner_util.build reads .files and [key])"""

    def __init__(self, d):
        self.d, self.files = d, list(d)

    def __getitem__(self, k):
        return self.d[k]


def _flip_one_bit(t, index):
    t.view(th.int32)[index] ^= 1


def test_load_models_refuses_checkpoints_that_are_not_tied(tmp_path):
    batch, mac, learner, _ = U.fixture_learner("both")
    for k in (1, 2):
        learner.train(batch, 0, k)
    tied_dir, untied_dir, adam_dir = (tmp_path / n for n in ("tied", "untied", "adam"))
    for d in (tied_dir, untied_dir, adam_dir):
        d.mkdir()
    learner.save_models(str(tied_dir))
    before = [p.detach().clone() for p in mac.parameters()]
    # a tied checkpoint loads (n equal copies: the format is the unshared one)
    _, mac2, other, _ = U.fixture_learner("both")
    other.load_models(str(tied_dir))
    assert all(th.equal(a, b) for a, b in zip(before, mac2.parameters()))
    # an unshared run's checkpoint: refused with the key on, taken with the key off
    b0, _, plain, _ = U.fixture_learner("none")
    for k in (1, 2):
        plain.train(b0, 0, k)
    plain.save_models(str(untied_dir))
    kept = [p.detach().clone() for p in mac2.parameters()]
    for share in ("both", "env", "inc"):
        _, m, l, _ = U.fixture_learner(share)
        with pytest.raises(ValueError, match="shared run cannot continue an unshared one"):
            l.load_models(str(untied_dir))
    with pytest.raises(ValueError, match="differs across agents"):
        other.load_models(str(untied_dir))
    assert all(th.equal(a, b) for a, b in zip(kept, mac2.parameters()))        # refused BEFORE anything was loaded
    U.fixture_learner("none")[2].load_models(str(untied_dir))
    # tied parameters, one bit of one agent's Adam moment moved: refused, naming the moment
    for key, fname in (("exp_avg", "opt_env.th"), ("exp_avg_sq", "opt_inc.th")):
        learner.save_models(str(adam_dir))
        sd = th.load(str(adam_dir / fname), weights_only=True)
        idx = len(sd["state"]) - 1                                             # the group's last parameter: a dueling bias of that head
        assert sd["state"][idx][key].shape[:2] == (1, 5)
        _flip_one_bit(sd["state"][idx][key], (0, 3, 0, 0))
        th.save(sd, str(adam_dir / fname))
        with pytest.raises(ValueError, match="Adam %s .*shared run cannot continue an unshared one" % key):
            other.load_models(str(adam_dir))
    # ... which the group that is not tied does not look at
    _, _, env_only, _ = U.fixture_learner("env")
    env_only.load_models(str(adam_dir))                                       # (opt_inc.th's moved moment belongs to an inc tensor)


# ---- 3. the invariant over six calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", ["both", "env", "inc"])
def test_six_train_calls_keep_the_tied_copies_equal_to_the_bit(share):
    batch, mac, learner, seen = U.fixture_learner(share)
    conv0 = [p.detach().clone() for p in mac.agent.conv_to_fc.parameters()]
    for k in range(1, 7):
        learner.train(batch, 0, k)
        U.assert_invariant(mac, learner, U.TAGS[share], "%s call %d" % (share, k))
        for tag in ("env", "inc"):
            assert (U.head_spread_np(mac.agent, tag) == 0.0) == (tag in U.TAGS[share])
    assert not any(th.equal(a, b) for a, b in zip(conv0, mac.agent.conv_to_fc.parameters()))       # the encoder moves, shared as before


def test_key_none_is_the_learner_without_the_key():
    runs = []
    for share in (None, "none"):
        batch, mac, learner, _ = U.fixture_learner(share)
        assert learner.share_tags == () and learner._tied == []
        for k in range(1, 5):
            learner.train(batch, 0, k)
        state = [st[key].clone() for opt in (learner.optimiser_inc, learner.optimiser_env) for p in opt.param_groups[0]["params"]
                 for st in (opt.state[p],) for key in ("step", "exp_avg", "exp_avg_sq")]
        runs.append([p.detach().clone() for p in mac.parameters()] + [p.detach().clone() for p in learner.target_mac.parameters()] + state)
    assert len(runs[0]) == len(runs[1]) > 0 and all(th.equal(a, b) for a, b in zip(*runs))


# ---- 4. the reference's own train() under the rule -----------------------------------------------------------------------------------------
def test_fixture_holds_results_only_and_its_arms_are_apart():
    zs, meta = su.load_fixture("learner_share_heads.npz")
    assert meta["batch"] == "learner_cleanup5.npz" and meta["overrides"] == dict(target_update_interval=2)
    assert not [k for k in zs.files if k.startswith("batch_") or k.startswith("w_")]
    assert int(zs["n_calls"]) == 6 and sorted(meta["arms"]) == ["both_", "bothtau0.25_", "env_", "inc_", "mean_", "none_"]
    sync = su.load_fixture("learner_target_sync.npz")[0]
    for k in range(1, 7):                                                     # the unpatched arm is the reference's plain run
        for key in mu.LOG_KEYS:
            assert float(zs["none_call%d_%s" % (k, key)]) == float(sync["call%d_%s" % (k, key)])
    print("both against none, TD losses:", ["%.1f" % v for v in zs["power_both_vs_none"]])
    print("both against mean, TD losses:", ["%.2f" % v for v in zs["power_both_vs_mean"]], " Adam's first moments:", ["%.0f" % v for v in zs["power_moment_both_vs_mean"]])
    assert zs["power_both_vs_none"][1:].min() >= U.POWER_BARS
    # a mean in place of the sum is invisible to the losses (Adam does not see a gradient's scale) and plain in Adam's moments
    assert zs["power_both_vs_mean"].max() < 1 and zs["power_moment_both_vs_mean"].min() >= U.POWER_BARS
    for arm, tags in (("both", ("env", "inc")), ("env", ("env",)), ("inc", ("inc",)), ("none", ()), ("bothtau0.25", ("env", "inc"))):
        s = zs["spread_" + arm]
        assert s.shape == (6, 2) and all(((s[:, c] == 0.0) == (t in tags)).all() for c, t in enumerate(("env", "inc")))


@pytest.mark.parametrize("share", ["both", "env", "inc", "none"])
def test_six_train_calls_match_the_reference_under_the_rule(share):
    """every call at the golden's bars -- logs, parameter checksums and Adam's first moments (where a mean in place of the sum would
    show: more than 10 bars from the mean arm at every call); from call 2 on the other arms' recordings are missed by more than 10 bars"""
    zs, arm = U.golden(), U.ARMS[share]
    batch, mac, learner, seen = U.fixture_learner(share)
    assert [str(x) for x in zs["param_names"]] == list(mac.agent.state_dict().keys())
    for k in range(1, 7):
        learner.train(batch, 0, k)
        assert len(seen) == k
        su.assert_call(zs, arm, k, seen[-1], mac)
        err, bar = U.moment_error(zs, arm, k, learner)
        print("%s call %d: Adam first moments at %.3f of their bar" % (arm, k, err / bar))
        assert err < bar, (arm, k, err, bar)
        if share == "both":
            miss = U.moment_error(zs, "mean_", k, learner, bars=arm)
            assert miss[0] > U.POWER_BARS * miss[1], (k, miss)
        if k >= 2:
            miss = {o: su.power(zs, arm, o, k, seen[-1], mac) for o in U.ARMS.values() if o != arm}
            print("%s call %d: distance from the other arms in bars %s" % (arm, k, {o: "%.1f" % v for o, v in miss.items()}))
            assert min(miss.values()) > U.POWER_BARS, (k, miss)


def test_tied_heads_under_polyak_updates_match_the_reference():
    zs, arm = U.golden(), "bothtau0.25_"
    batch, mac, learner, seen = U.fixture_learner("both", target_tau=0.25, target_update_interval=1)
    for k in range(1, 7):
        learner.train(batch, 0, k)
        su.assert_call(zs, arm, k, seen[-1], mac)
        U.assert_invariant(mac, learner, U.TAGS["both"], "tau 0.25 call %d" % k)
        assert not any(th.equal(a, b) for a, b in zip(learner.target_mac.parameters(), mac.parameters()))


# ---- the logged spreads --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", ["none", "env", "both"])
def test_head_spreads_are_logged_at_the_float64_value(share):
    batch, mac, learner, _ = U.fixture_learner(share, learner_log_interval=1)
    stats = []
    learner.logger = SimpleNamespace(log_stat=lambda k, v, t: stats.append((k, v, t)), console_logger=None)
    zs = U.golden()
    for k in range(1, 4):
        learner.train(batch, 10 * k, k)
        for col, tag in enumerate(("env", "inc")):
            got = [v for key, v, t in stats if key == "head_spread_" + tag and t == 10 * k]
            want = U.head_spread_np(mac.agent, tag)
            assert len(got) == 1 and isinstance(got[0], float)
            if tag in U.TAGS[share]:
                assert got[0] == 0.0 == want
            else:
                assert want > 0 and abs(got[0] - want) <= U.SPREAD_RTOL * want
                ref = float(zs["spread_%s" % share][k - 1, col])                  # the reference's own parameters after the same call
                assert abs(got[0] - ref) <= mu.SQ_TOL * ref, (k, tag, got[0], ref)        # (a quotient of square sums: param_sq's two-step bar)


# ---- 5. two ranks ------------------------------------------------------------------------------------------------------------------------
def test_two_gloo_ranks_hold_the_same_tied_copies():
    """two ranks on two episodes each against the one-process learner on all four: the tie comes after the all-reduce, so the tied
    copies (asserted by the ranks after every step) and every replica are equal to the bit; the parameters within the bars of
    tests/dp_util.check_lambda_steps (1e-5: param heads absolute, checksums over max(1, |ref|))"""
    from tests.dp_util import bit_equal
    from tests.learner_util import param_checksums
    ranks = U.run_ranks(2, "both")
    assert bit_equal(ranks[0]["flat"], ranks[1]["flat"]) and bit_equal(ranks[0]["grads"], ranks[1]["grads"])
    batch, mac, learner, _ = U.fixture_learner("both")
    off, spans = 0, []
    for name, p in mac.agent.named_parameters():
        if name in dict(mac.agent.tied_parameters()):
            spans.append((off, p.shape[1], p.numel() // p.shape[1]))
        off += p.numel()
    assert len(spans) == 36
    for g in ranks[0]["grads"]:                                               # the gradient both optimisers saw: tied in every tensor
        for o, n, inner in spans:
            block = g[o:o + n * inner].reshape(n, inner)
            assert (block.view(np.uint32) == block[:1].view(np.uint32)).all()
    for step in range(2):
        learner.cal_loss_and_step(batch)
        sums, sqs, heads = param_checksums(mac)
        for r, z in enumerate(ranks):
            e_head = float(np.abs(z["heads"][step] - heads).max())
            e_sum = float((np.abs(z["sums"][step] - sums) / np.maximum(1.0, np.abs(sums))).max())
            e_sq = float((np.abs(z["sqs"][step] - sqs) / np.maximum(1.0, np.abs(sqs))).max())
            print("step %d rank %d: param heads %.3e, checksums %.3e / %.3e (bar 1e-5 each)" % (step, r, e_head, e_sum, e_sq))
            assert e_head < 1e-5 and e_sum <= 1e-5 and e_sq <= 1e-5
