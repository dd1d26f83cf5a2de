"""The hip_graph runner's own choices (runners/hip_graph_runner.py plan_runner) on the CPU: storage path, timesteps per rollout graph,
pipelined or four-launch timestep, start of the exploration draw counter.  Every expected value is worked out by hand from the rule
(the arithmetic is in the comments), over plan_rollout's plans of the stand-in controllers of tests/policy_cases.py."""
from types import SimpleNamespace

import pytest

from homophily_marl_amd import abi
from homophily_marl_amd.runners.hip_graph_runner import plan_runner
from tests.policy_cases import SHIPPED_WORD, host_plan

OTHERS, GATHER = abi.INPUT_OTHERS_LAST_ACTION, abi.INPUT_GATHER_ONEHOT


def _plan(T, plan=None, fmt=abi.OBS_F32, **keys):
    return plan_runner(host_plan(15) if plan is None else plan, SimpleNamespace(**keys), T, fmt)


def test_timesteps_per_graph_and_the_pipelined_timestep():
    # 14 % 10, 14 % 9, 14 % 8 != 0, 14 % 7 == 0: K = 7, odd, so a captured graph cannot alternate the input buffers
    rp = _plan(14, steps_per_graph=10)
    assert rp == (True, True, True, 7, False, 0)
    assert (rp.fast, rp.direct_obs, rp.fold_store, rp.graph_steps, rp.pipe, rp.counter_start) == (True, True, True, 7, False, 0)
    assert _plan(14) == rp                                                      # steps_per_graph defaults to 10
    for spg in (2, 14):
        assert _plan(14, steps_per_graph=spg) == (True, True, True, spg, True, 0), spg
    assert _plan(14, steps_per_graph=0).graph_steps == 1 and not _plan(14, steps_per_graph=0).pipe      # max(1, 0) = 1: odd
    assert _plan(100).graph_steps == 10 and _plan(100).pipe                     # the benched configuration
    # eager timesteps take their parity from t: an odd K does not stand in the way
    assert _plan(14, steps_per_graph=10, rollout_graph=False) == (True, True, True, 7, True, 0)
    assert not _plan(14, steps_per_graph=2, pipeline_encode=False).pipe
    # the store-step launch next to the encoder-fused observation store: never pipelined
    assert _plan(14, steps_per_graph=2, fold_store=False) == (True, True, False, 2, False, 0)
    # no act_inc_encode at this edge without the key: four launches
    assert _plan(14, host_plan(11), steps_per_graph=2) == (True, True, True, 2, False, 0)


@pytest.mark.parametrize("flags", [SHIPPED_WORD | OTHERS, SHIPPED_WORD | GATHER, SHIPPED_WORD | OTHERS | GATHER])
def test_the_previous_action_records_ask_for_an_even_graph(flags):
    for keys in (dict(), dict(pipeline_gathered=True)):
        plan, pipe = host_plan(15, flags, **keys), bool(keys)
        assert plan.needs_prev_rec and plan.inc_encode == pipe
        # T = 14: K = 7 is odd; the even k in 2, 4, 6 that divide 14: 2
        assert _plan(14, plan, steps_per_graph=10) == (True, True, True, 2, pipe, int(pipe))
        # T = 15: 15 % 10 .. 15 % 6 != 0, K = 5; neither 2 nor 4 divides 15: K = 0, eager timesteps (0 % 2 == 0: pipelined with the key)
        assert _plan(15, plan, steps_per_graph=10) == (True, True, True, 0, pipe, int(pipe))
        assert _plan(15, plan, steps_per_graph=10, rollout_graph=False) == (True, True, True, 0, pipe, int(pipe))
        # T = 9, 3 steps per graph: range(2, 3, 2) holds 2 alone, which does not divide 9
        assert _plan(9, plan, steps_per_graph=3).graph_steps == 0
        assert _plan(14, plan, steps_per_graph=14) == (True, True, True, 14, pipe, int(pipe))
        # the generic timestep keeps no records: K stays odd
        assert _plan(14, plan, steps_per_graph=10, fast_policy=False) == (False, False, False, 7, False, 0)


def test_the_draw_counter_starts_at_one_exactly_where_the_pipeline_is_new():
    """pipe and (V not in (15, 31) or needs_prev_rec)"""
    for V in (3, 11, 15, 21, 31, 63):
        for flags in (SHIPPED_WORD, SHIPPED_WORD | OTHERS, SHIPPED_WORD | GATHER):
            plan = host_plan(V, flags, pipeline_any_view=True, pipeline_gathered=True)
            assert plan.inc_encode
            ahead = int(V not in (15, 31) or flags != SHIPPED_WORD)
            assert _plan(14, plan, steps_per_graph=2) == (True, True, True, 2, True, ahead), (V, flags)
            assert _plan(14, plan, steps_per_graph=2, fold_store=False).counter_start == 0
            assert _plan(14, plan, steps_per_graph=2, pipeline_encode=False).counter_start == 0
    assert _plan(14, host_plan(11, pipeline_any_view=True), steps_per_graph=7).counter_start == 0           # K = 7: four launches
    assert _plan(14, host_plan(11, pipeline_any_view=True), steps_per_graph=7, rollout_graph=False).counter_start == 1


def test_storage_formats_and_controllers_the_kernels_do_not_take():
    no_enc = host_plan(16)                                                      # an even edge: the fused heads without the fused encoder
    assert no_enc.supported and no_enc.fused and not no_enc.fused_enc
    assert _plan(14, no_enc, steps_per_graph=2) == (True, False, False, 2, False, 0)
    assert _plan(14, no_enc, steps_per_graph=2, fmt=abi.OBS_CODE) == (False, False, False, 2, False, 0)    # only the fused encoder reads codes
    assert _plan(14, fmt=abi.OBS_CODE, steps_per_graph=2) == (True, True, True, 2, True, 0)
    assert _plan(14, steps_per_graph=2, fast_policy=False) == (False, False, False, 2, False, 0)
    unsupported = SimpleNamespace(**dict(vars(no_enc), supported=False))
    assert _plan(14, unsupported, steps_per_graph=2) == (False, False, False, 2, False, 0)
