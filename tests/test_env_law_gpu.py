"""GPU suite: the env step kernel's COUNTER-mode draws against the law of the reference (tests/env_law_util.py).

Everything is measured on the device's own exported states and step outputs; no oracle takes part.  The cases hold each instantiation
of the step kernel to the law directly: Cleanup default5 with 5 agents, default10 with 10, default3 with 3 (the run-time team size),
Harvest with 5, and Cleanup default5 stepped through the step-and-observe request with class codes, the instantiation the rollout
launches.  Seeds, N and T are those of tests/test_env_law_host.py (env_law_util.SWEEPS), which asserts the same bars on the CPU oracle
and shows, against a deliberately wrong law, that every one of these samples sees a 3 % error.  |z| < 4 for every binomial count
and every sqrt(R) r; the 0.9999 quantile of chi-square for every table; every statistic is printed next to its bar (pytest -s).
HipEnv.close() asserts that the device error word is 0.

    A, B, F  test_cleanup_sweep        4096 envs (default10: 16384, default3: 32768, what their rarer events take) x 40 steps,
                                       every agent stays, the state re-imported every 8 steps
    C        test_harvest_sweep
    D, F     test_move_contest         16384 envs x 1 step: 2 / 3 / 5 agents into one free cell, at call index 1 and 4
    E        test_spawns               8192 envs x 2 resets under random spawn points and rotations"""
import pytest

from tests import env_law_util as W

pytestmark = pytest.mark.gpu


def _sweep(name):
    from tests.hip_adapter import HipEnv
    env, L, seed, code = W.make_sweep(name, HipEnv)
    try:
        return L, W.sweep_run(env, L, seed, W.EPISODES, W.T_EPISODE, W.EVERY, code)
    finally:
        env.close()


@pytest.mark.parametrize("name", [k for k, v in W.SWEEPS.items() if v[0] == "cleanup"])
def test_cleanup_sweep(name):
    L, run = _sweep(name)
    W.hold_cleanup(name, W.SWEEPS[name][1], L, run)


def test_harvest_sweep():
    L, run = _sweep("harvest5")
    W.hold_harvest("harvest5", L, run)


@pytest.mark.parametrize("k,earlier", W.CONTESTS)
def test_move_contest(k, earlier):
    from tests.hip_adapter import HipEnv
    env, L, seed = W.make_contest(k, earlier, HipEnv)
    try:
        run = W.contest_run(env, L, k, seed, earlier)
    finally:
        env.close()
    W.hold_contest("%d contestants at call %d" % (k, earlier + 1), "default5", L, run, k)


def test_spawns():
    from tests.hip_adapter import HipEnv
    env, L = W.make_spawn(HipEnv)
    try:
        perm, orient = W.spawn_run(env, L)
    finally:
        env.close()
    W.hold_spawns("spawns", perm, orient)
