"""GPU suite: the env step kernel (k_env) against the CPU oracle where the beams of one step meet.

k_env applies the CLEAN beams one shooter after the other, and the next shooter sees the map the earlier ones left.  Random
actions from reset or from clustered positions decide that order in one or two dozen env-steps of the whole suite; the cases here
(tests/beam_util.py) cluster the team within 1 to 3 cells of a waste site and let most of it CLEAN, so that in hundreds of
env-steps per case a later shooter's beam runs over a cell an earlier one cleaned, and every stop reason occurs at every index for
every beam and orientation.  The compile-time team sizes (3 / 5 / 10), the run-time one (2 / 4 / 6 / 7), a walled layout with
pillars inside the waste field, and Harvest (FIRE only) are covered.

COUNTER RNG; the states are imported every second step, so half the steps follow a move.  step_observe and step + observe
alternate, the observation format rotates over the four, and after every call the step outputs, the observation, positions,
orientations and the whole exported state are compared with the oracle; HipEnv.close() asserts that the device error bits are 0.
Each case then asserts its census (beam_util.require), computed from the oracle's side of the run and the tracer alone: a run that
missed a regime fails.  tests/test_env_beams_host.py holds the tracer to the reference's recordings and asserts the same minimums
without a GPU.

In render mode (the REC instantiation: beam_record runs before clean_beams for each shooter) the frame of every env after every
step must equal beam_util.frame_of exactly, and the dynamics must still equal the oracle's."""
import pytest

from tests import beam_util as B
from tests.test_env_domain import _compare_obs, _compare_state, _compare_step

pytestmark = pytest.mark.gpu


def _lockstep(name, **how):
    from oracle.oracle_py import OracleEnv
    from tests.hip_adapter import HipEnv
    dev, orc = B.make_envs(name, HipEnv, OracleEnv, full_colour=how.get("full_colour", False))
    try:
        steps = B.run_case(name, orc, dev, (_compare_step, _compare_obs, _compare_state), **how)
    finally:
        dev.close(); orc.close()
    return B.require(name, B.beam_census(B.CASES[name].the_layout(), steps))


@pytest.mark.parametrize("name", list(B.CASES))
def test_beams_in_lockstep_with_the_oracle(name):
    print(name, _lockstep(name))


@pytest.mark.parametrize("name", B.RENDER_CASES)
def test_render_mode_frames_and_dynamics(name):
    print(name, _lockstep(name, render=True))


def test_full_colour_observations():
    """obs_color: full -- the observation kernels the rollout does not take by default (no class codes: three formats)"""
    print(B.FULL_COLOUR_CASE, _lockstep(B.FULL_COLOUR_CASE, full_colour=True))
