"""GPU suite: the env step kernel (k_env) against the CPU oracle from states a rollout that starts at reset never reaches.

Every other comparison of k_env starts at reset and takes at most 100 random steps, which keeps the waste count near n_waste, the
orchard dense and the one-step change of the apple count within [-4, +20].  The cases here import swept grids (every waste count
0..n_waste, every Harvest apple count), run layouts with 256 waste sites and no apple site (or the reverse), and override rule
constants, so that the device reads every entry of its probability table -- from the prefetched lane window on a step that carries
its counts, from global memory on the step after an import -- takes both out-of-window branches of the apple-density lookup, draws
past the first 64 free waste sites, ends a draw loop without a success, and selects the (J + 1)-th smallest site for J up to 255.

COUNTER RNG.  After every call the step outputs, the observation (the format rotating over the four), positions, orientations
and the whole exported state are compared with the oracle; HipEnv.close() asserts that the device error bits are 0.  Each case
then asserts its census (tests/env_state_util.require), computed from the oracle's side of the same run: a run that did not reach
its regime fails.  tests/test_env_states_host.py asserts the same minimums without a GPU.

The cases with overridden rule constants (waste_draw_index, p_waste_*, p_apple_*, harvest_p_0101) and with custom layouts have no
counterpart in the reference: they pin the device to the oracle only.  The oracle itself is pinned to the reference in these
regimes by oracle/check_vs_reference.py --warm and the warm golden trajectories (tests/golden/traj_*_{warm,clean,empty,sparse}.npz),
which test_hip_parity replays through the kernel's TAPE instantiation."""
import pytest

from tests import env_state_util as U
from tests.test_env_domain import _compare_obs, _compare_state, _compare_step

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(U.CASES))
def test_states_past_a_reset_rollout(name):
    from oracle.oracle_py import OracleEnv
    from tests.hip_adapter import HipEnv
    dev, orc = U.make_envs(name, HipEnv, OracleEnv)
    try:
        cen = U.run_case(name, orc, dev, (_compare_step, _compare_obs, _compare_state))
    finally:
        dev.close(); orc.close()
    print(name, U.require(name, cen))
