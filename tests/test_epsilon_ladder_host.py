"""The per-env epsilon ladder (config key epsilon_ladder_alpha; include/ssd_hip.h: ssd_policy_head.epsilon_rows) without a device: the
exponents epsilon_schedules.ladder_exponents forms, the formula eps ** exponent on the host, run.py's validation, the ABI mirror's field,
and the law of the contract on its restatement (tests/explore_util.py): a row explores iff its 24-bit uniform lies below ITS OWN rate.
The kernels are held to the restatement in tests/test_epsilon_ladder_gpu.py."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from homophily_marl_amd import abi
from homophily_marl_amd.components.epsilon_schedules import ladder_exponents
from tests import explore_util as xu

ALPHAS = (0.5, 7.0)
TOTALS = (1, 2, 48, 4096)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("G", TOTALS)
def test_ladder_exponents_are_the_formula_rounded_to_f32(alpha, G):
    got = ladder_exponents(alpha, 0, G, G)
    assert got.dtype == np.float32 and got.shape == (G,)
    if G == 1:
        assert got.tolist() == [1.0]
        return
    want = np.array([np.float32(1.0 + alpha * g / (G - 1)) for g in range(G)], dtype=np.float32)      # python floats: float64
    assert np.array_equal(got, want)
    assert got[0] == 1.0 and got[-1] == np.float32(1.0 + alpha) and (np.diff(got.astype(np.float64)) > 0).all()


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("G", (2, 48, 4096))
def test_two_shards_hold_the_slices_of_the_unsharded_vector(alpha, G):
    whole = ladder_exponents(alpha, 0, G, G)
    halves = np.concatenate([ladder_exponents(alpha, 0, G // 2, G), ladder_exponents(alpha, G // 2, G - G // 2, G)])
    assert np.array_equal(whole, halves)


def test_ladder_exponents_refuse_envs_outside_the_job():
    for base, n, total in ((0, 0, 4), (3, 2, 4), (-1, 2, 4), (0, 5, 4)):
        with pytest.raises(ValueError):
            ladder_exponents(7.0, base, n, total)


def _rates(eps, alpha, G):
    """the table's values as the contract states them: float64(f32 eps) ** exponent"""
    return np.float64(np.float32(eps)) ** ladder_exponents(alpha, 0, G, G).astype(np.float64)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("G", (2, 48, 4096))
def test_formula_on_the_host(alpha, G):
    for eps in (0.05, 0.3, 0.5, 0.999):
        r = _rates(eps, alpha, G)
        e = float(np.float32(eps))
        assert r[0] == e and math.isclose(r[-1], e ** (1.0 + alpha), rel_tol=1e-12)
        assert (np.diff(r) < 0).all()                                   # strictly decreasing in the env id for 0 < eps < 1
    assert (_rates(1.0, alpha, G) == 1.0).all() and (_rates(0.0, alpha, G) == 0.0).all()
    assert _rates(0.5, alpha, 1).tolist() == [0.5]


# ---- run.py's validation -----------------------------------------------------------------------------------------------------------------
def _args(runner="hip_graph", **keys):
    return SimpleNamespace(runner=runner, **keys)


def test_validation_passes_with_the_key_off_on_any_runner():
    from homophily_marl_amd.run import _check_epsilon_ladder
    for runner in ("hip_graph", "hip_vec", "episode"):
        for keys in ({}, dict(epsilon_ladder_alpha=0), dict(epsilon_ladder_alpha=0.0), dict(epsilon_ladder_alpha=None)):
            for fused in (True, False):
                a = _args(runner, **keys)
                assert _check_epsilon_ladder(a, fused_heads=fused) == 0.0 and a.epsilon_ladder_alpha == 0.0
    a = _args("hip_graph", epsilon_ladder_alpha=7)
    assert _check_epsilon_ladder(a, fused_heads=True) == 7.0 and a.epsilon_ladder_alpha == 7.0


@pytest.mark.parametrize("label,runner,alpha,fused", [("negative", "hip_graph", -0.5, True), ("NaN", "hip_graph", float("nan"), True),
                                                      ("infinite", "hip_graph", float("inf"), True),
                                                      ("negative with the key's runner absent", "hip_vec", -1.0, False),
                                                      ("hip_vec", "hip_vec", 7.0, True), ("episode", "episode", 0.5, True),
                                                      ("generic timestep / per-layer heads", "hip_graph", 7.0, False)])
def test_validation_refuses_by_name(label, runner, alpha, fused):
    from homophily_marl_amd.run import _check_epsilon_ladder
    with pytest.raises(ValueError, match="epsilon_ladder_alpha"):
        _check_epsilon_ladder(_args(runner, epsilon_ladder_alpha=alpha), fused_heads=fused)


def test_default_config_has_the_key_off():
    from homophily_marl_amd.run import load_config
    for kind in ("cleanup", "harvest"):
        assert load_config(kind)["epsilon_ladder_alpha"] == 0.0


# ---- the ABI mirror ---------------------------------------------------------------------------------------------------------------------
def test_policy_head_ends_with_epsilon_rows():
    """(tests/test_abi_layout.py holds the whole struct to the C compiler's layout of include/ssd_hip.h)"""
    name, ctype = abi.SsdPolicyHead._fields_[-1]
    assert name == "epsilon_rows" and ctype is abi.C.c_void_p
    assert abi.SsdPolicyHead().epsilon_rows is None                     # zero = as before
    assert abi.SsdPolicyHead.epsilon_rows.offset % 8 == 0 and abi.SsdPolicyHead.epsilon_rows.offset > abi.SsdPolicyHead.pipeline_gather.offset


# ---- the law of the contract, on the restatement ---------------------------------------------------------------------------------------
def test_each_rate_of_a_table_flags_its_own_share_of_rows():
    """10^6 rows, a table of eight distinct rates dealt to the rows in turn: the flagged share of each rate's rows is within |z| < 4 of
    the rate -- explores(x0, table[:, None]) compares every row with its own entry."""
    R, n = 1_000_000, 2
    rates = np.array([0.0, 0.01, 0.05, 0.2, 0.5, 0.8, 0.97, 1.0], dtype=np.float32)
    table = rates[np.arange(R) % 8]
    x0, _ = xu.draws(0x2545F491, 17, xu.env_keys(R, n, 4096 * 7 + 3))
    flag = xu.explores(x0, table[:, None])
    assert flag.shape == (R, n)
    for k, p in enumerate(rates.astype(np.float64)):
        f = flag[k::8]
        if p in (0.0, 1.0):
            assert f.all() == (p == 1.0) and f.any() == (p == 1.0)
            continue
        z = (int(f.sum()) - f.size * p) / math.sqrt(f.size * p * (1 - p))
        assert abs(z) < 4.0, (k, p, z)
    # a row's flag is its own rate's: the same draws against the table shifted by one rate differ
    assert (flag != xu.explores(x0, np.roll(table, 1)[:, None])).any()
