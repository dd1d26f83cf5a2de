"""tests/arena_util.py on a CPU arena: a correct run passes check(), and every way a bounds case can go wrong -- a write one byte past a
reserved output, a read-through of one poisoned f32, ... -- is reported (the GPU cases of tests/test_learner_kernel_bounds.py can fail)."""
import re

import numpy as np
import pytest

from tests import arena_util


def test_a_clean_case_passes_and_the_fills_are_in_place():
    a, x, ids, y, raw, yv, xv = arena_util.selftest_case()
    a.check()
    assert np.array_equal(y.array()[:, :3], (np.arange(8, dtype=np.float32) * 2).reshape(2, 4)[:, :3])
    assert np.isnan(xv[0]) and np.isnan(xv[9])                                      # NaN on either side of the f32 operand
    assert raw[ids.start - 8:ids.start].view(np.int64)[0] == 7 and raw[ids.start + ids.nbytes:][:8].view(np.int64)[0] == 7


@pytest.mark.parametrize("fault", sorted(arena_util.SELFTEST_FAULTS))
def test_check_reports(fault):
    mutate, text = arena_util.SELFTEST_FAULTS[fault]
    case = arena_util.selftest_case()
    mutate(*case)
    with pytest.raises(arena_util.ArenaError, match=re.escape(text)):
        case[0].check()
