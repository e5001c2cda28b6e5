"""walker_gym_amd.ranges: the pure split functions behind BatchedPhysicsEnv's walker ranges, against values computed
with the formulas they replaced (the three copies of the uniform split, the two of the plan-block split, and the body of
BatchedPhysicsEnv._caller_bounds).  No GPU, no library."""
import numpy as np
import pytest

from walker_gym_amd.ranges import block_bounds, caller_bounds, uniform_bounds

PLAN = np.arange(0, 18, 2, dtype=np.int32)   # 8 blocks of two stored walkers
ROW_A = np.array([3, 0, 2, 1, 4, 5, 7, 6, 9, 8, 10, 11, 12, 15, 14, 13])
ROW_B = np.array([0, 1, 2, 3, 4, 5, 7, 9, 6, 8, 10, 11, 12, 13, 14, 15])


@pytest.mark.parametrize("args,expected", [((130, 2), [0, 128, 130]),          # a two-walker last range
                                           ((200, 3), [0, 128, 192, 200]),
                                           ((128, 2), [0, 64, 128]),
                                           ((1000, 3), [0, 384, 704, 1000]),
                                           ((65536, 2), [0, 32768, 65536])])
def test_uniform_bounds(args, expected):
    assert uniform_bounds(*args) == expected


@pytest.mark.parametrize("args,expected", [((130, 2), [0, 65, 130]), ((193, 3), [0, 64, 128, 193])])
def test_block_bounds(args, expected):
    assert block_bounds(*args) == expected


@pytest.mark.parametrize("lanes,bounds,contiguous", [
    (1, [0, 8], [True]),
    (2, [0, 4, 8], [True, True]),
    (3, [0, 2, 5, 8], [True, True, True]),
    (4, [0, 2, 4, 6, 8], [True] * 4),
    (8, list(range(9)), [False, False, True, True, True, True, False, False])])
def test_caller_bounds_first_row_order(lanes, bounds, contiguous):
    assert caller_bounds(8, PLAN, ROW_A, lanes) == (bounds, contiguous)


def test_caller_bounds_identity_order():
    assert caller_bounds(8, PLAN, None, 3) == ([0, 2, 5, 8], [True, True, True])


def test_caller_bounds_moves_a_split_off_a_bad_block():
    """Block 4 (stored walkers 0..7) holds caller rows 7 and 9 but not 6: the even split is no good block, so it moves
    to block 3, after which the stored prefix is caller rows 0..5."""
    assert caller_bounds(8, PLAN, ROW_B, 2) == ([0, 3, 8], [True, True])
