"""Goal pool, the checks that need no GPU: the restated row rule, the Python helpers' argument checks, the new
symbols of include/roboy_sim.h in the library, and the input qualification of tests/test_goal_pool_gpu.py's settle test - on its
exact seeds and sizes the C oracle alone, in fp32 and in fp64, must take (almost) the same keep decisions and land on the same
poses, or a GPU-against-fp64 comparison of those decisions would test the inputs' conditioning and not the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

import goal_pool_util as gp
from gym_roboy_amd import _native as nat
from gym_roboy_amd.envs.goals import GoalPool, default_settle_tol, goal_rows, settle_batch_size, settle_setpoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()


def test_restated_row_rule():
    ids = np.arange(4096)
    for m in (1, 7, 16384, 2**32 - 1):
        for draw in range(4):
            k = gp.pool_row(3, ids, draw, m)
            assert k.min() >= 0 and k.max() < m
    assert not gp.pool_row(3, ids, 0, 1).any()
    used = np.concatenate([gp.pool_row(3, ids, draw, 7) for draw in range(4)])
    assert np.array_equal(np.unique(used), np.arange(7))
    counts = np.bincount(used, minlength=7)                     # 16 384 draws over 7 rows: 2 341 each, sigma 45
    assert np.abs(counts - len(used) / 7).max() < 5 * 45
    # a per-env draw number gives what the scalar form gives, and the stream is its own (not the box goals')
    draws = (ids % 4).astype(np.uint32)
    k = gp.pool_row(3, ids, draws, 7)
    for d in range(4):
        assert np.array_equal(k[draws == d], gp.pool_row(3, ids[draws == d], d, 7))
    from oracle import philox_np as ph
    assert not np.array_equal(ph.draw(3, ids.astype(np.uint64), 0, ph.STREAM_GOALS, 0), ph.draw(3, ids.astype(np.uint64), 0, gp.STREAM_GOAL_POOL, 0))
    assert "STREAM_GOAL_POOL = %d" % gp.STREAM_GOAL_POOL in open(os.path.join(ROOT, "gym_roboy_amd", "csrc", "philox.hpp")).read()


def test_python_helpers_check_their_arguments():
    lo, hi = np.full(3, -np.pi, np.float32), np.full(3, np.pi, np.float32)
    good = np.float32([[0.1, 0.2, 0.3], [0.0, -0.4, 0.5]])
    rows = goal_rows(good, 3, lo, hi)
    assert rows.dtype == np.float32 and rows.flags["C_CONTIGUOUS"] and np.array_equal(rows, good)
    assert np.array_equal(goal_rows(GoalPool(good, {"m": 2}), 3, lo, hi, m=2), good)
    assert np.array_equal(goal_rows(good.astype(np.float64)[:, ::1], 3, lo, hi), good)
    for bad in (good[0], good[:, :2], good[None], np.zeros((0, 3), np.float32)):              # wrong shape
        with pytest.raises(ValueError, match="shape"):
            goal_rows(bad, 3, lo, hi)
    nan = good.copy(); nan[1, 2] = np.nan
    inf = good.copy(); inf[0, 0] = np.inf
    for bad in (nan, inf):
        with pytest.raises(ValueError, match="finite"):
            goal_rows(bad, 3, lo, hi)
    out = good.copy(); out[1, 1] = -3.2
    with pytest.raises(ValueError, match="angle box"):
        goal_rows(out, 3, lo, hi)
    with pytest.raises(ValueError, match="2 rows"):                                           # a second size
        goal_rows(np.zeros((3, 3), np.float32), 3, lo, hi, m=2)
    with pytest.raises(ValueError):
        GoalPool(good[0])
    pool = GoalPool(good.astype(np.float64), {"seed": 1})
    assert pool.q.dtype == np.float32 and len(pool) == 2 and pool.recipe == {"seed": 1}


def test_recipe_helpers_are_what_the_tests_restate():
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    for robot, m in ((MsjRobot(), 256), (UpperBodyRobot(), 64), (MsjRobot(), 1), (MsjRobot(), 129)):
        n = settle_batch_size(m)
        assert n == gp.batch_envs(m) and n % 256 == 0 and n >= 2 * m and n - 2 * m < 256
        assert np.array_equal(settle_setpoints(robot, 5, 1, n), gp.setpoints(robot, 5, 1, n))
        assert default_settle_tol(robot) == pytest.approx(gp.vel_tol(robot) / 20, rel=1e-6)
    assert default_settle_tol(MsjRobot()) == pytest.approx(0.018, abs=5e-4)                   # DESIGN.md §22's table
    assert default_settle_tol(UpperBodyRobot()) == pytest.approx(0.047, abs=5e-4)


def test_header_symbols_are_in_the_library():
    names = ("rb_env_goal_pool_set", "rb_env_goal_pool_ptr")
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert re.search(r"\bint %s\(rb_sim \*sim" % name, HEADER), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
    assert int(re.search(r"#define RB_ABI_VERSION (\d+)", HEADER).group(1)) == 6 == nat.load().rb_abi_version()
    # without a handle the calls fail with a code and a message
    lib.rb_env_goal_pool_set.argtypes = nat.SIGNATURES["rb_env_goal_pool_set"][1]
    assert lib.rb_env_goal_pool_set(None, None, 1) == nat.RB_EINVAL


def test_train_parallel_goals_argument():
    from gym_roboy_amd.train_parallel import DEFAULT_GOAL_POOL, parse_goals
    assert parse_goals("") == 0 and parse_goals("reachable") == DEFAULT_GOAL_POOL == 16384 and parse_goals("reachable:512") == 512
    for bad in ("box", "reachable:0", "reachable:x", "reachable:-4"):
        with pytest.raises(SystemExit):
            parse_goals(bad)


@pytest.mark.parametrize("case", sorted(gp.SETTLE_CASES))
def test_settle_inputs_decide_the_same_in_fp32_and_fp64(case):
    """The cap is a condition on the inputs, not a measurement of the kernels: keep decisions of the fp32 and the fp64 C oracle differ
    in at most 1 % of the batch, and rows both keep differ by less than goal_angle_tol / 4 (as an L2 distance, the norm the tolerance
    is defined in)."""
    make, m, _, _ = gp.SETTLE_CASES[case]
    robot = make()
    q32, _, keep32 = gp.settled(case, "f32")
    q64, _, keep64 = gp.settled(case, "f64")
    n = gp.batch_envs(m)
    assert len(keep64) == n
    differ = int(np.sum(keep32 != keep64))
    both = keep32 & keep64
    worst = float(np.linalg.norm(q32[both].astype(np.float64) - q64[both], axis=1).max())
    print("%s: kept %d / %d of %d (fp32 / fp64), decisions differ in %d, largest pose difference %.3g (bound %.3g)"
          % (case, keep32.sum(), keep64.sum(), n, differ, worst, gp.angle_tol(robot) / 4))
    assert differ <= n // 100
    assert worst < gp.angle_tol(robot) / 4
    assert keep64.sum() >= m                                     # batch 0 alone fills the pool: the GPU test reads no second batch
    desc = robot.get_description()
    assert np.all(q64[keep64] >= desc.q_lo) and np.all(q64[keep64] <= desc.q_hi)
