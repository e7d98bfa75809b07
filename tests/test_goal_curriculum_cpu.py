"""Goal curriculum, the checks that need no GPU: the window, the row and the level rule of csrc/env_goal.hpp compiled
into a stand-alone host program and compared, output for output, with the numpy restatement of tests/goal_curriculum_util.py; the
restatement's own properties; GoalPool.ordered; the Python helpers' argument checks, the CLI parse helper and the new symbols of
include/roboy_sim.h in the library."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import goal_curriculum_util as gc
import goal_pool_util as gp
from gym_roboy_amd import _native as nat
from gym_roboy_amd.envs.goals import GoalPool, goal_curriculum_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from build_dir import build_dir  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()
CSRC = os.path.join(ROOT, "gym_roboy_amd", "csrc")

SIZES = (1, 7, 256, 16384, 2**31 + 5)
UP_DOWN = (0, 1, 3)
# (seed, global env id, draw): ids and draws across 2^32
DRAWS = ((0, 0, 0), (3, 1, 1), (3, 1000, 2**31), (2**63 + 11, 2**32 - 1, 2**32 - 1), (7, 2**32, 5), (7, 2**40 + 3, 2**32 - 2))


def levels_of(m):
    return sorted({n_levels for n_levels in (1, 2, 7, min(m, 256)) if n_levels <= min(m, 256)})


def grid():
    """rows (m, L, l, reached, up, down, seed, gid, draw): every level where L <= 7, the edges and the middle otherwise"""
    rows = []
    for m in SIZES:
        for n_levels in levels_of(m):
            levels = range(n_levels) if n_levels <= 7 else sorted({0, 1, n_levels // 2, n_levels - 4, n_levels - 2, n_levels - 1})
            for level in levels:
                for reached in (0, 1):
                    for up in UP_DOWN:
                        for down in UP_DOWN:
                            for seed, gid, draw in DRAWS:
                                rows.append((m, n_levels, level, reached, up, down, seed, gid, draw))
    return rows


@pytest.fixture(scope="module")
def host_program():
    exe = os.path.join(build_dir(), "goal_curriculum_host")
    src = os.path.join(ROOT, "tests", "hostmath", "goal_curriculum_host.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("env_goal.hpp", "philox.hpp", "rtc_compat.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, src])
    return exe


def test_host_program_equals_the_restatement(host_program):
    rows = grid()
    assert {r[0] for r in rows} == set(SIZES) and {r[1] for r in rows if r[0] == 16384} == {1, 2, 7, 256}
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    out = subprocess.run([host_program], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)
    assert got.shape == (len(rows), 3)
    want = np.empty_like(got)
    for i, (m, n_levels, level, reached, up, down, seed, gid, draw) in enumerate(rows):
        want[i, 0] = gc.hi(level, m, n_levels)
        want[i, 1] = gc.row(seed, np.array([gid], dtype=np.uint64), draw, level, m, n_levels)[0]
        want[i, 2] = gc.next_level(level, reached, up, down, n_levels)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "host program off the restatement in %d of %d rows, first %r: %r, restated %r" % (
        bad.size, len(rows), rows[bad[0]], got[bad[0]], want[bad[0]])
    assert (got[:, 1] < got[:, 0]).all()                        # every row inside its window


def test_window_properties():
    for m in SIZES + (2, 255, 257, 2**32 - 1):
        for n_levels in sorted(set(levels_of(m)) | {min(m, 3), min(m, 255)}):
            h = gc.hi(np.arange(n_levels), m, n_levels)
            assert h[0] >= 1 and h[-1] == m and np.all(np.diff(h) >= 0), (m, n_levels)
            assert h[0] == m // n_levels


def test_top_level_row_is_the_pool_row():
    ids = np.arange(4096) + 2**32 - 2048
    for m in (1, 7, 256, 16384, 2**31 + 5):
        for n_levels in levels_of(m):
            for draw in (0, 1, 2**32 - 1):
                assert np.array_equal(gc.row(5, ids, draw, n_levels - 1, m, n_levels), gp.pool_row(5, ids, draw, m))
    # below the top the rows stay inside the window, and a per-env level gives what the scalar form gives
    level = ids % 7
    k = gc.row(5, ids, 2, level, 16384, 7)
    assert np.all(k < gc.hi(level, 16384, 7))
    for lv in range(7):
        assert np.array_equal(k[level == lv], gc.row(5, ids[level == lv], 2, lv, 16384, 7))
    assert not gc.row(5, ids, 0, 0, 7, 7).any()                 # hi(0) = 1: row 0 only


def test_level_rule():
    lv = np.arange(8)
    assert np.array_equal(gc.next_level(lv, True, 1, 1, 8), [1, 2, 3, 4, 5, 6, 7, 7])
    assert np.array_equal(gc.next_level(lv, False, 1, 1, 8), [0, 0, 1, 2, 3, 4, 5, 6])
    assert np.array_equal(gc.next_level(lv, True, 3, 0, 8), [3, 4, 5, 6, 7, 7, 7, 7])
    assert np.array_equal(gc.next_level(lv, False, 0, 3, 8), [0, 0, 0, 0, 1, 2, 3, 4])
    assert np.array_equal(gc.next_level(lv, lv % 2 == 0, 0, 0, 8), lv)
    assert np.array_equal(gc.next_level([0], [True], 5, 5, 1), [0])


def test_goal_pool_ordered():
    rng = np.random.default_rng(0)
    q = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    q[10] = q[3]                                                # ties: an equal row, and another row at the same distance
    q[20] = -q[3]
    source = np.stack((np.arange(64) // 32, np.arange(64)), axis=1)
    pool = GoalPool(q, {"m": 64, "seed": 0}, source)
    ordered = pool.ordered()
    assert ordered is not pool and np.array_equal(pool.q, q) and "ordered" not in pool.recipe
    assert ordered.recipe == {"m": 64, "seed": 0, "ordered": "rest_distance"}
    order = ordered.source[:, 1]                                # the source column carries the permutation
    assert np.array_equal(np.sort(order), np.arange(64))
    assert np.array_equal(ordered.q, q[order]) and np.array_equal(ordered.source, source[order])
    d = np.sqrt(np.sum(np.square(ordered.q.astype(np.float64)), axis=1))
    assert np.all(np.diff(d) >= 0)
    tied = [int(np.nonzero(order == i)[0][0]) for i in (3, 10, 20)]
    assert tied == sorted(tied) and tied[-1] - tied[0] == 2    # equal distance: adjacent, in pool order
    assert np.array_equal(ordered.ordered().q, ordered.q)
    assert GoalPool(q).ordered().source is None
    with pytest.raises(ValueError, match="rest_distance"):
        pool.ordered("volume")


def test_python_helpers_check_their_arguments():
    assert goal_curriculum_spec(None) is None
    assert goal_curriculum_spec(8) == {"levels": 8, "up": 1, "down": 1, "start": 0}
    assert goal_curriculum_spec(np.int64(8), m=8) == {"levels": 8, "up": 1, "down": 1, "start": 0}
    assert goal_curriculum_spec({"levels": 4, "up": 2, "down": 0, "start": 3}) == {"levels": 4, "up": 2, "down": 0, "start": 3}
    assert goal_curriculum_spec(256)["levels"] == 256 and goal_curriculum_spec(1, m=1)["levels"] == 1
    for bad in (0, -1, 257, True, 2.0, "8", {"up": 1}, {"levels": 4, "rate": 1}, {"levels": 4, "up": -1}, {"levels": 4, "down": -1},
                {"levels": 4, "start": 4}, {"levels": 4, "start": -1}, {"levels": 4.0}, (4, 1, 1)):
        with pytest.raises(ValueError, match="goal_curriculum"):
            goal_curriculum_spec(bad)
    with pytest.raises(ValueError, match="1\\.\\.7"):
        goal_curriculum_spec(8, m=7)
    # the option is refused before anything touches a GPU: without goals, and on the single-env client and env
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.roboy_env import RoboyEnv
    from gym_roboy_amd.envs.simulations import HipSimulationClient
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    with pytest.raises(ValueError, match="needs goals"):
        RoboyVecEnv(MsjRobot(), 256, goal_curriculum=4)
    with pytest.raises(ValueError, match="goal_curriculum"):
        RoboyVecEnv(MsjRobot(), 256, goals=np.zeros((4, 3), np.float32), goal_curriculum=0)
    with pytest.raises(ValueError, match="vectorised env"):
        HipSimulationClient(MsjRobot(), goals=np.zeros((4, 3), np.float32), goal_curriculum=2)
    with pytest.raises(ValueError, match="vectorised env"):
        RoboyEnv(goals=np.zeros((4, 3), np.float32), goal_curriculum=2)


def test_train_parallel_goal_level_arguments():
    from gym_roboy_amd.train_parallel import level_summary, parse_goal_curriculum
    assert parse_goal_curriculum(0, None, None, 0) is None and parse_goal_curriculum(0, None, None, 16384) is None
    assert parse_goal_curriculum(8, None, None, 16384) == {"levels": 8, "up": 1, "down": 1, "start": 0}
    assert parse_goal_curriculum(8, 2, 0, 512) == {"levels": 8, "up": 2, "down": 0, "start": 0}
    assert parse_goal_curriculum(256, 0, 3, 256)["levels"] == 256
    for bad in ((8, None, None, 0), (0, 1, None, 512), (0, None, 1, 512), (257, None, None, 16384), (8, None, None, 7), (-2, None, None, 512),
                (8, -1, None, 512), (8, None, -1, 512)):
        with pytest.raises(SystemExit):
            parse_goal_curriculum(*bad)
    assert level_summary([2, 0, 0, 2]) == {"mean_level": 1.5, "top_level_share": 0.5}
    assert level_summary([4]) == {"mean_level": 0.0, "top_level_share": 1.0}


def test_header_symbols_are_in_the_library():
    names = ("rb_env_goal_curriculum_configure", "rb_env_goal_level_ptr", "rb_env_goal_index_ptr", "rb_env_goal_levels_set",
             "rb_env_goal_level_hist_dev", "rb_env_goal_level_hist")
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert re.search(r"\bint %s\(rb_sim \*sim" % name, HEADER), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
    assert int(re.search(r"#define RB_ABI_VERSION (\d+)", HEADER).group(1)) == 6 == nat.load().rb_abi_version()
    assert int(re.search(r"#define RB_GOAL_LEVELS_MAX (\d+)", HEADER).group(1)) == nat.RB_GOAL_LEVELS_MAX == 256
    assert int(re.search(r"#define RB_GOAL_INDEX_NONE 0x([0-9A-F]+)u", HEADER).group(1), 16) == nat.RB_GOAL_INDEX_NONE == gc.INDEX_NONE
    # without a handle the calls fail with a code and a message
    lib.rb_env_goal_curriculum_configure.argtypes = nat.SIGNATURES["rb_env_goal_curriculum_configure"][1]
    assert lib.rb_env_goal_curriculum_configure(None, 4, 1, 1, 0) == nat.RB_EINVAL


def test_new_kernels_are_shipped_without_scratch_or_spills():
    import code_object_meta as com
    meta = {com.short(k): v for k, v in com.kernel_metadata(nat.LIB_PATH).items()}
    for name in ("rbg::goal_curriculum_kernel", "rbg::goal_level_hist_kernel"):
        hits = [v for k, v in meta.items() if k.startswith(name)]
        assert len(hits) == 1, (name, sorted(k for k in meta if "rbg::" in k))
        assert hits[0]["private_segment_fixed_size"] == 0 and hits[0]["vgpr_spill_count"] == 0, (name, hits[0])
