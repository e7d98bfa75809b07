"""Outcome counts per pool row, the checks that need no GPU: reach_rate_order against a comparator over cross-multiplied
Python ints (tests/goal_stats_util.py), with counts at which a float64 key merges distinct rates; GoalPool.ordered by that key; the
argument checks of RoboyVecEnv and of the training CLI; the new symbols of include/roboy_sim.h in the library and the new kernels'
resources; and the qualification of the GPU tests' inputs against oracle/philox_np.py."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import goal_stats_util as gs
from gym_roboy_amd import _native as nat
from gym_roboy_amd.envs.goals import GoalPool, reach_rate_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()

# two rows whose rates differ as rationals and agree as float64 under the default prior (1, 2): (r + 1) / (a + 2)
BIG = 2**40
NEAR = ((BIG + 1, BIG - 2), (BIG + 2, BIG - 1))                 # (attempts, reached): rates (2^40 - 1) / (2^40 + 3) and 2^40 / (2^40 + 4)


def count_cases():
    """name -> (attempts, reached): random counts with zeros, ties and rows with reached == attempts; counts near 2^40"""
    rng = np.random.default_rng(0)
    cases = {}
    att = rng.integers(0, 50, 200)
    att[rng.integers(0, 200, 40)] = 0                           # unvisited rows: all tie at a / b
    rch = (att * rng.uniform(0, 1, 200)).astype(np.int64)
    rch[::7] = att[::7]                                         # reached == attempts
    att[100:110], rch[100:110] = att[50:60], rch[50:60]         # equal rows
    att[110:115], rch[110:115] = 2 * att[60:65] + 2, 2 * rch[60:65] + 1      # another row at the same rate: (2 r + 2) / (2 a + 4)
    cases["small"] = (att, rch)
    att = rng.integers(BIG - 1000, BIG + 1000, 64)
    rch = att - rng.integers(0, 1000, 64)
    att[:2], rch[:2] = [NEAR[0][0], NEAR[1][0]], [NEAR[0][1], NEAR[1][1]]
    cases["near 2^40"] = (att.astype(np.uint64), rch.astype(np.uint64))
    cases["unvisited"] = (np.zeros(9, np.int64), np.zeros(9, np.int64))
    cases["one row"] = (np.array([3]), np.array([3]))
    return cases


def test_the_near_pair_is_one_a_float64_key_merges():
    (a0, r0), (a1, r1) = NEAR
    assert Fraction(r0 + 1, a0 + 2) != Fraction(r1 + 1, a1 + 2)
    assert np.float64(r0 + 1) / np.float64(a0 + 2) == np.float64(r1 + 1) / np.float64(a1 + 2)
    assert Fraction(r1 + 1, a1 + 2) > Fraction(r0 + 1, a0 + 2)   # the second row is the better one: it sorts first
    order = reach_rate_order([a0, a1], [r0, r1])
    assert order.tolist() == [1, 0] == gs.rate_order([a0, a1], [r0, r1]).tolist()


@pytest.mark.parametrize("name", sorted(count_cases()))
@pytest.mark.parametrize("prior", [(1, 2), (0, 1), (3, 3), (2, 7)])
def test_reach_rate_order_equals_the_comparator(name, prior):
    att, rch = count_cases()[name]
    order = reach_rate_order(att, rch, prior=prior)
    assert order.dtype == np.int64 and order.shape == (len(att),)
    assert np.array_equal(np.sort(order), np.arange(len(att)))                       # a permutation
    assert np.array_equal(order, gs.rate_order(att, rch, *prior))
    a, b = prior
    rate = [Fraction(int(rch[j]) + a, int(att[j]) + b) for j in order]
    for x, y, i, j in zip(rate, rate[1:], order, order[1:]):
        assert x > y or (x == y and i < j)                                           # descending, and stable
    if name == "small":
        assert len(set(rate)) < len(rate) and (att == 0).sum() > 1 and (rch == att).sum() > 1
    if name == "unvisited":
        assert np.array_equal(order, np.arange(9))
    # ordering an ordered pool again changes nothing
    again = reach_rate_order(np.asarray(att)[order], np.asarray(rch)[order], prior=prior)
    assert np.array_equal(again, np.arange(len(att)))


def test_reach_rate_order_refuses():
    good = ([4, 2, 0], [1, 2, 0])
    assert reach_rate_order(*good).tolist() == [1, 2, 0]         # rates 2/6, 3/4, 1/2
    for att, rch in (([4, 2], [1, 2, 0]), ([4, -2, 0], [1, -2, 0]), ([4, 2, 0], [-1, 2, 0]), ([4, 2, 0], [5, 2, 0]), ([[4, 2, 0]], [[1, 2, 0]]),
                     ([4.0, 2.0, 0.0], [1.0, 2.0, 0.0])):
        with pytest.raises(ValueError):
            reach_rate_order(att, rch)
    for prior in ((-1, 2), (1, 0), (1, -2), (3, 2), (0, 0), 1, (1, 2, 3), ("a", "b")):
        with pytest.raises(ValueError, match="prior"):
            reach_rate_order(*good, prior=prior)


def test_goal_pool_ordered_by_reach_rate():
    rng = np.random.default_rng(1)
    q = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    source = np.stack((np.arange(64) // 32, np.arange(64)), axis=1)
    pool = GoalPool(q, {"m": 64, "seed": 0}, source)
    assert pool.order is None
    att = rng.integers(0, 30, 64)
    rch = (att * rng.uniform(0, 1, 64)).astype(np.int64)
    want = gs.rate_order(att, rch)
    got = pool.ordered(key="reach_rate", attempts=att, reached=rch)
    assert got is not pool and np.array_equal(pool.q, q) and "ordered" not in pool.recipe and pool.order is None
    assert got.recipe == {"m": 64, "seed": 0, "ordered": "reach_rate"}
    assert got.order.dtype == np.int64 and np.array_equal(got.order, want)
    assert got.q.tobytes() == q[want].tobytes() and np.array_equal(got.source, source[want])
    other = pool.ordered(key="reach_rate", attempts=att, reached=rch, prior=(0, 1))
    assert np.array_equal(other.order, gs.rate_order(att, rch, 0, 1)) and not np.array_equal(other.order, want)
    assert GoalPool(q).ordered("reach_rate", attempts=att, reached=rch).source is None
    for kw in (dict(), dict(attempts=att), dict(attempts=att[:-1], reached=rch[:-1]), dict(attempts=att, reached=att + 1)):
        with pytest.raises(ValueError):
            pool.ordered(key="reach_rate", **kw)
    # rest_distance: what it always gave, bit for bit, and the permutation it applied
    rest = pool.ordered()
    order = np.argsort(np.sqrt(np.sum(np.square(q.astype(np.float64)), axis=1)), kind="stable")
    assert rest.q.tobytes() == q[order].tobytes() and np.array_equal(rest.source, source[order])
    assert rest.recipe == {"m": 64, "seed": 0, "ordered": "rest_distance"}
    assert rest.order.dtype == np.int64 and np.array_equal(rest.order, order)
    assert pool.ordered("rest_distance").q.tobytes() == rest.q.tobytes()
    with pytest.raises(ValueError, match="reach_rate"):
        pool.ordered("rest_distance", attempts=att, reached=rch)


def test_the_env_refuses_counts_without_a_curriculum_before_any_gpu_call(monkeypatch):
    import gym_roboy_amd.envs.vec_env as vec_env
    from gym_roboy_amd.envs.robots import MsjRobot

    def no_sim(*a, **kw):
        raise AssertionError("a simulation handle was asked for")
    monkeypatch.setattr(vec_env, "HipBatchSimulation", no_sim)
    with pytest.raises(ValueError, match="goal_row_stats needs goal_curriculum"):
        vec_env.RoboyVecEnv(MsjRobot(), 256, goals=np.zeros((4, 3), np.float32), goal_row_stats=True)
    with pytest.raises(ValueError, match="goal_row_stats needs goal_curriculum"):
        vec_env.RoboyVecEnv(MsjRobot(), 256, goal_row_stats=True)
    with pytest.raises(AssertionError, match="handle was asked for"):                # with a curriculum the check passes
        vec_env.RoboyVecEnv(MsjRobot(), 256, goals=np.zeros((4, 3), np.float32), goal_curriculum=1, goal_row_stats=True)


def test_train_parallel_goal_order_arguments():
    import gym_roboy_amd.train_parallel as tp
    curriculum = {"levels": 8, "up": 1, "down": 1, "start": 0}
    assert tp.parse_goal_order("rest_distance", 1, None) is False and tp.parse_goal_order("rest_distance", 1, curriculum) is False
    assert tp.parse_goal_order("reach_rate", 1, curriculum) is True and tp.parse_goal_order("reach_rate", 3, curriculum) is True
    for bad in (("reach_rate", 1, None), ("volume", 1, curriculum), ("reach_rate", 0, curriculum), ("reach_rate", -1, curriculum),
                ("rest_distance", 2, curriculum)):
        with pytest.raises(SystemExit):
            tp.parse_goal_order(*bad)
    # the refusals come before anything touches a GPU
    for argv in (["256", "--goal-order", "reach_rate"], ["256", "--goals", "reachable:256", "--goal-order", "reach_rate"],
                 ["256", "--goals", "reachable:256", "--goal-levels", "4", "--goal-order", "volume"],
                 ["256", "--goals", "reachable:256", "--goal-levels", "4", "--goal-order", "reach_rate", "--goal-reorder-every", "0"]):
        with pytest.raises(SystemExit):
            tp.main(argv)
    assert tp.reach_rate_summary([4, 4, 0, 8], [1, 3, 0, 0], 2) == {"reach_rate_first_level": 0.5, "reach_rate_whole_pool": 0.25}
    assert tp.reach_rate_summary([0, 0], [0, 0], 1) == {"reach_rate_first_level": 0.0, "reach_rate_whole_pool": 0.0}


def test_header_symbols_are_in_the_library():
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in ("rb_env_goal_row_stats_enable", "rb_env_goal_row_stats_ptr", "rb_env_goal_row_stats_read", "rb_env_goal_row_stats_set",
                 "rb_env_goal_pool_permute"):
        assert re.search(r"\bint %s\(rb_sim \*sim" % name, HEADER), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
    assert int(re.search(r"#define RB_ABI_VERSION (\d+)", HEADER).group(1)) == 6 == nat.load().rb_abi_version()
    # without a handle the calls fail with a code
    for name in ("rb_env_goal_row_stats_enable",):
        getattr(lib, name).argtypes = nat.SIGNATURES[name][1]
        assert getattr(lib, name)(None) == nat.RB_EINVAL
    lib.rb_env_goal_pool_permute.argtypes = nat.SIGNATURES["rb_env_goal_pool_permute"][1]
    assert lib.rb_env_goal_pool_permute(None, None) == nat.RB_EINVAL


def test_new_kernels_are_shipped_without_scratch_or_spills():
    import code_object_meta as com
    meta = {com.short(k): v for k, v in com.kernel_metadata(nat.LIB_PATH).items()}
    for name in ("rbg::goal_curriculum_stats_kernel", "rbg::goal_index_permute_kernel"):
        hits = [v for k, v in meta.items() if k.startswith(name)]
        assert len(hits) == 1, (name, sorted(k for k in meta if "rbg::" in k))
        assert hits[0]["private_segment_fixed_size"] == 0 and hits[0]["vgpr_spill_count"] == 0, (name, hits[0])


# ---- the GPU tests' inputs, qualified ----
@pytest.mark.parametrize("n_levels,start", gs.MIXED_LEVELS)
def test_mixed_case_puts_envs_on_row_0_and_on_other_rows(n_levels, start):
    rows = gs.first_reset_rows(n_levels, start)
    assert rows.shape == (gs.MIXED_N,) and rows.min() == 0 and rows.max() < gs.MIXED_M
    assert (rows == 0).sum() >= 1 and (rows != 0).sum() >= 1
    from gym_roboy_amd.envs.robots import MsjRobot
    pool = gs.mixed_pool(MsjRobot().get_description())
    assert pool.shape == (gs.MIXED_M, 3) and not pool[0].any() and np.abs(pool[1:]).min() > 0


def test_two_rank_reorder_equals_the_single_rank_result_on_the_sums():
    """train_parallel's arithmetic per re-ordering: every rank sums the [2 m] blocks (float64: exact below 2^53), orders by the sums,
    permutes and halves its own counts.  The ranks end with the same order, and their halved counts sum to the single-rank result up
    to the one unit per rank and row the shift drops."""
    rng = np.random.default_rng(3)
    m = 97
    att = rng.integers(0, 2**20, (2, m)).astype(np.uint64)
    rch = (att * rng.uniform(0, 1, (2, m))).astype(np.uint64)
    att[:, :5], rch[:, :5] = 0, 0
    # through float64, as sharding.allreduce_stats carries the block
    block = np.concatenate((att, rch), axis=1).astype(np.float64).sum(axis=0)
    assert block.max() < 2**53
    s_att, s_rch = block[:m].astype(np.uint64), block[m:].astype(np.uint64)
    assert np.array_equal(s_att, att.sum(axis=0)) and np.array_equal(s_rch, rch.sum(axis=0))
    orders = [reach_rate_order(s_att, s_rch) for _ in range(2)]                      # what each rank computes
    single, one_a, one_r = gs.reorder_model(s_att[None], s_rch[None])
    assert np.array_equal(orders[0], orders[1]) and np.array_equal(orders[0], single)
    order, two_a, two_r = gs.reorder_model(att, rch)
    assert np.array_equal(order, single)
    for halves, per_rank, one, whole in ((two_a, att, one_a[0], s_att), (two_r, rch, one_r[0], s_rch)):
        assert np.array_equal(halves, per_rank[:, order] >> np.uint64(1))
        total = halves.sum(axis=0)
        assert np.all(total <= one) and np.all(one - total <= 1) and np.array_equal(one, whole[order] >> np.uint64(1))
    assert np.all(two_r <= two_a)                                # a halved plane is still one rb_env_goal_row_stats_set takes
