"""TEST HELPER for the outcome counts per pool row (include/roboy_sim.h: rb_env_goal_row_stats_*, rb_env_goal_pool_permute;
csrc/env_goal.hpp): a follower that extends goal_curriculum_util.CurriculumFollower by the model's attempts / reached
arrays and by a permutation of the live pool, the comparator the ordering key is held to, and the inputs of the mixed-outcome GPU case,
which tests/test_goal_stats_cpu.py qualifies.  Nothing here imports the product's goals module."""
import functools

import numpy as np

import goal_curriculum_util as gc
import goal_pool_util as gp

# the mixed-outcome case of tests/test_goal_stats_gpu.py: (levels, start level) pairs over a pool of 7 rows whose row 0 is the zero pose
MIXED_SEED, MIXED_N, MIXED_M = 5, 257, 7
MIXED_LEVELS = ((7, 3), (1, 0))


def mixed_pool(desc):
    """row 0: the zero pose, which an env at rest under zero actions reaches in its first step; rows 1..6: small_pool's, half-way to
    the limits and beyond, which it never reaches"""
    rows = gp.small_pool(desc, m=MIXED_M).copy()
    rows[0] = 0.0
    assert len({r.tobytes() for r in rows}) == MIXED_M
    return rows


def first_reset_rows(n_levels, start, seed=MIXED_SEED, n=MIXED_N, m=MIXED_M):
    """the rows the envs hold behind the first reset (draw 1: construction drew 0)"""
    return gc.row(seed, np.arange(n), 1, start, m, n_levels)


def rate_order(attempts, reached, a=1, b=2):
    """the order reach_rate_order must give, by a comparator over cross-multiplied Python ints: descending (reached + a) / (attempts +
    b), ties by current position"""
    att, rch = [int(x) for x in attempts], [int(x) for x in reached]

    def cmp(i, j):
        lhs, rhs = (rch[i] + a) * (att[j] + b), (rch[j] + a) * (att[i] + b)       # rate_i > rate_j  <=>  lhs > rhs
        if lhs != rhs:
            return -1 if lhs > rhs else 1
        return -1 if i < j else (1 if i > j else 0)
    return np.asarray(sorted(range(len(att)), key=functools.cmp_to_key(cmp)), dtype=np.int64)


def reorder_model(attempts, reached, halve=True):
    """sum over ranks -> order -> every rank's counts permuted and halved: what train_parallel does per re-ordering.  attempts,
    reached: [ranks, m].  Returns (order, attempts', reached') with the rank axis kept"""
    attempts, reached = np.asarray(attempts, dtype=np.uint64), np.asarray(reached, dtype=np.uint64)
    order = rate_order(attempts.sum(axis=0), reached.sum(axis=0))
    a, r = attempts[:, order], reached[:, order]
    if halve:
        a, r = a >> np.uint64(1), r >> np.uint64(1)
    return order, a, r


class StatsFollower(gc.CurriculumFollower):
    """CurriculumFollower plus the counts.  An episode end is first counted against the row the env was aimed at (self.index before
    it moves; INDEX_NONE and -1 are no row) with the follower's own outcome witness, then the level moves and the env draws.
    self.attempts / self.reached are the model's planes; check_planes also holds the env's counts to them."""

    def __init__(self, vec, pool, seed, levels, up=1, down=1, start=0, offset=0, auto_reset=True, outcome="truncated"):
        self.attempts = np.zeros(len(pool), np.uint64)
        self.reached = np.zeros(len(pool), np.uint64)
        super().__init__(vec, pool, seed, levels, up, down, start, offset=offset, auto_reset=auto_reset, outcome=outcome)

    def goal_of(self, mask):
        if self._ending:
            hit = ~np.asarray(self.vec.truncated())[mask] if self.outcome == "truncated" else np.zeros(int(mask.sum()), bool)
            k0 = self.index[mask]
            row = (k0 >= 0) & (k0 < len(self.pool))
            np.add.at(self.attempts, k0[row], np.uint64(1))
            np.add.at(self.reached, k0[row & hit], np.uint64(1))
        return super().goal_of(mask)

    def check_planes(self):
        super().check_planes()
        counts = self.vec.goal_row_stats()
        assert counts["attempts"].dtype == np.uint64 and counts["reached"].dtype == np.uint64
        assert np.array_equal(counts["attempts"], self.attempts), "attempts off the model: %r, model %r" % (counts["attempts"], self.attempts)
        assert np.array_equal(counts["reached"], self.reached), "reached off the model: %r, model %r" % (counts["reached"], self.reached)

    def permute(self, order):
        """the env's pool and the model's, re-ordered: new row j is old row order[j]"""
        order = np.asarray(order, dtype=np.int64)
        self.vec.permute_goal_pool(order)
        inv = np.empty(len(order), np.int64)
        inv[order] = np.arange(len(order))
        self.pool = self.pool[order]
        row = (self.index >= 0) & (self.index < len(order))
        self.index[row] = inv[self.index[row]]
        self.attempts, self.reached = self.attempts[order], self.reached[order]
        self.check_planes()
