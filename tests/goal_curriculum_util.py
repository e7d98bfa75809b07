"""TEST HELPER for the goal curriculum (include/roboy_sim.h: rb_env_goal_curriculum_*; csrc/env_goal.hpp): the numpy
restatement of the window hi(l), of the row an env at level l draws (over oracle/philox_np.py) and of the level rule, and a follower
that extends goal_pool_util.Follower by a level per env.  Nothing here imports the product's goals module."""
import numpy as np

import goal_pool_util as gp
from oracle import philox_np as ph

INDEX_NONE = 0xFFFFFFFF


def hi(level, m, n_levels):
    """hi(l) = uint32((uint64(l + 1) * m) / L): Python ints or int64 arrays (l + 1 <= 256 and m < 2^32: no overflow in int64)"""
    return (np.asarray(level, dtype=np.int64) + 1) * int(m) // int(n_levels)


def row(seed, gids, draw, level, m, n_levels):
    """k = (uint64(w) * uint64(hi(l))) >> 32 with the goal pool's word w; level: a number or [len(gids)]"""
    w = ph.draw(int(seed), np.asarray(gids, dtype=np.uint64), draw, gp.STREAM_GOAL_POOL, 0)[..., 0]
    h = np.broadcast_to(hi(level, m, n_levels), w.shape).astype(np.uint64)
    return ((w.astype(np.uint64) * h) >> np.uint64(32)).astype(np.int64)


def next_level(level, reached, up, down, n_levels):
    """reached: l <- min(l + up, L - 1); not reached: l <- l - min(l, down)"""
    level = np.asarray(level, dtype=np.int64)
    return np.where(np.asarray(reached, dtype=bool), np.minimum(level + int(up), int(n_levels) - 1), level - np.minimum(level, int(down)))


class CurriculumFollower(gp.Follower):
    """goal_pool_util.Follower with a level per env.  An episode end first moves the env's level by its outcome, then draws at the new
    level.  The outcome is a witness of the follower's own: `outcome="truncated"` reads vec.truncated() (reached = done and not
    truncated; needs report_truncation), `outcome="never"` takes every episode end for a time-out (the caller asserts afterwards that
    the statistics count no goal reached).  self.level and self.index are the model's planes."""

    def __init__(self, vec, pool, seed, levels, up=1, down=1, start=0, offset=0, auto_reset=True, outcome="truncated"):
        self.n_levels, self.up, self.down, self.outcome = int(levels), int(up), int(down), outcome
        self.level = np.full(vec.num_envs, int(start), np.int64)
        self.index = np.full(vec.num_envs, -1, np.int64)
        self.promotions = self.demotions = self.ends = 0
        self._ending = False
        super().__init__(vec, pool, seed, offset=offset, auto_reset=auto_reset)

    def goal_of(self, mask):
        if self._ending:                  # called by Follower.step for the envs that are done: their levels move first
            reached = ~np.asarray(self.vec.truncated())[mask] if self.outcome == "truncated" else np.zeros(int(mask.sum()), bool)
            new = next_level(self.level[mask], reached, self.up, self.down, self.n_levels)
            self.promotions += int(np.sum(new > self.level[mask]))
            self.demotions += int(np.sum(new < self.level[mask]))
            self.ends += int(mask.sum())
            self.level[mask] = new
        k = row(self.seed, self.gids[mask], (self.count[mask] - 1).astype(np.uint32), self.level[mask], len(self.pool), self.n_levels)
        self.index[mask] = k
        return self.pool[k]

    def step(self, act):
        self._ending = True
        try:
            out = super().step(act)
        finally:
            self._ending = False
        self.check_planes()
        return out

    def reset(self):
        obs = super().reset()
        self.check_planes()
        return obs

    def check_planes(self):
        level, index = np.asarray(self.vec.goal_levels()).astype(np.int64), np.asarray(self.vec.goal_index()).astype(np.int64)
        bad = np.nonzero(level != self.level)[0]
        assert bad.size == 0, "levels off the model in %d envs (first env %d: %d, model %d)" % (bad.size, bad[0], level[bad[0]], self.level[bad[0]])
        bad = np.nonzero(index != self.index)[0]
        assert bad.size == 0, "indices off the model in %d envs (first env %d: %d, model %d)" % (bad.size, bad[0], index[bad[0]], self.index[bad[0]])
