"""TEST HELPER for the action rows in the fused env step's observation (include/roboy_sim.h: rb_env_action_obs_*; csrc/env_hist.hpp;
DESIGN.md §18): the K blocks stated over the list of everything an env was handed, and the ring's slot count."""
import numpy as np

MAX_ROWS = 8


def ring_slots(rows, delay_hi):
    """S: the smallest power of two above max(delay_hi, rows - 1); 0 without a delay range and without rows"""
    if rows <= 0 and delay_hi <= 0:
        return 0
    s = 1
    while s <= max(delay_hi, rows - 1):
        s *= 2
    return s


def clip_action(a):
    """fminf(fmaxf(x, -1), 1) in fp32"""
    return np.minimum(np.maximum(np.asarray(a, np.float32), np.float32(-1.0)), np.float32(1.0))


class HistoryBook:
    """The K action blocks of every row an env-step writes, in the style of env_io_util.DelayBook: nothing but the list of the
    slabs handed in so far and each env's episode step.  With s the step counter as the step leaves it (k + 1, or 1 behind an
    auto-reset), block j is the clamped row handed at episode step s - 1 - j of the same episode - handed j launches ago - and zeros
    where s - 1 - j < 1."""

    def __init__(self, n, n_t, rows):
        self.k = np.ones(n, np.int64)            # the episode step the next launch computes
        self.handed = []                         # every action slab handed in so far, clamped
        self.n, self.n_t, self.rows = n, n_t, rows

    def reset(self):
        self.k[:] = 1

    def reset_blocks(self):
        return np.zeros((self.n, self.rows * self.n_t), np.float32)

    def blocks(self, act, done, auto_reset=True):
        """[n, rows n_t]: the action columns of the rows the step writes that was handed `act` and reported `done`"""
        self.handed.append(clip_action(act))
        t = len(self.handed) - 1
        s = np.where(np.asarray(done, bool) & bool(auto_reset), 1, self.k + 1)
        out = np.zeros((self.n, self.rows, self.n_t), np.float32)
        for j in range(self.rows):
            live = s - 1 - j >= 1
            if live.any():                       # (s - 1 = k launches of this episode lie behind such an env: t - j >= 0)
                out[live, j] = self.handed[t - j][live]
        self.k = s
        return out.reshape(self.n, self.rows * self.n_t)
