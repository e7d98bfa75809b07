"""TEST HELPER for the fused env step's action latency and sensor noise (include/roboy_sim.h: rb_env_io_*; csrc/env_io.hpp;
DESIGN.md §14): the two draws restated from oracle/philox_np.py, and the host bookkeeping of a delayed action sequence."""
import numpy as np

from oracle import philox_np

STREAM_SENSOR, STREAM_DELAY = 4, 5
MAX_DELAY = 7
NOISE_TOL = 2e-3          # tests/test_policy_scale_gpu.py's bound on this Box-Muller expression in fp32 (observed there: 1.6e-6)


def sensor_noise64(seed, gids, rows, obs_dim, dtype=np.float64):
    """z [n, obs_dim] of the envs with global ids gids for their row numbers `rows` (a scalar or [n]); every operation in `dtype`.
    Written like oracle/policy_ref.policy_noise, with stream 4 and index = row number: the column at row position c takes component
    c & 3 of block c >> 2."""
    ids = np.asarray(gids, dtype=np.uint64).reshape(-1)
    rows = np.broadcast_to(np.asarray(rows, dtype=np.uint32), ids.shape)
    f = np.dtype(dtype).type
    out = np.empty((ids.shape[0], obs_dim), dtype=dtype)
    for block in range((obs_dim + 3) // 4):
        w = philox_np.draw(int(seed), ids, rows, STREAM_SENSOR, block)
        for pair in range(2):
            u1 = ((w[:, 2 * pair] >> np.uint32(8)).astype(dtype) + f(1.0)) * f(1.0 / 16777216.0)
            u2 = (w[:, 2 * pair + 1] >> np.uint32(8)).astype(dtype) * f(1.0 / 16777216.0)
            rad = np.sqrt(f(-2.0) * np.log(u1))
            ang = f(2.0 * np.pi) * u2
            for k, e in ((0, rad * np.cos(ang)), (1, rad * np.sin(ang))):
                j = 4 * block + 2 * pair + k
                if j < obs_dim:
                    out[:, j] = e
    return out


def delay_draw(seed, gids, m, lo, hi):
    """d [n] (int64) of draw number m (a scalar or [n]) of the envs with global ids gids: lo + ((w >> 8) (hi - lo + 1) >> 24), integers"""
    ids = np.asarray(gids, dtype=np.uint64).reshape(-1)
    m = np.broadcast_to(np.asarray(m, dtype=np.uint32), ids.shape)
    w = philox_np.draw(int(seed), ids, m, STREAM_DELAY, 0)[:, 0].astype(np.int64)
    return int(lo) + (((w >> 8) * (int(hi) - int(lo) + 1)) >> 24)


def column_sigmas(n_q, n_t, channels, sigma, scale=None):
    """sigma x scale per row position [obs_dim] (fp64, signed; 0 for the goal and for columns without noise); `sigma`: {'q', 'qd',
    channel: value}, `channels` in row order"""
    scale = dict(scale or {})
    s = [float(sigma.get("q", 0.0))] * n_q + [float(sigma.get("qd", 0.0))] * n_q + [0.0] * n_q
    for c in channels:
        s += [float(sigma.get(c, 0.0)) * float(scale.get(c, 1.0))] * n_t
    return np.asarray(s, np.float64)


class DelayBook:
    """What a handle WITHOUT delay has to be fed so that it steps like one with per-env delays d: per env the action handed in d
    steps earlier in the same episode, or - while the episode is younger than that - the rest command."""

    def __init__(self, n, n_t):
        self.k = np.ones(n, np.int64)            # the episode step the next launch computes
        self.handed = []                         # every action slab handed in so far
        self.n, self.n_t = n, n_t

    def shifted(self, act, d):
        """(actions [n, n_t] to feed, rest [n] bool) for the step that is handed `act`, under the delays d [n]"""
        self.handed.append(np.asarray(act, np.float32))
        t = len(self.handed) - 1
        d = np.asarray(d, np.int64)
        rest = self.k - d < 1
        out = np.zeros((self.n, self.n_t), np.float32)
        for dd in np.unique(d):
            sel = (d == dd) & ~rest
            if sel.any():
                out[sel] = self.handed[t - dd][sel]
        return out, rest

    def advance(self, done, auto_reset=True):
        self.k = np.where(np.asarray(done, bool) & auto_reset, 1, self.k + 1)
