"""TEST HELPER for the start poses behind the fused env step (include/roboy_sim.h: rb_env_start_poses_*; csrc/env_start.hpp; DESIGN.md
§30): the rule restated over oracle/philox_np.py - decision, row and counter as integers - a follower of the two planes, the pool the
GPU tests use, and the twin run tests/test_start_poses_gpu.py shares."""
import numpy as np

from oracle import philox_np

STREAM_START = 7
INDEX_REST = 0xFFFFFFFF
N, STEPS, MAX_LEN, SEED, PROB, M = 200, 12, 5, 11, 0.5, 7      # one partial group of 256 lanes; every env auto-resets twice


def threshold_of(prob):
    return int(round(float(prob) * 2 ** 24))


def draw(seed, gids, d, threshold, m):
    """start number d (a scalar or [n]) of the envs with global ids gids -> (from_pool [n] bool, row [n] int64): the decision is
    (w.v[1] >> 8) < threshold, the row (uint64(w.v[0]) m) >> 32; integers only"""
    ids = np.asarray(gids, dtype=np.uint64).reshape(-1)
    d = np.broadcast_to(np.asarray(d, dtype=np.uint32), ids.shape)
    w = philox_np.draw(int(seed), ids, d, STREAM_START, 0)
    from_pool = (w[:, 1].astype(np.int64) >> 8) < int(threshold)
    row = [(int(x) * int(m)) >> 32 for x in w[:, 0]]          # (Python ints: a 64-bit product)
    return from_pool, np.asarray(row, dtype=np.int64)


def index_of(seed, gids, d, threshold, m):
    """the index plane's word of start number d: the row, or INDEX_REST"""
    from_pool, row = draw(seed, gids, d, threshold, m)
    return np.where(from_pool, row, INDEX_REST).astype(np.uint32)


class Book:
    """The two planes restated: count and index of n envs with global ids gid0 .. gid0 + n - 1, from a configuration on."""

    def __init__(self, seed, n, threshold, m, gid0=0):
        self.seed, self.threshold, self.m = int(seed), int(threshold), int(m)
        self.gids = np.arange(gid0, gid0 + n, dtype=np.uint64)
        self.count = np.zeros(n, np.uint32)
        self.index = np.full(n, INDEX_REST, np.uint32)

    def start(self, who=None):
        """the envs `who` ([n] bool; None: all, a reset) start an episode -> started [n] bool: those that start at a pool row"""
        who = np.ones(self.count.shape, bool) if who is None else np.asarray(who, bool)
        new = index_of(self.seed, self.gids, self.count, self.threshold, self.m)
        self.index = np.where(who, new, self.index)
        self.count = (self.count + who.astype(np.uint32)).astype(np.uint32)
        return who & (new != INDEX_REST)


def pool_of(desc, m=M, seed=3):
    """m poses inside 0.5 of the joint limits"""
    return np.random.default_rng(seed).uniform(0.5 * desc.q_lo, 0.5 * desc.q_hi, (m, desc.n_q)).astype(np.float32)


# ---- the device side ----
def planes(env):
    """(count, index) [n] uint32 of a RoboyVecEnv with start poses, read behind a synchronisation"""
    _, d_count, d_index = env._start_planes()
    env.sim.synchronize()
    return tuple(env.sim.download(p, (env.num_envs,), np.uint32) for p in (d_count, d_index))


def hand_poses(twin, started, index, pool):
    """the started envs of a handle WITHOUT the option take their pose: read the state, patch those lanes (q = the row, qd = 0,
    feasible), write it back"""
    q, qd, feas = twin.sim.read_state()
    q[started] = pool[index[started].astype(np.int64)]
    qd[started] = 0.0
    feas[started] = True
    twin.sim.set_state(q, qd, feas)


def replaced(started, n_q, obs_dim):
    """[n, obs_dim] bool: the row columns the kernel replaces - [0, 2 n_q) of the started envs"""
    out = np.zeros((started.shape[0], obs_dim), bool)
    out[started, :2 * n_q] = True
    return out


def check_rows(obs_a, obs_b, started, index, pool, n_q, where):
    """a's rows against the twin's: every column outside the replaced ones bit-equal; the replaced ones [pose, 0] exactly"""
    rep = replaced(started, n_q, obs_a.shape[1])
    assert np.array_equal(obs_a[~rep], obs_b[~rep]), where
    pose = pool[index[started].astype(np.int64)]
    assert np.array_equal(obs_a[started, :n_q], pose) and not obs_a[started, n_q:2 * n_q].any(), where


def twin_steps(a, b, acts, pool, extra=None, rows=check_rows, gid0=0, seed=SEED, prob=PROB):
    """Resets and steps env ``a`` (start poses) and env ``b`` (none) through ``acts``; behind the reset and every step b's started
    lanes are handed a's pose.  Asserts the planes equal to the restated book, and q, qd, feasible, reward, done (and whatever
    ``extra(env, started)`` returns: a tuple of arrays) equal WITHOUT a tolerance; ``rows(obs_a, obs_b, started, index, pool, n_q,
    where)`` judges the observation rows.  -> (done counts [n], starts from the pool, starts at rest)"""
    n, nq = a.num_envs, a.n_q
    book = Book(seed, n, threshold_of(prob), pool.shape[0], gid0)
    n_done, from_pool, at_rest = np.zeros(n, int), 0, 0

    def behind(t, ra, rb, who):
        nonlocal from_pool, at_rest
        started = book.start(who)
        count, index = planes(a)
        assert np.array_equal(count, book.count) and np.array_equal(index, book.index), t
        hand_poses(b, started, index, pool)
        from_pool, at_rest = from_pool + int(started.sum()), at_rest + int((np.ones(n, bool) if who is None else who).sum() - started.sum())
        rows(ra[0], rb[0], started, index, pool, nq, t)
        sa, sb = tuple(a.sim.read_state()), tuple(b.sim.read_state())
        assert np.array_equal(sa[0][started], pool[index[started].astype(np.int64)]) and not sa[1][started].any() and sa[2][started].all(), t
        xa = ra[1:] + sa + (tuple(extra(a, started)) if extra else ())
        xb = rb[1:] + sb + (tuple(extra(b, started)) if extra else ())
        for k, (x, y) in enumerate(zip(xa, xb)):
            assert np.array_equal(x, y), (t, k)

    behind("reset", (a.reset(),), (b.reset(),), None)
    for t, act in enumerate(acts):
        ra, rb = a.step(act)[:3], b.step(act)[:3]
        behind(t, ra, rb, ra[2])
        n_done += ra[2]
    return n_done, from_pool, at_rest
