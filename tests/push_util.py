"""TEST HELPER for the random pushes in front of the fused env step (include/roboy_sim.h: rb_env_push_*; csrc/env_push.hpp; DESIGN.md
§28): the rule restated over oracle/philox_np.py - the decision as integers, the deviates in float64 - a follower of the four planes,
and the twin runs tests/test_push_gpu.py shares."""
import ctypes

import numpy as np

from env_io_util import NOISE_TOL      # the project's bound on this fp32 Box-Muller expression, here relative to sigma
from oracle import philox_np

STREAM_PUSH = 6
N, STEPS, MAX_LEN, SEED, PROB = 200, 12, 5, 11, 0.25      # one partial group of 256 lanes; every env auto-resets twice


def threshold_of(prob):
    return int(round(float(prob) * 2 ** 24))


def decision(seed, gids, m, threshold):
    """pushed [n] bool of the envs with global ids gids at their step counts m (a scalar or [n]): (w >> 8) < threshold, integers"""
    ids = np.asarray(gids, dtype=np.uint64).reshape(-1)
    m = np.broadcast_to(np.asarray(m, dtype=np.uint32), ids.shape)
    w = philox_np.draw(int(seed), ids, m, STREAM_PUSH, 0)[:, 0].astype(np.int64)
    return (w >> 8) < int(threshold)


def z64(seed, gids, m, n_q):
    """z [n, n_q] in float64: joint j takes component j & 3 of block 1 + (j >> 2) of the same draw; Box-Muller over pairs (0,1), (2,3),
    u1 = ((w >> 8) + 1) / 2^24, u2 = (w >> 8) / 2^24, cosine to the even component, sine to the odd"""
    ids = np.asarray(gids, dtype=np.uint64).reshape(-1)
    m = np.broadcast_to(np.asarray(m, dtype=np.uint32), ids.shape)
    out = np.empty((ids.shape[0], n_q), dtype=np.float64)
    for b in range((n_q + 3) // 4):
        w = philox_np.draw(int(seed), ids, m, STREAM_PUSH, 1 + b)
        for pair in range(2):
            u1 = ((w[:, 2 * pair] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
            u2 = (w[:, 2 * pair + 1] >> np.uint32(8)).astype(np.float64) / 16777216.0
            rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
            for k, e in ((0, rad * np.cos(ang)), (1, rad * np.sin(ang))):
                j = 4 * b + 2 * pair + k
                if j < n_q:
                    out[:, j] = e
    return out


class Book:
    """The integer planes restated: count, last, n_pushes of n envs with global ids gid0 .. gid0 + n - 1, from a configuration on."""

    def __init__(self, seed, n, threshold, gid0=0):
        self.seed, self.threshold = int(seed), int(threshold)
        self.gids = np.arange(gid0, gid0 + n, dtype=np.uint64)
        self.count, self.last, self.n_pushes = (np.zeros(n, np.uint32) for _ in range(3))

    def step(self):
        """one env step of every env: -> (pushed [n] bool, the counts m [n] the draws were made at)"""
        m = self.count.copy()
        pushed = decision(self.seed, self.gids, m, self.threshold)
        self.count = m + np.uint32(1)
        self.last = np.where(pushed, self.count, self.last)
        self.n_pushes = self.n_pushes + pushed.astype(np.uint32)
        return pushed, m


def schedule(seed, n, steps, prob, gid0=0):
    """pushed [steps, n] of a fresh configuration"""
    book = Book(seed, n, threshold_of(prob), gid0)
    return np.array([book.step()[0] for _ in range(steps)])


# ---- the robots and the device side ----
def robot_of(which):
    """(robot, desc) - 'baked': MsjRobot; 'kernarg': MsjRobot with other constants; 'ball12': 12 tendons; 'upper': the upper body"""
    if which == "upper":
        from gym_roboy_amd.envs.robots import UpperBodyRobot
        r = UpperBodyRobot()
    else:
        from test_env_params_gpu import _ball12, _kernarg_msj, _msj
        r = {"baked": _msj, "kernarg": _kernarg_msj, "ball12": _ball12}[which]()
    return r, r.get_description()


def sigma_of(desc):
    """2 qd_max per joint: some pushed joint then has |impulse| > 2 qd_max, a clamp whatever its velocity (tests/test_push_cpu.py)"""
    return [float(v) for v in 2.0 * np.asarray(desc.qd_max, np.float32)]


def planes(env):
    """(count, last, n_pushes [n] uint32, impulse [n, n_q] float32) of a RoboyVecEnv with pushes, read behind a synchronisation"""
    d_count, d_last, d_n, d_imp = env._push_planes()
    env.sim.synchronize()
    n = env.num_envs
    return tuple(env.sim.download(p, (n,), np.uint32) for p in (d_count, d_last, d_n)) + (env.sim.download(d_imp, (n, env.n_q)),)


def _is_tree(env):
    return env.n_q != 3                # (of robot_of's robots: the ball-joint ones have 3 joints, the upper body 20)


def read_qd(env):
    """[n, n_q] from the handle's own velocity array (rb_state_ptrs): planes [n_q][n] for ball joints, rows [n][n_q] for joint trees"""
    env.sim.synchronize()
    d_qd = env.sim.state_ptrs()[1]
    n, nq = env.num_envs, env.n_q
    return env.sim.download(d_qd, (n, nq)) if _is_tree(env) else env.sim.download(d_qd, (nq, n)).T.copy()


def write_qd(env, qd):
    env.sim.synchronize()
    qd = np.asarray(qd, np.float32)
    env.sim.upload(env.sim.state_ptrs()[1], qd if _is_tree(env) else qd.T)
    env.sim.synchronize()


def apply_pushes(twin, pushed, impulse, qd_max):
    """The rule's last line in numpy float32 on a handle WITHOUT the option: qd <- clamp(fl32(qd + impulse), -qd_max, qd_max) for the
    pushed envs.  -> (joints the clamp changed, joints it left alone) among the pushed"""
    qd = read_qd(twin)
    vmax = np.asarray(qd_max, np.float32)
    moved = (qd + impulse.astype(np.float32)).astype(np.float32)
    new = np.clip(moved, -vmax, vmax).astype(np.float32)
    qd[pushed] = new[pushed]
    write_qd(twin, qd)
    changed = (new != moved)[pushed]
    return int(changed.sum()), int((~changed).sum())


def twin_steps(a, b, acts, qd_max, extra=None):
    """Steps env ``a`` (pushes) and env ``b`` (none) through ``acts``; before each of b's steps its velocities take the impulses a's
    step applied.  Asserts obs, reward, done, q, qd and the feasibility flags equal WITHOUT a tolerance (and whatever ``extra(env)``
    returns: a tuple of arrays).  -> (done counts [n], clamped joints, unclamped joints, pushes)"""
    n_done, clamped, free, pushes = np.zeros(a.num_envs, int), 0, 0, 0
    for t, act in enumerate(acts):
        ra = a.step(act)[:3] + tuple(a.sim.read_state()) + (tuple(extra(a)) if extra else ())
        count, last, _, imp = planes(a)
        pushed = last == count
        c, f = apply_pushes(b, pushed, imp, qd_max)
        clamped, free, pushes = clamped + c, free + f, pushes + int(pushed.sum())
        rb = b.step(act)[:3] + tuple(b.sim.read_state()) + (tuple(extra(b)) if extra else ())
        for k, (x, y) in enumerate(zip(ra, rb)):
            assert np.array_equal(x, y), (t, k, np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max())
        n_done += ra[2]
    return n_done, clamped, free, pushes


def push_cfg(nat, threshold, sigma):
    cfg = nat.EnvPushConfig()
    cfg.threshold = int(threshold)
    for j, v in enumerate(sigma):
        cfg.sigma[j] = float(v)
    return cfg


def configure(nat, env, cfg):
    """rb_env_push_configure on the env's handle -> the return code (cfg None: NULL)"""
    return nat.load().rb_env_push_configure(env.sim.handle, None if cfg is None else ctypes.byref(cfg))
