"""Running return normalisation of the reward restated in numpy from the definition alone - a per-step loop in float64,
independent of gym_roboy_amd/ppo.py - with the bounds the tests hold the torch statement and the kernel to."""
import numpy as np

DONE_PATTERNS = ("none", "all", "first_step", "last_step", "random")


def done_pattern(kind, T, N, rng):
    """int32 [T, N]: the done flags of the named pattern (random: 5 % of the steps)"""
    done = np.zeros((T, N), np.int32)
    if kind == "all":
        done[:] = 1
    elif kind == "first_step":
        done[0] = 1
    elif kind == "last_step":
        done[-1] = 1
    elif kind == "random":
        done = (rng.random((T, N)) < 0.05).astype(np.int32)
    else:
        assert kind == "none"
    return done


def scaled(rew_raw, scale):
    """r_s = fl32(rew_raw * reward_scale)"""
    r = rew_raw.astype(np.float32) * np.float32(scale)
    assert r.dtype == np.float32
    return r


def normalised(r_s, rstd, clip):
    """r~ = min(max(fl32(r_s * rstd), -clip), clip) in float32"""
    c = np.float32(clip)
    out = np.minimum(np.maximum(r_s * np.float32(rstd), -c), c)
    assert out.dtype == np.float32
    return out


def scan(r_s, done, gamma, carry):
    """The forward scan per env: R = gamma R + r_s in float64, recorded, then zeroed where the step ended an episode.
    -> (returns [T, N] float64 as recorded, the carry after the last step, A: the same recurrence on |r_s| from |carry| - the
    a-priori magnitude the rounding bound of the carry scales with)"""
    T = r_s.shape[0]
    R, A = np.array(carry, np.float64), np.abs(np.array(carry, np.float64))
    rets = np.empty(r_s.shape, np.float64)
    for t in range(T):
        R = gamma * R + r_s[t].astype(np.float64)
        A = gamma * A + np.abs(r_s[t].astype(np.float64))
        rets[t] = R
        R = np.where(done[t] != 0, 0.0, R)
        A = np.where(done[t] != 0, 0.0, A)
    return rets, R, A


def carry_bound(T, A):
    """4 T 2^-53 A: the recurrence's a-priori rounding bound with either contraction choice"""
    return 4.0 * T * 2.0 ** -53 * A


def assert_return_moments(mean, var, count, returns):
    """mean / var / count against numpy's two-pass float64 moments of all the returns: 1e-8 relative on var, 1e-8 std on mean (the
    bound of tests/test_obs_norm_cpu.py)."""
    x = np.concatenate([np.asarray(r, np.float64).reshape(-1) for r in returns])
    m, v = x.mean(), x.var()
    assert count == x.size, (count, x.size)
    assert abs(var - v) <= 1e-8 * v, (var, v)
    assert abs(mean - m) <= 1e-8 * np.sqrt(v), (mean, m, np.sqrt(v))


def rstd_of(var, eps=1e-8):
    return np.float32(1.0 / np.sqrt(var + eps))
