"""TEST HELPER for the action-box clamp of the fused env step (include/roboy_sim.h: rb_env_step_dev; NEXT.md names the eleven places
that hold it): actions far outside [-1, 1] with the edge values planted, robots with a narrower set-point box, the fp64 rescale of
the clipped action, and the (robot, box, start state) combinations that tests/test_action_box_gpu.py runs and
tests/test_action_box_cpu.py qualifies.

Why the inputs need qualifying: on MsjRobot at the rest pose with its own box (+-0.3 m) an unclamped set-point changes nothing -
kp sigma 0.3 / l0 = 1.4, the activation is saturated at both box edges - so a test that feeds wide actions there proves nothing.
Every combination below moves when the clamp is dropped (test_action_box_cpu.py holds each to that)."""
import numpy as np

from env_obs_util import env_rescale64

STEPS, MAX_LEN = 12, 5              # two auto-resets per env
N_BALL, N_TREE = 321, 130           # a full group of 256, a full wave and a wave of one lane; the tree tests' size for the split form

_ONE = np.float32(1.0)
SPECIALS = np.array([1.0, -1.0, np.nextafter(_ONE, np.float32(2.0)), np.nextafter(-_ONE, np.float32(-2.0)), 1e30, -1e30,
                     np.inf, -np.inf, -0.0], dtype=np.float32)
PLANTED_ENVS = 8                    # each special value sits in this many different envs, in every step


def planted_positions(n, n_t):
    """(env [S, 8], tendon [S, 8]) of the planted values: special j, copy m in env (j + S m) stride, tendon (j + m) mod n_t - spread
    over the whole batch, the same in every step."""
    s = len(SPECIALS)
    if n < s * PLANTED_ENVS:
        raise ValueError("wide_actions needs at least %d envs" % (s * PLANTED_ENVS))
    stride = n // (s * PLANTED_ENVS)
    j, m = np.meshgrid(np.arange(s), np.arange(PLANTED_ENVS), indexing="ij")
    return (j + s * m) * stride, (j + m) % n_t


def wide_actions(n, n_t, steps, seed):
    """[steps, n, n_t] float32 from U(-2, 2) with SPECIALS planted at planted_positions in every step.  Never NaN: what a NaN action
    does is the caller's to avoid (include/roboy_sim.h), not pinned by these tests."""
    act = np.random.default_rng(seed).uniform(-2.0, 2.0, (steps, n, n_t)).astype(np.float32)
    env, ten = planted_positions(n, n_t)
    act[:, env, ten] = SPECIALS[:, None]
    assert not np.isnan(act).any()
    return act


def outside(act):
    """the entries outside the box [-1, 1]"""
    return np.abs(act) > 1.0


def narrow_box(robot, half=0.1):
    """`robot` with the set-point box [-half, half] m; the description - and with it the kernel instances that apply - untouched"""
    from gym_roboy_amd._gymcompat import spaces
    shape = robot.get_action_space().shape

    class NarrowBox(type(robot)):
        @classmethod
        def get_action_space(cls):
            return spaces.Box(low=-half, high=half, shape=shape, dtype="float32")
    return NarrowBox()


def clipped_rescale64(robot, act):
    """fp64 set-points (m) of the actions as every env-step kernel must apply them: clipped to [-1, 1], then into the box"""
    return env_rescale64(robot, np.clip(np.asarray(act, np.float64), -1.0, 1.0))


def raw_rescale64(robot, act):
    """the same map WITHOUT the clip: what a kernel that lost its clamp would apply"""
    box = robot.get_action_space()
    lo, hi = float(box.low[0]), float(box.high[0])
    return lo + (np.asarray(act, np.float64) + 1.0) * (hi - lo) / 2.0


# ---- the inputs of tests/test_action_box_gpu.py ----
def _turned():
    """MsjRobot turned by 90 degrees about z (tests/test_physics_gpu.py: the other mirror plane, kernarg constants)"""
    from gym_roboy_amd.envs.robots import MsjRobot
    from test_mirror_pairs import _rotated_msj
    desc = _rotated_msj()

    class Turned(MsjRobot):
        @classmethod
        def get_description(cls):
            return desc
    return Turned()


def _upper():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    return UpperBodyRobot()


def _robot(name):
    from test_env_params_gpu import _ball12, _kernarg_msj, _msj
    return {"msj_narrow": lambda: narrow_box(_msj()), "msj_shipped": _msj, "kernarg": _kernarg_msj, "turned": _turned,
            "ball12": _ball12, "upper": _upper}[name]()


# name: (envs, start state, seed).  "random": 0.9 of the joint limits, |qd| <= qd_max, written behind reset(); "rest": reset()'s.
# MsjRobot with its own box from the rest pose is NOT here and must not be (see the module docstring).
INPUTS = {"msj_narrow": (N_BALL, "random", 31), "msj_shipped": (N_BALL, "random", 32), "kernarg": (N_BALL, "random", 33),
          "turned": (N_BALL, "random", 34), "ball12": (N_BALL, "random", 35), "upper": (N_TREE, "rest", 36)}
RESET_ROW_INPUTS = ("msj_narrow", "ball12")       # the robots of the cases that read tendon columns on auto-reset rows

_cache = {}


def inputs(name):
    """(robot, desc, q, qd, actions [STEPS, n, n_t]) of INPUTS[name]: computed once, shared, read-only"""
    if name not in _cache:
        n, start, seed = INPUTS[name]
        robot = _robot(name)
        desc = robot.get_description()
        rng = np.random.default_rng(seed)
        if start == "random":
            q = rng.uniform(0.9 * desc.q_lo, 0.9 * desc.q_hi, (n, desc.n_q)).astype(np.float32)
            qd = rng.uniform(-desc.qd_max, desc.qd_max, (n, desc.n_q)).astype(np.float32)
        else:
            q, qd = np.zeros((n, desc.n_q), np.float32), np.zeros((n, desc.n_q), np.float32)
        act = wide_actions(n, desc.n_t, STEPS, seed)
        for a in (q, qd, act):
            a.setflags(write=False)
        _cache[name] = (robot, desc, q, qd, act)
    return _cache[name]
