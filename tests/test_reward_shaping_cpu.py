"""Reward shaping without a GPU: the option's spec and the trainer's command-line form accept and reject what the
contract says, and self-checks of tests/shaping_util.py's float64 statement, which the GPU tests hold the kernels to."""
import numpy as np
import pytest

import shaping_util as su
from conftest import random_states
from gym_roboy_amd import _native as nat
from gym_roboy_amd.envs.vec_env import parse_reward_shaping, reward_shaping_weights


def test_spec_accepts_and_rejects():
    assert nat.REWARD_SHAPING_TERMS == su.TERMS
    assert reward_shaping_weights(None) is None
    assert reward_shaping_weights({}) is None
    assert reward_shaping_weights({"action_rate": 0, "tension": 0.0}) is None
    got = reward_shaping_weights({"tension": 0.01})
    assert got == {"action_rate": 0.0, "tension": float(np.float32(0.01)), "activation": 0.0} and list(got) == list(su.TERMS)
    assert reward_shaping_weights({"action_rate": np.float32(0.5), "activation": 2})["activation"] == 2.0
    for bad in ({"jerk": 1.0}, {"tension": -0.1}, {"action_rate": np.inf}, {"activation": np.nan}, {"tension": True}):
        with pytest.raises(ValueError):
            reward_shaping_weights(bad)


def test_command_line_form():
    assert parse_reward_shaping("") is None and parse_reward_shaping(None) is None
    assert parse_reward_shaping("action_rate=0.05,tension=0.01") == {"action_rate": 0.05, "tension": 0.01}
    assert parse_reward_shaping("activation=1e-3,") == {"activation": 1e-3}
    for bad in ("action_rate", "action_rate=x", "speed=1", "tension=-1", "tension=1,tension=2", "activation=inf"):
        with pytest.raises(ValueError):
            parse_reward_shaping(bad)


def test_binding_declares_the_entry_points():
    import ctypes
    assert ctypes.sizeof(nat.EnvShapingConfig) == 16
    assert [f[0] for f in nat.EnvShapingConfig._fields_][:3] == list(su.TERMS)
    for name in ("rb_env_shaping_configure", "rb_env_shaping_cost_ptr", "rb_env_shaping_stats"):
        assert name in nat.SIGNATURES
    header = open(nat.os.path.join(nat._HERE, "..", "include", "roboy_sim.h")).read()
    for name in ("rb_env_shaping_configure", "rb_env_shaping_cost_ptr", "rb_env_shaping_stats", "rb_env_shaping_config"):
        assert name in header


def _msj(n=64, seed=5):
    from gym_roboy_amd.envs.robots import MsjRobot
    robot = MsjRobot()
    desc = robot.get_description()
    q, qd, _ = random_states(desc, n, seed)
    rng = np.random.default_rng(seed + 1)
    act, prev = (rng.uniform(-1.5, 1.5, (n, desc.n_t)).astype(np.float32) for _ in range(2))
    first = np.arange(n) % 4 == 0
    return robot, desc, q, qd, act, prev, first


def test_statement_zero_weights_first_steps_and_clamp():
    robot, desc, q, qd, act, prev, first = _msj()
    assert not su.cost64(desc, robot, q, qd, act, prev, first, {}).any()
    rate = su.cost64(desc, robot, q, qd, act, prev, first, {"action_rate": 1.0})
    assert not rate[first].any() and np.all(rate[~first] > 0)
    assert np.array_equal(rate, su.cost64(desc, robot, q, qd, np.clip(act, -1, 1), np.clip(prev, -1, 1), first, {"action_rate": 1.0}))
    assert np.allclose(rate[~first], np.mean((np.clip(act, -1, 1).astype(np.float64) - np.clip(prev, -1, 1)) ** 2, axis=1)[~first], rtol=1e-15)
    # weights enter as the float32 values the library holds, and linearly
    both = su.cost64(desc, robot, q, qd, act, prev, first, {"tension": 0.5, "activation": 0.25})
    t, _, _ = su.terms64(desc, robot, q, qd, act, prev, first)
    assert np.allclose(both, 0.5 * t[1] + 0.25 * t[2], rtol=1e-15) and np.all(t[1] >= 0) and np.all((t[2] >= 0) & (t[2] <= 1))
    assert np.array_equal(su.rate64(np.stack((prev, act)), np.zeros((2, len(first)), bool))[1][~first], t[0][~first])
    tol = su.cost_tolerance(desc, robot, q, qd, act, prev, first, su.ALL)
    assert np.all(tol > 0) and np.all(tol < 1e-3 * su.cost64(desc, robot, q, qd, act, prev, first, su.ALL) + 1e-6)


def test_rate_term_is_invariant_under_the_tendon_permutation():
    robot, desc, q, qd, act, prev, first = _msj()
    w = {"action_rate": 0.7}
    image = 7 - np.arange(8)
    a = su.cost64(desc, robot, q, qd, act, prev, first, w)
    b = su.cost64(desc, robot, q, qd, act[:, image], prev[:, image], first, w)
    assert np.abs(a - b).max() <= 1e-15


def test_cost_of_a_mirrored_pair_is_the_originals():
    """symmetry="augment" stays valid under the option: the twin (M s, P a) of a transition costs what the original costs"""
    from gym_roboy_amd.envs.symmetry import mirror_rows, row_mirror_map
    from symmetry_util import JOINT_SIGN, MSJ_IMAGE
    robot, desc, q, qd, act, prev, first = _msj()
    src, sign, act_src = row_mirror_map(desc.n_q, desc.n_t, JOINT_SIGN[0], MSJ_IMAGE)
    obs = np.concatenate((q, qd, np.zeros_like(q)), axis=1)
    m = mirror_rows(obs, src, sign)
    mq, mqd = m[:, :desc.n_q], m[:, desc.n_q:2 * desc.n_q]
    a = su.cost64(desc, robot, q, qd, act, prev, first, su.ALL)
    b = su.cost64(desc, robot, mq, mqd, mirror_rows(act, act_src), mirror_rows(prev, act_src), first, su.ALL)
    assert a.max() > 0 and np.abs(a - b).max() <= 1e-12
