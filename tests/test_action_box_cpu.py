"""The INPUTS of tests/test_action_box_gpu.py, qualified without a GPU: every (robot, box, start state) it steps must be one where
dropping the action clamp changes the result - otherwise "raw equals clipped" would hold of a kernel without a clamp too (MsjRobot
with its own box at the rest pose is such a combination: the activation is saturated at both box edges).  These are conditions on
the test inputs, not tolerances on any kernel."""
import numpy as np
import pytest

from action_box_util import (INPUTS, PLANTED_ENVS, RESET_ROW_INPUTS, SPECIALS, clipped_rescale64, inputs, narrow_box, outside,
                             planted_positions, raw_rescale64, wide_actions)
from env_obs_util import column_tolerances, env_rescale64, expected_columns, readout64

MOVED, SHARE = 1e-4, 0.25


def _moved_share(desc, q, qd, sp_raw, sp_clip, has_outside):
    """share of the envs holding an out-of-box entry whose q or qd after one fp64 step differs by more than 1e-4 (a state that is
    not finite under the raw set-points differs)"""
    from oracle.c_oracle import COracle
    orc = COracle(desc, "f64")
    with np.errstate(all="ignore"):
        a, b = orc.step(q, qd, sp_raw), orc.step(q, qd, sp_clip)
        diff = np.maximum(np.abs(a[0] - b[0]).max(axis=1), np.abs(a[1] - b[1]).max(axis=1))
    assert np.isfinite(b[0]).all() and np.isfinite(b[1]).all()
    return float(np.mean(~(diff[has_outside] <= MOVED)))


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_dropping_the_clamp_moves_the_first_step(name):
    robot, desc, q, qd, act = inputs(name)
    a0 = act[0]
    has_outside = outside(a0).any(axis=1)
    assert has_outside.mean() > 0.9
    sp_raw = raw_rescale64(robot, np.clip(a0, -1e30, 1e30))       # +-inf as +-1e30: the oracle's activation clips either to 0 or 1
    share = _moved_share(desc, q, qd, sp_raw, clipped_rescale64(robot, a0), has_outside)
    print("%s: %.0f %% of the envs with an out-of-box entry move by more than %g without the clamp" % (name, 100 * share, MOVED))
    assert share >= SHARE


def test_msj_robot_with_its_own_box_at_the_rest_pose_would_prove_nothing():
    """the combination the GPU file must not use, kept here as the reason: nothing moves at all"""
    from test_env_params_gpu import _msj
    robot = _msj()
    desc = robot.get_description()
    n = 321
    a0 = wide_actions(n, desc.n_t, 1, 1)[0]
    z = np.zeros((n, 3))
    share = _moved_share(desc, z, z, raw_rescale64(robot, np.clip(a0, -1e30, 1e30)), clipped_rescale64(robot, a0), outside(a0).any(axis=1))
    assert share == 0.0


@pytest.mark.parametrize("name", RESET_ROW_INPUTS)
def test_dropping_the_clamp_moves_the_tendon_columns_of_a_reset_row(name):
    """An env that auto-resets reports its tendon columns at the zero pose under the action just applied (csrc/env_obs.hpp,
    csrc/env_io.hpp: the refresh of the reset rows): there the activation or the force must tell raw from clipped by more than ten
    tolerances in a quarter of the out-of-box entries."""
    robot, desc, _, _, act = inputs(name)
    a0 = act[0]
    n, nt = a0.shape
    z = np.zeros((n, 3))
    ch = ("activation", "force")
    clip_cols, o = expected_columns(robot, desc, z, z, np.clip(a0, -1, 1), ch)
    again, _ = expected_columns(robot, desc, z, z, a0, ch)
    assert np.array_equal(clip_cols, again)                        # expected_columns clips: the raw columns come from the readout itself
    with np.errstate(all="ignore"):
        raw = readout64(desc, z, z, raw_rescale64(robot, np.clip(a0, -1e30, 1e30)))[0]
    raw_cols = np.concatenate([raw[c] for c in ch], axis=1)
    tol = column_tolerances(o, ch)
    far = ~(np.abs(raw_cols - clip_cols) <= 10 * tol)
    far = far[:, :nt] | far[:, nt:]
    share = float(far[outside(a0)].mean())
    print("%s: %.0f %% of the out-of-box entries differ by more than 10 tolerances in activation or force at the zero pose" % (name, 100 * share))
    assert share >= SHARE
    assert not far[~outside(a0)].any()


@pytest.mark.parametrize("n,n_t", [(321, 8), (321, 12), (130, 38), (1000, 5)])
def test_wide_actions_hold_the_planted_values_and_no_nan(n, n_t):
    act = wide_actions(n, n_t, 12, 7)
    assert act.dtype == np.float32 and act.shape == (12, n, n_t) and not np.isnan(act).any()
    assert np.array_equal(act, wide_actions(n, n_t, 12, 7))
    env, ten = planted_positions(n, n_t)
    assert len(np.unique(env)) == env.size == len(SPECIALS) * PLANTED_ENVS and env.max() < n
    for t in range(12):
        for j, v in enumerate(SPECIALS):
            got = act[t, env[j], ten[j]]
            assert np.array_equal(got, np.full(PLANTED_ENVS, v)) and np.array_equal(np.signbit(got), np.full(PLANTED_ENVS, np.signbit(v)))
    for v in (1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2)), 1e30, -1e30, np.inf, -np.inf):
        assert len(np.unique(np.nonzero(act[0] == np.float32(v))[0])) >= 8
    assert len(np.unique(np.nonzero((act[0] == 0) & np.signbit(act[0]))[0])) >= 8
    body = np.abs(act[np.isfinite(act) & (np.abs(act) < 1e29)])
    assert body.max() <= 2.0 and 0.4 < np.mean(body > 1.0) < 0.6   # about half of all entries lie outside the box
    assert 1.0 < SPECIALS[2] < 1.0000002 and -1.0000002 < SPECIALS[3] < -1.0


def test_narrow_box_changes_the_box_and_nothing_else():
    from test_env_params_gpu import _msj
    base = _msj()
    robot = narrow_box(base)
    box = robot.get_action_space()
    assert np.all(box.low == np.float32(-0.1)) and np.all(box.high == np.float32(0.1)) and box.shape == base.get_action_space().shape
    assert robot.get_description() is base.get_description() and isinstance(robot, type(base))
    assert np.all(base.get_action_space().high == np.float32(0.3))
    a = np.array([[-np.inf, -2.0, -1.0, 0.0, 0.5, 1.0, 1e30, np.inf]])
    want = np.array([[-0.1, -0.1, -0.1, 0.0, 0.05, 0.1, 0.1, 0.1]])
    assert np.allclose(clipped_rescale64(robot, a), want, atol=1e-8) and np.array_equal(clipped_rescale64(robot, a), env_rescale64(robot, a))
    assert np.allclose(raw_rescale64(robot, a[:, 1:6]), 0.1 * a[:, 1:6], atol=1e-8)
