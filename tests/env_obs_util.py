"""TEST HELPER for the tendon channels in the fused env step's observation (include/roboy_sim.h: rb_env_obs_*): the
expected tendon columns in fp64 from the oracle (oracle/physics_np.TendonRobotOracle: tendon_geometry, muscle_force), the env
layer's rescale and each env's own physical parameters (tests/env_params_util.py), in the conventions of
tests/test_tendon_state_cpu.py (_oracle_readout): length m, rate m/s (> 0 lengthening), activation in [0, 1], force N."""
import numpy as np

CHANNELS = ("length", "rate", "activation", "force")
BITS = {"length": 1, "rate": 2, "activation": 4, "force": 8}


def mask_of(channels):
    return sum(BITS[c] for c in channels)


def channels_of(mask):
    return tuple(c for c in CHANNELS if mask & BITS[c])


def env_rescale64(robot, act):
    """The env layer's rescale of actions in [-1, 1] (clamped) into the robot's set-point box, fp64."""
    box = robot.get_action_space()
    lo, hi = float(box.low[0]), float(box.high[0])
    return lo + (np.clip(np.asarray(act, np.float64), -1.0, 1.0) + 1.0) * (hi - lo) / 2.0


def readout64(desc, q, qd, sp, par=None):
    """{'length', 'rate', 'activation', 'force'} [n, n_t] in fp64 at the states q, qd under the set-points sp (m).  par [n, P]:
    each env's parameters (planes of rb_params_*, env-major) - the set-point offset adds to sp, the force scale multiplies f_max;
    mass and damping scales do not enter a tendon's state.  Vectorised over the envs: the tendon force is linear in f_max, so
    env i's force is the nominal robot's times force_scale[i] (test_env_obs_cpu checks this against env_params_util.perturbed)."""
    from oracle.physics_np import TendonRobotOracle
    o = TendonRobotOracle(desc)
    q, qd, sp = (np.asarray(a, np.float64) for a in (q, qd, sp))
    nt = desc.n_t
    fs = np.ones_like(sp)
    if par is not None:
        par = np.asarray(par, np.float64)
        sp = sp + par[:, nt:2 * nt]
        fs = par[:, :nt]
    length, L = o.tendon_geometry(q)
    rate = np.einsum("nkj,nj->nk", L, qd)
    act = np.clip(o.kp * (length - o.l0 - o.sigma * sp) / o.l0, 0.0, 1.0)
    return {"length": length, "rate": rate, "activation": act, "force": o.muscle_force(length, rate, sp) * fs}, o


def expected_columns(robot, desc, q, qd, actions, channels, scale=None, par=None):
    """The tendon columns [n, C n_t] (fp64) of the rows an env step reports at (q, qd) after applying `actions` (in [-1, 1];
    None: every set-point 0, the reset's row), channels in row order, each times its scale."""
    n = np.asarray(q).shape[0]
    sp = np.zeros((n, desc.n_t)) if actions is None else env_rescale64(robot, actions)
    ref, o = readout64(desc, q, qd, sp, par)
    scale = dict(scale or {})
    cols = [ref[c] * float(scale.get(c, 1.0)) for c in CHANNELS if c in channels]
    return np.concatenate(cols, axis=1), o


def column_tolerances(o, channels, scale=None):
    """[C n_t] tolerances of the fp32 columns against fp64: the readout's own (tests/test_tendon_state_gpu.py: _tolerances) times
    |scale| per channel"""
    from test_tendon_state_gpu import _tolerances
    tol = _tolerances(o)
    scale = dict(scale or {})
    return np.concatenate([tol[c] * abs(float(scale.get(c, 1.0))) for c in CHANNELS if c in channels])
