"""The action-box clamp of every fused env-step kernel form on the GPU (include/roboy_sim.h: rb_env_step_dev).  The clamp is
written out in eleven places (NEXT.md, hand-over notes), and PPO's fused rollout hands the kernels the policy's raw Gaussian
samples - a third of them outside [-1, 1] at log_std = 0 - so out-of-box actions are these kernels' ordinary input.

3a. Two identical handles, A stepped with actions from U(-2, 2) with +-1, their fp32 neighbours outside the box, +-1e30, +-inf and
    -0.0 planted (tests/action_box_util.py), B with np.clip of the same array: 12 steps, episodes of 5, every output of every step
    bit-equal.  One case at least per place that holds the clamp, the form that ran asserted wherever the handle tells.
3b. A's first step against the fp64 C oracle at the fp64 rescale of the CLIPPED actions, one case per kernel family, within the
    tolerances of tests/test_physics_gpu.py and tests/test_tree_robot_gpu.py.

The inputs are qualified in tests/test_action_box_cpu.py: on each of them a step without the clamp lands elsewhere."""
import numpy as np
import pytest

from action_box_util import INPUTS, MAX_LEN, STEPS, clipped_rescale64, inputs, outside
from env_obs_util import CHANNELS, channels_of
from gym_roboy_amd import _native as nat
from test_env_golden_gpu import pin_form
from test_env_io_gpu import SIGMA, _io_cfg, _plane, _set_delay, _start
from test_env_obs_gpu import _vec
from test_physics_gpu import TOL as BALL_TOL
from test_tree_robot_gpu import LANE, OCTET, SPLIT, SPLIT2, TOL as TREE_TOL

pytestmark = pytest.mark.gpu

REFUSES = {"params": "per-env parameters are enabled", "channels": "tendon channels are set", "io": "io configuration"}


def _case(copies, inp, integ, kernel=None, row=(), form="nominal", mask=0, io=None):
    """copies: the places of the clamp this case runs (numbers of NEXT.md's list).  kernel: rb_select_kernel's form (ball joints: pinned
    by row name, with the parts `row` of the row's id; joint trees: rb_info's kernel).  form: 'nominal', 'params' (nominal planes),
    'randomized' (redrawn on auto-reset).  mask: tendon channels.  io: None, 'plane' (noise on the selected channels, delay plane
    i mod 4) or 'redraw' (noise on all columns, delays 0-3 redrawn on auto-reset)."""
    parts = ["c" + "+".join(map(str, copies)), inp, integ] + (["k%d" % kernel] if kernel else []) + ([form] if form != "nominal" else []) \
        + (["mask%d" % mask] if mask else []) + (["io-" + io] if io else [])
    return pytest.param(dict(copies=copies, inp=inp, integ=integ, kernel=kernel, row=row, form=form, mask=mask, io=io), id="-".join(parts))


CASES = [
    # 1: RB_MSJ_ENV_STEP_BODY - env per lane, baked / kernarg / ConstX instances, its tendon-channel and io expansions
    _case((1,), "msj_narrow", "euler", kernel=1, row=("ball8/", "/table/")),
    _case((1,), "msj_shipped", "rk4", kernel=1, row=("ball8/", "/table/")),
    _case((1,), "kernarg", "euler", kernel=1, row=("ball8/", "/kernarg/")),
    _case((1,), "ball12", "rk4", kernel=1, row=("ballx/",)),
    _case((1,), "msj_narrow", "rk4", mask=9),
    _case((1,), "msj_narrow", "euler", mask=9, io="plane"),
    # 2: two lanes per env, both mirror planes (the turned robot: kernarg constants)
    _case((2,), "msj_narrow", "rk4", kernel=5, row=("/table/",)),
    _case((2,), "turned", "euler", kernel=5, row=("/kernarg/",)),
    # 3: eight lanes per env
    _case((3,), "msj_narrow", "rk4", kernel=2),
    # 4: the parameter body, nominal planes and planes redrawn on auto-reset
    _case((4,), "msj_narrow", "euler", form="params"),
    _case((4,), "msj_narrow", "rk4", form="randomized"),
    _case((4,), "kernarg", "rk4", form="params"),
    _case((4,), "kernarg", "euler", form="randomized"),
    _case((4,), "ball12", "euler", form="params"),
    _case((4,), "ball12", "rk4", form="randomized"),
    # 5: the refresh of the rows of auto-reset envs, parameter form + tendon channels
    _case((4, 5), "msj_narrow", "euler", form="randomized", mask=15),
    _case((4, 5), "ball12", "rk4", form="randomized", mask=15),
    # 6: the same with an io configuration
    _case((4, 6), "msj_narrow", "rk4", form="randomized", mask=15, io="redraw"),
    _case((4, 6), "ball12", "euler", form="randomized", mask=15, io="redraw"),
    # 7 - 10: joint trees - octets, one wave per 64 envs, the split form (part and helper waves), the lean two-part form
    _case((7,), "upper", "euler", kernel=OCTET),
    _case((8,), "upper", "euler", kernel=LANE),
    _case((9, 10), "upper", "euler"),
    _case((9, 10), "upper", "rk4"),
    _case((9,), "upper", "euler", kernel=SPLIT2),
]


def _open(c):
    """A configured handle of the case, the form its env step takes asserted"""
    robot, desc, _, _, _ = inputs(c["inp"])
    n = INPUTS[c["inp"]][0]
    ch = channels_of(c["mask"])
    env = _vec(robot, n, c["integ"], tendon_obs=ch or None, seed=5, max_len=MAX_LEN, randomization=True if c["form"] == "randomized" else None)
    try:
        if c["form"] == "params":
            env.sim.enable_params()
        if c["io"]:
            env.sim.configure_io(_io_cfg(SIGMA, ch, delay=(0, 3)) if c["io"] == "plane" else _io_cfg(SIGMA, CHANNELS, delay=(0, 3), resample=True))
            assert env.sim.io_ptrs()["slots"] == 4
            if c["io"] == "plane":
                _set_delay(env, np.arange(n) % 4)
        if c["inp"] == "upper":
            if c["kernel"]:
                env.sim.select_kernel(c["kernel"])
            assert env.sim.info()["kernel"] == (c["kernel"] or SPLIT)          # the library's choice at 130 envs: the split form
        elif c["kernel"]:
            row = pin_form(env, c["kernel"])
            assert all(part in row["id"] for part in c["row"]), row["id"]
        else:
            # no row to name: an extension's kernels run, and the dispatch query says so (parameters first, then io, then channels)
            assert env.obs_dim == 9 + len(ch) * desc.n_t
            why = REFUSES["params" if c["form"] != "nominal" else "io" if c["io"] else "channels"]
            with pytest.raises(nat.NativeError, match=why):
                env.sim.dispatch("env_step")
    except BaseException:
        env.close()
        raise
    return env


def _same(t, name, a, b, done):
    """array_equal with a message that says where: which columns, and whether only on the envs that reset in this step"""
    if np.array_equal(a, b):
        return
    bad = a != b
    rows = np.nonzero(bad.reshape(len(a), -1).any(axis=1))[0]
    cols = np.nonzero(bad.reshape(len(a), -1).any(axis=0))[0]
    with np.errstate(all="ignore"):
        worst = np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))[bad])
    raise AssertionError("step %d: %s of raw and clipped actions differ in %d entries of %d envs (first env %d), columns %d..%d, "
                         "max |difference| %.3g; all of them envs that were done in this step: %s"
                         % (t, name, bad.sum(), len(rows), rows[0], cols.min(), cols.max(), worst, bool(done[rows].all())))


@pytest.mark.parametrize("c", CASES)
def test_raw_actions_give_bit_for_bit_what_clipped_actions_give(c, monkeypatch):
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")                  # a kernarg robot runs its kernarg rows
    _, desc, q, qd, act = inputs(c["inp"])
    clipped = np.clip(act, -1, 1)
    assert clipped.dtype == np.float32 and np.mean(outside(act)) > 0.4 and not outside(clipped).any()
    envs = []
    try:
        envs = [_open(c), _open(c)]
        a0, b0 = (_start(env, q, qd) for env in envs)
        assert np.array_equal(a0, b0)
        n = len(q)
        n_done, done_outside = np.zeros(n, int), 0
        for t in range(STEPS):
            ra = envs[0].step(act[t])[:3] + tuple(envs[0].sim.read_state())
            rb = envs[1].step(clipped[t])[:3] + tuple(envs[1].sim.read_state())
            done = ra[2]
            for name, x, y in zip(("obs", "reward", "done", "q", "qd", "feasible"), ra, rb):
                _same(t, name, x, y, done | rb[2])
            assert np.isfinite(ra[0]).all() and np.isfinite(ra[1]).all()
            n_done += done
            done_outside += int(np.sum(done & outside(act[t]).any(axis=1)))
        assert envs[0].stats() == envs[1].stats()
        assert n_done.min() >= 2                               # two auto-resets per env ...
        assert done_outside >= n                               # ... on steps whose action held an out-of-box entry (the reset rows' refresh)
        if c["io"]:
            for name in ("rows", "delay", "delay_draws"):
                assert np.array_equal(_plane(envs[0], name), _plane(envs[1], name)), name
            assert np.array_equal(_plane(envs[0], "rows"), np.full(n, 1 + STEPS, np.uint32))
            if c["io"] == "plane":                             # no reset redrew it: the delays 0-3 were the ones that ran
                assert np.array_equal(_plane(envs[0], "delay"), np.arange(n) % 4)
        if c["form"] == "randomized":
            assert np.array_equal(envs[0].sim.get_param_planes(), envs[1].sim.get_param_planes())
    finally:
        for env in envs:
            env.close()


FAMILIES = [
    _case((1,), "msj_narrow", "euler", kernel=1, row=("ball8/", "/table/")),
    _case((3,), "msj_narrow", "rk4", kernel=2),
    _case((2,), "msj_narrow", "euler", kernel=5),
    _case((4,), "ball12", "rk4", form="params"),
    _case((7,), "upper", "euler", kernel=OCTET),
    _case((9, 10), "upper", "rk4"),
]


@pytest.mark.parametrize("c", FAMILIES)
def test_first_step_with_raw_actions_matches_fp64_at_the_clipped_set_points(c, monkeypatch):
    """State after one env step with the wide actions against COracle(desc, "f64").step at the fp64 rescale of the clipped actions;
    feasibility flags as tests/test_physics_gpu.py's _check_step takes them (a mismatch only within 1e-5 of a joint limit)."""
    from oracle.c_oracle import COracle
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    robot, desc, q, qd, act = inputs(c["inp"])
    tol = TREE_TOL if c["inp"] == "upper" else BALL_TOL
    env = _open(c)
    try:
        _start(env, q, qd)
        _, _, done, _ = env.step(act[0])
        q1, qd1, f1 = env.sim.read_state()
    finally:
        env.close()
    qo, qdo, fo = COracle(desc, "f64").step(q, qd, clipped_rescale64(robot, act[0]), integrator=0 if c["integ"] == "euler" else 1)
    live = ~done                                               # an env that reached its goal in this step holds the reset's state
    assert live.mean() > 0.99
    eq, eqd = np.abs(q1 - qo)[live].max(), np.abs(qd1 - qdo)[live].max()
    print("%s: max |q - q64| %.3g, max |qd - qd64| %.3g (tolerance %g)" % (c["inp"], eq, eqd, tol))
    assert eq < tol and eqd < tol
    near = np.minimum(np.abs(qo - desc.q_lo), np.abs(qo - desc.q_hi)).min(axis=1) < 1e-5
    assert not np.any((f1 != fo) & ~near & live)
    from limit_edge_util import decided_envs                   # ... and wherever the oracle's angle before the clamp is clear of every limit
    assert not np.any((f1 != fo) & live & decided_envs(desc, q, qd, clipped_rescale64(robot, act[0]), c["integ"], 1, tol))
