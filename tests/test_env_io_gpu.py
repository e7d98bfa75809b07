"""Action latency and sensor noise of the fused env step on the GPU (include/roboy_sim.h: rb_env_io_*; csrc/env_io.hpp; DESIGN.md
§14): a configuration of zeros against the unconfigured handle, the noise against its fp64 restatement (tests/env_io_util.py), the
delay against a handle fed the shifted action sequence, the delay's redraw, both with parameters and tendon columns, graphs,
refusals, and PPO as a consumer.

Shapes: 321 envs = one full group of 256, then a full wave and a wave of one lane (the staged rows, the last wave's fallback, the
bounds); 577 envs where a sub-range is needed (ranges start at multiples of 256); episodes of 5 steps, 12 steps per run: two auto-resets per env."""
import ctypes

import numpy as np
import pytest

from env_io_util import NOISE_TOL, DelayBook, column_sigmas, delay_draw, sensor_noise64
from env_obs_util import channels_of, column_tolerances, env_rescale64, expected_columns
from gym_roboy_amd import _native as nat
from test_env_obs_gpu import RANGES, ROBOTS, _actions, _state, _vec
from test_env_params_gpu import _ball12, _msj

pytestmark = pytest.mark.gpu

N, N_RANGE, STEPS, MAX_LEN = 321, 577, 12, 5
SIGMA = {"q": 0.01, "qd": 0.05, "length": 5e-4, "rate": 1e-3, "activation": 0.02, "force": 2.0}


def _io_cfg(sigma=None, channels=(), delay=(0, 0), resample=False):
    cfg = nat.EnvIoConfig()
    sigma = sigma or {}
    cfg.sigma_q, cfg.sigma_qd = sigma.get("q", 0.0), sigma.get("qd", 0.0)
    for c, name in enumerate(("length", "rate", "activation", "force")):
        cfg.sigma_tendon[c] = sigma.get(name, 0.0) if name in channels else 0.0
    cfg.delay_lo, cfg.delay_hi, cfg.resample_on_reset = delay[0], delay[1], int(resample)
    return cfg


def _plane(env, name, dtype=np.uint32):
    env.sim.synchronize()
    return env.sim.download(env.sim.io_ptrs()[name], (env.num_envs,), dtype)


def _set_delay(env, d):
    env.sim.synchronize()
    env.sim.upload(env.sim.io_ptrs()["delay"], np.ascontiguousarray(d, dtype=np.uint32))


def _start(env, q, qd):
    """reset (row 0), then the given state under the reset's goal; returns the reset rows"""
    obs0 = env.reset()
    env.sim.set_state(q, qd)
    return obs0


def _run(env, q, qd, acts):
    """reset, the given state, then the actions: the reset rows, every output of every step and the statistics"""
    obs0 = _start(env, q, qd)
    out = []
    for a in acts:
        obs, rew, done, _ = env.step(a)
        out.append((obs, rew, done) + tuple(env.sim.read_state()))
    return obs0, out, env.stats()


def _make(which, n, integ, form, mask, scale=None, seed=5, **kw):
    env = _vec(ROBOTS[which](), n, integ, tendon_obs=channels_of(mask) or None, scale=scale, seed=seed, max_len=MAX_LEN,
               randomization=True if form == "randomized" else None, **kw)
    if form == "params":
        env.sim.enable_params()                   # the parameter kernels on nominal planes
    return env


def _inputs(which, n, seed):
    desc = ROBOTS[which]().get_description()
    rng = np.random.default_rng(seed)
    q, qd = _state(desc, n, rng)
    return desc, q, qd, _actions(desc, n, rng, STEPS)


# ---- 1. configured with zeros = not configured ----
@pytest.mark.parametrize("mask", [0, 9])
@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("which", ["baked", "kernarg", "ball12"])
@pytest.mark.parametrize("form", ["nominal", "params"])
def test_a_configuration_of_zeros_is_no_configuration(form, which, integ, mask, monkeypatch):
    """sigma = 0, delay = 0: obs, reward, done, state and statistics of 12 steps (two auto-resets) are, bit for bit, those of the
    handle without io - which runs the extended kernel (mask 9), the parameter kernel, or its env-per-lane row (hiprtc off, so that a
    kernarg robot runs its kernarg row)."""
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    desc, q, qd, acts = _inputs(which, N, 1)
    res = []
    for io in (False, True):
        env = _make(which, N, integ, form, mask)
        try:
            if form == "nominal" and not mask:
                env.sim.select_kernel(1)
                if not io:
                    assert "/env_per_lane/" in env.sim.dispatch("env_step")["id"]
            if io:
                env.sim.configure_io(_io_cfg())
                assert env.sim.io_ptrs()["history"] is None and env.sim.io_ptrs()["slots"] == 0      # no ring without a delay
            res.append(_run(env, q, qd, acts))
            if io:
                assert not _plane(env, "delay").any() and not _plane(env, "rows").any()
        finally:
            env.close()
    (ref0, ref, ref_stats), (got0, got, got_stats) = res
    assert np.array_equal(ref0, got0)
    n_done = np.zeros(N, int)
    for t, (r, g) in enumerate(zip(ref, got)):
        for a, b in zip(r, g):
            assert np.array_equal(a, b), (t, np.abs(a.astype(np.float64) - b).max())
        n_done += r[2]
    assert n_done.min() >= 2 and ref_stats == got_stats


# ---- 2. the noise ----
def _check_noise(desc, obs_a, obs_b, z, colsig, what):
    """|(obs_A - obs_B) - sigma scale z64| <= sigma |scale| NOISE_TOL + 4 ulp(|obs_A|) on every noised column; the others bit-equal"""
    noised = colsig != 0
    diff = obs_a.astype(np.float64) - obs_b.astype(np.float64)
    err = np.abs(diff - colsig * z)[:, noised]
    bound = (np.abs(colsig) * NOISE_TOL + 4 * np.spacing(np.abs(obs_a)).astype(np.float64))[:, noised]
    worst = (err / bound).max()
    print("%s: worst |noise - restated| / bound = %.3g, max error in sigmas %.3g" % (what, worst, (err / np.abs(colsig[noised])).max()))
    assert worst <= 1.0, what
    assert np.array_equal(obs_a[:, ~noised], obs_b[:, ~noised]), what
    assert np.mean(diff[:, noised] != 0) > 0.99


NOISE_CASES = [("baked", "euler", "nominal", 9), ("baked", "rk4", "randomized", 15), ("kernarg", "rk4", "params", 0),
               ("kernarg", "euler", "nominal", 6), ("ball12", "euler", "nominal", 0), ("ball12", "rk4", "randomized", 10)]


@pytest.mark.parametrize("which,integ,form,mask", NOISE_CASES)
def test_noise_is_the_restated_draw_and_touches_nothing_else(which, integ, form, mask, monkeypatch):
    """Handle A with noise, handle B without io, the same seed and actions, 12 steps with auto-resets (and redrawn parameters):
    reward, done, state and the goal columns bit-equal, every noised column the restated draw of (seed, env, row number) - the reset
    rows are row 0, rows count on through an auto-reset."""
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    desc, q, qd, acts = _inputs(which, N, 2)
    ch = channels_of(mask)
    scale = {"force": 1 / 400, "length": -4.0} if which == "baked" else None
    res = []
    for io in (True, False):
        env = _make(which, N, integ, form, mask, scale=scale, seed=7)
        try:
            if form == "nominal" and not mask:
                env.sim.select_kernel(1)
            if io:
                env.sim.configure_io(_io_cfg(SIGMA, ch))
                assert np.array_equal(_plane(env, "rows"), np.zeros(N, np.uint32))
            res.append(_run(env, q, qd, acts))
            if io:
                assert np.array_equal(_plane(env, "rows"), np.full(N, 1 + STEPS, np.uint32))
        finally:
            env.close()
    (a0, a, a_stats), (b0, b, b_stats) = res
    colsig = column_sigmas(3, desc.n_t, ch, SIGMA, scale)
    od = 9 + len(ch) * desc.n_t
    assert colsig.shape == (od,) and not colsig[6:9].any()
    gids = np.arange(N, dtype=np.uint64)
    _check_noise(desc, a0, b0, sensor_noise64(7, gids, 0, od), colsig, "reset rows")
    n_done = np.zeros(N, int)
    for t, (ra, rb) in enumerate(zip(a, b)):
        for x, y in zip(ra[1:], rb[1:]):                         # reward, done, q, qd, feasible
            assert np.array_equal(x, y), t
        _check_noise(desc, ra[0], rb[0], sensor_noise64(7, gids, t + 1, od), colsig, "step %d" % t)
        n_done += ra[2]
    assert n_done.min() >= 2 and a_stats == b_stats


@pytest.mark.parametrize("which,form,mask", [("baked", "nominal", 9), ("ball12", "randomized", 15), ("kernarg", "params", 0)])
def test_noise_is_keyed_by_the_global_env_id_and_sub_ranges_give_the_same_rows(which, form, mask):
    """A handle at env_id_offset = 1000: its rows carry the draws of the envs 1000 ..., and the batch stepped as two sub-ranges on two
    streams gives, bit for bit, the rows of the batch stepped whole."""
    import torch
    n, h = N_RANGE, 256
    desc, q, qd, acts = _inputs(which, n, 3)
    ch = channels_of(mask)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for mode in ("whole", "split", "quiet"):
        env = _make(which, n, "euler", form, mask, seed=3, env_id_offset=1000)
        try:
            if mode != "quiet":
                env.sim.configure_io(_io_cfg(SIGMA, ch, delay=(0, 3)))
                _set_delay(env, np.arange(n) % 4)
            assert env.range_capable()
            _start(env, q, qd)
            od = env.obs_dim
            d_act, d_obs, d_rew, d_done = env.sim.malloc(acts[0].nbytes), env.sim.malloc(n * od * 4), env.sim.malloc(n * 4), env.sim.malloc(n * 4)
            rows = []
            for a in acts[:6]:
                env.sim.upload(d_act, a)
                env.sim.synchronize()
                if mode == "split":
                    env.step_range_dev(0, h, streams[0].cuda_stream, d_act, d_obs, d_rew, d_done)
                    env.step_range_dev(h, n - h, streams[1].cuda_stream, d_act, d_obs, d_rew, d_done)
                    for s in streams:
                        s.synchronize()
                else:
                    env.step_dev(d_act, d_obs, d_rew, d_done)
                env.sim.synchronize()
                rows.append((env.sim.download(d_obs, (n, od)), env.sim.download(d_rew, (n,)), env.sim.download(d_done, (n,), np.uint32)))
            res.append(rows)
        finally:
            env.close()
    whole, split, quiet = res
    for t in range(6):
        for x, y in zip(whole[t], split[t]):
            assert np.array_equal(x, y), t
    # the first step of every env with d = 0 is the undelayed handle's: the difference is the noise of global env 1000 + i, row 1
    colsig = column_sigmas(3, desc.n_t, ch, SIGMA)
    z = sensor_noise64(3, np.arange(n, dtype=np.uint64) + np.uint64(1000), 1, 9 + len(ch) * desc.n_t)
    d0 = np.arange(n) % 4 == 0
    _check_noise(desc, whole[0][0][d0], quiet[0][0][d0], z[d0], colsig, "offset 1000")
    assert np.abs(whole[0][0][d0] - quiet[0][0][d0] - colsig * sensor_noise64(3, np.arange(n, dtype=np.uint64), 1, len(colsig))[d0]).max() > 1e-3


# ---- 3. the delay ----
def _symmetric_box(robot):
    box = robot.get_action_space()
    return bool(np.all(box.low == -box.high)) and not env_rescale64(robot, np.zeros((1, box.shape[0]))).any()


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("which", ["baked", "kernarg", "ball12"])
@pytest.mark.parametrize("form", ["nominal", "randomized"])
def test_delay_is_the_shifted_action_sequence(form, which, integ):
    """Handle A: the delay plane written as d_i = i mod 4, a recorded random action sequence.  Handle B: the same io configuration, the
    plane all zeros - the same kernels - fed per env the action A was handed d_i steps earlier in the same episode, or the action 0
    while the episode is younger than that: these robots' set-point boxes are symmetric, so rescale(0) is exactly 0 m, the rest
    command.  Obs, state, reward and done bit-identical over 12 steps, two auto-resets per env (the host restarts k at every done)."""
    robot = ROBOTS[which]()
    assert _symmetric_box(robot)
    desc, q, qd, acts = _inputs(which, N, 4)
    d = np.arange(N) % 4
    envs = [_make(which, N, integ, form, 0, seed=9) for _ in range(2)]
    try:
        for env, plane in zip(envs, (d, np.zeros(N, int))):
            env.sim.configure_io(_io_cfg(delay=(0, 3)))
            assert env.sim.io_ptrs()["slots"] == 4 and env.sim.io_ptrs()["history"]
            _set_delay(env, plane)
        a0, b0 = (_start(env, q, qd) for env in envs)
        assert np.array_equal(a0, b0)
        book = DelayBook(N, desc.n_t)
        n_done = np.zeros(N, int)
        for t, act in enumerate(acts):
            fed, rest = book.shifted(act, d)
            assert not fed[rest].any() and (t > 0 or np.array_equal(rest, d > 0))
            ra = envs[0].step(act)[:3] + tuple(envs[0].sim.read_state())
            rb = envs[1].step(fed)[:3] + tuple(envs[1].sim.read_state())
            for x, y in zip(ra, rb):
                assert np.array_equal(x, y), t
            book.advance(ra[2])
            n_done += ra[2]
        assert n_done.min() >= 2
        assert np.array_equal(_plane(envs[0], "delay"), d)               # no redraw without resample_on_reset
    finally:
        for env in envs:
            env.close()


def _asymmetric_ball12():
    """ball12 with the set-point box [-0.1, 0.3] m: rescale(0) = 0.1 m is NOT the rest command"""
    from gym_roboy_amd._gymcompat import spaces
    base = _ball12()

    class Lopsided(type(base)):
        @classmethod
        def get_action_space(cls):
            return spaces.Box(low=-0.1, high=0.3, shape=base.get_action_space().shape, dtype="float32")
    return Lopsided()


@pytest.mark.parametrize("form", ["nominal", "randomized"])
def test_tendon_columns_report_the_applied_command_on_an_asymmetric_box(form):
    """mask = length | force: the columns of every row match the fp64 restatement under the set-points that were APPLIED - the
    delayed action's, or 0 m (plus the env's offset) while the episode is younger than the delay - at the state the row reports and,
    randomized, under the env's parameters after the step."""
    robot = _asymmetric_ball12()
    assert not _symmetric_box(robot)
    desc = robot.get_description()
    ch = ("length", "force")
    rng = np.random.default_rng(5)
    q, qd = _state(desc, N, rng)
    acts = _actions(desc, N, rng, STEPS)
    d = np.arange(N) % 4
    env = _vec(robot, N, "euler", tendon_obs=ch, seed=4, max_len=MAX_LEN, randomization=True if form == "randomized" else None)
    try:
        env.sim.configure_io(_io_cfg(delay=(0, 3)))
        _set_delay(env, d)
        _start(env, q, qd)
        book = DelayBook(N, desc.n_t)
        seen_rest_after_reset = 0
        for t, act in enumerate(acts):
            fed, rest = book.shifted(act, d)
            obs, _, done, _ = env.step(act)
            par = env.sim.get_param_planes().T if form == "randomized" else None
            want, o = expected_columns(robot, desc, obs[:, 0:3], obs[:, 3:6], fed, ch, None, par)
            at_rest, _ = expected_columns(robot, desc, obs[:, 0:3], obs[:, 3:6], None, ch, None, par)
            want[rest] = at_rest[rest]
            tol = column_tolerances(o, ch)
            worst = (np.abs(obs[:, 9:].astype(np.float64) - want) / tol).max()
            assert worst <= 1.0, (t, worst)
            # ... and NOT under rescale(0) = 0.1 m: the force column tells the two apart on the envs at rest
            if rest.any():
                wrong, _ = expected_columns(robot, desc, obs[:, 0:3], obs[:, 3:6], np.zeros_like(fed), ch, None, par)
                assert (np.abs(wrong[rest] - want[rest]) / tol).max() > 10
            seen_rest_after_reset += int(t > 3 and rest.any())
            book.advance(done)
        assert seen_rest_after_reset >= 2
    finally:
        env.close()


# ---- 4. the delay's redraw ----
def test_configure_and_sample_delay_dev_give_the_restated_integers():
    n = N_RANGE
    env = _make("baked", n, "euler", "nominal", 0, seed=11, env_id_offset=1000)
    try:
        gids = np.arange(n, dtype=np.uint64) + np.uint64(1000)
        env.sim.configure_io(_io_cfg(delay=(1, 3)))
        d0 = _plane(env, "delay").astype(np.int64)
        assert np.array_equal(d0, delay_draw(11, gids, 0, 1, 3)) and set(d0) == {1, 2, 3}
        assert np.array_equal(_plane(env, "delay_draws"), np.ones(n, np.uint32))
        mask = np.arange(n) % 3 == 0
        env.sim.sample_io_delay(mask)
        want = np.where(mask, delay_draw(11, gids, 1, 1, 3), d0)
        assert np.array_equal(_plane(env, "delay"), want) and np.array_equal(_plane(env, "delay_draws"), 1 + mask.astype(np.uint32))
        env.sim.sample_io_delay()
        assert np.array_equal(_plane(env, "delay"), delay_draw(11, gids, 1 + mask.astype(np.uint32), 1, 3))
        env.sim.configure_io(_io_cfg(delay=(1, 3)))               # again: planes and counters start over
        assert np.array_equal(_plane(env, "delay"), d0) and np.array_equal(_plane(env, "delay_draws"), np.ones(n, np.uint32))
        env.sim.configure_io(_io_cfg(delay=(0, 7)))
        assert env.sim.io_ptrs()["slots"] == 8 and set(_plane(env, "delay")) == set(range(8))
        env.sim.configure_io(_io_cfg(delay=(4, 4)))
        assert env.sim.io_ptrs()["slots"] == 8 and set(_plane(env, "delay")) == {4}
        env.sim.configure_io(_io_cfg(delay=(1, 1)))
        assert env.sim.io_ptrs()["slots"] == 2
    finally:
        env.close()


@pytest.mark.parametrize("which,integ,form", [("baked", "euler", "nominal"), ("kernarg", "rk4", "randomized"), ("ball12", "euler", "randomized")])
def test_done_envs_redraw_their_delay_and_the_ending_step_used_the_old_one(which, integ, form):
    """resample_on_reset: exactly the envs that reported done hold their next draw behind that step.  Handle B (plane zeros, no
    redraw) is fed the sequence shifted by the delays A held WHEN each step ran - read back before the step - and stays bit-identical:
    the step that ended an episode used the old delay, the new episode's steps the new one."""
    assert _symmetric_box(ROBOTS[which]())
    desc, q, qd, acts = _inputs(which, N, 6)
    gids = np.arange(N, dtype=np.uint64)
    envs = [_make(which, N, integ, form, 0, seed=13) for _ in range(2)]
    try:
        envs[0].sim.configure_io(_io_cfg(delay=(0, 3), resample=True))
        envs[1].sim.configure_io(_io_cfg(delay=(0, 3)))
        _set_delay(envs[1], np.zeros(N, int))
        for env in envs:
            _start(env, q, qd)
        book = DelayBook(N, desc.n_t)
        draws = np.ones(N, np.uint32)
        d = _plane(envs[0], "delay").astype(np.int64)
        assert np.array_equal(d, delay_draw(13, gids, 0, 0, 3))
        moved = 0
        for t, act in enumerate(acts):
            fed, _ = book.shifted(act, d)
            ra = envs[0].step(act)[:3] + tuple(envs[0].sim.read_state())
            rb = envs[1].step(fed)[:3] + tuple(envs[1].sim.read_state())
            for x, y in zip(ra, rb):
                assert np.array_equal(x, y), t
            done = ra[2]
            new = _plane(envs[0], "delay").astype(np.int64)
            assert np.array_equal(new[~done], d[~done])
            assert np.array_equal(new[done], delay_draw(13, gids[done], draws[done], 0, 3))
            moved += int(np.sum(new != d))
            draws = draws + done.astype(np.uint32)
            assert np.array_equal(_plane(envs[0], "delay_draws"), draws)
            d = new
            book.advance(done)
        assert draws.min() >= 3 and moved > N
    finally:
        for env in envs:
            env.close()


# ---- 5. composition ----
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_parameters_channels_noise_and_delay_together(integ):
    """ball12, parameter form with resample_on_reset, mask 15, noise and a redrawn delay.  Handle B: the same handle without io, fed
    the shifted actions (symmetric box).  Reward, done and state bit-equal; the first nine columns equal B's after the restated noise
    is taken off (within the noise check's bound); the tendon columns - whose set-points A holds in other registers than B computes
    them in - within the readout's tolerances after the same subtraction."""
    which, mask = "ball12", 15
    ch = channels_of(mask)
    assert _symmetric_box(ROBOTS[which]())
    desc, q, qd, acts = _inputs(which, N, 8)
    gids = np.arange(N, dtype=np.uint64)
    od = 9 + 4 * desc.n_t
    colsig = column_sigmas(3, desc.n_t, ch, SIGMA)
    envs = [_make(which, N, integ, "randomized", mask, seed=17) for _ in range(2)]
    try:
        envs[0].sim.configure_io(_io_cfg(SIGMA, ch, delay=(0, 3), resample=True))
        a0, b0 = (_start(env, q, qd) for env in envs)
        _check_noise(desc, a0, b0, sensor_noise64(17, gids, 0, od), colsig, "reset rows")
        book = DelayBook(N, desc.n_t)
        from oracle.physics_np import TendonRobotOracle
        tol = column_tolerances(TendonRobotOracle(desc), ch)
        n_done = np.zeros(N, int)
        for t, act in enumerate(acts):
            d = _plane(envs[0], "delay").astype(np.int64)
            fed, rest = book.shifted(act, d)
            ra = envs[0].step(act)[:3] + tuple(envs[0].sim.read_state())
            rb = envs[1].step(fed)[:3] + tuple(envs[1].sim.read_state())
            for x, y in zip(ra[1:], rb[1:]):
                assert np.array_equal(x, y), t
            assert np.array_equal(envs[0].sim.get_param_planes(), envs[1].sim.get_param_planes())
            z = sensor_noise64(17, gids, t + 1, od)
            _check_noise(desc, ra[0][:, :9], rb[0][:, :9], z[:, :9], colsig[:9], "step %d, columns 0-8" % t)
            clean = ra[0][:, 9:].astype(np.float64) - colsig[9:] * z[:, 9:]
            bound = 2 * tol + np.abs(colsig[9:]) * NOISE_TOL + 4 * np.spacing(np.abs(ra[0][:, 9:])).astype(np.float64)
            assert (np.abs(clean - rb[0][:, 9:]) / bound).max() <= 1.0, t
            book.advance(ra[2])
            n_done += ra[2]
        assert n_done.min() >= 2 and (_plane(envs[0], "delay_draws") >= 3).all()
    finally:
        for env in envs:
            env.close()


# ---- 6. a captured graph ----
def test_a_captured_graph_of_io_steps_replays_with_counters_and_history_on_the_device():
    import torch
    robot = _msj()
    n, T = N, 4
    kw = dict(tendon_obs=("length", "force"), randomization=True, seed=4, max_len=MAX_LEN)
    env, ref = _vec(robot, n, "rk4", **kw), _vec(robot, n, "rk4", **kw)
    try:
        for e in (env, ref):
            e.sim.configure_io(_io_cfg(SIGMA, ("length", "force"), delay=(0, 3), resample=True))
        dev = torch.device("cuda", 0)
        acts = torch.rand((3, T, n, 8), device=dev) * 2 - 1
        slab = torch.zeros((T, n, 8), device=dev)
        obs = torch.zeros((T, n, env.obs_dim), device=dev)
        rew, done = torch.zeros((T, n), device=dev), torch.zeros((T, n), dtype=torch.int32, device=dev)
        assert np.array_equal(env.reset(), ref.reset())
        side = torch.cuda.Stream(device=dev)
        env.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for t in range(T):
                env.step_dev(slab[t].data_ptr(), obs[t].data_ptr(), rew[t].data_ptr(), done[t].data_ptr())
        n_done = 0
        for r in range(3):                       # 12 steps: rows, history and delays carry over from replay to replay
            slab.copy_(acts[r])
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            for t in range(T):
                o, w, dn, _ = ref.step(acts[r, t].cpu().numpy())
                assert np.array_equal(obs[t].cpu().numpy(), o) and np.array_equal(rew[t].cpu().numpy(), w), (r, t)
                assert np.array_equal(done[t].cpu().numpy().astype(bool), dn)
                n_done += dn.sum()
        assert n_done >= 2 * n
        env.set_stream(0)
        for name in ("delay", "delay_draws", "rows"):
            assert np.array_equal(_plane(env, name), _plane(ref, name))
        assert np.array_equal(_plane(env, "rows"), np.full(n, 13, np.uint32))
    finally:
        env.close(); ref.close()


# ---- 7. refusals, switching off ----
def test_refusals():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    env = _vec(_msj(), 256)
    try:
        lib, h = env.sim._lib, env.sim.handle
        assert lib.rb_env_io_ptr(h, None, None, None, None, None) == nat.RB_EINVAL                 # nothing configured
        assert lib.rb_env_io_sample_delay_dev(h, None) == nat.RB_EINVAL
        for bad in (-0.1, np.nan, np.inf):
            for field in ("sigma_q", "sigma_qd"):
                cfg = _io_cfg()
                setattr(cfg, field, bad)
                assert lib.rb_env_io_configure(h, ctypes.byref(cfg)) == nat.RB_EINVAL and b"finite" in lib.rb_last_error()
            cfg = _io_cfg()
            cfg.sigma_tendon[2] = bad
            assert lib.rb_env_io_configure(h, ctypes.byref(cfg)) == nat.RB_EINVAL
        for lo, hi in ((0, 8), (3, 1), (-1, 2), (8, 8)):
            assert lib.rb_env_io_configure(h, ctypes.byref(_io_cfg(delay=(lo, hi)))) == nat.RB_EINVAL and b"delay" in lib.rb_last_error()
        assert lib.rb_env_io_ptr(h, None, None, None, None, None) == nat.RB_EINVAL                 # a refused call leaves the handle as it was
        row = env.sim.dispatch("env_step")
        env.sim.configure_io(_io_cfg(delay=(0, 1)))
        with pytest.raises(nat.NativeError, match="io configuration"):
            env.sim.dispatch("env_step")
        assert env.sim.dispatch("step")["id"]                                                      # the step entry is untouched
        env.sim.configure_io(None)
        assert env.sim.dispatch("env_step")["id"] == row["id"]
    finally:
        env.close()
    bare = HipBatchSimulation(_msj(), 64)
    try:
        assert bare._lib.rb_env_io_configure(bare.handle, ctypes.byref(_io_cfg())) == nat.RB_EINVAL     # no rb_env_configure yet
        assert b"rb_env_configure" in bare._lib.rb_last_error()
    finally:
        bare.close()
    tree = _vec(UpperBodyRobot(), 64)
    try:
        assert tree.sim._lib.rb_env_io_configure(tree.sim.handle, ctypes.byref(_io_cfg(delay=(0, 1)))) == nat.RB_EUNSUPPORTED
        assert b"ball-joint" in tree.sim._lib.rb_last_error()
        with pytest.raises(nat.NativeError):
            _vec(UpperBodyRobot(), 64, action_delay=1)
    finally:
        tree.close()
    with pytest.raises(ValueError):
        _vec(_msj(), 64, sensor_noise={"force": 2.0})                                               # a channel that is not selected
    with pytest.raises(ValueError):
        _vec(_msj(), 64, action_delay=(0, 8))


@pytest.mark.parametrize("which,form,mask", [("baked", "nominal", 9), ("ball12", "params", 0), ("kernarg", "randomized", 15)])
def test_configure_null_restores_the_previous_rows(which, form, mask):
    """Six steps with noise and a ring (the delay plane written to zeros, so that the env's episodes, goal and parameter draws stay
    those of the plain handle), then rb_env_io_configure(NULL): the buffers are gone and the next 12 steps are the plain handle's, bit
    for bit."""
    desc, q, qd, acts = _inputs(which, N, 10)
    ch = channels_of(mask)
    plain, env = _make(which, N, "euler", form, mask, seed=19), _make(which, N, "euler", form, mask, seed=19)
    try:
        env.sim.configure_io(_io_cfg(SIGMA, ch, delay=(1, 3)))
        _set_delay(env, np.zeros(N, int))
        noisy, quiet = _run(env, q, qd, acts[:6]), _run(plain, q, qd, acts[:6])
        assert not np.array_equal(noisy[1][-1][0], quiet[1][-1][0])
        for x, y in zip(noisy[1][-1][1:], quiet[1][-1][1:]):
            assert np.array_equal(x, y)
        env.sim.configure_io(None)
        assert env.sim._lib.rb_env_io_ptr(env.sim.handle, None, None, None, None, None) == nat.RB_EINVAL
        ref, got = _run(plain, q, qd, acts), _run(env, q, qd, acts)
        assert np.array_equal(ref[0], got[0])
        for r, g in zip(ref[1], got[1]):
            for x, y in zip(r, g):
                assert np.array_equal(x, y)
    finally:
        plain.close(); env.close()


# ---- 8. the consumer ----
def test_vec_env_options_numpy_and_torch_paths():
    import torch
    from gym_roboy_amd.envs.params import ParamRanges
    n = 512
    kw = dict(tendon_obs=("length", "force"), scale={"force": 1 / 400}, randomization=ParamRanges(**RANGES), seed=21, max_len=MAX_LEN)
    sigma = {"q": 0.01, "qd": 0.05, "length": 5e-4, "force": 2.0}
    env = _vec(_msj(), n, sensor_noise=sigma, action_delay=(0, 3), **kw)
    quiet = _vec(_msj(), n, **kw)
    fixed = _vec(_msj(), n, action_delay=2)
    try:
        assert env.obs_dim == 25 and env.observation_space.shape == (25,)
        assert np.array_equal(env.observation_space.low, quiet.observation_space.low)               # unchanged, and nothing is clipped to it
        d = env.get_action_delay()
        assert d.shape == (n,) and set(d) == {0, 1, 2, 3} and np.array_equal(d, delay_draw(21, np.arange(n), 0, 0, 3))
        assert set(fixed.get_action_delay()) == {2} and fixed.action_delay == 2 and env.action_delay == (0, 3)
        env.set_action_delay(np.zeros(n, int))
        assert not env.get_action_delay().any()
        for bad in (np.full(n, 4), np.full(n, -1), np.zeros(n - 1, int), np.full(n, 0.5)):
            with pytest.raises(ValueError):
                env.set_action_delay(bad)
        with pytest.raises(RuntimeError):
            quiet.get_action_delay()
        env.set_action_delay(d)
        colsig = column_sigmas(3, 8, ("length", "force"), sigma, {"force": 1 / 400})
        o_a, o_b = env.reset(), quiet.reset()
        desc = _msj().get_description()
        _check_noise(desc, o_a, o_b, sensor_noise64(21, np.arange(n), 0, 25), colsig, "reset")
        acts = torch.rand((STEPS, n, 8), device="cuda") * 2 - 1
        for t in range(STEPS):
            obs, rew, done, _ = env.step(acts[t]) if t % 2 else env.step(acts[t].cpu().numpy())
            assert tuple(obs.shape) == (n, 25)
            assert torch.isfinite(obs).all() if t % 2 else np.isfinite(obs).all()
        assert set(env.get_action_delay()) == {0, 1, 2, 3} and np.any(env.get_action_delay() != d)    # redrawn on auto-reset
        assert np.array_equal(_plane(env, "rows"), np.full(n, 1 + STEPS, np.uint32))
    finally:
        env.close(); quiet.close(); fixed.close()


@pytest.mark.parametrize("graphs", [False, True])
def test_ppo_update_and_checkpoint_round_trip(graphs, tmp_path, capsys):
    import torch
    from gym_roboy_amd import visualize_agent
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.ppo import PPO
    sigma = {"q": 0.01, "qd": 0.05, "length": 5e-4, "force": 2.0}
    env = _vec(_msj(), 512, tendon_obs=("length", "force"), scale={"force": 1 / 400}, sensor_noise=sigma, action_delay=(0, 3),
               randomization=ParamRanges(force_scale=(0.8, 1.2), mass_scale=(0.8, 1.25)), seed=2, max_len=MAX_LEN)
    try:
        agent = PPO(env, n_steps=16, use_graphs=graphs, seed=3)
        assert agent._fused is not None and agent._fused.obs_dim == 25
        roll = agent.collect()
        assert tuple(roll["obs"].shape[1:]) == (512, 25) and torch.isfinite(roll["obs"]).all() and torch.isfinite(roll["act"]).all()
        stats = agent.update(roll)
        assert all(np.isfinite(v) for v in stats.values()) and all(torch.isfinite(p).all() for p in agent.policy.parameters())
        assert _plane(env, "rows").min() >= 16 and _plane(env, "delay_draws").min() >= 3
        path = str(tmp_path / "model.pkl")
        agent.save(path)
        ck = torch.load(path, map_location="cpu")
        assert ck["env_io"] == {"sensor_noise": {k: float(v) for k, v in sigma.items()}, "action_delay": [0, 3]}
    finally:
        env.close()
    if not graphs:
        total = visualize_agent.main([path, "--steps", "3", "--pause", "0"])
        assert np.isfinite(total) and capsys.readouterr().out.count("reward") == 3
