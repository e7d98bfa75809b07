"""Tendon channels in the fused env step's observation on the GPU (include/roboy_sim.h: rb_env_obs_*; csrc/env_obs.hpp; DESIGN.md
§13): the nine reference columns and every other output against the handle's kernels without the extension, the reference's golden
vectors through the extended kernels, the tendon columns against the fp64 restatement (tests/env_obs_util.py) on nominal and
randomized handles, consistency with the readout, auto-reset and redraw, ranges, graphs, scales, refusals, and PPO as a consumer."""
import ctypes

import numpy as np
import pytest

from env_obs_util import CHANNELS, channels_of, column_tolerances, expected_columns, mask_of
from gym_roboy_amd import _native as nat
from test_env_params_gpu import _ball12, _kernarg_msj, _msj

pytestmark = pytest.mark.gpu

ROBOTS = {"baked": _msj, "kernarg": _kernarg_msj, "ball12": _ball12}
RANGES = dict(force_scale=(0.7, 1.3), setpoint_offset=(-0.02, 0.02), mass_scale=(0.6, 1.6), damping_scale=(0.5, 2.0))


def _vec(robot, n, integ="euler", tendon_obs=None, scale=None, randomization=None, seed=5, max_len=400, **kw):
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    rnd = ParamRanges(**RANGES) if randomization is True else randomization
    return RoboyVecEnv(robot, n, seed=seed, integrator=integ, max_episode_length=max_len, tendon_obs=tendon_obs,
                       tendon_obs_scale=scale, randomization=rnd, **kw)


def _state(desc, n, rng):
    """states at 0.9 of the joint box, velocities within limits, actions from U[-1, 1]"""
    q = rng.uniform(0.9 * desc.q_lo, 0.9 * desc.q_hi, (n, 3)).astype(np.float32)
    qd = rng.uniform(-desc.qd_max, desc.qd_max, (n, 3)).astype(np.float32)
    return q, qd


def _actions(desc, n, rng, steps):
    return rng.uniform(-1, 1, (steps, n, desc.n_t)).astype(np.float32)


def _episode(env, q, qd, acts, step_num):
    """reset, the given state, then the actions: every output of every step, the final state and the statistics"""
    env.reset()
    env.sim.set_state(q, qd)
    goal = env.sim.download(env._d_obs, (env.num_envs, env.obs_dim))[:, 6:9]
    env.set_goal(goal, step_num=step_num)
    out = []
    for a in acts:
        obs, rew, done, _ = env.step(a)
        out.append((obs, rew, done) + tuple(env.sim.read_state()))
    return out, env.stats(), goal


# ---- 1. columns 0-8 and every other output ----
@pytest.mark.parametrize("n", [4097, 66819, 262144])
@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("which", ["baked", "kernarg", "ball12"])
@pytest.mark.parametrize("form", ["nominal", "params"])
def test_reference_columns_and_every_other_output_match_the_handle_without_channels(form, which, integ, n, monkeypatch):
    """Four steps across an auto-reset (episodes of 3 steps, counters staggered).  Reference: the same handle without the extension -
    nominal: the env-per-lane form selected, hiprtc off so that a kernarg robot runs its kernarg row; params: the parameter kernel,
    nominal planes.  Bit for bit wherever both run the same step text (RB_MSJ_ENV_STEP_BODY with the same UNROLL / the parameter
    body).  That is every case but three nominal ones at 4 097 envs, where the selectable env-per-lane row is the 64-thread one with
    its tendons written out (UNROLL 8) and the extended instance is the large-batch text - baked RK4 (rolled stages: another
    summation order of the stages) and kernarg Const8 (rolled tendon loop) share no integrator code with it: there one step, state and
    row within the step's parity tolerance 2e-6, done and feasibility on every env clear of a threshold, reward within 1e-4."""
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    robot = ROBOTS[which]()
    desc = robot.get_description()
    rng = np.random.default_rng(n + len(which))
    q, qd = _state(desc, n, rng)
    acts = _actions(desc, n, rng, 4)
    step_num = rng.integers(1, 4, n).astype(np.uint32)
    mask = {"baked": 9, "kernarg": 15, "ball12": 6}[which] if integ == "euler" else {"baked": 15, "kernarg": 2, "ball12": 9}[which]
    same_text = form == "params" or n > 65536 or which == "ball12" or (which == "baked" and integ == "euler")
    res = []
    for ext in (False, True):
        env = _vec(robot, n, integ, tendon_obs=channels_of(mask) if ext else None, max_len=3)
        try:
            if form == "params":
                env.sim.enable_params()
            elif not ext:
                env.sim.select_kernel(1)
                assert "/env_per_lane/" in env.sim.dispatch("env_step")["id"]
            assert env.obs_dim == 9 + (bin(mask).count("1") * desc.n_t if ext else 0)
            res.append(_episode(env, q, qd, acts if same_text else acts[:1], step_num))
            env_cfg, goal0 = env._cfg, res[-1][2]
        finally:
            env.close()
    (ref, ref_stats, _), (got, got_stats, _) = res
    assert any(r[2].any() for r in ref) or not same_text
    for t, (r, g) in enumerate(zip(ref, got)):
        g = (g[0][:, :9],) + g[1:]
        if same_text:
            for a, b in zip(r, g):
                assert np.array_equal(a, b), (t, np.abs(a.astype(np.float64) - b).max())
        else:
            assert np.abs(r[0] - g[0]).max() < 2e-6 and np.abs(r[3] - g[3]).max() < 2e-6 and np.abs(r[4] - g[4]).max() < 2e-6
            # done and feasibility on EVERY env that is clear of a threshold by more than the states may differ (5 x 2e-6): the goal
            # tolerances (raw joint-space distances, as the kernel compares them), the joint limits and the velocity limits.  An env
            # at the episode-length limit is done in both whatever its state.
            cfg = env_cfg
            timed_out = step_num + 1 > 3
            q1, v1, goal = r[3].astype(np.float64), r[4].astype(np.float64), goal0.astype(np.float64)
            m_goal = np.minimum(np.abs(np.linalg.norm(q1 - goal, axis=1) - cfg.goal_angle_tol), np.abs(np.linalg.norm(v1, axis=1) - cfg.goal_vel_tol))
            clear_done = timed_out | (m_goal > 1e-5)
            assert np.array_equal(r[2][clear_done], g[2][clear_done]) and clear_done.mean() > 0.99
            m_lim = np.minimum(np.minimum(np.abs(q1 - desc.q_lo), np.abs(q1 - desc.q_hi)).min(axis=1), np.abs(np.abs(v1) - desc.qd_max).min(axis=1))
            clear_feas = (m_lim > 1e-5) | (r[5] == g[5])
            both_clamped = (m_lim == 0) & ~r[5].astype(bool) & ~g[5].astype(bool)
            assert np.array_equal(r[5][m_lim > 1e-5], g[5][m_lim > 1e-5]) and (clear_feas | both_clamped).mean() > 0.99
            # reward: fp32 evaluation of -exp(-scaled distance) terms on states 2e-6 apart, the bonus and the boundary penalty where
            # done / feasibility are clear
            ok = clear_done & (m_lim > 1e-5) & ~(r[2] & ~timed_out)
            assert np.abs(r[1][ok] - g[1][ok]).max() < 1e-4 * max(1.0, np.abs(r[1][ok]).max())
    if same_text:
        assert ref_stats == got_stats
    else:
        assert ref_stats["n_env_steps"] == got_stats["n_env_steps"]
        assert abs(ref_stats["n_episodes"] - got_stats["n_episodes"]) <= np.sum(~clear_done)


# ---- 2. the reference's golden vectors ----
@pytest.mark.parametrize("mask", [1, 6, 9, 15])
@pytest.mark.parametrize("kind,integ,params", [("const8", "euler", False), ("const8", "rk4", False), ("constx", "euler", False),
                                               ("constx", "rk4", True), ("const8", "euler", True)])
def test_scripted_episode_of_the_reference_through_the_extended_kernels(kind, integ, params, mask):
    """tests/golden/env_layer.json's scripted episode, replayed as in tests/test_env_golden_gpu.py (parked robots: MsjRobot's own
    constants cannot park; an 8-tendon kernarg robot and a 5-tendon one).  The fixture's values are the reference's float64: the
    nine columns, reward and done agree with it within that test's tolerances (1 ulp of the landing, fp32 reward), AND they are,
    bit for bit, what the same handle without the extension gives - so the extended kernels reproduce the fixture exactly as far
    as any kernel of the library does."""
    from test_env_golden_gpu import _fixture, parked_ball_robot, parked_robot, pre_state
    fx = _fixture()
    ep = fx["episode"]
    steps, script = ep["steps"], ep["script"]
    idx = [t for t in range(len(steps)) if script[t][2]]
    robot = parked_robot() if kind == "const8" else parked_ball_robot(5)
    nt = robot.get_description().n_t
    q = np.array([script[t][0] for t in idx]); qd = np.array([script[t][1] for t in idx])
    goal = np.array([steps[t]["obs"][6:9] for t in idx])
    q_pre, qd32 = pre_state(q, qd)
    acts = np.asarray([ep["actions"][t] for t in idx], np.float32)[:, :nt]
    out = []
    for ext in (False, True):
        env = _vec(robot, len(idx), integ, tendon_obs=channels_of(mask) if ext else None, seed=2, auto_reset=False)
        try:
            if params:
                env.sim.enable_params()
            elif not ext:
                env.sim.select_kernel(1)
            env.reset()
            env.sim.set_state(q_pre, qd32)
            env.set_goal(goal, step_num=np.array([steps[t]["step_num"] - 1 for t in idx], np.uint32))
            out.append(env.step(acts)[:3])
        finally:
            env.close()
    (obs0, rew0, done0), (obs, rew, done) = out
    assert obs.shape == (len(idx), 9 + bin(mask).count("1") * nt) and np.all(np.isfinite(obs))
    assert np.array_equal(obs[:, :9], obs0) and np.array_equal(rew, rew0) and np.array_equal(done, done0)
    for k, t in enumerate(idx):
        assert np.abs(obs[k, :9] - np.asarray(steps[t]["obs"]).astype(np.float32)).max() < 5e-7
        np.testing.assert_allclose(rew[k], steps[t]["reward"], rtol=2e-5, atol=2e-4)
        assert bool(done[k]) == steps[t]["done"]
    assert done.any()


# ---- 3. tendon columns against fp64 ----
def _check_columns(cols, want, tol, what):
    worst = (np.abs(cols.astype(np.float64) - want) / tol).max()
    assert worst <= 1.0, "%s: %.2f x tolerance" % (what, worst)


@pytest.mark.parametrize("which,integ,mask", [("baked", "euler", 15), ("baked", "rk4", 9), ("kernarg", "euler", 15), ("kernarg", "rk4", 5),
                                              ("ball12", "euler", 15), ("ball12", "rk4", 10)])
@pytest.mark.parametrize("randomized", [False, True])
def test_tendon_columns_match_the_fp64_restatement_at_the_reported_state(which, integ, mask, randomized):
    """Every env, every selected channel, two steps: the columns of step t at the state step t reports (columns 0-5 of the same row)
    under the actions of step t; randomized handles under each env's own parameters, set-point offset and force scale included (the
    planes read after the step: what an env that reached its goal and was redrawn reports under).  Tolerances: the readout's own times |scale|."""
    robot = ROBOTS[which]()
    desc = robot.get_description()
    n, ch = 66819, channels_of(mask)
    scale = {"force": 1 / 400, "length": -4.0} if which == "baked" else None
    rng = np.random.default_rng(mask)
    q, qd = _state(desc, n, rng)
    acts = _actions(desc, n, rng, 2)
    env = _vec(robot, n, integ, tendon_obs=ch, scale=scale, randomization=randomized or None)
    try:
        env.reset()
        env.sim.set_state(q, qd)
        for a in acts:
            obs, _, done, _ = env.step(a)
            assert done.mean() < 0.01          # (a few envs may reach their goal: they report the zero pose, under redrawn parameters)
            par = env.sim.get_param_planes().T if randomized else None
            want, o = expected_columns(robot, desc, obs[:, 0:3], obs[:, 3:6], a, ch, scale, par)
            _check_columns(obs[:, 9:], want, column_tolerances(o, ch, scale), "%s %s" % (which, integ))
            if randomized:
                assert np.unique(par[:, 0]).size > n // 2
    finally:
        env.close()


# ---- 4. consistency with the readout ----
@pytest.mark.parametrize("which,integ", [("baked", "euler"), ("baked", "rk4"), ("kernarg", "euler"), ("ball12", "rk4")])
def test_columns_agree_with_tendon_state_called_after_the_step(which, integ):
    """Nominal handles: the columns against RoboyVecEnv.tendon_state() behind the same step (auto-reset envs included: both report
    the zero pose under the last actions).  They are NOT bit-equal (measured: a last-bit difference in a fraction of the values of
    every channel), and need not be: the readout is another kernel - robot constants through the kernarg where MsjRobot's env step
    has them as literals, the activation offset rounded before use (rbe::rounded_here) where the step's kernels leave the compiler
    free to contract its last product into the activation's fma - so the compiler contracts other products into other fmas, and
    the columns use the STEP's offsets by definition.  Both sit within the fp64 comparison's tolerances of the exact value, so they
    agree within twice those."""
    from oracle.physics_np import TendonRobotOracle
    robot = ROBOTS[which]()
    desc = robot.get_description()
    n = 66819
    rng = np.random.default_rng(3)
    q, qd = _state(desc, n, rng)
    acts = _actions(desc, n, rng, 3)
    env = _vec(robot, n, integ, tendon_obs=CHANNELS, max_len=2)
    try:
        env.reset()
        env.sim.set_state(q, qd)
        tol = column_tolerances(TendonRobotOracle(desc), CHANNELS)
        n_done = 0
        for a in acts:
            obs, _, done, _ = env.step(a)
            n_done += done.sum()
            ts = env.tendon_state()
            want = np.concatenate([ts[c] for c in CHANNELS], axis=1)
            nt = desc.n_t
            assert (np.abs(obs[:, 9:].astype(np.float64) - want) / (2 * tol)).max() <= 1.0
            print("bit-equal fraction per channel:", [float(np.mean(obs[:, 9 + c * nt:9 + (c + 1) * nt] == want[:, c * nt:(c + 1) * nt])) for c in range(4)])
        assert n_done >= n
    finally:
        env.close()


# ---- 5. auto-reset ----
@pytest.mark.parametrize("which", ["baked", "ball12"])
@pytest.mark.parametrize("randomized", [False, True])
def test_done_envs_report_the_zero_pose_under_the_last_actions_and_redrawn_parameters(which, randomized):
    robot = ROBOTS[which]()
    desc = robot.get_description()
    n, ch = 20001, CHANNELS
    rng = np.random.default_rng(11)
    q, qd = _state(desc, n, rng)
    a = _actions(desc, n, rng, 1)[0]
    ending = rng.random(n) < 0.4
    env = _vec(robot, n, "rk4", tendon_obs=ch, randomization=randomized or None, max_len=50)
    try:
        obs0 = env.reset()
        par0 = env.sim.get_param_planes().T.copy() if randomized else None
        # reset(): the zero pose, every set-point 0
        want, o = expected_columns(robot, desc, obs0[:, 0:3], obs0[:, 3:6], None, ch, None, par0)
        tol = column_tolerances(o, ch)
        assert not obs0[:, :6].any()
        _check_columns(obs0[:, 9:], want, tol, "reset")
        env.sim.set_state(q, qd)
        env.set_goal(obs0[:, 6:9], step_num=np.where(ending, 50, 1).astype(np.uint32))      # step_num + 1 > 50: the episode ends
        obs, _, done, _ = env.step(a)
        assert np.all(done[ending]) and np.mean(done & ~ending) < 0.01       # (a few more may have reached their goal)
        assert not obs[done, :6].any() and np.all(np.any(obs[~done, :6] != 0, axis=1))
        par = None
        if randomized:
            par = env.get_params()
            par = np.concatenate([par["force_scale"], par["setpoint_offset"], par["mass_scale"][:, None], par["damping_scale"]], axis=1)
            # exactly the done envs were redrawn: they report under the NEW parameters, the others under theirs
            assert np.all(np.any(par[done] != par0[done], axis=1)) and np.array_equal(par[~done], par0[~done])
        want, _ = expected_columns(robot, desc, obs[:, 0:3], obs[:, 3:6], a, ch, None, par)
        _check_columns(obs[:, 9:], want, tol, "step")
        if randomized:          # ... and NOT under the old ones: the force column tells them apart
            old, _ = expected_columns(robot, desc, obs[:, 0:3], obs[:, 3:6], a, ch, None, par0)
            nt = desc.n_t
            moved = np.abs(want[done, 3 * nt:] - old[done, 3 * nt:]).max(axis=1) > 4 * tol[3 * nt]
            assert moved.mean() > 0.5
            assert np.all(np.abs(obs[done][moved, 3 * nt + 9:] - old[done][moved, 3 * nt:]).max(axis=1) > 2 * tol[3 * nt])
    finally:
        env.close()


# ---- 6. ranges, graphs, scales, refusals ----
@pytest.mark.parametrize("which,randomized", [("baked", False), ("baked", True), ("ball12", True), ("kernarg", False)])
def test_two_halves_on_two_streams_equal_the_whole_batch(which, randomized):
    import torch
    robot = ROBOTS[which]()
    desc = robot.get_description()
    nt, n, ch = desc.n_t, 20001, ("length", "force")
    rng = np.random.default_rng(6)
    acts = _actions(desc, n, rng, 3)
    h = 256 * 39
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for split in (False, True):
        env = _vec(robot, n, "rk4", tendon_obs=ch, randomization=randomized or None, seed=3, max_len=2)
        try:
            assert env.range_capable()
            env.reset()
            od = env.obs_dim
            d_act, d_obs, d_rew, d_done = env.sim.malloc(acts[0].nbytes), env.sim.malloc(n * od * 4), env.sim.malloc(n * 4), env.sim.malloc(n * 4)
            for a in acts:
                env.sim.upload(d_act, a)
                env.sim.synchronize()
                if split:
                    env.step_range_dev(0, h, streams[0].cuda_stream, d_act, d_obs, d_rew, d_done)
                    env.step_range_dev(h, n - h, streams[1].cuda_stream, d_act, d_obs, d_rew, d_done)
                    for s in streams:
                        s.synchronize()
                else:
                    env.step_dev(d_act, d_obs, d_rew, d_done)
                env.sim.synchronize()
            res.append([*env.sim.read_state(), env.sim.download(d_obs, (n, od)), env.sim.download(d_rew, (n,)),
                        env.sim.download(d_done, (n,), np.uint32)])
        finally:
            env.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(res[0][3])) and res[0][3][:, 9:].any(axis=1).all()


def test_a_captured_graph_of_extended_steps_replays():
    import torch
    robot = _msj()
    n, T = 8192, 3
    env = _vec(robot, n, "rk4", tendon_obs=("length", "force"), randomization=True, seed=4)
    ref = _vec(robot, n, "rk4", tendon_obs=("length", "force"), randomization=True, seed=4)
    try:
        dev = torch.device("cuda", 0)
        acts = torch.rand((T, n, 8), device=dev) * 2 - 1
        obs = torch.zeros((T, n, env.obs_dim), device=dev)
        rew, done = torch.zeros((T, n), device=dev), torch.zeros((T, n), dtype=torch.int32, device=dev)
        env.reset(); ref.reset()
        side = torch.cuda.Stream(device=dev)
        env.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for t in range(T):
                env.step_dev(acts[t].data_ptr(), obs[t].data_ptr(), rew[t].data_ptr(), done[t].data_ptr())
        graph.replay()
        torch.cuda.synchronize()
        want = [ref.step(acts[t].cpu().numpy()) for t in range(T)]
        for t in range(T):
            assert np.array_equal(obs[t].cpu().numpy(), want[t][0]) and np.array_equal(rew[t].cpu().numpy(), want[t][1])
        first = obs.clone()
        graph.replay()                       # three more steps from where the first replay left the envs
        torch.cuda.synchronize()
        want = [ref.step(acts[t].cpu().numpy()) for t in range(T)]
        assert np.array_equal(obs[T - 1].cpu().numpy(), want[T - 1][0]) and not torch.equal(first, obs)
        env.set_stream(0)
    finally:
        env.close(); ref.close()


def test_mask_zero_restores_the_handles_kernels_and_scales_are_one_multiply():
    robot = _msj()
    desc = robot.get_description()
    n = 4096
    rng = np.random.default_rng(2)
    q, qd = _state(desc, n, rng)
    a = _actions(desc, n, rng, 1)[0]
    plain, env = _vec(robot, n), _vec(robot, n, tendon_obs=CHANNELS)
    try:
        lib, h = env.sim._lib, env.sim.handle
        row = plain.sim.dispatch("env_step")
        with pytest.raises(nat.NativeError, match="tendon channels are set"):
            env.sim.dispatch("env_step")
        assert env.sim.dispatch("step")["id"] == plain.sim.dispatch("step")["id"]        # the step entry is untouched
        outs = {}
        half = np.float32([0.5, 0.5, 0.5, 0.5])
        for key, scale in (("one", None), ("half", half)):
            nat.check(lib.rb_env_obs_configure(h, 15, None if scale is None else nat.fptr(scale)))
            env.reset(); env.sim.set_state(q, qd)
            env.set_goal(np.zeros((n, 3), np.float32) + 0.1, step_num=np.ones(n, np.uint32))
            outs[key] = env.step(a)[0]
        assert np.array_equal(outs["half"][:, :9], outs["one"][:, :9])
        assert np.array_equal(outs["half"][:, 9:], np.float32(0.5) * outs["one"][:, 9:]) and outs["one"][:, 9:].any()
        # mask 0: the previous kernels and rows of nine columns again
        nat.check(lib.rb_env_obs_configure(h, 0, None))
        dim = ctypes.c_int32()
        nat.check(lib.rb_env_obs_dim(h, ctypes.byref(dim)))
        assert dim.value == 9 and env.sim.dispatch("env_step")["id"] == row["id"]
        env.obs_dim = 9
        res = []
        for e in (plain, env):
            e.reset(); e.sim.set_state(q, qd)
            e.set_goal(np.zeros((n, 3), np.float32) + 0.1, step_num=np.ones(n, np.uint32))
            res.append(e.step(a)[:3])
        for x, y in zip(*res):
            assert np.array_equal(x, y)
    finally:
        plain.close(); env.close()


def test_refusals():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    env = _vec(_msj(), 256)
    try:
        lib, h = env.sim._lib, env.sim.handle
        assert lib.rb_env_obs_configure(h, 16, None) == nat.RB_EINVAL and b"unknown bits" in lib.rb_last_error()
        for bad in (np.nan, np.inf, -np.inf):
            s = np.float32([1, 1, bad, 1])
            assert lib.rb_env_obs_configure(h, 9, nat.fptr(s)) == nat.RB_EINVAL and b"finite" in lib.rb_last_error()
        dim = ctypes.c_int32()
        nat.check(lib.rb_env_obs_dim(h, ctypes.byref(dim)))
        assert dim.value == 9                                   # a refused call leaves the handle as it was
    finally:
        env.close()
    bare = HipBatchSimulation(_msj(), 64)
    try:
        assert bare._lib.rb_env_obs_configure(bare.handle, 9, None) == nat.RB_EINVAL          # no rb_env_configure yet
        assert b"rb_env_configure" in bare._lib.rb_last_error()
    finally:
        bare.close()
    tree = _vec(UpperBodyRobot(), 64)
    try:
        assert tree.sim._lib.rb_env_obs_configure(tree.sim.handle, 9, None) == nat.RB_EUNSUPPORTED
        assert b"ball-joint" in tree.sim._lib.rb_last_error()
        nat.check(tree.sim._lib.rb_env_obs_configure(tree.sim.handle, 0, None))
        with pytest.raises(nat.NativeError):
            _vec(UpperBodyRobot(), 64, tendon_obs=("force",))
    finally:
        tree.close()
    # the readout on a parameter handle is still refused, channels or not
    env = _vec(_msj(), 256, tendon_obs=("force",), randomization=True)
    try:
        d = env.sim.malloc(256 * 8 * 4)
        assert env.sim._lib.rb_tendon_state_dev(env.sim.handle, None, nat.RB_SP_ENV, 1.0, ctypes.c_void_p(d), None, None, None) == nat.RB_EUNSUPPORTED
    finally:
        env.close()


def test_observation_space_and_torch_path():
    import torch
    n = 1024
    env = _vec(_msj(), n, tendon_obs=("force", "length", "activation"), scale={"force": 1 / 400}, randomization=True)
    try:
        assert env.tendon_obs == ("length", "activation", "force") and env.obs_dim == 33
        sp = env.observation_space
        assert sp.shape == (33,) and np.all(sp.low[9:] == 0) and np.all(sp.high[9:17] == np.inf) and np.all(sp.high[17:25] == 1)
        obs = env.reset()
        assert obs.shape == (n, 33)
        obs_t, rew_t, done_t, _ = env.step(torch.rand((n, 8), device="cuda") * 2 - 1)
        assert obs_t.is_cuda and tuple(obs_t.shape) == (n, 33) and torch.isfinite(obs_t).all()
        o = obs_t.cpu().numpy()
        assert np.all(o[:, 9:] >= sp.low[9:]) and np.all(o[:, 9:] <= sp.high[9:])
    finally:
        env.close()


# ---- 7. consumer ----
@pytest.mark.parametrize("graphs", [False, True])
def test_ppo_update_runs_on_a_randomized_env_with_tendon_observations(graphs):
    import torch
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.ppo import PPO
    env = _vec(_msj(), 1024, tendon_obs=("length", "force"), scale={"force": 1 / 400},
               randomization=ParamRanges(force_scale=(0.8, 1.2), mass_scale=(0.8, 1.25)), seed=2)
    try:
        agent = PPO(env, n_steps=16, use_graphs=graphs, seed=3)
        assert agent._fused is not None and agent._fused.obs_dim == 25
        roll = agent.collect()
        assert tuple(roll["obs"].shape[1:]) == (1024, 25) and torch.isfinite(roll["obs"]).all() and torch.isfinite(roll["act"]).all()
        assert roll["obs"][:, :, 9:].abs().sum() > 0
        agent.update(roll)
        assert all(torch.isfinite(p).all() for p in agent.policy.parameters())
        assert env.sim.get_param_draws().max() >= 1
    finally:
        env.close()


def test_ppo_rollout_at_65536_envs_runs_as_two_chains():
    import torch
    from gym_roboy_amd.ppo import PPO
    env = _vec(_msj(), 65536, "rk4", tendon_obs=("length", "force"), scale={"force": 1 / 400}, randomization=True, seed=2)
    try:
        agent = PPO(env, n_steps=4, use_graphs=True, seed=3)
        assert agent._fused.obs_dim == 25 <= agent.CHAIN_MAX_OBS
        roll = agent.collect()
        assert agent.rollout_chains == 2
        assert torch.isfinite(roll["obs"]).all() and roll["obs"][:, :, 9:].abs().sum() > 0
        # the second half's rows are where the row stride puts them: columns of the last env are a tendon's, not zeros
        assert roll["obs"][-1, -1, 9:17].min() > 0
    finally:
        env.close()
