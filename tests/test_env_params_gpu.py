"""Per-env physical parameters on the GPU (include/roboy_sim.h: rb_params_*; csrc/env_params.hpp): nominal planes
against the env-per-lane kernel, random parameters against the fp64 oracle on each env's own description, the on-device draw
against its numpy restatement, the redraw on auto-reset, rollouts and sub-ranges, refusals, and the Python layer."""
import ctypes

import numpy as np
import pytest

from gym_roboy_amd import _native as nat
from env_params_util import ParamOracleStepper, draw, perturbed, random_params

pytestmark = pytest.mark.gpu

TOL = 2e-5            # the ball-joint tolerance of test_physics_gpu.py


def _msj():
    from gym_roboy_amd.envs.robots import MsjRobot
    return MsjRobot()


def _kernarg_msj():
    """MsjRobot with every muscle 2 % stronger (test_dispatch_table.py): constants that are not the ahead-of-time table's."""
    from gym_roboy_amd.envs.robots import MsjRobot, RobotDescription, msj_platform_spec
    spec = msj_platform_spec()
    for t in spec["tendons"]:
        t["f_max"] = 1.02 * t["f_max"]
    desc = RobotDescription(spec)

    class StrongerMsj(MsjRobot):
        @classmethod
        def get_description(cls):
            return desc
    return StrongerMsj()


def _ball12():
    from random_robots import random_ball_joint_robot
    return random_ball_joint_robot(7, n_t=12)[0]


def _sim(robot, n, integ="euler", seed=0, offset=0):
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    return HipBatchSimulation(robot, n, integrator=integ, seed=seed, env_id_offset=offset)


def _state(desc, n, rng):
    q = rng.uniform(0.9 * desc.q_lo, 0.9 * desc.q_hi, (n, 3)).astype(np.float32)
    qd = rng.uniform(-desc.qd_max, desc.qd_max, (n, 3)).astype(np.float32)
    sp = rng.uniform(-0.3, 0.3, (n, desc.n_t)).astype(np.float32)
    return q, qd, sp


# ---- 1. nominal planes against the existing env-per-lane kernel ----
@pytest.mark.parametrize("n", [4097, 66819, 262144])
@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("which", ["baked", "kernarg"])
def test_nominal_planes_match_the_env_per_lane_kernel(n, integ, which):
    """Within 2e-6 after one step everywhere.  Bit-equal for MsjRobot's baked table with Euler (the same arithmetic in the same
    order); not bit for bit otherwise: RK4 sums its stages in another order than the unrolled env-per-lane form
    (MsjModel::integrate_acc), and the kernarg instances' rolled tendon loop contracts the force scale into other fmas."""
    robot = _msj() if which == "baked" else _kernarg_msj()
    desc = robot.get_description()
    q, qd, sp = _state(desc, n, np.random.default_rng(n))
    ref, par = _sim(robot, n, integ), _sim(robot, n, integ)
    try:
        ref.select_kernel(1)
        assert par.enable_params() == 20
        out = []
        for s in (ref, par):
            s.set_state(q, qd)
            out.append(s.forward_step_command(sp))
        err = max(np.abs(out[0][0] - out[1][0]).max(), np.abs(out[0][1] - out[1][1]).max())
        assert err < 2e-6, err
        assert np.mean(out[0][2] == out[1][2]) > 0.999
        if integ == "euler" and which == "baked":
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    finally:
        ref.close(); par.close()


# ---- 2. random parameters against the fp64 oracle ----
@pytest.mark.parametrize("which,integ", [("baked", "euler"), ("baked", "rk4"), ("kernarg", "rk4"), ("ball12", "euler"),
                                         ("ball12", "rk4")])
def test_random_parameters_match_the_oracle_on_each_envs_description(which, integ):
    from oracle.c_oracle import COracle
    robot = {"baked": _msj, "kernarg": _kernarg_msj, "ball12": _ball12}[which]()
    desc = robot.get_description()
    nt, n = desc.n_t, 66819
    rng = np.random.default_rng(2)
    q, qd, sp = _state(desc, n, rng)
    pars = random_params(rng, nt, n).astype(np.float32)
    sim = _sim(robot, n, integ)
    try:
        sim.enable_params()
        d_p, _ = sim.params_ptr()
        sim.upload(d_p, np.ascontiguousarray(pars.T))
        sim.set_state(q, qd)
        q1, qd1, f1 = sim.forward_step_command(sp)
    finally:
        sim.close()
    idx = np.unique(np.linspace(0, n - 1, 64).astype(int))
    worst = 0.0
    for i in idx:
        p = pars[i].astype(np.float64)
        qo, qdo, fo = COracle(perturbed(desc, p), "f64").step(q[i:i + 1].astype(np.float64), qd[i:i + 1].astype(np.float64),
                                                              sp[i:i + 1].astype(np.float64) + p[nt:2 * nt],
                                                              integrator=0 if integ == "euler" else 1)
        worst = max(worst, np.abs(q1[i] - qo[0]).max(), np.abs(qd1[i] - qdo[0]).max())
    assert worst < TOL, worst


# ---- 3. the on-device draw ----
def _ranges(nt, rng):
    P = 2 * nt + 4
    lo = rng.uniform(0.2, 1.0, P).astype(np.float32)
    lo[nt:2 * nt] = rng.uniform(-0.05, 0.0, nt)
    hi = (lo + rng.uniform(0.0, 1.0, P)).astype(np.float32)
    return lo, hi


def test_sample_dev_matches_the_restatement_and_leaves_unmasked_envs_alone():
    robot = _msj()
    n, seed = 10007, 0xABCDEF12345
    rng = np.random.default_rng(4)
    lo, hi = _ranges(8, rng)
    sim = _sim(robot, n, seed=seed)
    try:
        sim.enable_params()
        nat.check(sim._lib.rb_params_set_ranges(sim.handle, nat.fptr(lo), nat.fptr(hi), 1))
        sim.sample_params()
        ids = np.arange(n, dtype=np.uint64)
        p0 = sim.get_param_planes().T
        assert p0.tobytes() == draw(seed, ids, 0, lo, hi).tobytes()
        assert np.all(sim.get_param_draws() == 1)
        mask = rng.random(n) < 0.3
        sim.sample_params(mask)
        p1, d1 = sim.get_param_planes().T, sim.get_param_draws()
        assert p1[mask].tobytes() == draw(seed, ids[mask], 1, lo, hi).tobytes()
        assert p1[~mask].tobytes() == p0[~mask].tobytes()
        assert np.array_equal(d1, np.where(mask, 2, 1).astype(np.uint32))
        # enabling again: nominal planes, zero counters
        sim.enable_params()
        nominal = np.concatenate([np.ones(8), np.zeros(8), np.ones(4)]).astype(np.float32)
        assert np.array_equal(sim.get_param_planes().T, np.broadcast_to(nominal, (n, 20)))
        assert np.all(sim.get_param_draws() == 0)
    finally:
        sim.close()


def test_draws_do_not_depend_on_sharding():
    robot, n, seed = _ball12(), 8192, 99
    lo, hi = _ranges(12, np.random.default_rng(5))
    planes = []
    for parts in ((0, n),), ((0, n // 2), (n // 2, n // 2)):
        got = []
        for off, cnt in parts:
            sim = _sim(robot, cnt, seed=seed, offset=off)
            try:
                sim.enable_params()
                nat.check(sim._lib.rb_params_set_ranges(sim.handle, nat.fptr(lo), nat.fptr(hi), 0))
                sim.sample_params(); sim.sample_params()
                got.append(sim.get_param_planes().T)
            finally:
                sim.close()
        planes.append(np.concatenate(got))
    assert planes[0].tobytes() == planes[1].tobytes()


def test_set_ranges_validation():
    sim = _sim(_msj(), 64)
    try:
        lo = np.concatenate([np.ones(8), np.zeros(8), np.ones(4)]).astype(np.float32)
        assert sim._lib.rb_params_set_ranges(sim.handle, nat.fptr(lo), nat.fptr(lo), 1) == nat.RB_EINVAL   # not enabled
        sim.enable_params()
        nat.check(sim._lib.rb_params_set_ranges(sim.handle, nat.fptr(lo), nat.fptr(lo), 1))
        for p, v in ((16, 0.0), (0, -0.5), (18, -1.0), (3, np.nan), (9, np.inf)):
            bad = lo.copy(); bad[p] = v
            assert sim._lib.rb_params_set_ranges(sim.handle, nat.fptr(bad), nat.fptr(lo if v != np.inf else bad), 1) == nat.RB_EINVAL, p
        hi = lo.copy(); hi[2] = 0.5
        assert sim._lib.rb_params_set_ranges(sim.handle, nat.fptr(lo), nat.fptr(hi), 1) == nat.RB_EINVAL
    finally:
        sim.close()


# ---- 4. fused env step: redraw on auto-reset, obs / reward against a host replay over the oracle ----
def test_env_step_redraws_exactly_the_done_envs_and_matches_a_host_replay():
    from host_env_model import HostEnvModel
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, n, seed, max_len = _msj(), 256, 21, 3
    ranges = ParamRanges(force_scale=(0.7, 1.3), setpoint_offset=(-0.02, 0.02), mass_scale=(0.6, 1.6), damping_scale=(0.5, 2.0))
    lo, hi = ranges.to_arrays(8)
    env = RoboyVecEnv(robot, n, seed=seed, max_episode_length=max_len, randomization=ranges)
    try:
        obs = env.reset()
        par, draws = env.sim.get_param_planes().T.copy(), env.sim.get_param_draws()
        assert par.tobytes() == draw(seed, np.arange(n, dtype=np.uint64), 0, lo, hi).tobytes() and np.all(draws == 1)
        host = HostEnvModel(robot, ParamOracleStepper(robot, n, seed, lo, hi, par, draws), n, seed, max_len, False, True, True)
        host.goal = host.draw(np.ones(n, bool))      # (the env's configure drew goal 0, reset() goal 1)
        assert np.array_equal(obs[:, 6:], host.goal)
        rng = np.random.default_rng(8)
        n_done = 0
        for t in range(2 * max_len + 1):
            act = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
            obs, rew, done, _ = env.step(act)
            ho, hr, hd, margin = host.step(act)
            p1, d1 = env.sim.get_param_planes().T, env.sim.get_param_draws()
            clear = margin > 1e-5
            assert np.array_equal(done[clear], hd[clear])
            assert np.array_equal(done, hd), "done flags diverged on a borderline env; host replay is no longer in step"
            n_done += done.sum()
            # exactly the done envs drew, with the restatement's values; the others are untouched
            assert p1[done].tobytes() == draw(seed, np.nonzero(done)[0].astype(np.uint64), draws[done], lo, hi).tobytes()
            assert p1[~done].tobytes() == par[~done].tobytes()
            assert np.array_equal(d1, draws + done.astype(np.uint32))
            assert np.abs(obs - ho).max() < TOL
            ok = margin > 1e-3
            assert np.abs(rew[ok] - hr[ok]).max() < 1e-3 * max(1.0, np.abs(hr[ok]).max())
            par, draws = p1.copy(), d1
            assert np.array_equal(host.stepper.par, par)
        assert n_done >= n
    finally:
        env.close()


# ---- 5. rollouts and sub-ranges ----
@pytest.mark.parametrize("chains", [1, 2])
@pytest.mark.parametrize("graph", [0, 1])
def test_rollout_dev_matches_single_parameter_steps(chains, graph):
    """rb_rollout_dev (twice: the second call replays a cached graph) against 2 K single rb_step_dev calls, bit for bit"""
    robot, n, K = _msj(), 262144, 4
    desc = robot.get_description()
    rng = np.random.default_rng(chains + 2 * graph)
    q, qd, _ = _state(desc, n, rng)
    ring = rng.uniform(-1, 1, (K, n, 8)).astype(np.float32)
    pars = random_params(rng, 8, n).astype(np.float32)
    out = []
    for mode in ("single", "rollout"):
        sim = _sim(robot, n, "rk4")
        try:
            sim.enable_params()
            sim.upload(sim.params_ptr()[0], np.ascontiguousarray(pars.T))
            sim.set_state(q, qd)
            d_ring = sim.malloc(ring.nbytes)
            sim.upload(d_ring, ring)
            if mode == "single":
                for k in range(2 * K):
                    sim.step_dev(d_ring + (k % K) * n * 8 * 4, 0.3)
            else:
                sim.set_rollout_chains(chains)
                for _ in range(2):
                    sim.rollout_dev(d_ring, K, K, 0.3, use_graph=bool(graph))
            sim.synchronize()
            out.append(sim.read_state())
        finally:
            sim.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("which", ["baked", "ball12"])
def test_step_and_env_step_ranges_over_two_halves_match_the_whole_batch(which):
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = _msj() if which == "baked" else _ball12()
    nt, n = robot.get_description().n_t, 20001
    rng = np.random.default_rng(6)
    ranges = ParamRanges(force_scale=(0.7, 1.3), mass_scale=(0.6, 1.6), setpoint_offset=(-0.02, 0.02))
    acts = rng.uniform(-1, 1, (3, n, nt)).astype(np.float32)
    res = []
    for split in (False, True):
        env = RoboyVecEnv(robot, n, seed=3, integrator="rk4", max_episode_length=2, randomization=ranges)
        try:
            env.reset()
            d_act = env.sim.malloc(acts[0].nbytes)
            d_obs, d_rew, d_done = env.sim.malloc(n * 9 * 4), env.sim.malloc(n * 4), env.sim.malloc(n * 4)
            h = 256 * 39                                  # (a range starts at a multiple of 256 envs)
            for a in acts:
                env.sim.upload(d_act, a)
                if split:
                    env.step_range_dev(0, h, None, d_act, d_obs, d_rew, d_done)
                    env.step_range_dev(h, n - h, None, d_act, d_obs, d_rew, d_done)
                    env.sim.step_range_dev(0, h, None, d_act, 1.0)
                    env.sim.step_range_dev(h, n - h, None, d_act, 1.0)
                else:
                    env.step_dev(d_act, d_obs, d_rew, d_done)
                    env.sim.step_dev(d_act, 1.0)
            env.sim.synchronize()
            res.append([*env.sim.read_state(), env.sim.download(d_obs, (n, 9)), env.sim.download(d_rew, (n,)),
                        env.sim.get_param_planes(), env.sim.get_param_draws()])
        finally:
            env.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- 6. refusals ----
def test_refusals_on_a_parameter_handle_and_a_clean_disable():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    tree = _sim(UpperBodyRobot(), 64)
    try:
        assert tree._lib.rb_params_enable(tree.handle, None) == nat.RB_EUNSUPPORTED
        assert b"ball-joint" in tree._lib.rb_last_error()
    finally:
        tree.close()
    robot, n = _msj(), 4096
    desc = robot.get_description()
    q, qd, sp = _state(desc, n, np.random.default_rng(9))
    sim, fresh = _sim(robot, n), _sim(robot, n)
    try:
        sim.enable_params()
        d_act = sim.malloc(n * 8 * 4)
        lib, h = sim._lib, sim.handle
        assert lib.rb_rollout_fused_dev(h, ctypes.c_void_p(d_act), 1, 1, ctypes.c_float(1.0)) == nat.RB_EUNSUPPORTED
        assert b"parameters" in lib.rb_last_error()
        assert lib.rb_tendon_state_dev(h, None, nat.RB_SP_SCALED, 1.0, ctypes.c_void_p(d_act), None, None, None) == nat.RB_EUNSUPPORTED
        row = nat.DispatchRow()
        assert lib.rb_dispatch_current(h, 0, ctypes.byref(row)) == nat.RB_EUNSUPPORTED
        sim.set_params(mass_scale=1.5)
        sim.forward_step_command(sp)
        sim.disable_params()
        with pytest.raises(Exception):
            sim.params_ptr()
        out = []
        for s in (sim, fresh):
            s.set_state(q, qd)
            out.append(s.forward_step_command(sp))
        for a, b in zip(*out):
            assert np.array_equal(a, b)
        assert sim.dispatch("step")["id"] == fresh.dispatch("step")["id"]
    finally:
        sim.close(); fresh.close()


# ---- 7. Python ----
def test_vec_env_with_randomization_numpy_and_torch_actions():
    import torch
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    n = 1024
    env = RoboyVecEnv(_msj(), n, seed=1, randomization=ParamRanges(force_scale=(0.5, 1.5), damping_scale=(0.5, 2.0)))
    try:
        obs = env.reset()
        p = env.get_params()
        assert p["force_scale"].shape == (n, 8) and p["setpoint_offset"].shape == (n, 8)
        assert p["mass_scale"].shape == (n,) and p["damping_scale"].shape == (n, 3)
        assert np.all(p["mass_scale"] == 1.0) and np.all(p["setpoint_offset"] == 0.0)
        assert p["force_scale"].min() >= 0.5 and p["force_scale"].max() < 1.5 and np.unique(p["force_scale"]).size > n
        obs, rew, done, _ = env.step(np.random.default_rng(0).uniform(-1, 1, (n, 8)).astype(np.float32))
        assert np.all(np.isfinite(obs)) and np.all(np.isfinite(rew))
        t_act = torch.rand((n, 8), device="cuda") * 2 - 1
        obs_t, rew_t, done_t, _ = env.step(t_act)
        assert obs_t.is_cuda and torch.isfinite(obs_t).all()
    finally:
        env.close()


def test_get_params_set_params_round_trip():
    robot, n = _ball12(), 777
    sim = _sim(robot, n)
    try:
        sim.enable_params()
        rng = np.random.default_rng(1)
        want = {"force_scale": rng.uniform(0.5, 1.5, (n, 12)).astype(np.float32),
                "setpoint_offset": rng.uniform(-0.01, 0.01, (n, 12)).astype(np.float32),
                "mass_scale": rng.uniform(0.5, 2, n).astype(np.float32),
                "damping_scale": rng.uniform(0, 2, (n, 3)).astype(np.float32)}
        sim.set_params(**want)
        got = sim.get_params()
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        sim.set_params(damping_scale=[1.0, 2.0, 3.0])
        assert np.array_equal(sim.get_params()["damping_scale"], np.broadcast_to(np.float32([1, 2, 3]), (n, 3)))
        assert np.array_equal(sim.get_params()["mass_scale"], want["mass_scale"])
    finally:
        sim.close()


@pytest.mark.parametrize("graphs", [False, True])
def test_ppo_update_runs_on_a_randomized_env(graphs):
    import torch
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env = RoboyVecEnv(_msj(), 1024, seed=2, randomization=ParamRanges(force_scale=(0.8, 1.2), mass_scale=(0.8, 1.25)))
    try:
        agent = PPO(env, n_steps=16, use_graphs=graphs, seed=3)
        roll = agent.collect()
        assert torch.isfinite(roll["act"]).all()
        agent.update(roll)
        assert all(torch.isfinite(p).all() for p in agent.policy.parameters())
        assert env.sim.get_param_draws().max() >= 1
    finally:
        env.close()
