"""GPU half of the velocity-product tests (tests/test_velocity_terms_cpu.py qualifies the robots and inputs, DESIGN.md §3 says why):
every ball-joint kernel form that can take another robot steps a HEAVY one - a body of 0.05 - 0.09 kg m^2 at up to 2.1 rad/s, on
which a Coriolis term 10 % off is worth 150 - 300 tolerances - once against the fp64 C oracle at the project's TOL = 2e-5.

  rows        every row of the dispatch table in the ball-joint classes whose constants are not the ahead-of-time table, reached
              by tests/test_dispatch_table.recipe(row) with its robots replaced by heavy ones (SUBSTITUTE); step rows against the
              oracle, env-step rows (the fused env kernels, forms 1 / 2 / 5 and the large-batch texts) by their state planes
              against the oracle fed the set-points of rbe::action_setpoint, fused-rollout rows bit for bit against single steps
  parameters  msj_params_step and the parameter env step with a mass scale per env; the BAKED parameter instance on MsjRobot
              itself with a mass scale of 60 - the one way to make a baked instance's velocity terms visible
  cross-check the joint-tree kernel on the same heavy body against the closed form (another algorithm)
  tree        one heavy joint tree through the four tree forms
What stays open: the plain baked MsjRobot instances cannot be given another body."""
import numpy as np
import pytest

import velocity_terms_util as vt
from conftest import random_states
from gym_roboy_amd import _native as nat
from limit_edge_util import decided_envs
from test_dispatch_table import BALL8, BALLX, IDS, LARGE, ROWS, recipe
from velocity_terms_util import TOL

pytestmark = pytest.mark.gpu

SUBSTITUTE = {"msj-kernarg": ("heavy_simple", "heavy_general"), "msj-turned": ("heavy_turned",), "ball-5-tendons": ("heavy_12",)}
LANE_PAIR = 5
N = vt.N_ENVS                          # wherever the recipe does not fix the size
CROSS_TOL = 5e-6                       # tests/test_physics_gpu.py: test_kernel_forms_agree_with_each_other


def _row(row_id):
    return ROWS[IDS.index(row_id)]


def robots_for(row_id):
    """the heavy robots that stand in for the recipe's robot of this row; () where this file does not know (the CPU file fails then)"""
    answer = recipe(_row(row_id))
    return SUBSTITUTE.get(answer[0], ()) if answer else ()


def _row_cases():
    """(row id, heavy robot, substeps): the row's integrator; 1 and 4 substeps at the recipe's small sizes, 1 at the large one"""
    out = []
    for row in ROWS:
        if row.robot_class not in (BALL8, BALLX) or nat.CONSTANTS_NAMES[row.constants] == "table":
            continue
        rid = row.row_id()
        n = recipe(row)[1]
        for name in robots_for(rid):
            refused = row.kernel == LANE_PAIR and name == "heavy_general"
            for nsub in ((1,) if n == LARGE or refused else (1, 4)):
                out.append((rid, name, nsub))
    return out


ROW_CASES = _row_cases()


def _sample(n):
    return slice(None) if n <= 8192 else np.arange(0, n, 97)          # the oracle on every 97th env of a large batch


def _compare(desc, q, qd, sp, got, integrator, nsub, label, oracle_of=None, tol=TOL):
    """One step `got` = (q1, qd1, f1) against the fp64 C oracle on the given envs: angles and velocities within tol, flags by the two
    rules of tests/test_physics_gpu._check_step.  oracle_of: env -> that env's own description (per-env parameters)."""
    from oracle.c_oracle import COracle
    integ = 0 if integrator == "euler" else 1
    q1, qd1, f1 = got
    if oracle_of is None:
        qo, qdo, fo = COracle(desc, "f64").step(q, qd, sp, integrator=integ, n_substeps=nsub)
        decided = decided_envs(desc, q, qd, sp, integrator, nsub, tol)
    else:
        qo, qdo, fo = np.empty(q.shape), np.empty(q.shape), np.empty(len(q), bool)
        for i in range(len(q)):
            a = COracle(oracle_of(i), "f64").step(q[i:i + 1], qd[i:i + 1], sp[i:i + 1], integrator=integ, n_substeps=nsub)
            qo[i], qdo[i], fo[i] = a[0][0], a[1][0], a[2][0]
        decided = np.zeros(len(q), bool)                                # (looked up below for the envs whose flags differ only)
        for i in np.nonzero(np.asarray(got[2], bool) != fo)[0]:
            decided[i] = decided_envs(oracle_of(i), q[i:i + 1], qd[i:i + 1], sp[i:i + 1], integrator, nsub, tol)[0]
    eq, eqd = np.abs(q1 - qo), np.abs(qd1 - qdo)
    print("%s: max |dq| %.3g, max |dqd| %.3g over %d envs (%d infeasible)" % (label, eq.max(), eqd.max(), len(q), int(np.sum(~fo))))
    assert np.all(eq < tol), (label, eq.max())
    assert np.all(eqd < tol), (label, eqd.max())
    near = np.minimum(np.abs(qo - desc.q_lo), np.abs(qo - desc.q_hi)).min(axis=1) < 1e-5
    mismatch = np.asarray(f1, bool) != fo
    assert not np.any(mismatch & ~near), label
    assert not np.any(mismatch & decided), label
    return eq.max(), eqd.max()


def _sim(robot, n, integrator, nsub=1, **kw):
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    return HipBatchSimulation(robot, n, integrator=integrator, n_substeps=nsub, **kw)


# ---- the dispatch rows ----
@pytest.mark.parametrize("row_id,name,nsub", ROW_CASES)
def test_every_ball_joint_row_off_the_table_steps_a_heavy_robot_like_the_oracle(row_id, name, nsub, monkeypatch):
    from action_box_util import clipped_rescale64
    row = _row(row_id)
    _, n, kernel, env = recipe(row)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    robot, desc = vt.robot_of(name)
    integrator = "euler" if row.integrator == 0 else "rk4"
    entry = nat.ENTRY_NAMES[row.entry]
    q, qd, sp = vt.inputs(name, n)
    s = _sample(n)
    label = "%s %s nsub %d" % (row_id, name, nsub)
    if kernel == LANE_PAIR and name == "heavy_general":
        # products of inertia, a centre of mass off the axis: no mirror plane - the form refuses the robot and the handle stays as it was
        sim = _sim(robot, n, integrator, nsub)
        try:
            before = sim.info()["kernel"]
            with pytest.raises(nat.NativeError, match="mirror plane"):
                sim.select_kernel(kernel)
            assert sim.info()["kernel"] == before
        finally:
            sim.close()
        return
    if entry == "step":
        sim = _sim(robot, n, integrator, nsub)
        try:
            sim.select_kernel(kernel)
            assert sim.dispatch("step")["id"] == row_id
            sim.set_state(q, qd)
            q1, qd1, f1 = sim.forward_step_command(sp)
            assert sim.dispatch("step")["id"] == row_id and sim.info()["kernel"] == row.kernel
        finally:
            sim.close()
        _compare(desc, q[s], qd[s], sp[s], (q1[s], qd1[s], f1[s]), integrator, nsub, label)
    elif entry == "env_step":
        from gym_roboy_amd.envs.vec_env import RoboyVecEnv
        vec = RoboyVecEnv(robot, n, seed=3, integrator=integrator, n_substeps=nsub, auto_reset=False)      # no lane restarts
        try:
            vec.sim.select_kernel(kernel)
            assert vec.sim.dispatch("env_step")["id"] == row_id
            vec.reset()
            vec.sim.set_state(q, qd)
            act = (sp / np.float32(0.3)).astype(np.float32)             # raw actions in [-1, 1]
            vec.step(act)
            assert vec.sim.dispatch("env_step")["id"] == row_id
            q1, qd1, f1 = vec.sim.read_state()                          # the state planes
        finally:
            vec.close()
        sp_used = clipped_rescale64(robot, act)
        _compare(desc, q[s], qd[s], sp_used[s], (q1[s], qd1[s], f1[s]), integrator, nsub, label)
    else:
        ring, steps = 3, 8
        sims = [_sim(robot, n, integrator, nsub, seed=11) for _ in range(2)]
        try:
            outs = []
            for fused, sim in zip((True, False), sims):
                sim.select_kernel(1)
                sim.set_state(q, qd)
                d_ring = sim.malloc(4 * ring * n * 8)
                for r in range(ring):
                    sim.fill_actions_dev(d_ring + 4 * r * n * 8, r)
                if fused:
                    assert sim.dispatch("fused_rollout")["id"] == row_id
                    sim.rollout_fused_dev(d_ring, ring, steps, 0.3)
                    assert sim.dispatch("fused_rollout")["id"] == row_id
                else:
                    for t in range(steps):
                        sim.step_dev(d_ring + 4 * (t % ring) * n * 8, 0.3)
                    assert sim.dispatch("step")["id"] == row_id.replace("fused_rollout", "step")     # the row held to the oracle above
                sim.synchronize()
                outs.append(sim.read_state())
        finally:
            for sim in sims:
                sim.close()
        assert all(np.array_equal(a, b) for a, b in zip(*outs)), label
        assert np.abs(outs[0][0] - q).max() > 0.01                      # it moved


def test_fused_open_loop_rollout_of_a_heavy_robot_equals_single_steps():
    """rb_rollout_fused_dev on heavy_simple, 4 096 envs and 8 steps, both integrators at two substeps: bit for bit, the last step's
    flags included (tests/test_physics_gpu.py: test_fused_open_loop_rollout_equals_single_steps does this for MsjRobot)"""
    robot, desc = vt.robot_of("heavy_simple")
    n, ring, steps = 4096, 3, 8
    q, qd, _ = vt.inputs("heavy_simple", n)
    for integrator in ("euler", "rk4"):
        sims = [_sim(robot, n, integrator, 2, seed=11) for _ in range(2)]
        try:
            outs = []
            for fused, sim in zip((True, False), sims):
                sim.select_kernel(1)
                assert sim.specialization() == "kernarg"
                sim.set_state(q, qd)
                d_ring = sim.malloc(4 * ring * n * 8)
                for r in range(ring):
                    sim.fill_actions_dev(d_ring + 4 * r * n * 8, r)
                if fused:
                    sim.rollout_fused_dev(d_ring, ring, steps, 0.9)
                else:
                    for t in range(steps):
                        sim.step_dev(d_ring + 4 * (t % ring) * n * 8, 0.9)
                sim.synchronize()
                outs.append(sim.read_state())
        finally:
            for sim in sims:
                sim.close()
        assert all(np.array_equal(a, b) for a, b in zip(*outs)), integrator
        assert np.abs(outs[0][0] - q).max() > 0.01


# ---- the parameter kernels ----
def _nominal_params(n, nt, mass):
    par = np.concatenate([np.ones(nt), np.zeros(nt), [1.0], np.ones(3)])[None].repeat(n, axis=0)
    par[:, 2 * nt] = mass
    return par.astype(np.float32)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("nsub", [1, 4])
def test_parameter_step_on_a_heavy_robot_with_a_mass_scale_per_env(integrator, nsub):
    """msj_params_step (kernarg constants) on heavy_general, mass scales in [0.5, 2] and every other parameter nominal: each env
    against the oracle on its own description (tests/env_params_util.perturbed)"""
    from env_params_util import perturbed
    robot, desc = vt.robot_of("heavy_general")
    q, qd, sp = vt.inputs("heavy_general")
    mass = np.random.default_rng(5).uniform(0.5, 2.0, N).astype(np.float32)
    par = _nominal_params(N, 8, mass)
    sim = _sim(robot, N, integrator, nsub)
    try:
        assert sim.enable_params() == 20
        sim.set_params(mass_scale=mass)
        assert np.array_equal(sim.get_param_planes().T, par) and sim.specialization() == "kernarg"
        sim.set_state(q, qd)
        got = sim.forward_step_command(sp)
    finally:
        sim.close()
    _compare(desc, q, qd, sp, got, integrator, nsub, "msj_params_step heavy_general %s nsub %d" % (integrator, nsub),
             oracle_of=lambda i: perturbed(desc, par[i].astype(np.float64)))


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_parameter_env_step_on_a_heavy_robot_with_a_mass_scale_per_env(integrator):
    """the parameter env step (kernarg constants) on heavy_general with the mass scales its own reset() drew from [0.5, 2]: the state
    planes after one step with raw actions"""
    from action_box_util import clipped_rescale64
    from env_params_util import perturbed
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, desc = vt.robot_of("heavy_general")
    q, qd, sp = vt.inputs("heavy_general")
    vec = RoboyVecEnv(robot, N, seed=3, integrator=integrator, auto_reset=False, randomization=ParamRanges(mass_scale=(0.5, 2.0)))
    try:
        vec.reset()
        par = vec.sim.get_param_planes().T.copy()
        assert np.array_equal(par, _nominal_params(N, 8, par[:, 16])) and 0.5 <= par[:, 16].min() < 0.6 and 1.9 < par[:, 16].max() <= 2.0
        assert vec.sim.specialization() == "kernarg"
        vec.sim.set_state(q, qd)
        act = (sp / np.float32(0.3)).astype(np.float32)
        vec.step(act)
        got = vec.sim.read_state()
    finally:
        vec.close()
    _compare(desc, q, qd, clipped_rescale64(robot, act), got, integrator, 1, "msj_params_env_step heavy_general %s" % integrator,
             oracle_of=lambda i: perturbed(desc, par[i].astype(np.float64)))


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("entry", ["step", "env_step"])
def test_baked_parameter_instance_with_sixty_times_the_mass(entry, integrator):
    """MsjRobot itself on its BAKED parameter instances with mass_scale = 60 on every env (the validator asks for > 0 only), from
    random_states: the body is then 0.018 / 0.018 / 0.03 kg m^2 and the Coriolis term worth 205 - 213 TOL (x 0.9 moves 21) - the one
    way to make the velocity terms of a baked instance visible.  One substep: the table is baked for MsjRobot's own step, and a
    handle with more substeps runs the kernarg instances held above."""
    nsub = 1
    from action_box_util import clipped_rescale64
    from env_params_util import perturbed
    from gym_roboy_amd.envs.robots import MsjRobot
    robot = MsjRobot()
    desc = robot.get_description()
    q, qd, sp = random_states(desc, N, 17)
    par = _nominal_params(N, 8, 60.0)
    heavy = perturbed(desc, par[0].astype(np.float64))
    label = "baked parameter %s x60 %s nsub %d" % (entry, integrator, nsub)
    if entry == "step":
        sim = _sim(robot, N, integrator, nsub)
        try:
            sim.enable_params()
            sim.set_params(mass_scale=60.0)
            assert np.array_equal(sim.get_param_planes().T, par) and sim.specialization() == "table"
            sim.set_state(q, qd)
            got = sim.forward_step_command(sp)
        finally:
            sim.close()
        _compare(heavy, q, qd, sp, got, integrator, nsub, label)
    else:
        from gym_roboy_amd.envs.params import ParamRanges
        from gym_roboy_amd.envs.vec_env import RoboyVecEnv
        vec = RoboyVecEnv(robot, N, seed=3, integrator=integrator, n_substeps=nsub, auto_reset=False,
                          randomization=ParamRanges(mass_scale=(60.0, 60.0)))
        try:
            vec.reset()
            assert np.array_equal(vec.sim.get_param_planes().T, par) and vec.sim.specialization() == "table"
            vec.sim.set_state(q, qd)
            act = (sp / np.float32(0.3)).astype(np.float32)
            vec.step(act)
            got = vec.sim.read_state()
        finally:
            vec.close()
        _compare(heavy, q, qd, clipped_rescale64(robot, act), got, integrator, nsub, label)


# ---- another algorithm on the same body ----
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_joint_tree_kernel_agrees_with_the_closed_form_on_the_heavy_body(integrator):
    """heavy_general through the joint-tree kernel (form 3; 1e-30 kg on a virtual link takes it out of the ball-joint class and
    changes nothing else) against the env-per-lane closed form on heavy_general: the bound of test_kernel_forms_agree_with_each_other"""
    q, qd, sp = vt.inputs("heavy_general")
    out = []
    for name, kernel in (("heavy_general", 1), ("general_as_tree", 3)):
        sim = _sim(vt.robot_of(name)[0], N, integrator)
        try:
            if kernel == 1:
                sim.select_kernel(kernel)
            assert sim.info()["kernel"] == kernel
            sim.set_state(q, qd)
            out.append(sim.forward_step_command(sp))
        finally:
            sim.close()
    eq, eqd = np.abs(out[0][0] - out[1][0]).max(), np.abs(out[0][1] - out[1][1]).max()
    print("joint-tree kernel against the closed form, heavy_general %s: |dq| %.3g |dqd| %.3g" % (integrator, eq, eqd))
    assert eq < CROSS_TOL and eqd < CROSS_TOL, (eq, eqd)
    assert np.mean(out[0][2] == out[1][2]) > 0.999


# ---- the tree companion ----
TREE_FORMS = {"env_per_wave": 3, "env_per_lane": 1, "env_per_lane_split": 4, "env_per_lane_split2": 6}


@pytest.mark.parametrize("form,integrator", [("env_per_wave", "euler"), ("env_per_wave", "rk4"), ("env_per_lane", "rk4"),
                                             ("env_per_lane_split", "rk4"), ("env_per_lane_split2", "rk4")])
def test_heavy_joint_tree_through_the_four_tree_forms(form, integrator):
    """random tree 5 with ten times its inertia tensors at 2 rad/s (tests/velocity_terms_util.heavy_tree; qualified on the CPU):
    octets, one wave, split and lean split - the last three built by hiprtc - against the oracle at test_random_robots_gpu.tolerance"""
    from test_random_robots_gpu import tolerance
    robot, desc = vt.heavy_tree()
    q, qd, sp = vt.inputs("heavy_tree")
    sim = _sim(robot, N, integrator)
    try:
        sim.select_kernel(TREE_FORMS[form])
        assert sim.info()["kernel"] == TREE_FORMS[form] and sim.specialization() == ("kernarg" if form == "env_per_wave" else "jit")
        sim.set_state(q, qd)
        got = sim.forward_step_command(sp)
    finally:
        sim.close()
    _compare(desc, q, qd, sp, got, integrator, 1, "heavy tree %s %s" % (form, integrator), tol=tolerance(desc, q, qd, sp))
