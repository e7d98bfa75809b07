"""The feasibility flag and the joint-limit edges of every step kernel form against the fp64 oracle.

The parity tests over random states excuse a flag mismatch wherever the oracle's state AFTER the clamp lies near a limit - which
is every env the oracle calls infeasible - so a kernel that never reports an infeasible env passes them.  Here every env's flag is
compared: the inputs (tests/limit_edge_util.py: edge_states) sit on and around the limits, beyond them moving either way, and
enter with speeds outside the velocity box, and each was redrawn until the oracle's angle BEFORE the clamp lies further than
twice the tolerance from every limit in every substep (step_with_margin), so its flag has one right answer.  tests/
test_limit_edges_cpu.py qualifies the same inputs without a GPU.

Asserted per case (limit_edge_util.check_against_oracle): angles and velocities within the tolerance the robot's own parity file
uses (2e-5; the random trees: test_random_robots_gpu.tolerance), flags equal on every env, every joint the last substep clamped
on float32(limit) bit for bit with no outward velocity, the inward velocity kept where a joint beyond its limit moves back in.
The fused env step keeps its own flag and count: n_infeasible_steps equals the oracle's count, the observation's q and qd columns
hold the same tolerance."""
import numpy as np
import pytest

import limit_edge_util as lu
from gym_roboy_amd import _native as nat
from conftest import random_states
from limit_edge_util import BALL_TOL, N_BALL, N_CHAIN, N_LARGE, N_TAIL, N_TREE

pytestmark = pytest.mark.gpu

KERNELS = {"env_per_lane": 1, "tendon_per_lane": 2, "lane_pair": 5}
LANE, OCTET, SPLIT, SPLIT2 = 1, 3, 4, 6
STRIDE = 61
# The 60x group is held to the file's tolerance like everything else, except where the device was measured above it there: the
# upper body under Euler at one substep, in a velocity - one-wave form 3.0e-5, octets 3.6e-5, split 3.3e-5, lean split 2.9e-5 against
# 2e-5 (the fp32 C oracle itself: 9.4e-6; every other case stays below 8e-6).  These hold it to 4x the fp32 C oracle's own distance
# from fp64 on the same envs, 3.75e-5 (limit_edge_util.far_group_tolerance).
WIDENED_60X = {(kernel, "euler", 1) for kernel in (LANE, OCTET, SPLIT, SPLIT2)}


def _step(robot, q, qd, sp, integrator, nsub, kernel=0, expect=None, params=False, block=None):
    """one forward_step_command from (q, qd) -> ((q1, qd1, f1), rb_specialization)"""
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    sim = HipBatchSimulation(robot, len(q), integrator=integrator, n_substeps=nsub)
    try:
        if kernel:
            sim.select_kernel(kernel)
        if params:
            assert sim.enable_params() == 2 * sim.n_t + 4
            with pytest.raises(nat.NativeError, match="the parameter kernels"):        # no row of the dispatch table any more:
                sim.dispatch("step")                                                    # the step launches csrc/env_params.hpp
        if expect is not None:
            assert sim.info()["kernel"] == expect
        if block is not None:
            assert sim.dispatch("step")["block"] == block
        sim.set_state(q, qd)
        return sim.forward_step_command(sp), sim.specialization()
    finally:
        sim.close()


def _check(name, integrator, nsub, n, label, widen_far=False, **kw):
    robot, desc = lu.robot_of(name)
    q, qd, sp, info = lu.states(name, integrator, nsub, n)
    got, spec = _step(robot, q, qd, sp, integrator, nsub, **kw)
    lu.check_against_oracle(desc, q, qd, sp, info, got, integrator, nsub, lu.tol_of(name), label="%s %s nsub %d n %d" % (label, integrator, nsub, n),
                            widen_far=widen_far)
    return spec


def _check_large(name, integrator, label, expect_spec, block=256, **kw):
    """N_LARGE envs: random states with the N_TAIL edge states behind them - the tail through the full comparison, a strided sample
    of the rest against the oracle with the flags of its decided envs."""
    robot, desc = lu.robot_of(name)
    eq, eqd, esp, info = lu.states(name, integrator, 1, N_TAIL)
    rq, rqd, rsp = random_states(desc, N_LARGE - N_TAIL, 5)
    q, qd, sp = np.concatenate([rq, eq]), np.concatenate([rqd, eqd]), np.concatenate([rsp, esp])
    (q1, qd1, f1), spec = _step(robot, q, qd, sp, integrator, 1, block=block, **kw)
    assert spec == expect_spec, spec
    tail = slice(N_LARGE - N_TAIL, N_LARGE)
    lu.check_against_oracle(desc, eq, eqd, esp, info, (q1[tail], qd1[tail], f1[tail]), integrator, 1, BALL_TOL,
                            label="%s %s n %d (tail)" % (label, integrator, N_LARGE))
    idx = np.arange(0, N_LARGE - N_TAIL, STRIDE)
    qo, qdo, fo, margin = lu.step_with_margin(desc, q[idx], qd[idx], sp[idx], integrator, 1)
    assert np.abs(q1[idx] - qo).max() < BALL_TOL and np.abs(qd1[idx] - qdo).max() < BALL_TOL
    dec = lu.decided(margin, BALL_TOL)
    assert dec.mean() > 0.99 and not np.any((f1[idx] != fo) & dec)


# ---- the ball-joint class ----
@pytest.mark.parametrize("nsub", [1, 4])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_msj_robot_every_form(kernel, integrator, nsub):
    """193 envs: three waves and one lane (env per lane), 24 eight-lane groups and one, 96 lane pairs and one"""
    _check("msj", integrator, nsub, N_BALL, kernel, kernel=KERNELS[kernel], expect=KERNELS[kernel])


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_msj_robot_256_thread_form(integrator):
    """the library's choice above 65 536 envs: env per lane, 256-thread workgroups (the rolled RK4 stages)"""
    _check_large("msj", integrator, "auto", "table", expect=KERNELS["env_per_lane"])


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_kernarg_instances(integrator, monkeypatch):
    """a robot whose constants are not the ahead-of-time table's, on the kernarg instances of both launch forms"""
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    assert _check("kernarg_msj", integrator, 1, N_BALL, "kernarg", kernel=KERNELS["env_per_lane"]) == "kernarg"
    if integrator == "euler":
        _check_large("kernarg_msj", integrator, "kernarg", "kernarg", kernel=KERNELS["env_per_lane"])


def test_hiprtc_instance_of_the_same_robot():
    """the run-time-compiled instance on the robot's own constants: built only above 65 536 envs (csrc/roboy_sim.hip: maybe_jit)"""
    _check_large("kernarg_msj", "rk4", "hiprtc", "jit", kernel=KERNELS["env_per_lane"])


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_general_inertia_ball_robot_with_twelve_tendons(integrator):
    """the run-time tendon count and the general branch of the rigid-body closed form; two substeps"""
    _check("ball12", integrator, 2, N_BALL, "ball12", expect=KERNELS["env_per_lane"])


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_per_env_parameter_kernels_with_nominal_planes(integrator):
    _check("msj", integrator, 1, N_BALL, "params", params=True)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_pair_form_on_the_turned_robot(integrator):
    """the y-z mirror plane (variant 1 of the lane-pair form), kernarg constants"""
    _check("turned", integrator, 1, N_BALL, "lane_pair/turned", kernel=KERNELS["lane_pair"], expect=KERNELS["lane_pair"])


# ---- joint trees: the flag is a reduction over lanes (octets), over the parts' LDS words (split forms) ----
@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("kernel", [LANE, OCTET, SPLIT, SPLIT2])
def test_upper_body_every_form(kernel, integrator, nsub):
    """257 envs: four waves of envs and one (lane and split forms), 128 waves of two envs and a half-filled one (octets)"""
    _check("upper", integrator, nsub, N_TREE, "upper/%d" % kernel, kernel=kernel, expect=kernel,
           widen_far=(kernel, integrator, nsub) in WIDENED_60X)


def test_random_tree_through_the_hiprtc_built_split_form():
    """18 joints in 4 parts, no trunk (tests/test_random_robots_gpu.py builds the same kernel for seed 9)"""
    assert _check("tree9", "rk4", 1, N_TREE, "tree9/split", kernel=SPLIT, expect=SPLIT) == "jit"


def test_thirty_two_link_chain_through_the_octets():
    """32 levels: the deepest tree the env-per-wave form takes, every level's lanes feeding the env's flag.

    This chain turns an absolute 2e-7 in a joint's sine and cosine into up to 7.5e-6 of its largest acceleration: it is why
    csrc/tree_aba.hpp evaluates them to the last place."""
    _check("chain32", "euler", 1, N_CHAIN, "chain32/octets", expect=OCTET)


# ---- the fused env step ----
def _fused(name, integrator, n, kernel, label, widen_far=False):
    from env_obs_util import env_rescale64
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, desc = lu.robot_of(name)
    q, qd, sp, info = lu.states(name, integrator, 1, n)
    hi = float(robot.get_action_space().high[0])
    act = np.clip(sp / np.float32(hi), -1, 1).astype(np.float32)
    sp64 = env_rescale64(robot, act)
    qo, qdo, fo, margin = lu.step_with_margin(desc, q, qd, sp64, integrator, 1)
    tol = lu.tol_of(name)
    assert lu.decided(margin, tol).all()                       # (the rescale moves a set-point by an ulp: nothing becomes undecided)
    vec = RoboyVecEnv(robot, n, seed=3, auto_reset=False, integrator=integrator)
    try:
        if kernel:
            vec.sim.select_kernel(kernel)
            assert vec.sim.info()["kernel"] == kernel
        vec.reset()
        vec.sim.set_state(q, qd)
        vec.stats(reset=True)
        obs, rew, done, _ = vec.step(act)
        stats = vec.stats()
        form = vec.sim.info()["kernel"]
    finally:
        vec.close()
    nq = desc.n_q
    eq, eqd = np.abs(obs[:, :nq] - qo).max(), np.abs(obs[:, nq:2 * nq] - qdo).max()
    print("%s (kernel %d) %s fused: max |q - q64| %.3g, max |qd - qd64| %.3g; %d infeasible steps counted, the oracle has %d"
          % (label, form, integrator, eq, eqd, stats["n_infeasible_steps"], int(np.sum(~fo))))
    assert stats["n_env_steps"] == n
    assert stats["n_infeasible_steps"] == int(np.sum(~fo))
    held = np.full((n, 1), tol)
    if widen_far:
        held = lu.far_group_tolerance(desc, q, qd, sp64, info, integrator, 1, held)
    assert np.all(np.abs(obs[:, :nq] - qo) < held) and np.all(np.abs(obs[:, nq:2 * nq] - qdo) < held)
    return form


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_fused_env_step_counts_the_infeasible_envs_msj(kernel, integrator):
    _fused("msj", integrator, N_BALL, KERNELS[kernel], kernel)


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
def test_fused_env_step_counts_the_infeasible_envs_upper_body(integrator):
    assert _fused("upper", integrator, N_TREE, 0, "upper", widen_far=(SPLIT, integrator, 1) in WIDENED_60X) == SPLIT          # the library's choice at this batch size
