"""The INPUTS of tests/test_limit_edges_gpu.py, qualified by the reference alone (as tests/test_action_box_cpu.py does for the
action box): every (robot, integrator, substeps, batch) it steps must visit the limit edges it claims to visit, with every env's
flag decided - otherwise "flags equal on every env" would hold of a kernel that never reports an infeasible env.  These are
conditions on the test inputs and on tests/limit_edge_util.py, not tolerances on any kernel; the last test runs the product's
closed form built for the host through the comparison the GPU file makes."""
import ctypes

import numpy as np
import pytest

import limit_edge_util as lu
from limit_edge_util import BAND, BEYOND_IN, BEYOND_OUT, FAST, INPUTS, INTERIOR, STRATA, TWO_JOINTS

IDS = ["%s-%s-%d-%d" % c for c in INPUTS]
MIN_CALM_TREE_ENVS = 4          # envs of a joint tree's 60x group (Euler) whose result carries the tendon forces at v < -1
MIN_SLOW_FIBRES = 100           # tendon evaluations with v < -1 in the 60x groups of MsjRobot's Euler inputs, all inputs together


def _reference(name, integrator, nsub, n):
    desc = lu.robot_of(name)[1]
    q, qd, sp, info = lu.states(name, integrator, nsub, n)
    return desc, q, qd, sp, info, lu.step_with_margin(desc, q, qd, sp, integrator, nsub, detail=True)


@pytest.mark.parametrize("name,integrator,nsub,n", INPUTS, ids=IDS)
def test_the_substep_loop_equals_the_oracles_step_bit_for_bit(name, integrator, nsub, n):
    from oracle.c_oracle import COracle
    desc, q, qd, sp, info, (qo, qdo, fo, margin, hit, jm, ever) = _reference(name, integrator, nsub, n)
    want = COracle(desc, "f64").step(q, qd, sp, integrator=0 if integrator == "euler" else 1, n_substeps=nsub)
    assert np.array_equal(want[0], qo) and np.array_equal(want[1], qdo) and np.array_equal(want[2], fo)
    assert np.isfinite(qo).all() and np.isfinite(qdo).all()
    again = lu.edge_states(desc, n, lu.SEED, integrator, nsub, lu.tol_of(name), band_sp=lu.BAND_SP.get(name, 0.3))
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], (q, qd, sp)))                 # deterministic


def test_the_substep_loop_on_the_numpy_oracle(msj_oracle, msj_robot):
    """the same loop written out against oracle/physics_np.py, the statement of the model"""
    q, qd, sp, _ = lu.states("msj", "rk4", 4, lu.N_BALL)
    a, b, ok = q.astype(np.float64), qd.astype(np.float64), np.ones(len(q), bool)
    for _ in range(4):
        a, b, f = msj_oracle.step(a, b, sp.astype(np.float64), step_size=0.1 / 4, integrator=1, n_substeps=1)
        ok &= f
    want = msj_oracle.step(q.astype(np.float64), qd.astype(np.float64), sp.astype(np.float64), integrator=1, n_substeps=4)
    assert np.array_equal(want[0], a) and np.array_equal(want[1], b) and np.array_equal(want[2], ok)
    got = lu.step_with_margin(msj_robot.get_description(), q, qd, sp, "rk4", 4)
    assert np.abs(got[0] - a).max() < 1e-13 and np.abs(got[1] - b).max() < 1e-12 and np.array_equal(got[2], ok)


@pytest.mark.parametrize("name,integrator,nsub,n", INPUTS, ids=IDS)
def test_every_env_is_decided_and_every_stratum_does_what_it_says(name, integrator, nsub, n):
    desc, q, qd, sp, info, (qo, qdo, fo, margin, hit, jm, ever) = _reference(name, integrator, nsub, n)
    tol = lu.tol_of(name)
    tol = np.asarray(tol(q, qd, sp) if callable(tol) else tol).reshape(-1)
    assert np.sum(~lu.decided(margin, tol)) == 0                                             # no env is left out of the flag comparison
    st, j, sd = info["stratum"], info["joint"], info["side"]
    h = 0.1 / nsub
    for s in range(len(STRATA)):
        assert np.sum(st == s) >= n // len(STRATA) - 1, STRATA[s]
    assert np.array_equal(st[:-1], (np.arange(n) % len(STRATA))[:-1])                        # interleaved env by env
    assert not fo[0] and not fo[-1]
    assert fo[st == INTERIOR].all() and fo[st == FAST].all()
    assert not fo[np.isin(st, (BEYOND_OUT, BEYOND_IN, TWO_JOINTS))].any()
    inside = np.all((q >= 0.9 * desc.q_lo - 1e-6) & (q <= 0.9 * desc.q_hi + 1e-6), axis=1)
    assert inside[st == INTERIOR].all() and inside[st == FAST].all()
    rows = np.arange(n)
    lim = np.where(sd > 0, desc.q_hi[np.maximum(j, 0)], desc.q_lo[np.maximum(j, 0)])
    start, v0 = q[rows, np.maximum(j, 0)].astype(np.float64), qd[rows, np.maximum(j, 0)].astype(np.float64)
    # band: inside, within one substep's travel of the limit, moving towards it; it crosses exactly where it was asked to
    k = st == BAND
    gap = (lim - start) * sd
    assert np.all((gap[k] > 0) & (gap[k] <= h * desc.qd_max[j[k]])) and np.all(v0[k] * sd[k] > 0)
    assert np.array_equal(~fo[k], info["want_cross"][k])
    # beyond: 0.06 - 0.2 rad outside, further than a step travels; outward / inward
    k = np.isin(st, (BEYOND_OUT, BEYOND_IN, TWO_JOINTS))
    assert np.all((-gap[k] >= 0.06 - 1e-6) & (-gap[k] <= 0.2 + 1e-6) & (-gap[k] > 0.1 * desc.qd_max[j[k]]))
    assert np.all(v0[st == BEYOND_OUT] * sd[st == BEYOND_OUT] > 0) and np.all(v0[st == BEYOND_IN] * sd[st == BEYOND_IN] < 0)
    k = st == BEYOND_IN                                                                      # clamped, flagged, the inward velocity kept
    assert np.all(ever[k, j[k]] == np.where(sd[k] > 0, 2, 1)) and np.all(qdo[k, j[k]] * sd[k] < -0.1 * desc.qd_max[j[k]])
    k = st == BEYOND_OUT
    assert np.all(ever[k, j[k]] == np.where(sd[k] > 0, 2, 1))
    if nsub == 1:                                                                            # no outward velocity is left, and some envs' was dropped
        assert np.all(qdo[k, j[k]] * sd[k] <= 0.0) and np.sum(qdo[k, j[k]] == 0.0) >= 2
    k = st == TWO_JOINTS                                                                     # two different joints beyond opposite limits
    j2 = info["joint2"][k]
    assert np.all(j2 != j[k]) and np.all(ever[k, j[k]] == np.where(sd[k] > 0, 2, 1)) and np.all(ever[k, j2] == np.where(sd[k] > 0, 1, 2))
    # fast entries: up to 3x the box on every joint; the 60x group at 45x - 60x on every joint but its calm one, which starts and
    # ends the step inside the velocity box while at least MIN_LOADED active tendons that turn it shorten faster than v_max
    k, far, calm = (st == FAST) & ~info["far"], info["far"], info["calm"]
    ratio = np.abs(qd) / desc.qd_max
    assert far.sum() >= 2 * k.sum() > 0 and np.all(ratio[k] <= lu.FAST_BOX + 1e-5) and np.mean(ratio[k] > 1.0) > 0.4
    fast_joint = np.ones(q.shape, bool)
    has = far & (calm >= 0)
    fast_joint[rows[has], calm[has]] = False
    assert np.all((ratio[far] >= 0.75 * lu.FAST_FAR - 1e-3) & (ratio[far] <= lu.FAST_FAR + 1e-3) | ~fast_joint[far])
    assert np.all(ratio[rows[has], calm[has]] <= 1.0 + 1e-6) and np.all(np.abs(qdo[rows[has], calm[has]]) < lu.CALM_BOX * desc.qd_max[calm[has]])
    assert np.all(lu.loaded_fibres(desc, q[has], qd[has], sp[has], calm[has]) >= lu.MIN_LOADED)
    # (joint trees: the fast joints' Coriolis terms saturate most joints, and few envs find a calm one; RK4 never reaches the clamp)
    print("%s %s nsub %d: %d of the %d envs of the 60x group have a calm joint" % (name, integrator, nsub, has.sum(), far.sum()))
    if name in lu.BALL_ROBOTS:
        assert has.sum() == far.sum() and len(set(calm[has])) == 3
    elif integrator == "euler":
        assert has.sum() >= MIN_CALM_TREE_ENVS
    hits = [(jj, side) for jj in range(desc.n_q) for side in (1, 2) if np.any(ever[:, jj] & side)]
    if name in lu.BALL_ROBOTS:
        # every (joint, side): at least 2 band envs that cross and 2 that stop short
        for jj in range(3):
            for side in (-1, 1):
                k = (st == BAND) & (j == jj) & (sd == side)
                assert np.sum(~fo[k]) >= 2 and np.sum(fo[k]) >= 2, (jj, side, int(np.sum(~fo[k])), int(np.sum(fo[k])))
    assert len(hits) == 2 * desc.n_q                                                         # every joint is clamped onto both of its limits


@pytest.mark.parametrize("name,form", [("upper", 0), ("upper", 1), ("tree9", 0)])
def test_every_part_of_the_split_forms_owns_a_clamped_joint(name, form, tmp_path):
    """The split forms keep one flag word per part (csrc/tree_lane_split.hpp): in every input of these robots every part owns a
    joint that some env clamps - and, the more telling case, an env whose ONLY clamped joints lie in that part."""
    import gen_tree_lane_baked as gen
    desc = lu.robot_of(name)[1]
    parts = np.array(gen.generate_split(desc, str(tmp_path / "split.hpp"), *gen.library_split_form(form))["part_of_joint"])
    assert parts.max() >= 1
    for case in [c for c in INPUTS if c[0] == name]:
        ever = _reference(*case)[5][6]
        for p in range(parts.max() + 1):
            own = (ever[:, parts == p] != 0).any(axis=1)
            others = (ever[:, parts != p] != 0).any(axis=1)
            assert own.any() and (own & ~others).any(), (case, p)


class _NoLowerClamp:
    """oracle/physics_np.py's muscle with the force-velocity curve left unclamped below v = -1 and not floored at zero, as the
    closed form of csrc/msj_math.hpp would be without the lower bound of p = clamp(1 + v, 0, 1): the defect the 60x group is for"""

    def __init__(self, desc):
        from oracle.physics_np import TendonRobotOracle

        class Broken(TendonRobotOracle):
            def muscle_force(self, length, length_rate, setpoint):
                l0 = self.l0
                act = np.clip(self.kp * (length - l0 - self.sigma * setpoint) / l0, 0.0, 1.0)
                ln = length / l0
                f_l = np.exp(-((ln - 1.0) / self.fl_width) ** 2)
                v = length_rate / (self.v_max * l0)
                c1 = np.where(v > 0.0, self.fv_long[0], self.fv_short[0])
                c2 = np.where(v > 0.0, self.fv_long[1], self.fv_short[1])
                f_v = (1.0 + c1 * v) / (1.0 + c2 * v)                       # no max(v, -1), no max(., 0)
                f_pe = np.maximum((np.exp(self.kpe * (ln - 1.0) / self.e0) - 1.0) / (np.exp(self.kpe) - 1.0), 0.0)
                return self.f_max * (act * f_l * f_v + f_pe)
        self.good, self.broken = TendonRobotOracle(desc), Broken(desc)


@pytest.mark.parametrize("name,integrator,nsub,n", [c for c in INPUTS if c[0] in lu.BALL_ROBOTS and c[1] == "euler"],
                         ids=[i for i, c in zip(IDS, INPUTS) if c[0] in lu.BALL_ROBOTS and c[1] == "euler"])
def test_dropping_the_force_velocity_clamp_moves_the_60x_group(name, integrator, nsub, n):
    """v < -1 (shortening faster than v_max l0) in the acceleration evaluation at the entry speeds - Euler's only one; RK4
    saturates its stage velocities first.  The group's result must DEPEND on the clamp: without it the calm joint's velocity after
    the step moves by more than ten tolerances in most of the group's envs (and nothing else of the input moves at all: the
    clamp is reached nowhere else)."""
    desc = lu.robot_of(name)[1]
    q, qd, sp, info = lu.states(name, integrator, nsub, n)
    far, calm = info["far"], info["calm"]
    o = _NoLowerClamp(desc)
    a = o.good.step(q.astype(np.float64), qd.astype(np.float64), sp.astype(np.float64), integrator=0, n_substeps=nsub)
    b = o.broken.step(q.astype(np.float64), qd.astype(np.float64), sp.astype(np.float64), integrator=0, n_substeps=nsub)
    moved = np.maximum(np.abs(a[0] - b[0]), np.abs(a[1] - b[1]))
    at_calm = np.abs(a[1] - b[1])[np.nonzero(far)[0], calm[far]]
    slow = int(np.sum(lu.fibre_speed(desc, q[far], qd[far]) < -1.0))
    print("%s euler nsub %d n %d: %d of %d tendon evaluations of the 60x group have v < -1; without the clamp the calm joint's "
          "velocity moves by %.3g (median) / %.3g (least); %d of %d envs by more than 10 tolerances"
          % (name, nsub, n, slow, far.sum() * desc.n_t, np.median(at_calm), at_calm.min(), int(np.sum(at_calm > 10 * lu.BALL_TOL)), far.sum()))
    assert slow >= lu.MIN_LOADED * far.sum()
    # one substep: every env; more: the later substeps run inside the box and may saturate the joint or damp the difference away
    per_env = moved[far].max(axis=1)
    assert np.sum(per_env > 10 * lu.BALL_TOL) >= (1.0 if nsub == 1 else 0.5) * far.sum() - (nsub == 1)
    assert moved[~far].max() < 1e-12


def test_the_60x_groups_of_msj_robot_hold_a_hundred_fast_fibres():
    desc = lu.robot_of("msj")[1]
    total = 0
    for name, integrator, nsub, n in INPUTS:
        if name == "msj" and integrator == "euler":
            q, qd, sp, info = lu.states(name, integrator, nsub, n)
            total += int(np.sum(lu.fibre_speed(desc, q[info["far"]], qd[info["far"]]) < -1.0))
    assert total >= MIN_SLOW_FIBRES


@pytest.mark.parametrize("name,integrator,nsub,n", [c for c in INPUTS if c[0] in lu.BALL_ROBOTS], ids=[i for i, c in zip(IDS, INPUTS) if c[0] in lu.BALL_ROBOTS])
def test_the_closed_form_built_for_the_host_passes_the_full_comparison(hostmath_lib, name, integrator, nsub, n):
    """hm_step_f32: csrc/msj_math.hpp in fp32 on the host, through the comparison of tests/test_limit_edges_gpu.py - angles and
    velocities within the tolerance, flags equal on every env, clamped joints on float32(limit) bit for bit."""
    desc = lu.robot_of(name)[1]
    q, qd, sp, info = lu.states(name, integrator, nsub, n)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    q1, qd1, sp1, f1 = q.copy(), qd.copy(), sp.copy(), np.zeros(n, np.uint8)
    rc = hostmath_lib.hm_step_f32(ctypes.byref(desc.as_c_struct()), ctypes.c_double(0.1), nsub, 0 if integrator == "euler" else 1,
                                  ctypes.c_long(n), P(q1, ctypes.c_float), P(qd1, ctypes.c_float), P(sp1, ctypes.c_float), P(f1, ctypes.c_ubyte))
    assert rc == 0
    lu.check_against_oracle(desc, q, qd, sp, info, (q1, qd1, f1.astype(bool)), integrator, nsub, lu.BALL_TOL, label="host fp32 %s" % name)
