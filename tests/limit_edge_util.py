"""Inputs and the reference for the feasibility flag and the joint-limit edges of the step kernels (tests/test_limit_edges_cpu.py
qualifies them without a GPU, tests/test_limit_edges_gpu.py runs them).

The flag is a discontinuity: a kernel within its tolerance of the oracle may still land on the other side of a limit.  Whether an
env's flag is DECIDED is therefore read off the oracle's angle BEFORE the clamp: step_with_margin steps, beside every substep of
the oracle, a second oracle whose limits are out of reach (+-10 rad) from the same state, and reports the smallest distance of
that free angle from any limit over substeps, joints and both sides.  An env whose margin exceeds twice the tolerance the angles
are held to has one right answer for its flag, whichever side of the limit it is on.  (The older rule of the parity tests took the
distance AFTER the clamp: an env the oracle calls infeasible sits exactly on a limit there, so its flag was always excused.)

edge_states draws states that visit the edges - on and around the limits, beyond them moving either way, entry speeds outside
the velocity box - and redraws every env until it is decided, so a test over them compares the flag of every env."""
import numpy as np

STRATA = ("beyond_out", "interior", "band", "beyond_in", "fast", "two_joints")
(BEYOND_OUT, INTERIOR, BAND, BEYOND_IN, FAST, TWO_JOINTS) = range(6)
FAST_BOX, FAST_FAR = 3.0, 60.0         # entry speeds as multiples of the velocity box: RK4's first stage saturates; the f_V clamp at v = -1
FREE_LIMIT = 10.0                      # rad: the limits of the second oracle
BAND_CANDIDATES = 24
BAND_GIVE_UP = 40                      # rounds after which a band env that does not cross is asked to stop short
FAST_CANDIDATES = 16
FAST_JOINTS_TRIED = 8                  # ... and joints after which it runs every joint fast (joint trees: the fast joints' Coriolis terms saturate most joints)
FAST_GIVE_UP = 12                      # rounds after which an env of the 60x group takes the next joint as its calm one
CALM_BOX, MIN_LOADED = 0.9, 2            # the 60x group: its calm joint ends the step inside 0.9 of the velocity box; loaded fibres per env
DECIDED = 2.0                        # an env is decided when its margin exceeds DECIDED * tol (the kernel's error at the
                                       # intermediate substeps, which nothing asserts directly, is covered by the factor)

_ORACLES = {}


def _integ(integrator):
    return {"euler": 0, "rk4": 1}.get(integrator, integrator)


def free_description(desc):
    """a copy of the description with every joint limit moved out of reach"""
    from gym_roboy_amd.envs.robots import RobotDescription
    spec = desc.to_dict()
    for j in spec["joints"]:
        j["limit"] = [-FREE_LIMIT, FREE_LIMIT]
    return RobotDescription(spec)


def fresh_oracles(desc):
    """(COracle of the description, COracle of its limit-free copy), fp64"""
    from oracle.c_oracle import COracle
    return COracle(desc, "f64"), COracle(free_description(desc), "f64")


def oracles(desc):
    """the same pair, kept for the session - for the descriptions of the named inputs (robot_of), which live that long anyway"""
    if id(desc) not in _ORACLES:
        _ORACLES[id(desc)] = (desc,) + fresh_oracles(desc)
    return _ORACLES[id(desc)][1:]


def step_with_margin(desc, q, qd, sp, integrator, nsub, step_size=0.1, detail=False, threads=1, pair=None):
    """One env step of the fp64 oracle, one substep at a time -> (q', qd', feasible, margin); margin[i] is the smallest
    |q_free - limit| over substeps, joints and both limits, q_free being the angle the substep reaches without the clamp.
    detail: also (hit [n, n_q] in {-1, 0, +1}: the joints the LAST substep clamped onto their lower / upper limit, joint_margin
    [n, n_q]: that substep's distance of each free angle from its nearer limit, ever [n, n_q]: bit 0 / 1 set where some substep
    clamped the joint onto its lower / upper limit)."""
    orc, free = pair or oracles(desc)
    integ = _integ(integrator)
    q = np.array(q, dtype=np.float64).reshape(-1, desc.n_q)
    qd = np.array(qd, dtype=np.float64).reshape(-1, desc.n_q)
    sp = np.array(sp, dtype=np.float64).reshape(-1, desc.n_t)
    h = step_size / nsub
    feasible = np.ones(q.shape[0], bool)
    margin = np.full(q.shape[0], np.inf)
    hit = joint_margin = None
    ever = np.zeros(q.shape, np.int8)
    for _ in range(nsub):
        qf = free.step(q, qd, sp, step_size=h, integrator=integ, n_substeps=1, threads=threads)[0]
        joint_margin = np.minimum(np.abs(qf - desc.q_lo), np.abs(qf - desc.q_hi))
        hit = (qf > desc.q_hi).astype(np.int8) - (qf < desc.q_lo).astype(np.int8)
        ever |= (hit < 0) * np.int8(1) + (hit > 0) * np.int8(2)
        margin = np.minimum(margin, joint_margin.min(axis=1))
        q, qd, ok = orc.step(q, qd, sp, step_size=h, integrator=integ, n_substeps=1, threads=threads)
        feasible &= ok
    if detail:
        return q, qd, feasible, margin, hit, joint_margin, ever
    return q, qd, feasible, margin


def fibre_speed(desc, q, qd):
    """v [n, n_t] = tendon length rate / (v_max l0), < 0 shortening: the force-velocity curve is clamped below v = -1"""
    orc = oracles(desc)[0]
    _, L = orc.tendon_geometry(np.asarray(q, np.float64))
    return np.einsum("nkj,nj->nk", L, np.asarray(qd, np.float64)) / (desc.muscle["v_max"] * orc.rest_lengths())


def loaded_fibres(desc, q, qd, sp, joint=None):
    """[n]: the tendons of each env that shorten faster than v_max l0 (v < -1) while their muscle is active (activation > 0.1) -
    where the force-velocity curve's clamp at v = -1 decides the force; joint [n]: only tendons with a moment arm about that joint"""
    orc = oracles(desc)[0]
    length, L = orc.tendon_geometry(np.asarray(q, np.float64))
    l0 = orc.rest_lengths()
    v = np.einsum("nkj,nj->nk", L, np.asarray(qd, np.float64)) / (desc.muscle["v_max"] * l0)
    act = np.clip(desc.muscle["kp"] * (length - l0 - desc.muscle["setpoint_scale"] * np.asarray(sp, np.float64)) / l0, 0.0, 1.0)
    arm = True if joint is None else (np.abs(L[np.arange(len(L)), :, np.maximum(joint, 0)]) > 1e-3) | (np.asarray(joint) < 0)[:, None]
    return np.sum((v < -1.0) & (act > 0.1) & arm, axis=1)


def decided(margin, tol):
    return margin > DECIDED * np.asarray(tol).reshape(-1)


def decided_envs(desc, q, qd, sp, integrator, nsub, tol):
    """[n] bool: the envs whose feasibility flag after this step has one right answer at the tolerance tol (a number, [n] or
    [n, 1]) - for the parity tests over random states, which assert the flags of these"""
    # (the callers make a description per test: nothing of it is kept)
    return decided(step_with_margin(desc, q, qd, sp, integrator, nsub, threads=8 if len(q) > 4096 else 1, pair=fresh_oracles(desc))[3], tol)


def strata_of(n):
    """stratum of every env: interleaved env by env, so that every wave, 8-lane group and lane pair mixes outcomes; env 0 and
    env n - 1 are ones that start beyond a limit"""
    s = np.arange(n) % len(STRATA)
    if s[-1] not in (BEYOND_OUT, BEYOND_IN, TWO_JOINTS):
        s[-1] = BEYOND_OUT
    return s


def _free_displacement(desc, q, qd, sp, integ, h, nsteps):
    free = oracles(desc)[1]
    q1 = free.step(q, qd, sp, step_size=h * nsteps, integrator=integ, n_substeps=nsteps)[0]
    return q1 - q


def edge_states(desc, n, seed, integrator, nsub, tol=2e-5, step_size=0.1, max_rounds=400, band_sp=0.3):
    """tol: the tolerance the caller holds the angles to - a number, or a function (q, qd, sp) -> [n, 1] or [n] where it depends
    on the state.  band_sp: the largest set-point magnitude of the band stratum (0.3: the action box of every robot here, as everywhere
    else; the plain step takes set-points as they come, and some robots reach some limits from inside only under stronger ones).
    -> q, qd, sp (float32) and info: 'stratum' [n], 'joint' / 'side' [n] (the target joint and limit of the band and beyond
    strata; the first of the two for two_joints; -1 / 0 elsewhere), 'joint2' [n], 'want_cross' [n] (band), 'far' [n] (the 60x
    group of the fast stratum), 'calm' [n] (its joint that stays inside the velocity box, -1 elsewhere).  Deterministic in its arguments.  Every env is redrawn until step_with_margin calls it decided
    at this integrator and substep count, and until it does what its stratum says:
      interior    inside 0.9 of the box, feasible
      band        the target joint within h * qd_max of its limit, moving towards it; every second one of a (joint, side) crosses,
                  the others stop short (the start angle is solved for from a drawn overshoot / shortfall)
      beyond_out  the target joint 0.06 - 0.2 rad beyond its limit (more than one step's travel), moving further out
      beyond_in   the same start, moving back in: clamped, flagged, and the saturated inward velocity is kept
      fast        inside the box, |qd| up to 3x the velocity box on every joint; three of four envs at 45x - 60x on every joint
                  but one, which ends the step inside the velocity box; feasible
      two_joints  two different joints beyond opposite limits"""
    integ = _integ(integrator)
    rng = np.random.default_rng([seed, n, integ, nsub])
    nq, nt = desc.n_q, desc.n_t
    h = step_size / nsub
    lo, hi, vmax = desc.q_lo, desc.q_hi, desc.qd_max
    lim = np.stack([lo, hi])                                         # [side index 0 / 1][joint]
    stratum = strata_of(n)
    rank = np.zeros(n, np.int64)                                     # position of the env inside its stratum
    for s in range(len(STRATA)):
        rank[stratum == s] = np.arange(np.sum(stratum == s))
    combo = rank % (2 * nq)                                          # round robin over all joints and both sides
    joint = np.where(np.isin(stratum, (BAND, BEYOND_OUT, BEYOND_IN, TWO_JOINTS)), combo // 2, -1)
    side = np.where(joint >= 0, 2 * (combo % 2) - 1, 0)              # -1: the lower limit, +1: the upper
    joint2 = np.where(stratum == TWO_JOINTS, (joint + 1 + (rank // (2 * nq)) % max(nq - 1, 1)) % nq, -1)
    want_cross = (stratum == BAND) & ((rank // (2 * nq) + combo) % 2 == 0)
    far = (stratum == FAST) & (rank % 4 != 0)
    calm = np.where(far, rank % nq, -1)                              # the 60x group's joint that stays inside the velocity box
    q = np.zeros((n, nq), np.float32); qd = np.zeros((n, nq), np.float32); sp = np.zeros((n, nt), np.float32)
    todo = np.arange(n)
    fails = np.zeros(n, np.int64)
    for _round in range(max_rounds):
        m = len(todo)
        st, j, sd = stratum[todo], joint[todo], side[todo]
        rows = np.arange(m)
        tq = rng.uniform(0.9 * lo, 0.9 * hi, (m, nq))
        tv = rng.uniform(-vmax, vmax, (m, nq))
        ts = rng.uniform(-0.3, 0.3, (m, nt))
        u = rng.uniform(0.0, 1.0, (m, 4))
        jj = np.maximum(j, 0)
        limit_j, vmax_j = lim[(sd[rows] > 0).astype(int), jj], vmax[jj]
        # fast entries.  The 60x group leaves one joint per env inside the velocity box: every other joint comes out of the step
        # at +-qd_max whatever its acceleration was, this one carries the tendon forces of the evaluation at the entry speeds -
        # where, under Euler, fibres shorten faster than v_max (the f_V clamp at v = -1).  Its tendons all pull (set-points below
        # zero), and of FAST_CANDIDATES directions of the fast joints the one with most LOADED fibres (v < -1, activation > 0.1) is kept.
        k = st == FAST
        fr = far[todo]
        cj = np.maximum(calm[todo], 0)
        fc = fr & (calm[todo] >= 0)                                   # (an env that found no calm joint runs every joint fast)
        scale = np.where(fr, FAST_FAR, FAST_BOX)[:, None]
        mag = np.where(fr[:, None], rng.uniform(0.75, 1.0, (m, nq)), rng.uniform(0.0, 1.0, (m, nq)))
        tq[k] *= 0.5 / 0.9                                            # room for one step at the saturated speed
        ts[fr] = -rng.uniform(0.05, 0.3, (m, nt))[fr]
        calm_v = rng.uniform(-1.0, 1.0, m) * vmax[cj]
        most = np.full(m, -1)
        for c in range(FAST_CANDIDATES):
            sign = np.where(rng.uniform(size=(m, nq)) < 0.5, -1.0, 1.0)
            cv = sign * mag * scale * vmax
            cv[rows[fc], cj[fc]] = calm_v[fc]
            count = loaded_fibres(desc, tq, cv, ts, np.where(fc, cj, -1))
            better = k & ((count > most) | ~fr)
            most = np.where(better, count, most)
            tv[better] = cv[better]
        # beyond a limit: further than one env step travels, so that moving inward does not bring it back inside
        k = np.isin(st, (BEYOND_OUT, BEYOND_IN, TWO_JOINTS))
        depth_lo = np.maximum(0.06, step_size * vmax_j + 0.008)
        depth = depth_lo + u[:, 0] * (0.2 - depth_lo)
        outward = np.where(st == BEYOND_IN, -1.0, 1.0) * sd
        tq[rows[k], jj[k]] = (limit_j + sd * depth)[k]
        tv[rows[k], jj[k]] = (outward * (0.3 + 0.7 * u[:, 1]) * vmax_j)[k]
        k = st == TWO_JOINTS
        j2 = np.maximum(joint2[todo], 0)
        depth2_lo = np.maximum(0.06, step_size * vmax[j2] + 0.008)
        tq[rows[k], j2[k]] = (lim[(sd[rows] < 0).astype(int), j2] - sd * (depth2_lo + u[:, 2] * (0.2 - depth2_lo)))[k]
        # the band: velocity towards the limit; the start angle from the displacement the free oracle gives and a drawn
        # overshoot (crossing in the first substep) or shortfall (over the whole step)
        k = st == BAND
        if k.any():
            cross = want_cross[todo][k]
            bq, bv, bs = tq[k], tv[k], ts[k]
            bj, bsd, blim, bvm = jj[k], sd[k], limit_j[k], vmax_j[k]
            br = np.arange(len(bj))
            speed = np.where(cross, 0.3 + 0.7 * u[k, 1], (0.1 + 0.5 * u[k, 1]) / nsub)
            bv[br, bj] = bsd * speed * bvm
            over = np.where(cross, 1.0, -1.0) * (1e-3 + u[k, 0] * 0.25 * h * bvm)
            bq[br, bj] = blim - bsd * 0.5 * h * bvm
            # near most limits the muscles push back harder than the entry speed carries, near others they carry the joint the
            # whole way: of BAND_CANDIDATES draws of the other joints' state and the set-points (half of them from the corners
            # of the action box) keep the one that travels furthest towards the limit in the first substep (to cross), or whose
            # travel over the step comes nearest to half of what the band leaves (to stop short)
            best = np.full(len(bj), -np.inf)
            aim = 0.5 * (h * bvm - np.abs(over))
            for c in range(BAND_CANDIDATES):
                cq = rng.uniform(0.9 * lo, 0.9 * hi, bq.shape)
                cv = rng.uniform(-vmax, vmax, bq.shape)
                cs = rng.uniform(-0.3, 0.3, bs.shape)
                if c % 2:
                    cs = band_sp * np.sign(cs)
                cq[br, bj], cv[br, bj] = bq[br, bj], bv[br, bj]
                gain = _free_displacement(desc, cq, cv, cs, integ, h, 1)[br, bj] * bsd
                if nsub > 1 and not cross.all():
                    whole = _free_displacement(desc, cq, cv, cs, integ, h, nsub)[br, bj] * bsd
                    gain = np.where(cross, gain, whole)
                gain = np.where(cross, gain, -np.abs(gain - aim))
                better = gain > best
                best = np.where(better, gain, best)
                bq[better], bv[better], bs[better] = cq[better], cv[better], cs[better]
            for _ in range(4):
                d1 = _free_displacement(desc, bq, bv, bs, integ, h, 1)[br, bj]
                dn = _free_displacement(desc, bq, bv, bs, integ, h, nsub)[br, bj] if nsub > 1 else d1
                bq[br, bj] = blim + bsd * over - np.where(cross, d1, dn)
            # (where the muscles push a joint away from its limit whatever the draw, stopping short needs no solving)
            gap = (blim - bq[br, bj]) * bsd
            bq[br, bj] = np.where(cross | ((gap > 0) & (gap <= h * bvm)), bq[br, bj], blim - bsd * (0.1 + 0.8 * u[k, 2]) * h * bvm)
            tq[k], tv[k], ts[k] = bq, bv, bs
        tq, tv, ts = tq.astype(np.float32), tv.astype(np.float32), ts.astype(np.float32)
        _, v1, feas, margin = step_with_margin(desc, tq, tv, ts, integ, nsub, step_size)
        ok = decided(margin, tol(tq, tv, ts) if callable(tol) else tol)
        ok &= np.where(st == BEYOND_IN, v1[rows, jj] * sd < -0.1 * vmax_j, True)   # still moving inward after the step, clearly
        ok &= np.where(np.isin(st, (INTERIOR, FAST)), feas, True)
        ok &= np.where(fc, (np.abs(v1[rows, cj]) < CALM_BOX * vmax[cj]) & (loaded_fibres(desc, tq, tv, ts, cj) >= MIN_LOADED), True)
        ok &= np.where(np.isin(st, (BEYOND_OUT, BEYOND_IN, TWO_JOINTS)), ~feas, True)
        start = tq[rows, jj].astype(np.float64)
        in_band = (np.abs(start - limit_j) <= h * vmax_j) & ((start - limit_j) * sd < 0)
        ok &= np.where(st == BAND, (feas != want_cross[todo]) & in_band, True)
        q[todo[ok]], qd[todo[ok]], sp[todo[ok]] = tq[ok], tv[ok], ts[ok]
        todo = todo[~ok]
        if not len(todo):
            break
        fails[todo] += 1
        stuck = todo[(stratum[todo] == BAND) & (fails[todo] >= BAND_GIVE_UP)]
        want_cross[stuck] = False                                     # nothing carries this joint over this limit from inside: it stops short
        # (an idle joint - no mass, no tendon - that a substep clamps rests exactly on its limit in the next one: margin 0 whatever
        # the draw.  Such an env takes the next joint as its target.)
        stuck = todo[far[todo] & (fails[todo] % FAST_GIVE_UP == 0)]        # (a joint no tendon turns, or one the fast joints always saturate)
        calm[stuck] = np.where((fails[stuck] >= FAST_GIVE_UP * FAST_JOINTS_TRIED) | (calm[stuck] < 0), -1, (calm[stuck] + 1) % nq)
        stuck = todo[np.isin(stratum[todo], (BEYOND_OUT, BEYOND_IN, TWO_JOINTS)) & (fails[todo] % BAND_GIVE_UP == 0)]
        joint[stuck] = (joint[stuck] + 1) % nq
        joint2[stuck] = np.where(joint2[stuck] >= 0, (joint[stuck] + 1) % nq, -1)
    else:
        raise RuntimeError("edge_states: %d envs left undecided after %d rounds (strata %s)"
                           % (len(todo), max_rounds, sorted(set(STRATA[s] for s in stratum[todo]))))
    info = dict(stratum=stratum, joint=joint, side=side, joint2=joint2, want_cross=want_cross, far=far, calm=calm)
    return q, qd, sp, info


def far_group_tolerance(desc, q, qd, sp, info, integrator, nsub, tol):
    """The tolerance of the 60x group of the fast stratum: four times the distance of the fp32 C oracle from the fp64 one over that
    group on these inputs, and never below tol ([n, 1]) - at those speeds one acceleration evaluation is 3 600 times the usual
    Coriolis terms, and fp32 arithmetic of any order loses what the generic fp32 restatement loses."""
    from oracle.c_oracle import COracle
    far = info["far"]
    if not far.any():
        return tol
    integ = _integ(integrator)
    a = COracle(desc, "f64").step(q[far], qd[far], sp[far], integrator=integ, n_substeps=nsub)
    b = COracle(desc, "f32").step(q[far], qd[far], sp[far], integrator=integ, n_substeps=nsub)
    own = max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())
    out = tol.copy()
    out[far] = np.maximum(tol[far], 4.0 * own)
    return out


def check_against_oracle(desc, q, qd, sp, info, got, integrator, nsub, tol, label="", widen_far=False):
    """The full comparison of one kernel step (got = q1, qd1, f1) from edge states against step_with_margin: angles and
    velocities within tol (a number, [n, 1], or a function of the state; widen_far: the 60x group to far_group_tolerance, for
    the cases measured above tol there), flags equal on
    every env - all are decided -, every joint the last substep clamped sits on float32(limit) bit for bit with no outward
    velocity, and the beyond_in stratum keeps its inward velocity.  Returns (max |dq|, max |dqd|) after printing them."""
    q1, qd1, f1 = got
    qo, qdo, fo, margin, hit, jm, _ = step_with_margin(desc, q, qd, sp, integrator, nsub, detail=True)
    if callable(tol):
        tol = tol(q, qd, sp)
    tol = np.broadcast_to(np.asarray(tol, np.float64).reshape(-1, 1), (len(q), 1)).copy()
    dec = decided(margin, tol[:, 0])
    assert dec.all(), "%s: %d undecided envs" % (label, int(np.sum(~dec)))
    eq, eqd = np.abs(q1 - qo), np.abs(qd1 - qdo)
    far = info["far"]
    held = far_group_tolerance(desc, q, qd, sp, info, integrator, nsub, tol) if widen_far else tol
    print("%s: max |q - q64| %.3g, max |qd - qd64| %.3g (60x group: %.3g, %.3g, held to %.3g); %d of %d envs infeasible"
          % (label, eq.max(), eqd.max(), eq[far].max() if far.any() else 0.0, eqd[far].max() if far.any() else 0.0,
             held[far].min() if far.any() else 0.0, int(np.sum(~fo)), len(fo)))
    clamp_tol, tol = tol, held
    wrong = np.asarray(f1, bool) != fo
    assert not wrong.any(), "%s: %d wrong flags (%d oracle-infeasible envs called feasible), first envs %s" % (
        label, int(wrong.sum()), int(np.sum(wrong & ~fo)), np.nonzero(wrong)[0][:8])
    lim32 = np.where(hit > 0, desc.q_hi, desc.q_lo).astype(np.float32)
    clamped = hit != 0
    assert (jm[clamped] > DECIDED * np.broadcast_to(clamp_tol, jm.shape)[clamped]).all()
    assert np.array_equal(q1[clamped].view(np.uint32), lim32[clamped].view(np.uint32)), "%s: a clamped joint is not on its limit" % label
    assert np.all(qd1[clamped] * hit[clamped] <= 0), "%s: outward velocity kept at a limit" % label
    k = np.nonzero(info["stratum"] == BEYOND_IN)[0]
    j, sd = info["joint"][k], info["side"][k]
    assert np.all(qdo[k, j] * sd < -0.05 * desc.qd_max[j])            # (the oracle keeps an inward velocity far from zero there)
    assert np.all(qd1[k, j] * sd < 0), "%s: inward velocity dropped at a limit" % label
    # the tolerance last, so that a miss in the last digits does not hide what the flags and the clamp did
    worst = np.maximum(eq, eqd).max(axis=1) / tol[:, 0]
    over = np.nonzero(~(worst < 1.0))[0]
    assert not len(over), "%s: %d envs beyond the tolerance: %s" % (label, len(over), ", ".join(
        "env %d (%s) |dq| %.3g |dqd| %.3g tol %.3g" % (i, STRATA[info["stratum"][i]], eq[i].max(), eqd[i].max(), tol[i, 0]) for i in over[:6]))
    return eq.max(), eqd.max()


# ---- the inputs of tests/test_limit_edges_gpu.py, by name: tests/test_limit_edges_cpu.py qualifies every one of them ----
BALL_TOL = 2e-5                        # tests/test_physics_gpu.py, tests/test_random_robots_gpu.py (ball joints), tests/test_env_params_gpu.py
TREE_TOL = 2e-5                        # tests/test_tree_robot_gpu.py
N_BALL, N_TREE, N_TAIL, N_LARGE = 193, 257, 449, 65536 + 193
N_CHAIN = 385                          # 64 (joint, side) pairs in each of the six strata, and one env
SEED = 7
BALL_ROBOTS = ("msj", "kernarg_msj", "ball12", "turned")
TREE_ROBOTS = ("upper", "tree9", "chain32")
INPUTS = ([("msj", i, s, N_BALL) for i in ("euler", "rk4") for s in (1, 4)] + [("msj", i, 1, N_TAIL) for i in ("euler", "rk4")]
          + [("kernarg_msj", i, 1, n) for i in ("euler", "rk4") for n in (N_BALL, N_TAIL)]
          + [("ball12", i, 2, N_BALL) for i in ("euler", "rk4")] + [("turned", i, 1, N_BALL) for i in ("euler", "rk4")]
          + [("upper", i, s, N_TREE) for i in ("euler", "rk4") for s in (1, 2)]
          + [("tree9", "rk4", 1, N_TREE), ("chain32", "euler", 1, N_CHAIN)])
BAND_SP = {"ball12": 1.0}               # its joint 1 does not reach its lower limit from inside under set-points of the action box
_ROBOTS, _STATES = {}, {}


def robot_of(name):
    """(robot, description) of an input's robot, one object per name"""
    if name not in _ROBOTS:
        from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
        from random_robots import random_ball_joint_robot, random_tree_robot
        if name == "msj":
            robot = MsjRobot()
        elif name == "upper":
            robot = UpperBodyRobot()
        elif name == "kernarg_msj":
            from test_env_params_gpu import _kernarg_msj
            robot = _kernarg_msj()
        elif name == "turned":
            from test_mirror_pairs import _rotated_msj
            desc = _rotated_msj()

            class Turned(MsjRobot):
                @classmethod
                def get_description(cls):
                    return desc
            robot = Turned()
        elif name == "ball12":                                        # general inertia (seed 7 is not a principal-axis robot), 12 tendons
            robot = random_ball_joint_robot(7, 12)[0]
        elif name == "tree9":                                         # 18 joints in 4 parts: tests/test_random_robots_gpu.py builds its split forms
            robot = random_tree_robot(9)[0]
        elif name == "chain32":                                       # 32 levels: the deepest reduction of the one-wave form
            from test_random_robots_gpu import EXTREMES
            robot = random_tree_robot(100 + sorted(EXTREMES).index("chain32"), **EXTREMES["chain32"])[0]
        else:
            raise KeyError(name)
        _ROBOTS[name] = (robot, robot.get_description())
    return _ROBOTS[name]


def tol_of(name):
    """the tolerance the GPU files hold this robot's angles and velocities to: a number, or for the random trees the function of
    the state tests/test_random_robots_gpu.py uses"""
    if name in BALL_ROBOTS:
        return BALL_TOL
    if name == "upper":
        return TREE_TOL
    from test_random_robots_gpu import tolerance
    desc = robot_of(name)[1]
    return lambda q, qd, sp: tolerance(desc, q, qd, sp)


def states(name, integrator, nsub, n, seed=SEED):
    """edge_states of a named input, computed once per session and handed out read-only"""
    key = (name, integrator, nsub, n, seed)
    if key not in _STATES:
        q, qd, sp, info = edge_states(robot_of(name)[1], n, seed, integrator, nsub, tol_of(name), band_sp=BAND_SP.get(name, 0.3))
        for a in (q, qd, sp) + tuple(info.values()):
            a.setflags(write=False)
        _STATES[key] = (q, qd, sp, info)
    return _STATES[key]
