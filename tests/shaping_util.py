"""TEST HELPER for reward shaping (include/roboy_sim.h: rb_env_shaping_*; csrc/env_shaping.hpp): the float64 statement
of the cost, the tolerance of the fp32 kernels against it, and the twin-env runs that tests/test_reward_shaping_gpu.py shares."""
import numpy as np

TERMS = ("action_rate", "tension", "activation")


def weights_of(weights):
    """a dict with any of TERMS -> (w_r, w_f, w_a) as the library holds them: rounded to float32"""
    return tuple(float(np.float32(dict(weights or {}).get(k, 0.0))) for k in TERMS)


def terms64(desc, robot, q, qd, act, prev, first):
    """The three costs [3][n] in float64 at the states ``q, qd`` [n, n_q] under the action rows ``act`` [n, n_t]: built from
    oracle.physics_np.TendonRobotOracle the way tests/test_tendon_state_gpu.py builds its readout (``_oracle`` on the set-points of
    ``_env_rescale64``).  ``prev``: the previous step's action rows, raw or clamped (clamped here; None: zeros); ``first`` [n] bools:
    the env is in its episode's first step, where the rate term is 0."""
    from test_tendon_state_gpu import _env_rescale64, _oracle
    a = np.clip(np.asarray(act, np.float64), -1.0, 1.0)
    p = np.zeros_like(a) if prev is None else np.clip(np.asarray(prev, np.float64), -1.0, 1.0)
    rate = np.where(np.asarray(first, bool), 0.0, np.mean((a - p) ** 2, axis=1))
    ref, o, _ = _oracle(desc, q, qd, _env_rescale64(robot, act))
    tension = np.mean((ref["force"] / o.f_max) ** 2, axis=1)
    activation = np.mean(ref["activation"] ** 2, axis=1)
    return np.stack((rate, tension, activation)), ref, o


def cost64(desc, robot, q, qd, act, prev, first, weights):
    """cost[n] = w_r c_rate + w_f c_tension + w_a c_activation in float64"""
    t, _, _ = terms64(desc, robot, q, qd, act, prev, first)
    w = weights_of(weights)
    return w[0] * t[0] + w[1] * t[1] + w[2] * t[2]


def cost_tolerance(desc, robot, q, qd, act, prev, first, weights):
    """[n]: how far the fp32 cost may lie from cost64, from numbers the project already holds.  The readout's own tolerances
    (tests/test_tendon_state_gpu.py, imported): delta_force,k = FORCE_REL max(F_max) / F_max,k on F / F_max and delta_act =
    kp LEN_REL + 1e-6 on the activation.  A mean of squares moves by at most mean_k (2 |x_k| + delta_k) delta_k; the fp32 squares
    and the ordered sum add (n_t + 3) 2^-23 of the value.  The rate term has no reading in it: only that last part."""
    from test_tendon_state_gpu import FORCE_REL, LEN_REL
    t, ref, o = terms64(desc, robot, q, qd, act, prev, first)
    w = weights_of(weights)
    d_force = FORCE_REL * np.max(o.f_max) / o.f_max
    d_act = o.kp * LEN_REL + 1e-6
    x_force, x_act = np.abs(ref["force"]) / o.f_max, np.abs(ref["activation"])
    moved = (w[1] * np.mean((2.0 * x_force + d_force) * d_force, axis=1) + w[2] * np.mean((2.0 * x_act + d_act) * d_act, axis=1))
    value = w[0] * t[0] + w[1] * t[1] + w[2] * t[2]
    return moved + (desc.n_t + 3) * 2.0 ** -23 * value


def rate64(act, done):
    """c_rate [T, n] in float64 of a rollout's action rows ``act`` [T, n, n_t] and done flags ``done`` [T, n] that started behind a
    reset: 0 in step 0 and in the step behind a done one (auto-reset), else the mean squared change of the clamped rows."""
    a = np.clip(np.asarray(act, np.float64), -1.0, 1.0)
    out = np.zeros(a.shape[:2])
    out[1:] = np.mean((a[1:] - a[:-1]) ** 2, axis=2)
    out[1:][np.asarray(done, bool)[:-1]] = 0.0
    return out


# ---- twin runs: an env with shaping and one without, equal seed and actions ----
STEPS, MAX_LEN = 12, 5
ALL = {"action_rate": 0.1, "tension": 0.05, "activation": 0.02}


def robot_of(which):
    """(robot, desc, n) of the twin tests: two 256-groups with the second partial for the ball-joint class, 130 envs for joint trees"""
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    from random_robots import random_ball_joint_robot, random_tree_robot
    if which == "msj":
        r = MsjRobot()
        return r, r.get_description(), 300
    if which == "upper":
        r = UpperBodyRobot()
        return r, r.get_description(), 130
    if which.startswith("ball"):
        n_t = int(which[4:])
        r, d = random_ball_joint_robot(60 + n_t, n_t)
        return r, d, 300
    r, d = random_tree_robot(int(which[4:]))
    return r, d, 130


def _early_goals(make, desc, acts):
    """Goals [n, n_q] under which some envs' first episode ends on its SECOND step, where the rate term is live, and the envs [n]
    that do (possibly none).  A scout env finds them - the motion behind a reset does not depend on the goal: every env gets the pose
    it will be in after two steps for a goal; the scout then runs the two steps again under those goals and reports the envs that
    were done in the second step and not in the first (the others are there too early, or too fast for the goal test's velocity bound)."""
    scout = make()
    try:
        scout.reset()
        for t in range(2):
            scout.step(acts[t])
        goal = scout.sim.read_state()[0].copy()
        scout.reset()
        scout.set_goal(goal)
        done = [scout.step(acts[t])[2] for t in range(2)]
    finally:
        scout.close()
    return goal, done[1] & ~done[0]


def twin_run(which, integrator, kernel=None, weights=ALL, seed=3, steps=STEPS, plant=True, **kw):
    """STEPS steps of a shaped env and its plain twin under wide actions.  Returns a dict of per-step lists: ``act`` and, for both
    envs (``s_*`` shaped, ``p_*`` plain), ``obs, rew, done`` and the state ``q, qd`` after the step; ``cost``; and at the end
    ``stats`` / ``twin_stats`` (``stats()``) and ``shaping_stats``.  ``plant``: the action seed is the first of seed + 1 .. seed + 4
    under which ``_early_goals`` finds an env, and those goals are set in both envs."""
    from action_box_util import wide_actions
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, desc, n = robot_of(which)
    make = lambda **o: RoboyVecEnv(robot, n, seed=seed, integrator=integrator, max_episode_length=MAX_LEN, **kw, **o)
    acts, goal = wide_actions(n, desc.n_t, steps, seed + 1), None
    if plant:
        for action_seed in range(seed + 1, seed + 5):
            acts = wide_actions(n, desc.n_t, steps, action_seed)
            goal, early = _early_goals(make, desc, acts)
            if early.any():
                break
    shaped, plain = make(reward_shaping=weights), make()
    out = {k: [] for k in ("act", "cost", "s_obs", "s_rew", "s_done", "s_q", "s_qd", "p_obs", "p_rew", "p_done", "p_q", "p_qd")}
    try:
        for env in (shaped, plain):
            if kernel is not None:
                env.sim.select_kernel(kernel)
            env.reset()
            if goal is not None:
                env.set_goal(goal)
        out["kernel"] = (shaped.sim.info()["kernel"], plain.sim.info()["kernel"])
        for t in range(steps):
            out["act"].append(acts[t])
            for tag, env in (("s", shaped), ("p", plain)):
                obs, rew, done, _ = env.step(acts[t])
                q, qd = env.sim.read_state()[:2]
                for k, v in (("obs", obs), ("rew", rew), ("done", done), ("q", q), ("qd", qd)):
                    out["%s_%s" % (tag, k)].append(v)
            out["cost"].append(shaped.shaping_cost())
        out["stats"], out["twin_stats"] = shaped.stats(), plain.stats()
        out["shaping_stats"] = shaped.shaping_stats()
    finally:
        shaped.close(); plain.close()
    return out
