"""The reference's own env-layer vectors (tests/golden/env_layer.json) through EVERY env-step row of the dispatch table that a
parked robot can reach, pinned by row id, and through the per-env-parameter env kernels (csrc/env_params.hpp).

tests/test_env_golden_gpu.py explains the parking construction and runs the rows by form on the 8-tendon robot under Euler.
Here the same rows run under both integrators on every ball-joint env row (8 tendons: parked_robot, its y-z-mirror twin for the
lane-pair form's variant 1; 5 tendons: parked_ball_robot(5)) and on every joint-tree env row (parked_tree_robot: a three-root
forest, which the split forms cut into one part per joint).  A row that ends an episode is also checked for the goal the kernel
draws next, bit for bit against oracle/philox_np.goals.

tests/test_dispatch_table.py fails if an env-step row of the table is neither in GOLDEN_ENV_ROWS nor in EXEMPT, or if a
per-env-parameter env-step instance of the library is neither in GOLDEN_PARAM_INSTANCES nor in PARAM_EXEMPT.

Cost: the joint limits are literals of the hiprtc-built kernels (jit rows), so every infeasible row's robot is a build of its
own there; the jit rows run JIT_INFEASIBLE_PER_JOINT infeasible rows per joint under Euler only (RK4 is covered by the feasible
rows, whose robot is one build).
"""
import numpy as np
import pytest

from gym_roboy_amd import _native as nat
from oracle import philox_np as ph
from test_env_golden_gpu import _fixture, _margin, limits_hitting, parked_ball_robot, parked_robot, parked_tree_robot, pre_state

GOLDEN_ENV_ROWS = (
    "ball8/env_step/env_per_lane/euler/b64/kernarg/v0",
    "ball8/env_step/env_per_lane/rk4/b64/kernarg/v0",
    "ball8/env_step/env_per_lane/euler/b256/kernarg/v0",
    "ball8/env_step/env_per_lane/rk4/b256/kernarg/v0",
    "ball8/env_step/env_per_lane/euler/b256/jit/v0",
    "ball8/env_step/env_per_lane/rk4/b256/jit/v0",
    "ball8/env_step/tendon_per_lane/euler/b64/kernarg/v0",
    "ball8/env_step/tendon_per_lane/rk4/b64/kernarg/v0",
    "ball8/env_step/lane_pair/euler/b64/kernarg/v0",
    "ball8/env_step/lane_pair/euler/b64/kernarg/v1",
    "ball8/env_step/lane_pair/rk4/b64/kernarg/v0",
    "ball8/env_step/lane_pair/rk4/b64/kernarg/v1",
    "ball8/env_step/lane_pair/euler/b256/kernarg/v0",
    "ball8/env_step/lane_pair/euler/b256/kernarg/v1",
    "ball8/env_step/lane_pair/rk4/b256/kernarg/v0",
    "ball8/env_step/lane_pair/rk4/b256/kernarg/v1",
    "ballx/env_step/env_per_lane/euler/b64/kernarg/v0",
    "ballx/env_step/env_per_lane/rk4/b64/kernarg/v0",
    "ballx/env_step/env_per_lane/euler/b256/kernarg/v0",
    "ballx/env_step/env_per_lane/rk4/b256/kernarg/v0",
    "tree/env_step/env_per_wave/euler/b0/kernarg/v1",
    "tree/env_step/env_per_wave/rk4/b0/kernarg/v1",
    "tree/env_step/env_per_lane/euler/b64/jit/v0",
    "tree/env_step/env_per_lane/rk4/b64/jit/v0",
    "tree/env_step/env_per_lane_split/euler/b0/jit/v0",
    "tree/env_step/env_per_lane_split/rk4/b0/jit/v0",
    "tree/env_step/env_per_lane_split2/euler/b0/jit/v0",
    "tree/env_step/env_per_lane_split2/rk4/b0/jit/v0",
)
NOT_PARKABLE = "table constants (baked MsjRobot / upper body: not parkable)"
NO_WIDE_LEVEL = "octet variant a 3-joint robot cannot reach"
EXEMPT = dict(
    [(r, NOT_PARKABLE) for r in (
        "ball8/env_step/env_per_lane/euler/b64/table/v0",
        "ball8/env_step/env_per_lane/rk4/b64/table/v0",
        "ball8/env_step/env_per_lane/euler/b256/table/v0",
        "ball8/env_step/env_per_lane/rk4/b256/table/v0",
        "ball8/env_step/lane_pair/euler/b64/table/v0",
        "ball8/env_step/lane_pair/rk4/b64/table/v0",
        "ball8/env_step/lane_pair/euler/b256/table/v0",
        "ball8/env_step/lane_pair/rk4/b256/table/v0",
        "tree/env_step/env_per_lane/euler/b64/table/v0",
        "tree/env_step/env_per_lane/rk4/b64/table/v0",
        "tree/env_step/env_per_lane_split/euler/b0/table/v0",
        "tree/env_step/env_per_lane_split/rk4/b0/table/v0",
        "tree/env_step/env_per_lane_split2/euler/b0/table/v0",
        "tree/env_step/env_per_lane_split2/rk4/b0/table/v0")]
    # variant 0 = tables without single-pass levels: a level wider than 4 joints (csrc/tree_build.hpp, chain_ok)
    + [(r, NO_WIDE_LEVEL) for r in ("tree/env_step/env_per_wave/euler/b0/kernarg/v0", "tree/env_step/env_per_wave/rk4/b0/kernarg/v0")])

# the per-env-parameter env kernels (not rows: dispatch() refuses while parameters are enabled), by short kernel name
GOLDEN_PARAM_INSTANCES = {
    "rbp::msj_params_env_step<0, 256, rb::MsjConst<float, 8>, false>": ("const8", "euler"),
    "rbp::msj_params_env_step<1, 256, rb::MsjConst<float, 8>, false>": ("const8", "rk4"),
    "rbp::msj_params_env_step<0, 256, rb::MsjConst<float, 16>, false>": ("constx", "euler"),
    "rbp::msj_params_env_step<1, 256, rb::MsjConst<float, 16>, false>": ("constx", "rk4"),
}
PARAM_EXEMPT = {
    "rbp::msj_params_env_step<0, 256, rb::MsjConst<float, 8>, true>": "baked MsjRobot constants: MsjRobot itself, not parkable",
    "rbp::msj_params_env_step<1, 256, rb::MsjConst<float, 8>, true>": "baked MsjRobot constants: MsjRobot itself, not parkable",
}

FORM_OF = {name: k for k, name in nat.KERNEL_NAMES.items()}
LARGE = 66560                      # envs: the 256-thread side of every block-size switch (rb_launch_thresholds: 65 536)
# the parts of parked_tree_robot's joints in the split forms (checked against the generator by test_env_golden_gpu.py)
SPLIT_PART_OF_JOINT = {"env_per_lane_split": (0, 1, 2), "env_per_lane_split2": (0, 1, 0)}
JIT_INFEASIBLE_PER_JOINT = 3
# the lane-pair form's mirror plane (variant 0: x-z, 1: y-z) maps the angle of the joint turning about its normal (y: joint 1,
# x: joint 0) onto itself and negates the other two: a one-sided limit on any other joint has no mirror image
MIRROR_KEEPS_JOINT = {0: 1, 1: 0}
FLAGS = [(False, False), (False, True), (True, False), (True, True)]


def parse(row_id):
    cls, entry, form, integ, block, consts, variant = row_id.split("/")
    assert entry == "env_step"
    return dict(cls=cls, form=form, kernel=FORM_OF[form], integ=integ, block=int(block[1:]), consts=consts, variant=int(variant[1:]))


def robot_for(row_id, limits=None):
    r = parse(row_id)
    if r["cls"] == "ball8":
        return parked_robot(limits, turned=r["variant"] == 1)
    if r["cls"] == "ballx":
        return parked_ball_robot(5, limits)
    return parked_tree_robot(limits)


def copies_for(row_id, k):
    """Copies of k rows that make a batch of the row's block size: at least LARGE envs for the 256-thread rows."""
    return -(-LARGE // k) if parse(row_id)["block"] == 256 else 1


def open_row(row_id, robot, n, monkeypatch, seed=3, pen=False, bonus=True):
    """A RoboyVecEnv whose next env step takes the row row_id (asserted); raises nat.NativeError where the library refuses the
    row's form for this robot."""
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    r = parse(row_id)
    if r["cls"] == "ball8" and r["kernel"] == 1 and r["block"] == 256:
        monkeypatch.setenv("ROBOY_SIM_JIT", "1" if r["consts"] == "jit" else "0")
    vec = RoboyVecEnv(robot, n, seed=seed, joint_vel_penalty=pen, is_agent_getting_bonus_for_reaching_goal=bonus,
                      auto_reset=False, integrator=r["integ"])
    try:
        vec.sim.select_kernel(r["kernel"])
        got = vec.sim.dispatch("env_step")["id"]
    except nat.NativeError:
        vec.close()
        raise
    assert got == row_id
    return vec


def tile(a, copies):
    a = np.asarray(a)
    return np.tile(a, (copies,) + (1,) * (a.ndim - 1))


def check_goal_redraw(vec, seed, done, goal_before, goal_after):
    """The goal in effect during the next step: where the step returned done (auto_reset off), draw 2 of the env's goal stream
    (draw 0 was rb_env_configure's reset, draw 1 reset()'s) in the description's joint box, bit for bit; elsewhere the goal it
    had."""
    desc = vec.robot.get_description()
    ids = np.nonzero(done)[0]
    want = ph.goals(seed, ids, 2, desc.q_lo, desc.q_hi)
    assert np.array_equal(goal_after[done], want), (goal_after[done][:4], want[:4])
    assert np.array_equal(goal_after[~done], goal_before[~done])


def run_rows(vec, seed, q, qd, goal, step_num, actions=None, q_start=None):
    """One step from the parked pre-state of (q, qd) (or from q_start: limits_hitting's, beyond the joint limit) under goal /
    step counter, then one more; checks the goal drawn where the first step returned done, returns that step's (obs, reward,
    done, feasible)."""
    n = vec.num_envs
    vec.reset()
    q_pre, qd32 = pre_state(q, qd)
    if q_start is not None:
        q_pre = np.asarray(q_start, np.float32)
    vec.sim.set_state(q_pre, qd32)
    vec.set_goal(goal, step_num=np.asarray(step_num, np.uint32))
    a = np.zeros((n, vec.n_t), np.float32) if actions is None else actions
    obs, rew, done, _ = vec.step(a)
    _, _, feas = vec.sim.read_state()
    obs2, _, _, _ = vec.step(np.zeros((n, vec.n_t), np.float32))
    nq = vec.n_q
    check_goal_redraw(vec, seed, done, obs[:, 2 * nq:], obs2[:, 2 * nq:])
    return obs, rew, done, feas


def infeasible_cases(fx, joints=(0, 1, 2), per_joint=None):
    """(case, limits_hitting result) of the recorded infeasible rows: every row some joint of which can be clamped (per_joint
    None), or the first per_joint rows whose joint j can be (0: all of them), for each j in joints."""
    rows = [c for c in fx["reward_cases"] if not c["feasible"]]
    assert len(rows) == 40
    if per_joint is None:
        return [(c, h) for c, h in ((c, limits_hitting(c["q"], c["qd"])) for c in rows) if h is not None]
    out = []
    for j in joints:
        hits = [(c, h) for c, h in ((c, limits_hitting(c["q"], c["qd"], j)) for c in rows) if h is not None]
        assert len(hits) >= per_joint, j
        out += hits[:per_joint or None]
    return out


def _ids(rows):
    return [r.replace("/env_step/", "/").replace("/", "-") for r in rows]


# ---------------------------------------------------------------------------------------------------- rows of the table
@pytest.mark.gpu
@pytest.mark.parametrize("row_id", GOLDEN_ENV_ROWS, ids=_ids(GOLDEN_ENV_ROWS))
@pytest.mark.parametrize("pen,bonus", FLAGS)
def test_feasible_reward_cases(row_id, pen, bonus, monkeypatch):
    fx = _fixture()
    key = "pen%d_bonus%d" % (pen, bonus)
    feasible = [c for c in fx["reward_cases"] if c["feasible"]]
    assert len(feasible) == 40
    copies = copies_for(row_id, 40)
    q = tile([c["q"] for c in feasible], copies); qd = tile([c["qd"] for c in feasible], copies)
    goal = tile([c["goal_q"] for c in feasible], copies)
    want_r = tile([c["reward"][key] for c in feasible], copies)
    want_reached = tile([c["reached"] for c in feasible], copies)
    n = 40 * copies
    vec = open_row(row_id, robot_for(row_id), n, monkeypatch, seed=3, pen=pen, bonus=bonus)
    obs, rew, done, feas = run_rows(vec, 3, q, qd, goal, np.full(n, 7))
    assert feas.all()
    assert np.abs(obs[:, 0:3] - q.astype(np.float32)).max() < 5e-7
    assert np.abs(obs[:, 3:6] - qd.astype(np.float32)).max() < 1e-9
    assert np.array_equal(obs[:, 6:9], goal.astype(np.float32))
    np.testing.assert_allclose(rew, want_r, rtol=2e-5, atol=2e-4)
    clear = _margin(fx, q, qd, goal) > 1e-5
    assert clear.sum() >= 30 * copies and want_reached[clear].any() and (~want_reached[clear]).any()
    assert np.array_equal(done[clear], want_reached[clear])
    assert done.any()                                     # the goal-reached branch and its redraw ran
    assert vec.sim.dispatch("env_step")["id"] == row_id
    vec.close()


def _infeasible_plan(row_id):
    r = parse(row_id)
    fx = _fixture()
    if r["kernel"] == 5:
        # every row whose mirror-kept joint can be clamped, and the first three rows clamped on another joint (refused)
        keep = MIRROR_KEEPS_JOINT[r["variant"]]
        return (infeasible_cases(fx, joints=(keep,), per_joint=0) +
                [(c, h) for c, h in infeasible_cases(fx) if h[3] != keep][:3])
    if r["consts"] == "jit":
        return infeasible_cases(fx, per_joint=JIT_INFEASIBLE_PER_JOINT)
    return infeasible_cases(fx)


INFEASIBLE_ROWS = [r for r in GOLDEN_ENV_ROWS if parse(r)["consts"] != "jit" or parse(r)["integ"] == "euler"]


@pytest.mark.gpu
@pytest.mark.parametrize("row_id", INFEASIBLE_ROWS, ids=_ids(INFEASIBLE_ROWS))
def test_infeasible_reward_cases(row_id, monkeypatch):
    """The joint limit at the recorded angle: the step clamps onto it and the accountant subtracts the boundary penalty.  Split
    forms: every part's feasibility flag reaches the accountant wave from at least JIT_INFEASIBLE_PER_JOINT rows."""
    fx = _fixture()
    r = parse(row_id)
    copies = n = copies_for(row_id, 1)
    cases = _infeasible_plan(row_id)
    assert len(cases) >= (3 * JIT_INFEASIBLE_PER_JOINT if r["consts"] == "jit" else 11 if r["kernel"] == 5 else 30)
    ran, refused, checked_done = [], 0, 0
    for c, (lim, q_pre, qd32, j) in cases:
        robot = robot_for(row_id, lim)
        goal = tile([c["goal_q"]], copies)
        for pen, bonus in FLAGS:
            try:
                vec = open_row(row_id, robot, n, monkeypatch, seed=1, pen=pen, bonus=bonus)
            except nat.NativeError:
                # the lane-pair form needs a mirror plane, and a one-sided limit breaks it unless the plane keeps the joint
                assert r["kernel"] == 5 and j != MIRROR_KEEPS_JOINT[r["variant"]], (c["q"], j)
                refused += 1
                continue
            assert not (r["kernel"] == 5 and j != MIRROR_KEEPS_JOINT[r["variant"]])
            q = tile([c["q"]], copies)
            obs, rew, done, feas = run_rows(vec, 1, q, tile([c["qd"]], copies), goal, np.full(n, 3), q_start=tile([q_pre], copies))
            assert not feas.any()
            assert np.all(obs[:, j] == np.float32(c["q"][j]))                         # clamped onto the limit
            assert np.abs(obs[:, 0:3] - q.astype(np.float32)).max() < 5e-7
            assert np.abs(obs[:, 3:6] - qd32).max() < 1e-9
            np.testing.assert_allclose(rew, np.full(n, c["reward"]["pen%d_bonus%d" % (pen, bonus)]), rtol=2e-5, atol=2e-4)
            if _margin(fx, c["q"], c["qd"], np.asarray(c["goal_q"])) > 1e-5:
                assert np.all(done == c["reached"])
                checked_done += 1
            vec.close()
            ran.append(j)
    if r["kernel"] == 5:
        assert refused == 4 * 3 and len(ran) >= 4 * 8 and set(ran) == {MIRROR_KEEPS_JOINT[r["variant"]]}
    else:
        assert refused == 0 and checked_done >= 2 * len(cases)
    if r["form"] in SPLIT_PART_OF_JOINT:
        part = SPLIT_PART_OF_JOINT[r["form"]]
        per_part = np.bincount([part[j] for j in ran], minlength=max(part) + 1) // 4
        assert per_part.min() >= JIT_INFEASIBLE_PER_JOINT, per_part


@pytest.mark.gpu
@pytest.mark.parametrize("row_id", GOLDEN_ENV_ROWS, ids=_ids(GOLDEN_ENV_ROWS))
def test_scripted_episode(row_id, monkeypatch):
    """The 12-step episode recorded from the reference (no velocity penalty, bonus on): every step's (state, goal, step counter)
    replayed as one env of a batch; the goal after each step that ended the episode is the kernel's next draw."""
    fx = _fixture()
    ep = fx["episode"]
    steps, script = ep["steps"], ep["script"]
    r = parse(row_id)
    feas_idx = [t for t in range(len(steps)) if script[t][2]]
    infeas_idx = [t for t in range(len(steps)) if not script[t][2]]
    assert len(infeas_idx) >= 2 and any(steps[t]["done"] for t in feas_idx)

    def check(rows, obs, rew, done):
        for k, t in enumerate(rows):
            want = np.asarray(steps[t]["obs"])
            assert np.abs(obs[k] - want.astype(np.float32)).max() < 5e-7
            np.testing.assert_allclose(rew[k], steps[t]["reward"], rtol=2e-5, atol=2e-4)
            assert bool(done[k]) == steps[t]["done"]

    rows = feas_idx * copies_for(row_id, len(feas_idx))
    n = len(rows)
    vec = open_row(row_id, robot_for(row_id), n, monkeypatch, seed=2)
    obs, rew, done, _ = run_rows(vec, 2, [script[t][0] for t in rows], [script[t][1] for t in rows],
                                 [steps[t]["obs"][6:9] for t in rows], [steps[t]["step_num"] - 1 for t in rows],
                                 np.asarray([ep["actions"][t] for t in rows], np.float32)[:, :vec.n_t])
    check(rows, obs, rew, done)
    vec.close()
    replayed = refused = 0
    for t in infeas_idx:
        case = limits_hitting(script[t][0], script[t][1])
        if case is None:
            continue
        lim, q_pre, _, j = case
        try:
            copies = copies_for(row_id, 1)
            vec = open_row(row_id, robot_for(row_id, lim), copies, monkeypatch, seed=2)
        except nat.NativeError:
            assert r["kernel"] == 5 and j != MIRROR_KEEPS_JOINT[r["variant"]]
            refused += 1
            continue
        rows = [t] * copies
        obs, rew, done, feas = run_rows(vec, 2, [script[t][0]] * copies, [script[t][1]] * copies, [steps[t]["obs"][6:9]] * copies,
                                        [steps[t]["step_num"] - 1] * copies,
                                        np.asarray([ep["actions"][t]] * copies, np.float32)[:, :vec.n_t], q_start=[q_pre] * copies)
        assert not feas.any()
        check(rows, obs, rew, done)
        vec.close()
        replayed += 1
    assert replayed + refused >= 1 and (replayed >= 1 or r["kernel"] == 5)


@pytest.mark.gpu
@pytest.mark.parametrize("row_id", GOLDEN_ENV_ROWS, ids=_ids(GOLDEN_ENV_ROWS))
def test_episode_length(row_id, monkeypatch):
    """done when step_num > 400 (fixture 'episode_length', recorded from the reference); the goal drawn on that done."""
    fx = _fixture()["episode_length"]
    copies = copies_for(row_id, 3)
    n = 3 * copies
    vec = open_row(row_id, robot_for(row_id), n, monkeypatch, seed=4)
    far = np.full((n, 3), 1.5)
    q = np.full((n, 3), 0.1)
    _, _, done, _ = run_rows(vec, 4, q, np.zeros((n, 3)), far, tile([398, 399, 400], copies))
    assert list(done) == [False, fx["done_at_399_plus_1"], fx["done_at_400_plus_1"]] * copies
    vec.close()


# ---------------------------------------------------------------------------------------- per-env-parameter env kernels
PARAM_CASES = sorted(set(GOLDEN_PARAM_INSTANCES.values()))


def _param_vec(kind, integ, planes, n, seed, pen, bonus, limits=None):
    from env_params_util import random_params
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = parked_robot(limits) if kind == "const8" else parked_ball_robot(5, limits)
    vec = RoboyVecEnv(robot, n, seed=seed, joint_vel_penalty=pen, is_agent_getting_bonus_for_reaching_goal=bonus,
                      auto_reset=False, integrator=integ)
    vec.sim.enable_params()
    with pytest.raises(nat.NativeError, match="per-env parameters are enabled"):
        vec.sim.dispatch("env_step")                      # the parameter path is the one the next env step takes
    if planes == "random":
        pars = random_params(np.random.default_rng(n + seed), vec.n_t, n)
        d_p, _ = vec.sim.params_ptr()
        vec.sim.upload(d_p, np.ascontiguousarray(pars.T, dtype=np.float32))
        assert np.array_equal(vec.sim.get_param_planes(), pars.T.astype(np.float32))
    return vec


@pytest.mark.gpu
@pytest.mark.parametrize("kind,integ", PARAM_CASES)
@pytest.mark.parametrize("planes", ["nominal", "random"])
def test_param_kernels_on_the_reward_cases(kind, integ, planes):
    """Parked physics ignores every parameter (muscles of 1e-6 N, no damping, no gravity), so the recorded rows hold under any
    planes: the parameter kernels' env accounting (rbk::env_account with the parameter redraw hook) against the reference."""
    fx = _fixture()
    feasible = [c for c in fx["reward_cases"] if c["feasible"]]
    q = np.array([c["q"] for c in feasible]); qd = np.array([c["qd"] for c in feasible])
    goal = np.array([c["goal_q"] for c in feasible])
    n = len(feasible)
    clear = _margin(fx, q, qd, goal) > 1e-5
    for pen, bonus in FLAGS:
        key = "pen%d_bonus%d" % (pen, bonus)
        vec = _param_vec(kind, integ, planes, n, 3, pen, bonus)
        obs, rew, done, feas = run_rows(vec, 3, q, qd, goal, np.full(n, 7))
        assert feas.all()
        assert np.abs(obs[:, 0:3] - q.astype(np.float32)).max() < 5e-7
        assert np.abs(obs[:, 3:6] - qd.astype(np.float32)).max() < 1e-9
        np.testing.assert_allclose(rew, [c["reward"][key] for c in feasible], rtol=2e-5, atol=2e-4)
        assert np.array_equal(done[clear], np.array([c["reached"] for c in feasible])[clear]) and done.any()
        vec.close()
    covered = 0
    for c, (lim, q_pre, qd32, j) in infeasible_cases(fx):
        for pen, bonus in FLAGS:
            vec = _param_vec(kind, integ, planes, 1, 1, pen, bonus, lim)
            obs, rew, done, feas = run_rows(vec, 1, [c["q"]], [c["qd"]], [c["goal_q"]], [3], q_start=[q_pre])
            assert not feas[0] and obs[0, j] == np.float32(c["q"][j])
            assert np.abs(obs[0, 0:3] - np.asarray(c["q"], np.float32)).max() < 5e-7
            np.testing.assert_allclose(rew[0], c["reward"]["pen%d_bonus%d" % (pen, bonus)], rtol=2e-5, atol=2e-4)
            if _margin(fx, c["q"], c["qd"], np.asarray(c["goal_q"])) > 1e-5:
                assert bool(done[0]) == c["reached"]
            vec.close()
        covered += 1
    assert covered >= 30
