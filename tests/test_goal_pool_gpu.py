"""Goal pool on the GPU (include/roboy_sim.h: rb_env_goal_pool_*; csrc/env_goal.hpp; envs/goals.py): every goal an env
with a pool draws - at construction, at a reset, behind every episode end, in every kernel form of both robot classes and under every
extension - is row k(seed, global env id, draw) of the pool bit for bit (tests/goal_pool_util.py restates k), while the physics, the
counters and the neighbours' outputs are those of a twin env without a pool; then the single-env client, graphs, refusals, and
reachable_goals against the fp64 C oracle and end to end.

Envs of 300 (a partial wave, a second block of the trailing kernel) and 512; max_episode_length = 3, so every env ends an episode at
every third step.  The twins' comparison needs that no env REACHES a goal (it would reset in one twin only): asserted in every test
that compares twins; the seeds below are ones for which it holds."""
import ctypes

import numpy as np
import pytest

import goal_pool_util as gp
from gym_roboy_amd import _native as nat
from test_env_golden_gpu import pin_form
from test_env_params_gpu import _ball12, _kernarg_msj, _msj
from test_tree_robot_gpu import LANE, OCTET, SPLIT, SPLIT2

pytestmark = pytest.mark.gpu

MAX_LEN, STEPS, N_TREE = 3, 7, 130
N_LARGE = 66819                       # the 256-thread side of the block-size switch (rb_launch_thresholds: 65 536), where the hiprtc rows are
SEED = 4                              # no env of any twin below reaches a goal with it (asserted where twins are compared)
SIGMA = {"q": 0.01, "qd": 0.05}
RANGES = dict(force_scale=(0.7, 1.3), setpoint_offset=(-0.02, 0.02), mass_scale=(0.6, 1.6), damping_scale=(0.5, 2.0))


def _vec(robot, n, goals, seed=5, integ="euler", auto_reset=True, offset=0, **kw):
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    if kw.get("randomization") is True:
        kw["randomization"] = ParamRanges(**RANGES)
    return RoboyVecEnv(robot, n, seed=seed, integrator=integ, max_episode_length=MAX_LEN, auto_reset=auto_reset,
                       env_id_offset=offset, goals=goals, **kw)


def _actions(robot, n, seed, steps=STEPS):
    return np.random.default_rng(seed).uniform(-1, 1, (steps, n, robot.get_action_space().shape[0])).astype(np.float32)


def _twins(robot, n, seed=SEED, prepare=None, check=None, twin=True, **kw):
    """An env with a pool of 7 rows and its twin without, reset and stepped STEPS times with the same actions.  The pool env's goals
    follow the rule and the twin's the box draws (gp.Follower asserts both at every row of every step); done words, q, qd and the
    feasibility flag of the two are bit-identical at every step; nobody reached a goal.  prepare(env): what to do to each env behind
    its construction (select a kernel form); check(t, pool env, twin, follower): further assertions per step (t = -1: behind the reset).
    twin=False: the pool env alone, its goals against the rule (a batch so large that some env of a twin always reaches a box goal).
    Returns the two envs' statistics."""
    pool = gp.small_pool(robot.get_description())
    acts = _actions(robot, n, seed)
    envs = []
    try:
        for goals in (pool, None) if twin else (pool,):
            envs.append(_vec(robot, n, goals, seed=seed, **kw))
            if prepare:
                prepare(envs[-1])
        a = envs[0]
        assert np.array_equal(a.goal_pool(), pool)
        if not twin:
            f = gp.Follower(a, pool, seed, kw.get("offset", 0), kw.get("auto_reset", True))
            f.reset()
            n_done = sum(f.step(act)[2] for act in acts)
            assert n_done.min() >= 2
            return a.stats(), None
        b = envs[1]
        fa = gp.Follower(a, pool, seed, kw.get("offset", 0), kw.get("auto_reset", True))
        fb = gp.Follower(b, None, seed, kw.get("offset", 0), kw.get("auto_reset", True))
        fa.reset(), fb.reset()
        if check:
            check(-1, a, b, fa)
        n_done = np.zeros(n, int)
        for t in range(STEPS):
            _, _, da = fa.step(acts[t])
            _, _, db = fb.step(acts[t])
            assert np.array_equal(da, db), t
            for name, x, y in zip(("q", "qd", "feasible"), a.sim.read_state(), b.sim.read_state()):
                assert np.array_equal(x, y), (t, name)
            n_done += da
            if check:
                check(t, a, b, fa)
        sa, sb = a.stats(), b.stats()
        assert sa["n_goal_reached"] == 0 and sb["n_goal_reached"] == 0, "precondition: seed %d lets an env reach a goal" % seed
        assert n_done.min() >= 2                                   # two episode ends per env: counters as the model has them
        assert np.array_equal(fa.count, fb.count)
        for key in ("n_episodes", "sum_length", "n_goal_reached", "n_infeasible_steps", "n_env_steps"):
            assert sa[key] == sb[key], key
        return sa, sb
    finally:
        for env in envs:
            env.close()


# ---- 1. construction and reset ----
@pytest.mark.parametrize("offset", [0, 1000])
def test_construction_and_reset_draw_pool_rows(offset):
    """Behind construction every env's goal plane holds pool[k(gid, 0)] (read through the critic's state block, which copies the plane);
    behind reset() the plane and the observation's goal columns hold pool[k(gid, 1)]; env_id_offset shifts gid."""
    robot, n, seed = _msj(), 300, 5
    pool = gp.small_pool(robot.get_description())
    env = _vec(robot, n, pool, seed=seed, offset=offset, critic_obs=("state",))
    try:
        gids = offset + np.arange(n)
        k0 = gp.pool_row(seed, gids, 0, 7)
        assert np.array_equal(env.critic_obs()[:, 6:9], pool[k0])
        assert len(np.unique(k0)) == 7
        obs = env.reset()
        k1 = gp.pool_row(seed, gids, 1, 7)
        assert np.array_equal(obs[:, 6:9], pool[k1]) and np.array_equal(env.critic_obs()[:, 6:9], pool[k1])
        assert not obs[:, :6].any() and not np.array_equal(k0, k1)
        if offset:
            assert not np.array_equal(k1, gp.pool_row(seed, np.arange(n), 1, 7))
    finally:
        env.close()


def test_reset_on_a_joint_tree_writes_rows_of_twenty_joints():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    robot, seed = UpperBodyRobot(), 5
    desc = robot.get_description()
    pool = gp.small_pool(desc)
    env = _vec(robot, N_TREE, pool, seed=seed)
    try:
        f = gp.Follower(env, pool, seed)
        obs = f.reset()
        assert obs.shape == (N_TREE, 3 * desc.n_q) and not obs[:, :2 * desc.n_q].any()
    finally:
        env.close()


# ---- 2. episode ends ----
@pytest.mark.parametrize("n,auto_reset", [(512, True), (300, False)])
def test_episode_ends_draw_pool_rows_and_physics_is_the_twins(n, auto_reset):
    _twins(_msj(), n, auto_reset=auto_reset)


# ---- 3. every form by name ----
def _pin(kernel, *parts):
    def prepare(env):
        row = pin_form(env, kernel)
        assert all(p in row["id"] for p in parts), row["id"]
    return prepare


def _tree_form(kernel):
    def prepare(env):
        env.sim.select_kernel(kernel)
        assert env.sim.info()["kernel"] == kernel
    return prepare


def _upper():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    return UpperBodyRobot()


FORMS = {
    "msj-k1-table": dict(robot=_msj, n=300, prepare=_pin(1, "ball8/", "/table/")),
    "msj-k2": dict(robot=_msj, n=300, prepare=_pin(2)),
    "msj-k5": dict(robot=_msj, n=300, prepare=_pin(5), integ="rk4"),
    "ball12-k1": dict(robot=_ball12, n=300, prepare=_pin(1, "ballx/")),
    "kernarg-k1": dict(robot=_kernarg_msj, n=300, prepare=_pin(1, "ball8/", "/kernarg/"), jit="0"),
    "hiprtc-k1": dict(robot=_kernarg_msj, n=N_LARGE, prepare=_pin(1, "ball8/", "/b256/jit/"), jit="1", twin=False),
    "randomization": dict(robot=_msj, n=300, kw=dict(randomization=True)),
    "tendon_obs": dict(robot=_msj, n=300, kw=dict(tendon_obs=("length", "force")), obs_dim=25),
    "noise+delay": dict(robot=_msj, n=300, kw=dict(sensor_noise=SIGMA, action_delay=(0, 3))),
    "action_obs": dict(robot=_msj, n=300, kw=dict(action_obs=3), obs_dim=33),
    "all-together": dict(robot=_msj, n=300, integ="rk4", obs_dim=49,
                         kw=dict(randomization=True, tendon_obs=("length", "force"), sensor_noise=SIGMA, action_delay=(0, 3), action_obs=3)),
    "upper-lane": dict(robot=_upper, n=N_TREE, prepare=_tree_form(LANE)),
    "upper-octet": dict(robot=_upper, n=N_TREE, prepare=_tree_form(OCTET)),
    "upper-split": dict(robot=_upper, n=N_TREE, prepare=_tree_form(SPLIT)),
    "upper-split2": dict(robot=_upper, n=N_TREE, prepare=_tree_form(SPLIT2)),
}
FORM_SEEDS = {"ball12-k1": 19}                    # case -> seed where SEED lets an env reach a goal (the twins' precondition)


def _run_form(name, seed=None):
    c = FORMS[name]
    robot = c["robot"]()

    def check(t, a, b, f):
        if "obs_dim" in c:
            assert a.obs_dim == c["obs_dim"]
    return _twins(robot, c["n"], seed=FORM_SEEDS.get(name, SEED) if seed is None else seed, prepare=c.get("prepare"), check=check,
                  twin=c.get("twin", True), integ=c.get("integ", "euler"), **c.get("kw", {}))


@pytest.mark.parametrize("name", sorted(FORMS))
def test_every_form_and_extension_draws_pool_rows(name, monkeypatch):
    """The goal columns are compared exactly under sensor noise too: noise never touches them."""
    if "jit" in FORMS[name]:
        monkeypatch.setenv("ROBOY_SIM_JIT", FORMS[name]["jit"])
    _run_form(name)


# ---- 4. sub-ranges ----
def test_two_halves_on_two_streams_equal_the_whole_batch():
    import torch
    robot, n, h, seed = _msj(), 512, 256, 5
    pool = gp.small_pool(robot.get_description())
    acts = _actions(robot, n, seed)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for mode in ("whole", "split"):
        env = _vec(robot, n, pool, seed=seed)
        try:
            assert env.range_capable()
            env.reset()
            d_act, d_obs, d_rew, d_done = (env.sim.malloc(4 * n * w) for w in (env.n_t, env.obs_dim, 1, 1))
            rows = []
            for a in acts:
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
                rows.append((env.sim.download(d_obs, (n, 9)), env.sim.download(d_rew, (n,)), env.sim.download(d_done, (n,), np.uint32)))
            res.append(rows)
        finally:
            env.close()
    for t, (w, s) in enumerate(zip(*res)):
        for x, y in zip(w, s):
            assert np.array_equal(x, y), t
        assert gp.rows_in(w[0][:, 6:9], pool).all()
    assert sum(int(w[2].sum()) for w in res[0]) == 2 * n          # every env ended two episodes: both halves drew


# ---- 5. neighbours ----
def test_critic_rows_carry_the_pool_goal_and_truncation_codes_are_the_twins():
    def check(t, a, b, f):
        assert np.array_equal(a.critic_obs()[:, 6:9], f.held)     # the plane, behind the trailing kernel
        assert np.array_equal(a.critic_obs()[:, :6], b.critic_obs()[:, :6])
        if t >= 0:
            assert np.array_equal(a.truncated(), b.truncated())
            assert a.truncated().any() == ((t + 1) % MAX_LEN == 0)
    _twins(_msj(), 300, check=check, critic_obs=("state",), report_truncation=True)


# ---- 6. the torch path and graphs ----
def test_captured_rollouts_show_pool_rows_and_a_replaced_pool_on_the_next_replay():
    import torch
    from gym_roboy_amd.ppo import PPO
    robot, n = _msj(), 512
    desc = robot.get_description()
    pool, other = gp.small_pool(desc), gp.small_pool(desc, base=0.2, step=0.03)
    assert not gp.rows_in(other, pool).any()
    env = _vec(robot, n, pool, seed=2)
    try:
        agent = PPO(env, n_steps=8, use_graphs=True, seed=1, reward_scale=0.01)
        for _ in range(2):                                           # builds the graph, then replays it
            roll = agent.collect()
            goals = roll["obs"][:, :, 6:9].cpu().numpy().reshape(-1, 3)
            assert gp.rows_in(goals, pool).all()
            assert len(np.unique(goals, axis=0)) == 7
        with pytest.raises(ValueError, match="7 rows"):
            env.set_goal_pool(other[:3])
        env.set_goal_pool(other)
        assert np.array_equal(env.goal_pool(), other)
        roll = agent.collect()                                       # a replay: the trailing kernel reads the rows where they were
        goals, done = roll["obs"][:, :, 6:9].cpu().numpy(), roll["done"].cpu().numpy() != 0
        behind = done[:-1]                                           # row t + 1 of an env that was done at t shows the goal drawn there
        assert behind.sum() >= 2 * n
        assert gp.rows_in(goals[1:][behind], other).all()
        assert gp.rows_in(goals.reshape(-1, 3), np.concatenate((pool, other))).all()
        drawn = np.cumsum(done, axis=0)[:-1] > 0                     # ... and it stays until the env's next draw, again from the new rows
        assert gp.rows_in(goals[1:][drawn], other).all()
    finally:
        env.close()


# ---- 7. refusals ----
def test_refusals_leave_the_handle_usable():
    robot, n, seed = _msj(), 300, 5
    pool = gp.small_pool(robot.get_description())
    env = _vec(robot, n, pool, seed=seed)
    try:
        lib, h = env.sim._lib, env.sim.handle
        d_ring = env.sim.malloc(4 * n * env.n_t)
        env.sim.upload(d_ring, np.zeros((n, env.n_t), np.float32))
        assert lib.rb_rollout_fused_dev(h, ctypes.c_void_p(d_ring), 1, 1, ctypes.c_float(1.0)) == nat.RB_EUNSUPPORTED
        assert b"goal pool" in lib.rb_last_error()
        assert lib.rb_env_goal_pool_set(h, nat.fptr(np.ascontiguousarray(pool[:3])), 3) == nat.RB_EINVAL       # a second size
        assert lib.rb_env_goal_pool_set(h, nat.fptr(pool), 0) == nat.RB_EINVAL
        for bad in (4.0, -4.0, np.nan, np.inf):                      # outside the angle box of +-pi, or not finite
            rows = pool.copy()
            rows[6, 2] = bad
            assert lib.rb_env_goal_pool_set(h, nat.fptr(rows), 7) == nat.RB_EINVAL, bad
        with pytest.raises(ValueError):
            env.set_goal_pool(np.full((7, 3), 4.0, np.float32))
        assert np.array_equal(env.goal_pool(), pool)                 # nothing of the refused rows arrived
        f = gp.Follower(env, pool, seed)
        f.reset()
        for a in _actions(robot, n, seed, 4):
            f.step(a)
    finally:
        env.close()
    plain = _vec(robot, n, None, seed=seed)
    try:
        with pytest.raises(RuntimeError):
            plain.goal_pool()
        d_pool, m = ctypes.c_void_p(), ctypes.c_int64()
        assert plain.sim._lib.rb_env_goal_pool_ptr(plain.sim.handle, ctypes.byref(d_pool), ctypes.byref(m)) == nat.RB_EINVAL
    finally:
        plain.close()


# ---- 8. the single env ----
def test_single_env_client_and_roboy_env_draw_by_the_same_rule():
    import contextlib
    import io
    from gym_roboy_amd.envs import RoboyEnv
    from gym_roboy_amd.envs.simulations import HipSimulationClient
    robot, seed, idx = _msj(), 9, 3
    pool = gp.small_pool(robot.get_description())
    client = HipSimulationClient(robot, process_idx=idx, seed=seed, goals=pool)
    try:
        for draw in range(4):
            want = pool[gp.pool_row(seed, [idx], draw, 7)[0]]
            assert np.array_equal(client.get_new_goal_joint_angles(), want.astype(np.float64))
    finally:
        client.close()
    with contextlib.redirect_stdout(io.StringIO()):
        env = RoboyEnv(simulation_client=HipSimulationClient(robot, process_idx=idx, seed=seed, goals=pool))
    try:
        assert np.array_equal(env._goal_state.joint_angles, pool[gp.pool_row(seed, [idx], 0, 7)[0]].astype(np.float64))
        obs = env.reset()
        want = pool[gp.pool_row(seed, [idx], 1, 7)[0]].astype(np.float64)
        assert np.array_equal(env._goal_state.joint_angles, want) and np.array_equal(obs[6:9], want)
    finally:
        env._simulation_client.close()
    with pytest.raises(ValueError):                                  # outside the joint limits, the box the client's goals come from
        HipSimulationClient(robot, goals=np.full((2, 3), 1.0, np.float32))


# ---- 9. reachable_goals ----
@pytest.mark.parametrize("case", sorted(gp.SETTLE_CASES))
def test_reachable_goals_against_the_fp64_oracle_and_end_to_end(case):
    """Inputs qualified in tests/test_goal_pool_cpu.py (fp32 and fp64 oracle agree on them).  End to end: an env whose goal is pool row
    j, driven by the set-points that produced row j, reaches it within settle_steps + 1 steps - the goal is reachable by
    construction; the twin whose goal is 3 rad in every joint never does."""
    from gym_roboy_amd.envs.goals import reachable_goals
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    make, m, integ, seed = gp.SETTLE_CASES[case]
    robot = make()
    desc = robot.get_description()
    n = gp.batch_envs(m)
    pool = reachable_goals(robot, m, seed=seed, integrator=integ, settle_steps=gp.SETTLE_STEPS)
    again = reachable_goals(robot, m, seed=seed, integrator=integ, settle_steps=gp.SETTLE_STEPS)
    assert pool.q.shape == (m, desc.n_q) and pool.q.dtype == np.float32
    assert np.array_equal(pool.q.view(np.uint32), again.q.view(np.uint32)) and pool.recipe == again.recipe
    assert np.all(pool.q >= desc.q_lo) and np.all(pool.q <= desc.q_hi)
    assert pool.recipe["batches"] == 1 and pool.recipe["batch_envs"] == n and pool.recipe["settle_steps"] == gp.SETTLE_STEPS
    assert pool.recipe["settle_tol"] == pytest.approx(gp.vel_tol(robot) / 20, rel=1e-6)
    # keep decisions: the pool is the first m kept envs of batch 0 in env order, so every env up to the last source is decided
    q64, _, keep64 = gp.settled(case, "f64")
    src = pool.source[:, 1]
    assert np.all(pool.source[:, 0] == 0) and np.all(np.diff(src) > 0) and src[-1] < n
    decided = src[-1] + 1
    keep_gpu = np.zeros(decided, bool)
    keep_gpu[src] = True
    differ = int(np.sum(keep_gpu != keep64[:decided])) + abs(int(round(pool.recipe["yield"] * n)) - int(keep64.sum()))
    both = keep64[src]
    worst = float(np.linalg.norm(pool.q[both].astype(np.float64) - q64[src[both]], axis=1).max())
    print("%s: yield %.3f (fp64 oracle %.3f), decisions differ in %d of %d, largest pose difference %.3g (bound %.3g)"
          % (case, pool.recipe["yield"], keep64.mean(), differ, n, worst, gp.angle_tol(robot) / 4))
    assert differ <= n // 100
    assert worst < gp.angle_tol(robot) / 4
    # end to end
    act = robot.get_action_space()
    sp = gp.setpoints(robot, seed, 0, n)[src]
    a = np.clip(2.0 * (sp - act.low) / (act.high - act.low) - 1.0, -1.0, 1.0).astype(np.float32)
    out = {}
    for name, goal in (("pool", pool.q), ("far", np.full((m, desc.n_q), 3.0, np.float32))):
        env = RoboyVecEnv(robot, m, seed=seed, integrator=integ, report_truncation=True)
        try:
            env.reset()
            env.set_goal(goal)
            reached = np.zeros(m, bool)
            for t in range(gp.SETTLE_STEPS + 1):
                _, _, done, _ = env.step(a)
                reached |= done & ~env.truncated()
                if name == "pool" and reached.all():
                    break
            out[name] = (reached, env.stats()["n_goal_reached"], t + 1)
        finally:
            env.close()
    print("%s: %d of %d envs reached their pool goal within %d steps" % (case, out["pool"][0].sum(), m, out["pool"][2]))
    assert out["pool"][0].all() and out["pool"][1] >= m
    assert not out["far"][0].any() and out["far"][1] == 0
