"""Goal curriculum on the GPU (include/roboy_sim.h: rb_env_goal_curriculum_*; csrc/env_goal.hpp): at the top level an
env is bit for bit the env with the plain pool; below it every goal is the restated row inside the env's window; levels, indices and
goal columns follow tests/goal_curriculum_util.py's host follower through promotions and demotions, resets, set_goal, statistics
resets, every kernel form and extension, sub-ranges on two streams and a captured PPO rollout; the histogram equals np.bincount; and
every refusal leaves the handle usable."""
import ctypes

import numpy as np
import pytest

import goal_curriculum_util as gc
import goal_pool_util as gp
from gym_roboy_amd import _native as nat
from test_env_golden_gpu import pin_form
from test_env_params_gpu import _msj
from test_tree_robot_gpu import LANE, OCTET

pytestmark = pytest.mark.gpu

SIGMA = {"q": 0.01, "qd": 0.05}
RANGES = dict(force_scale=(0.7, 1.3), setpoint_offset=(-0.02, 0.02), mass_scale=(0.6, 1.6), damping_scale=(0.5, 2.0))


def _vec(robot, n, goals, curriculum, seed=5, max_len=5, **kw):
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    if kw.get("randomization") is True:
        kw["randomization"] = ParamRanges(**RANGES)
    return RoboyVecEnv(robot, n, seed=seed, max_episode_length=max_len, goals=goals, goal_curriculum=curriculum, **kw)


def _actions(robot, n, seed, steps):
    return np.random.default_rng(seed).uniform(-1, 1, (steps, n, robot.get_action_space().shape[0])).astype(np.float32)


# ---- 1. the top level is the plain pool ----
@pytest.mark.parametrize("auto_reset", [True, False])
def test_top_level_equals_the_plain_pool(auto_reset):
    robot, n, seed = _msj(), 300, 5
    pool = gp.small_pool(robot.get_description())
    acts = _actions(robot, n, seed, 13)
    a = _vec(robot, n, pool, dict(levels=4, start=3, up=0, down=0), seed=seed, auto_reset=auto_reset, critic_obs=("state",))
    b = _vec(robot, n, pool, None, seed=seed, auto_reset=auto_reset, critic_obs=("state",))
    try:
        assert a.goal_curriculum == {"levels": 4, "up": 0, "down": 0, "start": 3} and b.goal_curriculum is None
        fb = gp.Follower(b, pool, seed, auto_reset=auto_reset)

        def same(t):
            assert np.array_equal(a.critic_obs(), b.critic_obs()), t                  # q, qd and the goal PLANE
            for name, x, y in zip(("q", "qd", "feasible"), a.sim.read_state(), b.sim.read_state()):
                assert np.array_equal(x, y), (t, name)
            assert np.array_equal(a.goal_index(), gp.pool_row(seed, fb.gids, (fb.count - 1).astype(np.uint32), 7)), t
            assert np.array_equal(a.goal_levels(), np.full(n, 3)), t
        same("construction")
        n_done = 0
        for t, act in enumerate(acts):
            if t in (0, 7):
                assert a.reset().tobytes() == fb.reset().tobytes()
                same("reset")
            oa, ra, da, _ = a.step(act)
            ob, rb, db = fb.step(act)
            assert oa.tobytes() == ob.tobytes() and ra.tobytes() == rb.tobytes() and np.array_equal(da, db), t
            same(t)
            n_done += int(da.sum())
        assert n_done >= 2 * n
        assert a.stats() == b.stats()
    finally:
        a.close(), b.close()


# ---- 2. windows ----
@pytest.mark.parametrize("offset", [0, 1000])
def test_windows(offset):
    import torch
    robot, n, seed = _msj(), 300, 5
    pool = gp.small_pool(robot.get_description(), m=7)
    acts = _actions(robot, n, seed, 11)
    for start, rows in ((0, {0}), (2, {0, 1, 2})):
        assert gc.hi(start, 7, 7) == start + 1
        env = _vec(robot, n, pool, dict(levels=7, start=start, up=0, down=0), seed=seed, env_id_offset=offset)
        try:
            f = gc.CurriculumFollower(env, pool, seed, 7, 0, 0, start, offset=offset, outcome="never")
            f.check_planes()
            seen = set(f.index.tolist())
            f.reset()
            for act in acts:
                f.step(act)
                seen |= set(f.index.tolist())
                assert np.asarray(env.goal_index()).max() < gc.hi(start, 7, 7)
            assert seen == rows and f.ends >= 2 * n
            if offset:
                assert not np.array_equal(f.index, gc.row(seed, np.arange(n), (f.count - 1).astype(np.uint32), start, 7, 7)) or start == 0
            assert env.stats()["n_goal_reached"] == 0                # the follower's "never"
            # behind a torch step the accessors return CUDA tensors
            obs, _, _, _ = env.step(torch.zeros((n, env.n_t), device="cuda"))
            lv, ix, hist = env.goal_levels(), env.goal_index(), env.goal_level_histogram()
            assert all(torch.is_tensor(x) and x.is_cuda for x in (lv, ix, hist))
            assert np.array_equal(lv.cpu().numpy(), f.level) and ix.cpu().numpy().max() < start + 1
            assert np.array_equal(hist.cpu().numpy(), np.bincount(f.level, minlength=7))
            assert np.array_equal(obs[:, 6:9].cpu().numpy(), pool[ix.cpu().numpy()])
        finally:
            env.close()


# ---- 3. the staircase against the follower ----
_reachable = {}


def _reachable_pool():
    """reachable_goals(MsjRobot(), 256, seed=0), ordered; per row the actions that made it (the recipe's source through
    goal_pool_util.setpoints) and a row whose pose is more than four angle tolerances away (the farthest one)."""
    if not _reachable:
        from gym_roboy_amd.envs.goals import reachable_goals
        robot = _msj()
        pool = reachable_goals(robot, 256, seed=0).ordered()
        assert pool.recipe["ordered"] == "rest_distance"
        act = robot.get_action_space()
        batches = {int(b): gp.setpoints(robot, 0, int(b), gp.batch_envs(256)) for b in np.unique(pool.source[:, 0])}
        sp = np.stack([batches[int(b)][int(e)] for b, e in pool.source])
        a = np.clip(2.0 * (sp - act.low) / (act.high - act.low) - 1.0, -1.0, 1.0).astype(np.float32)
        d = np.linalg.norm(pool.q[:, None, :].astype(np.float64) - pool.q[None, :, :], axis=-1)
        far = d.argmax(axis=1)
        assert d[np.arange(256), far].min() > 4 * gp.angle_tol(robot)
        _reachable.update(pool=pool, act=a, far=far)
    return _reachable["pool"], _reachable["act"], _reachable["far"]


@pytest.mark.parametrize("up,down,steps,block", [(1, 1, 300, 36), (2, 1, 200, 25)])
def test_staircase_follows_the_host_model(up, down, steps, block):
    """An env in the GOOD role is driven at every step by the set-points that made the row it holds and reaches it; an env in the BAD
    role is driven by the set-points of a row far from its goal (the farthest; more than four angle tolerances, asserted) and runs
    into the limit of 120 steps.  The outcome the follower moves its levels by is vec.truncated(), not the curriculum's own plane.

    The split of the envs: group i % 8 is good during the steps [block g, block (g + 1)) of every 8 blocks and bad otherwise - one env
    in eight is good at a time, not one in two.  With the two halves fixed for the run (envs 0, 2, ... good, 1, 3, ... bad; 512 envs,
    300 steps, from level 3) the device and the model agreed at every step, but a driven env reaches its goal about every 11 steps,
    not every 100: 7 468 episode ends, of which 1 024 promotions (four per good env, then it sits at the top level) and 512
    demotions (two time-outs per bad env).  No fixed split meets "a quarter of the ends are promotions and a quarter demotions" with
    8 levels: a time-out takes 120 steps and a reach 11, and a good env has at most 7 promotions ahead of it.  With the rotating
    split reaches and time-outs occur at about the same rate and every env moves in both directions."""
    robot, n, seed, n_levels, start = _msj(), 512, 0, 8, 3
    pool, act_of, far = _reachable_pool()
    group = np.arange(n) % 8
    env = _vec(robot, n, pool, dict(levels=n_levels, up=up, down=down, start=start), seed=seed, max_len=120, report_truncation=True)
    try:
        assert env.goal_recipe["ordered"] == "rest_distance"
        f = gc.CurriculumFollower(env, pool.q, seed, n_levels, up, down, start, outcome="truncated")
        f.check_planes()
        f.reset()
        went_up, went_down, jump = np.zeros(n, bool), np.zeros(n, bool), 0
        for t in range(steps):
            good = group == (t // block) % 8
            before = f.level.copy()
            f.step(np.where(good[:, None], act_of[f.index], act_of[far[f.index]]))
            went_up |= f.level > before
            went_down |= f.level < before
            jump = max(jump, int((f.level - before).max()))
        print("up %d down %d: %d episode ends, %d promotions, %d demotions, %d envs moved both ways, levels %s" % (
            up, down, f.ends, f.promotions, f.demotions, (went_up & went_down).sum(), np.bincount(f.level, minlength=n_levels).tolist()))
        stats = env.stats()
        assert stats["n_episodes"] == f.ends and 0 < stats["n_goal_reached"] < f.ends
        assert (f.level > 0).any() and (f.level < n_levels - 1).any()
        if up == 1:
            assert 4 * f.promotions >= f.ends and 4 * f.demotions >= f.ends
        else:                                                        # the shorter case: an eighth of the envs each way, and a jump of two
            assert f.promotions >= n // 8 and f.demotions >= n // 8
            assert jump == up
    finally:
        env.close()


# ---- 4. reset, set_goal and stats ----
def test_reset_set_goal_and_stats_reset():
    """Zero actions from rest with the zero pose as the goal: reached at the first step (tests/test_truncation_gpu.py's trick); a goal
    at 3 rad in every joint or a pool row (half-way to the limits) is never reached under zero actions."""
    robot, n, seed = _msj(), 256, 5
    pool = gp.small_pool(robot.get_description())
    zero = np.zeros((n, 8), np.float32)
    chosen = np.arange(n) % 2 == 0
    goal = np.where(chosen[:, None], 0.0, 3.0).astype(np.float32) * np.ones((1, 3), np.float32)
    env = _vec(robot, n, pool, dict(levels=5, start=1), seed=seed, max_len=4)
    try:
        env.reset()
        env.set_goal(goal)
        assert (env.goal_index() == nat.RB_GOAL_INDEX_NONE).all() and (env.goal_levels() == 1).all()
        _, rew, done, _ = env.step(zero)
        assert np.array_equal(done, chosen) and (rew[chosen] > 0).all()
        assert np.array_equal(env.goal_levels(), np.where(chosen, 2, 1))           # promoted; the others still hold the set goal
        index = env.goal_index()
        assert (index[~chosen] == nat.RB_GOAL_INDEX_NONE).all()
        assert np.array_equal(index[chosen], gc.row(seed, np.arange(n)[chosen], 3, 2, 7, 5))     # draws 0, 1 (reset), then + 2
        # a reset keeps the levels; the chosen envs, one goal behind them, are demoted by their next time-out like everybody else
        obs = env.reset()
        level = np.where(chosen, 2, 1)
        assert np.array_equal(env.goal_levels(), level)
        draw = np.where(chosen, 4, 2)
        k = gc.row(seed, np.arange(n), draw.astype(np.uint32), level, 7, 5)
        assert np.array_equal(env.goal_index(), k) and np.array_equal(obs[:, 6:9], pool[k])
        for t in range(4):
            _, _, done, _ = env.step(zero)
            assert done.all() == (t == 3)
        assert np.array_equal(env.goal_levels(), level - 1)
        # stats(reset=True) zeroes the counters the outcome is read from: the next time-out is still a time-out
        env.set_goal(goal)
        _, _, done, _ = env.step(zero)
        assert np.array_equal(done, chosen)
        level = level - 1 + chosen
        assert np.array_equal(env.goal_levels(), level)
        assert env.stats(reset=True)["n_goal_reached"] == 2 * chosen.sum()
        for t in range(3):                                           # the others are three steps from their limit, the chosen four
            _, _, done, _ = env.step(zero)
            assert np.array_equal(done, ~chosen & (t == 2))
        assert np.array_equal(env.goal_levels(), np.where(chosen, 2, 0))
        _, _, done, _ = env.step(zero)
        assert np.array_equal(done, chosen) and np.array_equal(env.goal_levels(), np.where(chosen, 1, 0))       # demoted, two goals behind them
        assert env.stats()["n_goal_reached"] == 0
    finally:
        env.close()


# ---- 5. forms ----
def _run_follower(robot, n, kw=None, prepare=None, check=None, steps=9, seed=5, n_levels=4, max_len=3):
    """down = 1 from the top level under a short time limit: levels move without anybody reaching anything (asserted)."""
    pool = gp.small_pool(robot.get_description())
    env = _vec(robot, n, pool, dict(levels=n_levels, start=n_levels - 1, up=1, down=1), seed=seed, max_len=max_len, **(kw or {}))
    try:
        if prepare:
            prepare(env)
        f = gc.CurriculumFollower(env, pool, seed, n_levels, 1, 1, n_levels - 1, outcome="never")
        f.check_planes()
        f.reset()
        for act in _actions(robot, n, seed, steps):
            f.step(act)
            if check:
                check(env, f)
        assert env.stats()["n_goal_reached"] == 0 and f.ends >= 2 * n
        assert f.level.max() == n_levels - 1 - f.ends // n
        return f
    finally:
        env.close()


@pytest.mark.parametrize("kernel,integ", [(1, "euler"), (2, "euler"), (5, "rk4")])
def test_ball_joint_forms_by_name(kernel, integ):
    _run_follower(_msj(), 300, kw=dict(integrator=integ), prepare=lambda env: pin_form(env, kernel))


@pytest.mark.parametrize("kernel", [OCTET, LANE])
def test_upper_body_rows_of_twenty_goal_columns(kernel):
    from gym_roboy_amd.envs.robots import UpperBodyRobot

    def prepare(env):
        env.sim.select_kernel(kernel)
        assert env.sim.info()["kernel"] == kernel and env.obs_dim == 60 and env.n_q == 20
    _run_follower(UpperBodyRobot(), 64, prepare=prepare, steps=7)


def test_together_with_every_extension_and_the_critic_rows():
    def check(env, f):
        assert env.obs_dim == 49
        assert np.array_equal(env.critic_obs()[:, 6:9], f.held)      # the state block's goal: the plane behind the curriculum's kernel
    _run_follower(_msj(), 300, check=check, kw=dict(
        integrator="rk4", randomization=True, tendon_obs=("length", "force"), sensor_noise=SIGMA, action_delay=(0, 3), action_obs=3,
        critic_obs=("state", "age", "params", "delay", "actions")))


def test_two_halves_on_two_streams_equal_the_whole_batch():
    import torch
    robot, n, h, seed = _msj(), 512, 256, 5
    pool = gp.small_pool(robot.get_description())
    acts = _actions(robot, n, seed, 7)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for mode in ("whole", "split"):
        env = _vec(robot, n, pool, dict(levels=4, start=3), seed=seed, max_len=3)
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
                rows.append((env.sim.download(d_obs, (n, 9)), env.sim.download(d_rew, (n,)), env.sim.download(d_done, (n,), np.uint32),
                             env.goal_levels(), env.goal_index()))
            res.append(rows)
        finally:
            env.close()
    for t, (w, s) in enumerate(zip(*res)):
        for x, y in zip(w, s):
            assert np.array_equal(x, y), t
        assert np.array_equal(w[0][:, 6:9], pool[w[4]])
    assert np.array_equal(res[1][-1][3], np.full(n, 1))              # two time-outs each, in both halves


# ---- 6. histogram ----
@pytest.mark.parametrize("n", [1, 255, 256, 257, 66819])
def test_level_histogram_equals_bincount(n, monkeypatch):
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")                         # (no run-time builds at the large size: the step is not under test)
    robot = _msj()
    pool = gp.small_pool(robot.get_description(), m=256, base=0.3, step=0.002)
    rng = np.random.default_rng(n)
    for n_levels in (1, 7, 256):
        env = _vec(robot, n, pool, dict(levels=n_levels, start=n_levels - 1))
        try:
            assert np.array_equal(env.goal_level_histogram(), np.bincount(np.full(n, n_levels - 1), minlength=n_levels))     # one full bin
            for levels in (rng.integers(0, n_levels, n), 2 * rng.integers(0, (n_levels + 1) // 2, n), np.zeros(n, np.int64)):
                env.set_goal_levels(levels)
                assert np.array_equal(env.goal_levels(), levels)
                hist = env.goal_level_histogram()
                assert hist.dtype == np.int64 and hist.shape == (n_levels,) and hist.sum() == n
                assert np.array_equal(hist, np.bincount(levels, minlength=n_levels))
        finally:
            env.close()


# ---- 7. a captured PPO rollout ----
def test_captured_ppo_rollout_save_and_load(tmp_path):
    import torch
    from gym_roboy_amd.ppo import PPO
    robot, n, seed, n_levels = _msj(), 512, 2, 6
    pool = gp.small_pool(robot.get_description())
    env = _vec(robot, n, pool, dict(levels=n_levels, start=n_levels - 1), seed=seed, max_len=5)
    plain = _vec(robot, n, pool, None, seed=seed, max_len=5)
    try:
        agent = PPO(env, n_steps=16, use_graphs=True, seed=1, reward_scale=0.01)
        level, count, ends = np.full(n, n_levels - 1), np.full(n, 2), 0      # construction, then the first rollout's reset
        index = None
        for _ in range(3):                                           # builds the graph, then two replays
            done = agent.collect()["done"].cpu().numpy() != 0
            for d in done:
                level[d] = gc.next_level(level[d], False, 1, 1, n_levels)
                count[d] += 2
                ends += int(d.sum())
            index = gc.row(seed, np.arange(n), (count - 1).astype(np.uint32), level, 7, n_levels)
        stats = env.stats()
        assert stats["n_episodes"] == ends >= 8 * n and stats["n_goal_reached"] == 0      # the model saw every end, all of them time-outs
        assert np.array_equal(env.goal_levels(), level) and (level == 0).all()
        # (an env draws at its episode ends: the index plane holds the row of each env's last draw, at the level it had then)
        assert np.array_equal(env.goal_index(), index) and not index.any()
        pattern = np.arange(n) % n_levels
        env.set_goal_levels(pattern)
        path = str(tmp_path / "model.pkl")
        agent.save(path)
        ck = torch.load(path)
        assert {k: ck["goal_curriculum"][k] for k in ("levels", "up", "down")} == {"levels": n_levels, "up": 1, "down": 1}
        assert np.array_equal(ck["goal_curriculum"]["level"].numpy(), pattern)
        env.set_goal_levels(np.zeros(n, np.int64))
        agent.load(path)
        assert np.array_equal(env.goal_levels(), pattern) and agent.checkpoint_goal_curriculum is None
        # an env without the option: its checkpoint has no new key, and it records a curriculum checkpoint's levels without taking them
        other = PPO(plain, n_steps=2, use_graphs=False, seed=1, reward_scale=0.01)
        other.save(str(tmp_path / "plain.pkl"))
        assert "goal_curriculum" not in torch.load(str(tmp_path / "plain.pkl"))
        other.load(path)
        assert np.array_equal(other.checkpoint_goal_curriculum["level"].cpu().numpy(), pattern)
    finally:
        env.close(), plain.close()


# ---- 8. refusals ----
def test_refusals_leave_the_handle_usable():
    from gym_roboy_amd.envs.simulations import HipSimulationClient
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, n, seed = _msj(), 300, 5
    desc = robot.get_description()
    pool = gp.small_pool(desc)
    plain = RoboyVecEnv(robot, n, seed=seed, max_episode_length=3)
    try:
        assert plain.sim._lib.rb_env_goal_curriculum_configure(plain.sim.handle, 4, 1, 1, 0) == nat.RB_EINVAL      # no pool
        assert b"goal pool" in plain.sim._lib.rb_last_error()
        with pytest.raises(RuntimeError):
            plain.goal_levels()
    finally:
        plain.close()
    with pytest.raises(ValueError, match="1\\.\\.7"):
        _vec(robot, n, pool, 8)
    env = _vec(robot, n, gp.small_pool(desc, m=300, base=0.3, step=0.002), None, seed=seed, max_len=3)
    try:
        assert env.sim._lib.rb_env_goal_curriculum_configure(env.sim.handle, 257, 1, 1, 0) == nat.RB_EINVAL          # L > 256 (m = 300)
    finally:
        env.close()
    env = _vec(robot, n, pool, None, seed=seed, max_len=3)
    try:
        lib, h = env.sim._lib, env.sim.handle
        ptr = ctypes.c_void_p()
        assert lib.rb_env_goal_level_ptr(h, ctypes.byref(ptr)) == nat.RB_EINVAL                    # no curriculum yet
        for bad in ((8, 1, 1, 0), (0, 1, 1, 0), (4, 1, 1, 4), (4, 1, 1, -1), (4, -1, 1, 0), (4, 1, -1, 0)):        # L > m, L < 1, level0, up, down
            assert lib.rb_env_goal_curriculum_configure(h, *bad) == nat.RB_EINVAL, bad
        assert lib.rb_env_goal_level_ptr(h, ctypes.byref(ptr)) == nat.RB_EINVAL                    # nothing was configured
        f = gp.Follower(env, pool, seed)                                                           # ... and the plain pool still runs
        f.reset()
        f.step(_actions(robot, n, seed, 1)[0])
        assert lib.rb_env_goal_curriculum_configure(h, 4, 1, 1, 3) == nat.RB_OK
        env.goal_curriculum = {"levels": 4, "up": 1, "down": 1, "start": 3}
        assert lib.rb_env_goal_curriculum_configure(h, 4, 1, 1, 3) == nat.RB_EINVAL                # once per handle
        assert b"once per handle" in lib.rb_last_error()
        levels = np.arange(n) % 4
        env.set_goal_levels(levels)
        bad = levels.astype(np.uint32)
        bad[n - 1] = 4
        assert lib.rb_env_goal_levels_set(h, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == nat.RB_EINVAL
        for wrong in (bad, levels[:-1], levels.astype(np.float32), -levels):
            with pytest.raises(ValueError):
                env.set_goal_levels(wrong)
        assert np.array_equal(env.goal_levels(), levels)                                           # nothing has changed
        goals = np.empty((n, 3), np.float32)
        assert lib.rb_sample_goals(h, None, nat.fptr(goals)) == nat.RB_EUNSUPPORTED
        assert b"curriculum" in lib.rb_last_error()
        d_goal = env.sim.malloc(4 * n * 3)
        assert lib.rb_sample_goals_dev(h, None, ctypes.c_void_p(d_goal)) == nat.RB_EUNSUPPORTED
        # the handle goes on, from the levels just set
        fc = gc.CurriculumFollower(env, pool, seed, 4, 1, 1, 0, outcome="never")
        fc.level, fc.count = levels.copy(), f.count.copy()
        fc.reset()
        for act in _actions(robot, n, seed, 4):
            fc.step(act)
        assert fc.ends >= n and env.stats()["n_goal_reached"] == 0
    finally:
        env.close()
    with pytest.raises(ValueError, match="vectorised env"):
        HipSimulationClient(robot, goals=pool, goal_curriculum=2)


def test_an_unordered_goal_pool_is_ordered_with_a_warning():
    from gym_roboy_amd.envs.goals import GoalPool
    robot = _msj()
    rows = gp.small_pool(robot.get_description())[::-1].copy()       # farthest from the rest pose first
    want = rows[np.argsort(np.linalg.norm(rows.astype(np.float64), axis=1), kind="stable")]
    assert not np.array_equal(want, rows)
    with pytest.warns(UserWarning, match="not marked ordered"):
        env = _vec(robot, 256, GoalPool(rows, {"m": 7}), 7)
    try:
        assert np.array_equal(env.goal_pool(), want) and env.goal_recipe == {"m": 7, "ordered": "rest_distance"}
        assert not env.goal_index().any() and np.array_equal(env.reset()[:, 6:9], np.broadcast_to(want[0], (256, 3)))
    finally:
        env.close()
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*not marked ordered.*")      # marked pools and bare rows: taken as they are
        for goals in (GoalPool(rows, {"ordered": "rest_distance"}), rows):
            env = _vec(robot, 256, goals, 7)
            try:
                assert np.array_equal(env.goal_pool(), rows)
            finally:
                env.close()
