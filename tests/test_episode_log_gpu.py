"""The episode log behind the fused env step (csrc/env_episode_log.hpp; include/roboy_sim.h: rb_env_episode_log_*) on
the GPU.

The model check: the records equal tests/episode_log_util.py's numpy restatement of the lane rule fed with the rewards, dones and
``truncated()`` the env itself returned, bit for bit - the log is a pure function of what the step reports, so no physics oracle is
needed.  Shapes: MsjRobot at 300 envs (a 44-lane tail, five waves, two workgroups) and the upper body at 96 (a wave and a half);
E = 3, episodes of at most 6 steps, 24 steps of seeded random actions; every third env is sent to its goal at once (the zero pose
it rests at, the rest command), the way tests/test_truncation_gpu.py makes both outcomes.  That both outcomes and a saturated env
occur is asserted: conditions on the inputs.

Tolerances.  Counts are exact.  A sum over n fp32 values taken in fp64 in two orders (the device's block tree, numpy's pairwise sum,
the step kernels' per-env sums) differs by at most n 2^-52 times the sum of the magnitudes: each of at most n - 1 additions per
order rounds within 2^-53 of a partial sum that the magnitudes bound."""
import ctypes

import numpy as np
import pytest

import episode_log_util as elu
from gym_roboy_amd import _native as nat

pytestmark = pytest.mark.gpu

SEED, MAX_LEN, STEPS, E = 5, 6, 24, 3
SHAPES = {"msj": 300, "upper": 96}
LANE = 1                                        # RB_KERNEL_ENV_PER_LANE: takes sub-ranges


def _robot(which):
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    return MsjRobot() if which == "msj" else UpperBodyRobot()


def _env(which, capacity=E, n=None, **kw):
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    kw.setdefault("report_truncation", True)
    return RoboyVecEnv(_robot(which), n or SHAPES[which], seed=SEED, max_episode_length=MAX_LEN, episode_log=capacity, **kw)


def _scenario(env, steps=STEPS):
    """reset; every third env's goal is the pose it rests at and its first action the rest command -> actions [steps, n, n_t]"""
    obs0 = env.reset()
    n = env.num_envs
    goal = np.array(obs0[:, 2 * env.n_q:3 * env.n_q], np.float32)
    goal[np.arange(n) % 3 == 0] = 0.0
    env.set_goal(goal)
    acts = np.random.default_rng(SEED + n).uniform(-1.0, 1.0, (steps, n, env.n_t)).astype(np.float32)
    acts[0, np.arange(n) % 3 == 0] = 0.0
    return acts


def _codes(env):
    return env.sim.download(env._d_done, (env.num_envs,), np.uint32)


def _steps(env, model, acts, codes=None):
    """numpy steps; the model follows what the env returned"""
    for a in acts:
        _, rew, done, _ = env.step(a)
        trunc = env.truncated()
        assert not (trunc & ~done).any()
        model.step_outcome(rew, done, ~trunc)
        if codes is not None:
            codes.append(_codes(env))


def _assert_inputs_are_telling(log, capacity):
    kinds = log["kind"][np.arange(capacity)[None, :] < log["count"][:, None]]
    assert (kinds == elu.TERMINATED).sum() >= 8 and (kinds == elu.TRUNCATED).sum() >= 8, np.bincount(kinds)
    assert (log["count"] == capacity).sum() >= 8


def _planes(env):
    """everything the handle holds for the log, raw: count, ret, len, kind, full"""
    d_count, d_ret, d_len, d_kind, d_full = env._episode_log_planes()
    env.sim.synchronize()
    n, cap = env.num_envs, env.episode_log_capacity
    return (env.sim.download(d_count, (n,), np.uint32), env.sim.download(d_ret, (cap, n)), env.sim.download(d_len, (cap, n), np.uint32),
            env.sim.download(d_kind, (cap, n), np.uint32), env.sim.download(d_full, (1,), np.uint32))


def _assert_same_planes(a, b):
    for k, (x, y) in enumerate(zip(_planes(a), _planes(b))):
        assert x.tobytes() == y.tobytes(), k


# ---- 1. the records are the model's ----
@pytest.mark.parametrize("which", ["msj", "upper"])
def test_records_equal_the_model_and_the_codes(which):
    env, flags = _env(which), _env(which, report_truncation=False)
    try:
        acts = _scenario(env)
        assert np.array_equal(_scenario(flags), acts)
        model, codes = elu.EpisodeLogModel(env.num_envs, E), []
        _steps(env, model, acts, codes)
        log = env.episode_log()
        _assert_inputs_are_telling(log, E)
        assert elu.same_log(log, model.log())
        assert log["return"].dtype == np.float32 and log["count"].dtype == np.int64
        assert env.episode_log_full() == model.full == int((log["count"] == E).sum())
        # every record's kind is the code the step that ended the episode returned
        codes = np.stack(codes)
        for i in range(env.num_envs):
            ends = codes[:, i][codes[:, i] != 0]
            assert np.array_equal(log["kind"][i, :log["count"][i]], ends[:E]), i
        # the done words are read as flags: an env without the codes keeps the same planes
        for a in acts:
            flags.step(a)
        _assert_same_planes(env, flags)
    finally:
        env.close(); flags.close()


@pytest.mark.parametrize("which", ["msj", "upper"])
def test_sums_equal_the_step_kernels_own_statistics(which):
    """E above the number of episodes any env finishes: the log holds every episode stats() counted"""
    cap = 8
    env = _env(which, capacity=cap)
    try:
        acts = _scenario(env)
        for a in acts:
            env.step(a)
        log, stats = env.episode_log(), env.stats()
        assert log["count"].max() < cap and log["count"].min() >= 3
        s = env.episode_log_summary()
        assert s["n_records"] == stats["n_episodes"] == log["count"].sum()
        assert s["sum_length"] == stats["sum_length"] and s["n_terminated"] == stats["n_goal_reached"] > 0
        assert s["n_terminated"] + s["n_truncated"] == s["n_records"] and s["n_complete"] == 0 and s["complete"] is False
        magnitude = np.abs(log["return"].astype(np.float64)).sum()
        print("sum_return: log %r stats %r bound %r" % (s["sum_return"], stats["sum_return"], s["n_records"] * 2.0 ** -52 * magnitude))
        assert abs(s["sum_return"] - stats["sum_return"]) <= s["n_records"] * 2.0 ** -52 * magnitude
    finally:
        env.close()


# ---- 2. what happens between steps ----
def test_a_statistics_reset_in_the_middle_keeps_the_outcomes():
    """stats(reset=True) zeroes the goals-reached counters; the log's `seen` goes with them"""
    env = _env("msj", capacity=8)
    try:
        acts = _scenario(env)
        model = elu.EpisodeLogModel(env.num_envs, 8)
        _steps(env, model, acts[:9], None)
        before = model.log()
        reached_once = (before["kind"] == elu.TERMINATED).any(axis=1)
        env.stats(reset=True)
        model.counters_cleared()
        _steps(env, model, acts[9:], None)
        log = env.episode_log()
        assert elu.same_log(log, model.log())
        # the envs a stale `seen` would mislabel: reached a goal before the clear, ran into the time limit behind it
        later = np.arange(8)[None, :] >= before["count"][:, None]
        assert (reached_once & ((log["kind"] == elu.TRUNCATED) & later).any(axis=1)).sum() >= 8
    finally:
        env.close()


def test_a_reset_in_the_middle_drops_the_running_episode():
    env = _env("upper", capacity=8)
    try:
        acts = _scenario(env)
        model = elu.EpisodeLogModel(env.num_envs, 8)
        _steps(env, model, acts[:9], None)                       # (episodes end at steps 5 and 11: three steps under way)
        before = env.episode_log()
        env.reset()
        model.reset()
        assert elu.same_log(env.episode_log(), before)
        _steps(env, model, acts[9:], None)
        log = env.episode_log()
        assert elu.same_log(log, model.log())
        live = np.arange(8)[None, :] < before["count"][:, None]
        assert np.array_equal(log["return"][live], before["return"][live]) and np.array_equal(log["length"][live], before["length"][live])
        # behind the reset the time limit falls six steps on, not three: no record shorter than the limit among the truncated ones
        new = (np.arange(8)[None, :] >= before["count"][:, None]) & (np.arange(8)[None, :] < log["count"][:, None])
        assert (log["length"][new & (log["kind"] == elu.TRUNCATED)] == MAX_LEN).all() and new.sum() >= env.num_envs
    finally:
        env.close()


# ---- 3. with the other options ----
def _pool(env_robot, m=64):
    desc = env_robot.get_description()
    rows = np.random.default_rng(2).uniform(0.5 * desc.q_lo, 0.5 * desc.q_hi, (m, desc.n_q)).astype(np.float32)
    return rows[np.argsort(np.linalg.norm(rows, axis=1))]


def test_with_reward_shaping_the_records_hold_the_shaped_sums():
    shaped, plain = _env("msj", reward_shaping={"action_rate": 0.5}), _env("msj", capacity=None)
    try:
        acts = _scenario(shaped)
        assert np.array_equal(_scenario(plain), acts)
        model, task = elu.EpisodeLogModel(shaped.num_envs, E), elu.EpisodeLogModel(shaped.num_envs, E)
        for a in acts:
            _, rew, done, _ = shaped.step(a)
            _, rew0, done0, _ = plain.step(a)
            assert np.array_equal(done, done0) and (rew <= rew0).all()
            model.step_outcome(rew, done, ~shaped.truncated())
            task.step_outcome(rew0, done0, ~plain.truncated())
        log = shaped.episode_log()
        _assert_inputs_are_telling(log, E)
        assert elu.same_log(log, model.log())
        assert (log["return"] < task.log()["return"]).sum() >= shaped.num_envs        # the shaped sums, not the task's
        assert shaped.stats() == plain.stats()                                        # ... which stats() keeps
    finally:
        shaped.close(); plain.close()


@pytest.mark.parametrize("case", ["push", "goals", "curriculum"])
def test_with_pushes_a_goal_pool_and_a_curriculum(case):
    robot = _robot("msj")
    kw = {"push": dict(push={"prob": 0.25, "sigma": 1.0}), "goals": dict(goals=_pool(robot)),
          "curriculum": dict(goals=_pool(robot), goal_curriculum={"levels": 4, "up": 1, "down": 1}, goal_row_stats=True)}[case]
    env = _env("msj", **kw)
    try:
        acts = _scenario(env)
        model = elu.EpisodeLogModel(env.num_envs, E)
        _steps(env, model, acts, None)
        log = env.episode_log()
        _assert_inputs_are_telling(log, E)
        assert elu.same_log(log, model.log())
    finally:
        env.close()


# ---- 4. sub-ranges and a captured graph: the planes of the eager twin ----
def test_sub_ranges_on_a_callers_stream_write_their_own_envs():
    import torch
    n, split = SHAPES["msj"], 256
    whole, parts = _env("msj", report_truncation=False), _env("msj", report_truncation=False)
    try:
        for env in (whole, parts):
            env.sim.select_kernel(LANE)
        acts = _scenario(whole)
        assert np.array_equal(_scenario(parts), acts) and parts.range_capable()
        d = [parts.sim.malloc(4 * n * parts.n_t), parts.sim.malloc(4 * n * parts.obs_dim), parts.sim.malloc(4 * n), parts.sim.malloc(4 * n)]
        stream = torch.cuda.Stream()
        for t, a in enumerate(acts):
            whole.step(a)
            parts.sim.upload(d[0], a)
            parts.sim.synchronize()
            parts.step_range_dev(0, split, stream.cuda_stream, *d)
            if t == 0:                                               # the first range alone: the other envs' planes are untouched
                stream.synchronize()
                count = _planes(parts)[0]
                assert count[:split].sum() >= 8 and not count[split:].any()
            parts.step_range_dev(split, n - split, stream.cuda_stream, *d)
            stream.synchronize()
        _assert_same_planes(whole, parts)
        _assert_inputs_are_telling(parts.episode_log(), E)
    finally:
        whole.close(); parts.close()


@pytest.mark.parametrize("which", ["msj", "upper"])
def test_replays_of_a_captured_graph_and_a_clear_between_them(which):
    import torch
    T = 8
    eager, env = _env(which, report_truncation=False), _env(which, report_truncation=False)
    try:
        n = env.num_envs
        acts_np = _scenario(eager, steps=T)
        assert np.array_equal(_scenario(env, steps=T), acts_np)
        dev = torch.device("cuda", 0)
        acts = torch.from_numpy(acts_np).to(dev)
        obs, rew = torch.zeros((T, n, env.obs_dim), device=dev), torch.zeros((T, n), device=dev)
        done = torch.zeros((T, n), dtype=torch.int32, device=dev)
        side = torch.cuda.Stream(device=dev)
        env.set_stream(side.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for k in range(T):
                env.step_dev(acts[k].data_ptr(), obs[k].data_ptr(), rew[k].data_ptr(), done[k].data_ptr())
        for replay in range(3):
            graph.replay()
            torch.cuda.synchronize()
            for a in acts_np:
                eager.step(a)
            _assert_same_planes(eager, env)
        _assert_inputs_are_telling(env.episode_log(), E)
        assert env.episode_log_full() == eager.episode_log_full() > 0
        # a clear between replays: the same graph, the planes start over
        for e in (env, eager):
            e.clear_episode_log()
        torch.cuda.synchronize()
        assert env.episode_log_full() == 0 and not env.episode_log()["count"].any()
        graph.replay()
        torch.cuda.synchronize()
        for a in acts_np:
            eager.step(a)
        _assert_same_planes(eager, env)
        assert env.episode_log()["count"].sum() >= n
    finally:
        eager.close(); env.close()


# ---- 5. the summary kernel ----
def test_summary_against_numpy():
    env = _env("msj")
    try:
        acts = _scenario(env)
        for a in acts:
            env.step(a)
        log = env.episode_log()
        _assert_inputs_are_telling(log, E)
        n = env.num_envs
        for first_k in (1, 2, E, E + 2):                             # below, at and above the capacity
            want, mag, mag_sq = elu.summary_np(log, first_k)
            got = env.episode_log_summary(first_k)
            again = env.episode_log_summary(first_k)
            assert all(np.float64(got[k]).tobytes() == np.float64(again[k]).tobytes() for k in elu.SUMS)
            for k in ("n_records", "sum_length", "n_terminated", "n_truncated", "n_complete"):
                assert got[k] == want[k], (first_k, k)
            records = want["n_records"]
            assert abs(got["sum_return"] - want["sum_return"]) <= records * 2.0 ** -52 * mag
            assert abs(got["sum_return_sq"] - want["sum_return_sq"]) <= records * 2.0 ** -52 * mag_sq
            fig = elu.figures_np({k: got[k] for k in elu.SUMS}, n)
            for k, v in fig.items():
                if k != "complete":
                    assert got[k] == pytest.approx(v, rel=1e-14), (first_k, k)
            assert got["complete"] is (first_k <= E and bool((log["count"] >= first_k).all()))
        assert env.episode_log_summary()["n_records"] == log["count"].sum()
        assert env.episode_log_summary(E + 2)["n_complete"] == 0
        # the device form writes the same eight doubles
        d_out = env.sim.malloc(64)
        assert nat.load().rb_env_episode_log_summary_dev(env.sim.handle, 2, ctypes.c_void_p(d_out)) == nat.RB_OK
        env.sim.synchronize()
        dev = env.sim.download(d_out, (8,), np.float64)
        host = env.episode_log_summary(2)
        assert [dev[j] for j in range(7)] == [host[k] for k in elu.SUMS] and dev[7] == 0.0
        for bad in (0, -1):
            assert nat.load().rb_env_episode_log_summary_dev(env.sim.handle, bad, ctypes.c_void_p(d_out)) == nat.RB_EINVAL
        for bad in (0, True, 1.5):
            with pytest.raises(ValueError, match="first_k"):
                env.episode_log_summary(bad)
    finally:
        env.close()


# ---- 6. the constructor keyword, off, and the refusals ----
def test_the_constructor_keyword():
    env = _env("msj", capacity=1)
    try:
        assert env.episode_log_capacity == 1
        acts = _scenario(env, steps=7)
        model = elu.EpisodeLogModel(env.num_envs, 1)
        _steps(env, model, acts, None)
        log = env.episode_log()
        assert log["return"].shape == (env.num_envs, 1) and (log["count"] == 1).all() and elu.same_log(log, model.log())
        assert env.episode_log_full() == env.num_envs and env.episode_log_summary()["complete"] is True
    finally:
        env.close()
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    for bad in (0, 65, -1, True, 2.0):
        with pytest.raises(ValueError, match="episode_log"):
            RoboyVecEnv(_robot("msj"), 8, episode_log=bad)


def test_an_env_without_the_option_is_the_env_it_was():
    from gym_roboy_amd.envs.options import env_checkpoint_record
    plain, logged = _env("msj", capacity=None, report_truncation=False), _env("msj", capacity=64, report_truncation=False)
    try:
        assert plain.episode_log_capacity == 0
        assert env_checkpoint_record(plain) == {"tendon_obs": {"channels": [], "scale": [1.0] * 4}, "env_io": {"sensor_noise": {}, "action_delay": None}}
        assert env_checkpoint_record(logged) == dict(env_checkpoint_record(plain), episode_log=64)
        assert plain.sim.dispatch("env_step")["id"] == logged.sim.dispatch("env_step")["id"]
        for call in (plain.episode_log, plain.episode_log_summary, plain.episode_log_full, plain.clear_episode_log):
            with pytest.raises(RuntimeError, match="keeps no episode log"):
                call()
        lib, p = nat.load(), [nat._vp() for _ in range(5)]
        assert lib.rb_env_episode_log_ptr(plain.sim.handle, *p, None) == nat.RB_EINVAL and b"episode log is not configured" in lib.rb_last_error()
        assert lib.rb_env_episode_log_clear(plain.sim.handle) == nat.RB_EINVAL
        assert lib.rb_env_episode_log_summary(plain.sim.handle, 1, (ctypes.c_double * 8)()) == nat.RB_EINVAL
        # obs, reward, done and the statistics of the two are the same: the log changes nothing a step reports
        acts = _scenario(plain)
        assert np.array_equal(_scenario(logged), acts)
        for a in acts:
            for x, y in zip(plain.step(a)[:3], logged.step(a)[:3]):
                assert x.tobytes() == y.tobytes()
        assert plain.stats() == logged.stats()
        assert logged.episode_log()["count"].max() <= 64 and logged.episode_log_full() == 0
    finally:
        plain.close(); logged.close()


def test_refusals_leave_the_handle_as_it_was():
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    lib = nat.load()
    sim = HipBatchSimulation(_robot("msj"), 64, seed=SEED)
    try:                                                             # without rb_env_configure
        assert lib.rb_env_episode_log_configure(sim.handle, 2) == nat.RB_EINVAL and b"rb_env_configure" in lib.rb_last_error()
    finally:
        sim.close()
    env = _env("msj")
    try:
        acts = _scenario(env)
        for a in acts[:8]:
            env.step(a)
        before, ptrs = _planes(env), env._episode_log_planes()
        assert before[0].any()
        for bad in (65, -1, 2 ** 20):
            assert lib.rb_env_episode_log_configure(env.sim.handle, bad) == nat.RB_EINVAL and b"RB_EPISODE_LOG_MAX" in lib.rb_last_error()
        assert env._episode_log_planes() == ptrs
        # the fused rollout ends its episodes inside one kernel
        ring = env.sim.malloc(4 * env.num_envs * env.n_t)
        env.sim.upload(ring, np.zeros((env.num_envs, env.n_t), np.float32))
        with pytest.raises(nat.NativeError, match="episode log"):
            env.sim.rollout_fused_dev(ring, 1, 1)
        for x, y in zip(before, _planes(env)):
            assert x.tobytes() == y.tobytes()
        # reconfigure()'s rule for a handle that holds captured graphs (the plain rollout caches them): they are dropped, the call
        # succeeds, and the handle goes on - a successful call starts with every plane zero
        env.sim.rollout_dev(ring, 1, 4)
        assert lib.rb_env_episode_log_configure(env.sim.handle, 5) == nat.RB_OK
        env.episode_log_capacity = 5
        assert all(not p.any() for p in _planes(env))
        env.sim.rollout_dev(ring, 1, 4)
        model = elu.EpisodeLogModel(env.num_envs, 5)
        env.reset()
        _steps(env, model, acts[8:], None)
        assert elu.same_log(env.episode_log(), model.log()) and model.count.any()
        # capacity 0 switches the option off
        assert lib.rb_env_episode_log_configure(env.sim.handle, 0) == nat.RB_OK
        assert lib.rb_env_episode_log_ptr(env.sim.handle, *[nat._vp() for _ in range(5)], None) == nat.RB_EINVAL
        env.sim.rollout_fused_dev(ring, 1, 1)
    finally:
        env.close()
