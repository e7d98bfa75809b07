"""Start poses behind the fused env step on the GPU (include/roboy_sim.h: rb_env_start_poses_*; csrc/env_start.hpp): the
draw against its restatement (tests/start_pose_util.py), an env with the option against a twin without that is handed the same poses
(everything bit-equal), start_prob 0 and 1, global ids and launch ranges, the other options, a captured graph, the refusals, PPO,
the trainer and evaluate_agent.

Shapes: 200 envs = one partial group of 256 lanes; 386 where a sub-range or two shards are needed (ranges start at multiples of 256);
episodes of 5 steps, 12 steps per run: two auto-resets per env; a pool of 7 rows.  tests/test_start_poses_cpu.py qualifies seed and
probability on the restated rule.  Without the option every test here fails at the constructor or the flag."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import push_util as pu
import start_pose_util as su
from env_io_util import sensor_noise64
from gym_roboy_amd import _native as nat
from start_pose_util import M, MAX_LEN, N, PROB, SEED, STEPS
from test_push_gpu import LANE, TWINS, WAVE, _select

pytestmark = pytest.mark.gpu

NOISE_TOL = 2e-3          # the project's bound on this fp32 Box-Muller expression, in sigmas (tests/test_env_io_gpu.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vec(which, n=N, integ="euler", start=True, seed=SEED, prob=PROB, pool=None, **kw):
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, desc = pu.robot_of(which)
    if start:
        kw.update(start_poses=su.pool_of(desc) if pool is None else pool, start_prob=prob)
    return RoboyVecEnv(robot, n, seed=seed, integrator=integ, max_episode_length=MAX_LEN, **kw)


def _acts(which, n=N, steps=STEPS, seed=1):
    desc = pu.robot_of(which)[1]
    return np.random.default_rng(seed).uniform(-1, 1, (steps, n, desc.n_t)).astype(np.float32)


def _twin_pair(which, integ="euler", kernel=None, **kw):
    a, b = _vec(which, integ=integ, **kw), _vec(which, integ=integ, start=False, **kw)
    for env in (a, b):
        _select(env, kernel)
    return a, b


# ---- 1. the draw ----
@pytest.mark.parametrize("which", ["baked", "upper"])
def test_the_draw_is_the_restated_one(which):
    desc = pu.robot_of(which)[1]
    nq, pool = desc.n_q, su.pool_of(desc)
    env, plain = _vec(which), _vec(which, start=False)
    try:
        assert env.start_poses_size == M and env.start_prob == PROB and plain.start_poses_size == 0
        assert np.array_equal(env.start_pose_pool(), pool)
        count, index = su.planes(env)
        assert not count.any() and np.all(index == su.INDEX_REST)      # a configuration clears the planes
        book = su.Book(SEED, N, su.threshold_of(PROB), M)
        obs, obs_plain = env.reset(), plain.reset()
        started = book.start()
        for t, act in enumerate([None] + list(_acts(which))):
            if act is not None:
                obs, _, done, _ = env.step(act)
                started = book.start(done)
            count, index = su.planes(env)
            assert np.array_equal(count, book.count) and np.array_equal(index, book.index), t
            assert np.array_equal(env.start_index(), index)
            q, qd, feas = env.sim.read_state()
            assert np.array_equal(q[started], pool[index[started].astype(np.int64)]), t      # the pool row, bit for bit
            assert not qd[started].any() and feas[started].all(), t
            assert np.array_equal(obs[:, :nq], q) and np.array_equal(obs[:, nq:2 * nq], qd), t      # the row's columns are the planes
            if act is None:                                          # every other lane is an env without the option
                rest = ~started
                assert started.any() and rest.any()
                assert np.array_equal(obs[rest], obs_plain[rest]) and np.array_equal(obs[:, 2 * nq:], obs_plain[:, 2 * nq:])
                for x, y in zip((q, qd, feas), plain.sim.read_state()):
                    assert np.array_equal(x[rest], y[rest])
        assert book.count.min() >= 3                                  # the reset and two auto-resets
    finally:
        env.close(); plain.close()


# ---- 2. the twin, bit for bit ----
@pytest.mark.parametrize("which,integ,kernel", TWINS)
def test_a_twin_handed_the_poses_steps_bit_for_bit(which, integ, kernel, monkeypatch):
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")                         # (a kernarg robot runs its kernarg row)
    desc = pu.robot_of(which)[1]
    a, b = _twin_pair(which, integ, kernel)
    try:
        assert a.sim.dispatch("env_step")["id"] == b.sim.dispatch("env_step")["id"]
        n_done, from_pool, at_rest = su.twin_steps(a, b, _acts(which), su.pool_of(desc))
        print(a.sim.dispatch("env_step")["id"], "starts from the pool %d, at rest %d" % (from_pool, at_rest))
        assert n_done.min() >= 2 and from_pool > N // 2 and at_rest > N // 2
    finally:
        a.close(); b.close()


# ---- 3. start_prob 0 and 1 ----
def _outputs(env, act):
    return env.step(act)[:3] + tuple(env.sim.read_state())


@pytest.mark.parametrize("which", ["baked", "upper"])
def test_start_prob_0_is_an_env_without_the_option(which):
    env, plain = _vec(which, prob=0.0), _vec(which, start=False)
    try:
        assert env.start_poses_size == M and env.start_prob == 0.0
        assert np.array_equal(env.reset(), plain.reset())
        n_done = np.zeros(N, int)
        for act in _acts(which):
            ra, rb = _outputs(env, act), _outputs(plain, act)
            for x, y in zip(ra, rb):
                assert np.array_equal(x, y)
            n_done += ra[2]
            count, index = su.planes(env)
            assert np.all(index == su.INDEX_REST) and np.array_equal(count, 1 + n_done)      # counted, never drawn
        assert n_done.min() >= 2 and env.stats() == plain.stats()
    finally:
        env.close(); plain.close()


@pytest.mark.parametrize("which", ["baked", "upper"])
def test_start_prob_1_starts_every_episode_from_the_pool(which):
    desc = pu.robot_of(which)[1]
    pool = su.pool_of(desc)
    env = _vec(which, prob=1.0)
    try:
        env.reset()
        book = su.Book(SEED, N, 2 ** 24, M)
        book.start()
        for act in _acts(which, steps=6):
            book.start(env.step(act)[2])
            count, index = su.planes(env)
            assert np.all(index < M) and np.array_equal(index, book.index) and np.array_equal(count, book.count)
        assert book.count.min() >= 2
        assert set(index.tolist()) == set(range(M))
    finally:
        env.close()


# ---- 4. global ids and ranges ----
def _run(env, acts):
    out = [(env.reset(),) + tuple(env.sim.read_state()) + su.planes(env)]
    for act in acts:
        out.append(env.step(act)[:3] + tuple(env.sim.read_state()) + su.planes(env))
    return out


@pytest.mark.parametrize("which", ["baked", "upper"])
def test_two_shards_are_the_whole_batch(which):
    n, half = 386, 193
    acts = _acts(which, n=n)
    runs = []
    for cnt, off, sl in ((n, 0, slice(0, n)), (half, 0, slice(0, half)), (half, half, slice(half, n))):
        env = _vec(which, n=cnt, env_id_offset=off)
        try:
            _select(env, LANE)
            runs.append(_run(env, acts[:, sl]))
        finally:
            env.close()
    whole, lo, hi = runs
    for t in range(STEPS + 1):
        for k, x in enumerate(whole[t]):
            assert np.array_equal(x, np.concatenate((lo[t][k], hi[t][k]))), (t, k)
    index = whole[-1][-1]
    assert (index[:half] != su.INDEX_REST).any() and (index[half:] != su.INDEX_REST).any()


@pytest.mark.parametrize("which", ["baked", "upper"])
def test_two_ranges_on_two_streams_are_the_whole_batch(which):
    import torch
    n, split = 386, 256
    acts = _acts(which, n=n)
    whole, halves = _vec(which, n=n), _vec(which, n=n)
    try:
        for env in (whole, halves):
            _select(env, LANE)
        assert np.array_equal(whole.reset(), halves.reset())
        assert halves.range_capable()
        desc = pu.robot_of(which)[1]
        d = [halves.sim.malloc(4 * n * desc.n_t), halves.sim.malloc(4 * n * halves.obs_dim), halves.sim.malloc(4 * n), halves.sim.malloc(4 * n)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        n_done = np.zeros(n, int)
        for t, act in enumerate(acts):
            obs, rew, done, _ = whole.step(act)
            halves.sim.upload(d[0], act)
            halves.sim.synchronize()
            halves.step_range_dev(0, split, streams[0].cuda_stream, *d)
            halves.step_range_dev(split, n - split, streams[1].cuda_stream, *d)
            for s in streams:
                s.synchronize()
            got = (halves.sim.download(d[1], (n, halves.obs_dim)), halves.sim.download(d[2], (n,)), halves.sim.download(d[3], (n,), np.uint32) != 0)
            for k, (x, y) in enumerate(zip((obs, rew, done), got)):
                assert np.array_equal(x, y), (t, k)
            for k, (x, y) in enumerate(zip(su.planes(whole) + tuple(whole.sim.read_state()), su.planes(halves) + tuple(halves.sim.read_state()))):
                assert np.array_equal(x, y), (t, k)
            n_done += done
        index = su.planes(whole)[1]
        assert n_done.min() >= 2 and (index[:split] != su.INDEX_REST).any() and (index[split:] != su.INDEX_REST).any()
    finally:
        whole.close(); halves.close()


def test_a_refused_sub_range_moves_no_plane():
    env = _vec("upper", prob=1.0)
    try:
        _select(env, WAVE)                                           # a whole-batch-only form
        env.reset()
        assert not env.range_capable()
        acts = _acts("upper", steps=2)
        env.step(acts[0])
        before = su.planes(env) + tuple(env.sim.read_state())
        d = [env.sim.malloc(4 * N * env.n_t), env.sim.malloc(4 * N * env.obs_dim), env.sim.malloc(4 * N), env.sim.malloc(4 * N)]
        env.sim.upload(d[0], acts[1])
        with pytest.raises(nat.NativeError, match="whole batches only"):
            env.step_range_dev(0, 64, None, *d)
        for x, y in zip(before, su.planes(env) + tuple(env.sim.read_state())):
            assert np.array_equal(x, y)
    finally:
        env.close()


# ---- 5. with the other options, against the twin ----
def _goal_pool(desc, m=64, seed=2):
    """m poses inside 0.5 of the joint box, ordered by distance from rest (a curriculum takes the row order for difficulty order)"""
    rows = np.random.default_rng(seed).uniform(0.5 * desc.q_lo, 0.5 * desc.q_hi, (m, desc.n_q)).astype(np.float32)
    return rows[np.argsort(np.linalg.norm(rows, axis=1))]


def _log(env):
    log = env.episode_log()
    return tuple(log[k] for k in ("count", "return", "length", "kind"))


def test_every_ball_joint_option_together():
    from gym_roboy_amd.envs.params import ParamRanges
    from test_env_obs_gpu import RANGES
    desc = pu.robot_of("baked")[1]
    nq = desc.n_q
    kw = dict(randomization=ParamRanges(**RANGES), action_delay=(0, 3), action_obs=2, critic_obs=("state", "age"), report_truncation=True,
              goals=_goal_pool(desc), goal_curriculum={"levels": 4, "up": 1, "down": 1}, goal_row_stats=True,
              reward_shaping={"action_rate": 0.1}, push={"prob": 0.25, "sigma": pu.sigma_of(desc)}, episode_log=4)
    a, b = _twin_pair("baked", "rk4", None, **kw)
    try:
        def extra(env, started):
            rows = env.critic_obs().copy()
            if env is a:                                             # the privileged row reports the true start pose: the planes
                q, qd, _ = env.sim.read_state()
                assert np.array_equal(rows[:, :nq], q) and np.array_equal(rows[:, nq:2 * nq], qd)
                assert not started.any() or rows[started, :nq].any()
            rows[started, :2 * nq] = 0                               # (the twin's row was written before it was handed the pose)
            stats = env.goal_row_stats()
            return (rows, env.truncated(), env.shaping_cost(), env.goal_levels(), env.goal_index(), env.get_action_delay(),
                    stats["attempts"], stats["reached"], pu.planes(env)[3]) + _log(env)
        n_done, from_pool, at_rest = su.twin_steps(a, b, _acts("baked"), su.pool_of(desc), extra)
        assert n_done.min() >= 2 and from_pool > 0 and at_rest > 0
        assert a.stats() == b.stats() and a.shaping_stats() == b.shaping_stats() and a.push_count() == b.push_count() > 0
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("which,integ", [("baked", "euler"), ("kernarg", "rk4"), ("ball12", "euler")])
def test_sensor_noise_on_the_replaced_columns_is_the_rows_own(which, integ, monkeypatch):
    """Both envs carry the noise; the twin's rows show it on the zero pose.  The replaced columns must be the pose plus the float64
    restatement of the noise of that row number (0 at the reset, t + 1 behind step t) within NOISE_TOL sigmas, every other column
    bit-equal; the critic rows report the pose without noise."""
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    desc = pu.robot_of(which)[1]
    nq = desc.n_q
    sigma = {"q": 0.01, "qd": 0.05}
    colsig = np.asarray([sigma["q"]] * nq + [sigma["qd"]] * nq, np.float64)
    a, b = _twin_pair(which, integ, None, sensor_noise=sigma, critic_obs=("state",))
    worst = [0.0]

    def rows(obs_a, obs_b, started, index, pool, n_q, where):
        rep = su.replaced(started, n_q, obs_a.shape[1])
        assert np.array_equal(obs_a[~rep], obs_b[~rep]), where
        if not started.any():                                        # (a step that ended no episode)
            return
        r = 0 if where == "reset" else where + 1
        z = sensor_noise64(SEED, np.arange(N, dtype=np.uint64), r, 2 * n_q)
        value = np.concatenate((pool[index[started].astype(np.int64)].astype(np.float64), np.zeros((int(started.sum()), n_q))), axis=1)
        err = np.abs(obs_a[started, :2 * n_q].astype(np.float64) - (value + colsig * z[started])) / colsig
        worst[0] = max(worst[0], err.max())
        print(which, where, "started %d, max |row - (pose + sigma z64)| / sigma = %.3g" % (started.sum(), err.max()))
        assert np.all(err <= NOISE_TOL), where
        assert np.mean(obs_a[started, :2 * n_q] != value.astype(np.float32)) > 0.99      # noised
        # the same noise as the twin's row carries on the zero pose, to the last few bits of the larger value
        assert np.allclose(obs_a[started, :2 * n_q].astype(np.float64) - value, obs_b[started, :2 * n_q], rtol=0, atol=1e-6)

    def extra(env, started):
        c = env.critic_obs().copy()
        if env is a:
            q, qd, _ = env.sim.read_state()
            assert np.array_equal(c[:, :nq], q) and np.array_equal(c[:, nq:2 * nq], qd)
        c[started, :2 * nq] = 0
        return (c,)
    try:
        n_done, from_pool, at_rest = su.twin_steps(a, b, _acts(which), su.pool_of(desc), extra, rows=rows)
        assert n_done.min() >= 2 and from_pool > 0 and at_rest > 0 and worst[0] > 0
    finally:
        a.close(); b.close()


def test_sigma_0_is_exact():
    desc = pu.robot_of("baked")[1]
    a, b = _twin_pair("baked", "euler", None, sensor_noise={"q": 0.0, "qd": 0.0}, action_delay=1)
    try:
        n_done, from_pool, at_rest = su.twin_steps(a, b, _acts("baked"), su.pool_of(desc))      # (check_rows: [pose, 0] exactly)
        assert n_done.min() >= 2 and from_pool > 0
    finally:
        a.close(); b.close()


def test_noise_on_one_block_only():
    """sigma on qd alone: block 0 holds q0..q2 and qd0, block 1 qd1, qd2 - q stays the pool's bits"""
    desc = pu.robot_of("baked")[1]
    nq = desc.n_q
    a, b = _twin_pair("baked", "euler", None, sensor_noise={"qd": 0.05})

    def rows(obs_a, obs_b, started, index, pool, n_q, where):
        rep = su.replaced(started, n_q, obs_a.shape[1])
        assert np.array_equal(obs_a[~rep], obs_b[~rep]), where
        assert np.array_equal(obs_a[started, :n_q], pool[index[started].astype(np.int64)]), where
        assert np.array_equal(obs_a[started, n_q:2 * n_q], obs_b[started, n_q:2 * n_q]), where      # 0 + sigma z: the step's own bits
    try:
        n_done, from_pool, _ = su.twin_steps(a, b, _acts("baked"), su.pool_of(desc), rows=rows)
        assert n_done.min() >= 2 and from_pool > 0
    finally:
        a.close(); b.close()


def test_the_upper_body_with_pool_goals_shaping_pushes_and_the_log():
    desc = pu.robot_of("upper")[1]
    kw = dict(goals=_goal_pool(desc), reward_shaping={"action_rate": 0.1, "tension": 0.05, "activation": 0.02},
              push={"prob": 0.25, "sigma": pu.sigma_of(desc)}, episode_log=4, report_truncation=True)
    a, b = _twin_pair("upper", "euler", None, **kw)
    try:
        extra = lambda env, started: (env.shaping_cost(), env.truncated(), pu.planes(env)[3]) + _log(env)
        n_done, from_pool, at_rest = su.twin_steps(a, b, _acts("upper"), su.pool_of(desc), extra)
        assert n_done.min() >= 2 and from_pool > 0 and at_rest > 0
        assert a.stats() == b.stats() and a.shaping_stats() == b.shaping_stats()
    finally:
        a.close(); b.close()


# ---- 6. a captured graph ----
@pytest.mark.parametrize("which", ["baked", "upper"])
def test_a_captured_graph_replays_like_eager_and_reads_new_rows(which):
    import torch
    desc = pu.robot_of(which)[1]
    pool = su.pool_of(desc)
    other = su.pool_of(desc, seed=9)
    eager, env = _vec(which), _vec(which)
    try:
        assert np.array_equal(eager.reset(), env.reset())
        dev = torch.device("cuda", 0)
        T = 3
        acts_np = _acts(which, steps=T)
        acts = torch.from_numpy(acts_np).to(dev)
        obs = torch.zeros((T, N, env.obs_dim), device=dev)
        rew, done = torch.zeros((T, N), device=dev), torch.zeros((T, N), dtype=torch.int32, device=dev)
        side = torch.cuda.Stream(device=dev)
        env.set_stream(side.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for k in range(T):
                env.step_dev(acts[k].data_ptr(), obs[k].data_ptr(), rew[k].data_ptr(), done[k].data_ptr())
        n_done = np.zeros(N, int)
        for replay in range(6):
            if replay == 4:                                          # other rows, in place: no new capture
                eager.set_start_poses(other)
                env.set_start_poses(other)
                assert np.array_equal(env.start_pose_pool(), other)
            graph.replay()
            torch.cuda.synchronize()
            got = (obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy() != 0)
            for k in range(T):
                want = eager.step(acts_np[k])[:3]
                for j, (x, y) in enumerate(zip(want, (got[0][k], got[1][k], got[2][k]))):
                    assert np.array_equal(x, y), (replay, k, j)
                n_done += want[2]
            for x, y in zip(su.planes(eager) + tuple(eager.sim.read_state()), su.planes(env) + tuple(env.sim.read_state())):
                assert np.array_equal(x, y), replay
            if replay == 4:
                # steps 13 to 15 of episodes that are 5 steps long: the replay's last step ended every episode, and the lanes it
                # started from the pool hold rows of `other` - the graph read the new rows without a new capture
                index = su.planes(env)[1]
                lanes = got[2][T - 1] & (index != su.INDEX_REST)
                assert lanes.sum() > N // 4
                assert np.array_equal(env.sim.read_state()[0][lanes], other[index[lanes].astype(np.int64)])
        assert n_done.min() >= 3 and not np.array_equal(other, pool)
    finally:
        eager.close(); env.close()


# ---- 7. refusals ----
def _configure(env_or_sim, rows, m, prob):
    handle = getattr(env_or_sim, "handle", None) or env_or_sim.sim.handle
    return nat.load().rb_env_start_poses_configure(handle, None if rows is None else nat.fptr(rows), m, prob)


def _ptr(handle):
    p = [nat._vp() for _ in range(3)]
    m = ctypes.c_int64()
    return nat.load().rb_env_start_poses_ptr(handle, ctypes.byref(p[0]), ctypes.byref(m), ctypes.byref(p[1]), ctypes.byref(p[2])), [x.value for x in p], m.value


def test_refusals_leave_the_handle_as_it_was():
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    robot, desc = pu.robot_of("baked")
    lib = nat.load()
    pool = su.pool_of(desc)
    # without rb_env_configure
    sim = HipBatchSimulation(robot, N, seed=SEED)
    try:
        assert _configure(sim, pool, M, 0.5) == nat.RB_EINVAL and b"rb_env_configure" in lib.rb_last_error()
        assert _ptr(sim.handle)[0] == nat.RB_EINVAL and b"start poses are not configured" in lib.rb_last_error()
        assert lib.rb_env_start_poses_set(sim.handle, nat.fptr(pool), M) == nat.RB_EINVAL and b"start poses are not configured" in lib.rb_last_error()
    finally:
        sim.close()
    env = _vec("baked")
    try:
        env.reset()
        acts = _acts("baked", steps=3)
        env.step(acts[0])
        rc, ptrs, m = _ptr(env.sim.handle)
        assert rc == nat.RB_OK and all(ptrs) and m == M
        before = su.planes(env) + (env.start_pose_pool(),)
        row = env.sim.dispatch("env_step")["id"]
        outside = pool.copy()
        outside[3, 1] = np.float32(desc.q_hi[1]) * np.float32(1.01)
        nan = pool.copy()
        nan[0, 0] = np.nan
        for rows, count, prob, text in ((pool, -1, 0.5, b"m must be >= 1"), (pool, M, -0.01, b"prob must be in [0, 1]"),
                                        (pool, M, 1.5, b"prob must be in [0, 1]"), (pool, M, float("nan"), b"prob must be in [0, 1]"),
                                        (outside, M, 0.5, b"row 3, joint 1 is not finite or outside the joint limits"),
                                        (nan, M, 0.5, b"row 0, joint 0 is not finite"), (None, M, 0.5, b"null argument")):
            assert _configure(env, rows, count, prob) == nat.RB_EINVAL and text in lib.rb_last_error(), text
        for rows, count, text in ((pool[:5].copy(), 5, b"has 7 rows, fixed by rb_env_start_poses_configure; got 5"),
                                  (outside, M, b"outside the joint limits"), (None, M, b"null argument")):
            rc = lib.rb_env_start_poses_set(env.sim.handle, None if rows is None else nat.fptr(rows), count)
            assert rc == nat.RB_EINVAL and text in lib.rb_last_error(), text
        with pytest.raises(ValueError, match="has 7 rows"):
            env.set_start_poses(pool[:5])
        with pytest.raises(ValueError, match="start_poses: goals must lie inside"):
            env.set_start_poses(outside)
        # tendon channels, asked second
        assert lib.rb_env_obs_configure(env.sim.handle, 1, None) == nat.RB_EUNSUPPORTED
        assert b"start poses and tendon channels in the observation do not combine" in lib.rb_last_error()
        # the fused rollout resets inside one kernel
        ring = env.sim.malloc(4 * N * desc.n_t)
        with pytest.raises(nat.NativeError, match="cannot start them at poses from a pool"):
            env.sim.rollout_fused_dev(ring, 1, 1)
        assert _ptr(env.sim.handle)[1] == ptrs and env.sim.dispatch("env_step")["id"] == row
        for x, y in zip(before, su.planes(env) + (env.start_pose_pool(),)):
            assert np.array_equal(x, y)
        # the handle steps on as configured: the next starts are the restated ones
        done = env.step(acts[1])[2]
        count, index = su.planes(env)
        assert np.array_equal(index[done], su.index_of(SEED, np.arange(N), before[0], su.threshold_of(PROB), M)[done])
        assert np.array_equal(count, before[0] + done)
        # the planes stand through a statistics reset; a successful call clears them; m = 0 switches the option off
        env.stats(reset=True)
        assert np.array_equal(su.planes(env)[0], count)
        assert _configure(env, pool, M, 1.0) == nat.RB_OK
        count, index = su.planes(env)
        assert not count.any() and np.all(index == su.INDEX_REST) and _ptr(env.sim.handle)[1] == ptrs
        assert _configure(env, None, 0, 0.0) == nat.RB_OK
        assert _ptr(env.sim.handle)[0] == nat.RB_EINVAL and env.sim.dispatch("env_step")["id"] == row
    finally:
        env.close()


def test_tendon_channels_asked_first_and_the_accessors_of_an_env_without_the_option():
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, desc = pu.robot_of("baked")
    lib = nat.load()
    pool = su.pool_of(desc)
    with pytest.raises(ValueError, match="start_poses does not combine with tendon_obs"):
        RoboyVecEnv(robot, N, tendon_obs=("length",), start_poses=pool)
    with pytest.raises(ValueError, match="start_prob needs start_poses"):
        RoboyVecEnv(robot, N, start_prob=0.5)
    with pytest.raises(ValueError, match="start_prob must be in"):
        RoboyVecEnv(robot, N, start_poses=pool, start_prob=1.5)
    env = RoboyVecEnv(robot, N, seed=SEED, tendon_obs=("length",), max_episode_length=MAX_LEN)
    try:
        assert _configure(env, pool, M, 0.5) == nat.RB_EUNSUPPORTED
        assert b"start poses and tendon channels in the observation do not combine" in lib.rb_last_error()
        assert _ptr(env.sim.handle)[0] == nat.RB_EINVAL
        for call in (env.start_pose_pool, env.start_index, env.start_count, lambda: env.set_start_poses(pool)):
            with pytest.raises(RuntimeError, match="start_poses=None"):
                call()
        assert env.start_poses_size == 0 and env.start_prob == 1.0
    finally:
        env.close()


def test_start_index_numpy_and_torch_paths():
    import torch
    env = _vec("baked")
    try:
        env.reset()
        acts = _acts("baked", steps=2)
        env.step(acts[0])
        index = env.start_index()
        assert isinstance(index, np.ndarray) and index.dtype == np.uint32 and index.shape == (N,)
        env.step(torch.from_numpy(acts[1]).cuda())
        view = env.start_index()
        assert view.is_cuda and view.dtype == torch.int32 and tuple(view.shape) == (N,)
        torch.cuda.synchronize()
        assert np.array_equal(view.cpu().numpy().astype(np.uint32), su.planes(env)[1])
    finally:
        env.close()


# ---- 8. PPO, the trainer, evaluate_agent ----
@pytest.mark.parametrize("use_graphs", [True, False])
def test_ppo_rounds_with_start_poses_and_the_checkpoint_records_them(use_graphs, tmp_path):
    import torch
    from gym_roboy_amd.ppo import PPO
    n, T = 256, 8
    desc = pu.robot_of("baked")[1]
    pool = su.pool_of(desc)
    for start in (True, False):
        torch.manual_seed(0)
        env = _vec("baked", n=n, start=start)
        try:
            agent = PPO(env, n_steps=T, use_graphs=use_graphs, reward_scale=0.01, seed=0, device="cuda")
            for _ in range(2):
                stats = agent.update(agent.collect())
            torch.cuda.synchronize()
            assert isinstance(stats, dict)
            path = str(tmp_path / ("start%d.pkl" % start))
            agent.save(path)
            ck = torch.load(path)
            if start:
                count, index = su.planes(env)
                assert count.min() >= (2 * T) // MAX_LEN and (index != su.INDEX_REST).any() and (index == su.INDEX_REST).any()
                rec = ck["env_start_poses"]
                assert sorted(rec) == ["prob", "q", "recipe", "threshold"] and rec["prob"] == PROB and rec["threshold"] == su.threshold_of(PROB)
                assert np.array_equal(rec["q"].numpy(), pool) and rec["recipe"] == {}
                agent.load(path)
                assert agent.checkpoint_env_start_poses["prob"] == PROB
            else:
                assert "env_start_poses" not in ck
        finally:
            env.close()


def test_train_parallel_prints_the_share_and_evaluate_agent_takes_the_flag(tmp_path):
    run = lambda *argv: subprocess.run([sys.executable, "-m"] + list(argv), cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = run("gym_roboy_amd.train_parallel", "256", str(tmp_path / "results"), "--rounds", "2", "--steps-per-round", str(256 * 8), "--n-steps", "8",
              "--start-poses", "reachable:64", "--start-prob", "0.5")
    assert out.returncode == 0, out.stdout + out.stderr
    shares = [float(x) for x in re.findall(r"'start_pool_share': ([0-9.e+-]+)", out.stdout)]
    assert len(shares) == 2, out.stdout
    # 256 envs at P = 0.5: the share lies within five standard deviations of it
    assert all(abs(s - 0.5) < 5 * (0.25 / 256) ** 0.5 for s in shares), shares
    import torch
    model = str(tmp_path / "results" / "model.pkl")
    rec = torch.load(model)["env_start_poses"]
    assert rec["prob"] == 0.5 and rec["threshold"] == 2 ** 23 and tuple(rec["q"].shape) == (64, 3) and rec["recipe"]["seed"] == 1
    report = str(tmp_path / "eval.json")
    out = run("gym_roboy_amd.evaluate_agent", model, "--envs", "256", "--episodes", "1", "--max-episode-length", "20", "--json", report,
              "--start-poses", "reachable:64")
    assert out.returncode == 0, out.stdout + out.stderr
    summary = json.loads(out.stdout.strip().splitlines()[-1])
    assert summary["n_records"] == 256 and summary["complete"]
    with open(report) as f:
        said = json.load(f)
    assert said["flags"] == ["--start-poses"] and said["conditions"]["start_poses"] == {"rows": [64, 3]} and said["conditions"]["start_prob"] == 1.0
