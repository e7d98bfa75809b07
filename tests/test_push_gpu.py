"""Random velocity pushes in front of the fused env step on the GPU (include/roboy_sim.h: rb_env_push_*; csrc/env_push.hpp; DESIGN.md
§28): the draw against its restatement (tests/push_util.py), an env with pushes against a twin without that is handed the same impulses
(everything bit-equal), global ids and launch ranges, off = the parent, the other options, a captured graph, the refusals,
RoboyVecEnv's accessors, PPO and the trainer.

Shapes: 200 envs = one partial group of 256 lanes; 386 where a sub-range is needed (ranges start at multiples of 256); episodes of 5
steps, 12 steps per run: two auto-resets per env.  tests/test_push_cpu.py qualifies seed and probability on the restated rule.
The hiprtc-built ball-joint instances serve batches above 65 536 envs only and are not run here (as in tests/test_env_io_gpu.py)."""
import ctypes

import numpy as np
import pytest

import push_util as pu
from gym_roboy_amd import _native as nat
from push_util import MAX_LEN, N, NOISE_TOL, PROB, SEED, STEPS

pytestmark = pytest.mark.gpu

LANE, OCTET, WAVE, SPLIT, PAIR, SPLIT2 = 1, 2, 3, 4, 5, 6


def _vec(which, n=N, integ="euler", push=True, seed=SEED, prob=PROB, **kw):
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot, desc = pu.robot_of(which)
    if push is True:
        push = {"prob": prob, "sigma": pu.sigma_of(desc)}
    return RoboyVecEnv(robot, n, seed=seed, integrator=integ, max_episode_length=MAX_LEN, push=push or None, **kw)


def _acts(which, n=N, steps=STEPS, seed=1):
    desc = pu.robot_of(which)[1]
    return np.random.default_rng(seed).uniform(-1, 1, (steps, n, desc.n_t)).astype(np.float32)


def _select(env, kernel):
    if kernel is not None:
        env.sim.select_kernel(kernel)
        assert env.sim.dispatch("env_step")["kernel"] == kernel


# ---- 1. the draw ----
@pytest.mark.parametrize("which", ["baked", "upper"])
def test_the_draw_is_the_restated_one(which):
    desc = pu.robot_of(which)[1]
    sigma = np.asarray(pu.sigma_of(desc), np.float64)
    env = _vec(which)
    try:
        env.reset()
        book = pu.Book(SEED, N, pu.threshold_of(PROB))
        before = pu.planes(env)
        assert all(not p.any() for p in before)                      # a configuration zeroes all four planes
        for t, act in enumerate(_acts(which)):
            env.step(act)
            count, last, n_pushes, imp = pu.planes(env)
            pushed, m = book.step()
            assert np.array_equal(last == count, pushed), t
            assert np.array_equal(count, book.count) and np.array_equal(last, book.last) and np.array_equal(n_pushes, book.n_pushes), t
            ref = sigma * pu.z64(SEED, book.gids, m, desc.n_q)
            err = np.abs(imp.astype(np.float64) - ref)[pushed]
            print(which, t, "pushed %d, max |impulse - sigma z64| / sigma = %.3g" % (pushed.sum(), (err / sigma).max()))
            assert np.all(err <= sigma * NOISE_TOL), t
            assert np.array_equal(imp[~pushed], before[3][~pushed]), t          # unpushed rows keep their content
            before = (count, last, n_pushes, imp)
            pushed_v, imp_v = env.last_push()
            assert np.array_equal(pushed_v, pushed) and np.array_equal(imp_v, imp)
        assert env.push_count() == int(book.n_pushes.sum())
    finally:
        env.close()


# ---- 2. the twin, bit for bit ----
TWINS = [("baked", i, k) for i in ("euler", "rk4") for k in (LANE, OCTET, PAIR)] + \
        [(w, i, LANE if w == "kernarg" else None) for w in ("kernarg", "ball12") for i in ("euler", "rk4")] + \
        [("upper", "euler", k) for k in (WAVE, LANE, SPLIT, SPLIT2)] + [("upper", "rk4", k) for k in (WAVE, LANE, SPLIT)]


def _twin_pair(which, integ, kernel, **kw):
    a, b = _vec(which, integ=integ, **kw), _vec(which, integ=integ, push=False, **kw)
    for env in (a, b):
        _select(env, kernel)
        env.reset()
    return a, b


@pytest.mark.parametrize("which,integ,kernel", TWINS)
def test_a_twin_handed_the_impulses_steps_bit_for_bit(which, integ, kernel, monkeypatch):
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")                         # (a kernarg robot runs its kernarg row)
    desc = pu.robot_of(which)[1]
    a, b = _twin_pair(which, integ, kernel)
    try:
        assert a.sim.dispatch("env_step")["id"] == b.sim.dispatch("env_step")["id"]
        n_done, clamped, free, pushes = pu.twin_steps(a, b, _acts(which), desc.qd_max)
        print(a.sim.dispatch("env_step")["id"], "pushes %d, joints the clamp changed %d, left alone %d" % (pushes, clamped, free))
        assert n_done.min() >= 2                                     # every env auto-reset twice
        assert clamped > 0 and free > 0                              # both cases of the clamp were exercised
    finally:
        a.close(); b.close()


# ---- 3. global ids and ranges ----
def _run(env, acts):
    env.reset()
    out = []
    for act in acts:
        out.append(env.step(act)[:3] + tuple(env.sim.read_state()) + pu.planes(env))
    return out


@pytest.mark.parametrize("which", ["baked", "upper"])
def test_two_shards_are_the_whole_batch(which):
    acts = _acts(which)
    runs = []
    for n, off, sl in ((N, 0, slice(0, N)), (96, 0, slice(0, 96)), (104, 96, slice(96, N))):
        env = _vec(which, n=n, env_id_offset=off)
        try:
            _select(env, LANE)
            runs.append(_run(env, acts[:, sl]))
        finally:
            env.close()
    whole, lo, hi = runs
    for t in range(STEPS):
        for k, x in enumerate(whole[t]):
            assert np.array_equal(x, np.concatenate((lo[t][k], hi[t][k]))), (t, k)
    assert whole[-1][8].sum() > 0


@pytest.mark.parametrize("which", ["baked", "upper"])
def test_two_ranges_on_two_streams_are_the_whole_batch(which):
    import torch
    n, split = 386, 256
    acts = _acts(which, n=n, steps=4)
    whole = _vec(which, n=n)
    halves = _vec(which, n=n)
    try:
        for env in (whole, halves):
            _select(env, LANE)
            env.reset()
        assert halves.range_capable()
        desc = pu.robot_of(which)[1]
        d = [halves.sim.malloc(4 * n * desc.n_t), halves.sim.malloc(4 * n * halves.obs_dim), halves.sim.malloc(4 * n), halves.sim.malloc(4 * n)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
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
            for k, (x, y) in enumerate(zip(pu.planes(whole) + tuple(whole.sim.read_state()), pu.planes(halves) + tuple(halves.sim.read_state()))):
                assert np.array_equal(x, y), (t, k)
        assert pu.planes(whole)[2].sum() > 0
    finally:
        whole.close(); halves.close()


def test_a_refused_sub_range_moves_neither_counters_nor_velocities():
    env = _vec("upper", prob=1.0)
    try:
        _select(env, WAVE)                                           # a whole-batch-only form
        env.reset()
        assert not env.range_capable()
        acts = _acts("upper", steps=2)
        env.step(acts[0])
        before = pu.planes(env) + (pu.read_qd(env),)
        assert np.all(before[0] == 1) and np.all(before[1] == 1)
        d = [env.sim.malloc(4 * N * env.n_t), env.sim.malloc(4 * N * env.obs_dim), env.sim.malloc(4 * N), env.sim.malloc(4 * N)]
        env.sim.upload(d[0], acts[1])
        with pytest.raises(nat.NativeError, match="whole batches only"):
            env.step_range_dev(0, 64, None, *d)
        for x, y in zip(before, pu.planes(env) + (pu.read_qd(env),)):
            assert np.array_equal(x, y)
    finally:
        env.close()


# ---- 4. off is the parent ----
@pytest.mark.parametrize("how", ["threshold0", "sigma0", "null"])
def test_off_is_a_handle_without_the_option(how):
    desc = pu.robot_of("baked")[1]
    env, plain = _vec("baked", push=False), _vec("baked", push=False)
    try:
        if how == "threshold0":
            assert pu.configure(nat, env, pu.push_cfg(nat, 0, pu.sigma_of(desc))) == nat.RB_OK
        elif how == "sigma0":
            assert pu.configure(nat, env, pu.push_cfg(nat, 2 ** 24, [0.0] * desc.n_q)) == nat.RB_OK
        else:
            assert pu.configure(nat, env, pu.push_cfg(nat, 2 ** 24, pu.sigma_of(desc))) == nat.RB_OK
            p = [nat._vp() for _ in range(4)]
            assert nat.load().rb_env_push_ptr(env.sim.handle, *p) == nat.RB_OK and all(x.value for x in p)
            assert pu.configure(nat, env, None) == nat.RB_OK
        assert env.sim.dispatch("env_step")["id"] == plain.sim.dispatch("env_step")["id"]
        p = [nat._vp() for _ in range(4)]
        assert nat.load().rb_env_push_ptr(env.sim.handle, *p) == nat.RB_EINVAL
        env.reset(); plain.reset()
        for act in _acts("baked", steps=6):
            for x, y in zip(env.step(act)[:3] + tuple(env.sim.read_state()), plain.step(act)[:3] + tuple(plain.sim.read_state())):
                assert np.array_equal(x, y)
    finally:
        env.close(); plain.close()


# ---- 5. with the other options ----
def _pool(desc, m=64, seed=2):
    """m poses inside 0.5 of the joint box, ordered by distance from rest (a curriculum takes the row order for difficulty order)"""
    rows = np.random.default_rng(seed).uniform(0.5 * desc.q_lo, 0.5 * desc.q_hi, (m, desc.n_q)).astype(np.float32)
    return rows[np.argsort(np.linalg.norm(rows, axis=1))]


def _goal_planes(env):
    """the curriculum's planes (the goal itself is in the observation rows, columns 2 n_q .. 3 n_q, which no noise touches)"""
    return (env.goal_levels(), env.goal_index()) if env.goal_curriculum else ()


def test_every_ball_joint_option_together():
    from gym_roboy_amd.envs.params import ParamRanges
    from test_env_obs_gpu import RANGES
    desc = pu.robot_of("baked")[1]
    kw = dict(randomization=ParamRanges(**RANGES), tendon_obs=("length", "force"), sensor_noise={"q": 0.01, "qd": 0.05},
              action_delay=(0, 3), action_obs=2, critic_obs=("state", "age", "params", "delay", "actions"), report_truncation=True,
              goals=_pool(desc), goal_curriculum={"levels": 4, "up": 1, "down": 1}, reward_shaping={"action_rate": 0.1})
    a, b = _twin_pair("baked", "rk4", None, **kw)
    try:
        extra = lambda env: (env.critic_obs(), env.truncated(), env.shaping_cost()) + _goal_planes(env)
        n_done, clamped, free, pushes = pu.twin_steps(a, b, _acts("baked"), desc.qd_max, extra)
        assert n_done.min() >= 2 and clamped > 0 and free > 0
        assert a.stats() == b.stats() and a.shaping_stats() == b.shaping_stats()
    finally:
        a.close(); b.close()


def test_the_upper_body_with_pool_goals_and_all_shaping_terms():
    desc = pu.robot_of("upper")[1]
    kw = dict(goals=_pool(desc), reward_shaping={"action_rate": 0.1, "tension": 0.05, "activation": 0.02})
    a, b = _twin_pair("upper", "euler", None, **kw)
    try:
        # equal costs pin the order "push, then cost": the tension and activation terms read the velocities
        extra = lambda env: (env.shaping_cost(),) + _goal_planes(env)
        n_done, clamped, free, pushes = pu.twin_steps(a, b, _acts("upper"), desc.qd_max, extra)
        assert n_done.min() >= 2 and clamped > 0 and free > 0
        assert a.stats() == b.stats() and a.shaping_stats() == b.shaping_stats()
    finally:
        a.close(); b.close()


# ---- 6. a captured graph ----
@pytest.mark.parametrize("which", ["baked", "upper"])
def test_replays_of_a_captured_graph_advance_the_counters(which):
    import torch
    from gym_roboy_amd.envs.vec_env import _device_view_f32
    env = _vec(which)
    try:
        env.reset()
        dev = torch.device("cuda", 0)
        T = 3
        acts = torch.from_numpy(_acts(which, steps=T)).to(dev)
        obs = torch.zeros((T, N, env.obs_dim), device=dev)
        rew, done = torch.zeros((T, N), device=dev), torch.zeros((T, N), dtype=torch.int32, device=dev)
        pushed_dev = torch.zeros((T, N), dtype=torch.bool, device=dev)
        count_v, last_v = (_device_view_f32(p, N, dev).view(torch.int32) for p in env._push_planes()[:2])
        book = pu.Book(SEED, N, pu.threshold_of(PROB))
        side = torch.cuda.Stream(device=dev)
        env.set_stream(side.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for k in range(T):
                env.step_dev(acts[k].data_ptr(), obs[k].data_ptr(), rew[k].data_ptr(), done[k].data_ptr())
                pushed_dev[k] = count_v == last_v
        for replay in range(3):
            graph.replay()
            torch.cuda.synchronize()
            got = pushed_dev.cpu().numpy()
            for k in range(3):
                assert np.array_equal(got[k], book.step()[0]), (replay, k)
            count, last, n_pushes, _ = pu.planes(env)
            assert np.array_equal(count, book.count) and np.array_equal(last, book.last) and np.array_equal(n_pushes, book.n_pushes)
        assert np.all(pu.planes(env)[0] == 9) and env.push_count() == int(book.n_pushes.sum())
    finally:
        env.close()


# ---- 7. refusals ----
def test_refusals_leave_planes_and_dispatch_as_they_were():
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    robot, desc = pu.robot_of("baked")
    lib = nat.load()
    sigma = pu.sigma_of(desc)
    # without rb_env_configure
    sim = HipBatchSimulation(robot, N, seed=SEED)
    try:
        assert lib.rb_env_push_configure(sim.handle, ctypes.byref(pu.push_cfg(nat, 100, sigma))) == nat.RB_EINVAL
        assert b"rb_env_configure" in lib.rb_last_error()
        p = [nat._vp() for _ in range(4)]
        assert lib.rb_env_push_ptr(sim.handle, *p) == nat.RB_EINVAL
        total = ctypes.c_uint64()
        assert lib.rb_env_push_count(sim.handle, ctypes.byref(total), 0) == nat.RB_EINVAL
    finally:
        sim.close()
    env = _vec("baked")
    try:
        env.reset()
        acts = _acts("baked", steps=3)
        env.step(acts[0])
        ptrs = env._push_planes()
        before = pu.planes(env)
        row = env.sim.dispatch("env_step")["id"]
        assert before[0].all() and before[2].sum() > 0
        bad = [pu.push_cfg(nat, 2 ** 24 + 1, sigma), pu.push_cfg(nat, 100, [-1.0] + sigma[1:]), pu.push_cfg(nat, 100, sigma[:2] + [np.inf]),
               pu.push_cfg(nat, 100, [np.nan] + sigma[1:])]
        for cfg in bad:
            assert pu.configure(nat, env, cfg) == nat.RB_EINVAL and b"random pushes" in lib.rb_last_error()
        ok = pu.push_cfg(nat, 100, sigma)
        ok.sigma[desc.n_q] = -1.0                                    # (behind the first n_q: not read)
        assert env._push_planes() == ptrs and env.sim.dispatch("env_step")["id"] == row
        for x, y in zip(before, pu.planes(env)):
            assert np.array_equal(x, y)
        # the fused rollout steps inside one kernel
        ring = env.sim.malloc(4 * N * desc.n_t)
        with pytest.raises(nat.NativeError, match="random pushes"):
            env.sim.rollout_fused_dev(ring, 1, 1)
        for x, y in zip(before, pu.planes(env)):
            assert np.array_equal(x, y)
        # the handle steps on as configured: the next draw is the restated one
        env.step(acts[1])
        count, last, _, _ = pu.planes(env)
        assert np.array_equal(last == count, pu.decision(SEED, np.arange(N), 1, pu.threshold_of(PROB)))
        # a successful call zeroes all four planes (and ignores what lies behind the first n_q sigmas)
        assert pu.configure(nat, env, ok) == nat.RB_OK
        assert all(not p.any() for p in pu.planes(env))
        assert env.push_count(reset=True) == 0
    finally:
        env.close()


# ---- 8. RoboyVecEnv ----
@pytest.mark.parametrize("which", ["baked", "upper"])
def test_vec_env_numpy_and_torch_paths(which):
    import torch
    desc = pu.robot_of(which)[1]
    env, plain = _vec(which, prob=0.5), _vec(which, push=False)
    try:
        assert plain.push is None and env.push["threshold"] == 2 ** 23 and env.push["sigma"] == pu.sigma_of(desc)
        with pytest.raises(RuntimeError):
            plain.last_push()
        with pytest.raises(RuntimeError):
            plain.push_count()
        env.reset()
        assert not env.last_push()[0].any()                          # nobody was pushed before the first step
        acts = _acts(which, steps=2)
        env.step(acts[0])
        pushed, imp = env.last_push()
        assert isinstance(pushed, np.ndarray) and pushed.dtype == bool and pushed.shape == (N,) and imp.shape == (N, desc.n_q)
        assert np.array_equal(pushed, pu.decision(SEED, np.arange(N), 0, 2 ** 23)) and np.all(imp[~pushed] == 0) and np.all(imp[pushed] != 0)
        assert env.push_count() == int(pushed.sum())
        env.step(torch.from_numpy(acts[1]).cuda())
        pushed_t, imp_t = env.last_push()
        assert pushed_t.is_cuda and pushed_t.dtype == torch.bool and imp_t.is_cuda and tuple(imp_t.shape) == (N, desc.n_q)
        torch.cuda.synchronize()
        second = pu.decision(SEED, np.arange(N), 1, 2 ** 23)
        assert np.array_equal(pushed_t.cpu().numpy(), second)
        assert np.array_equal(imp_t.cpu().numpy(), pu.planes(env)[3])
        assert env.push_count(reset=True) == int(pushed.sum() + second.sum())
        assert env.push_count() == 0 and np.all(pu.planes(env)[0] == 2)      # the reset clears n_pushes, not the step counter
        env.reset()
        assert np.all(pu.planes(env)[0] == 2)                        # ... and neither does a reset
    finally:
        env.close(); plain.close()


# ---- 9. PPO and the trainer ----
@pytest.mark.parametrize("use_graphs", [True, False])
def test_ppo_rounds_push_and_the_checkpoint_records_the_option(use_graphs, tmp_path):
    import torch
    from gym_roboy_amd.ppo import PPO
    n, T = 256, 8
    for push in (True, False):
        torch.manual_seed(0)
        env = _vec("baked", n=n, push=push, prob=0.05)
        try:
            agent = PPO(env, n_steps=T, use_graphs=use_graphs, reward_scale=0.01, seed=0, device="cuda")
            for _ in range(2):
                stats = agent.update(agent.collect())
            torch.cuda.synchronize()
            assert isinstance(stats, dict)
            path = str(tmp_path / ("push%d.pkl" % push))
            agent.save(path)
            ck = torch.load(path)
            if push:
                count = pu.planes(env)[0]
                assert np.all(count == 2 * T)
                assert env.push_count() == int(pu.schedule(SEED, n, 2 * T, 0.05).sum()) > 0
                assert ck["env_push"] == {"prob": 0.05, "sigma": pu.sigma_of(pu.robot_of("baked")[1]), "threshold": pu.threshold_of(0.05)}
                agent.load(path)
                assert agent.checkpoint_env_push == ck["env_push"]
            else:
                assert "env_push" not in ck
        finally:
            env.close()


def test_train_parallel_prints_pushes_per_step(tmp_path):
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "gym_roboy_amd.train_parallel", "256", str(tmp_path / "results"), "--rounds", "2",
                          "--steps-per-round", str(256 * 8), "--n-steps", "8", "--push", "prob=0.05,sigma=0.5"],
                         cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rates = [float(x) for x in re.findall(r"'pushes_per_step': ([0-9.e+-]+)", out.stdout)]
    assert len(rates) == 2, out.stdout
    # 2 048 env steps per round at P = 0.05: the rate lies within five standard deviations of it
    assert all(abs(r - 0.05) < 5 * (0.05 * 0.95 / 2048) ** 0.5 for r in rates), rates
    import torch
    ck = torch.load(str(tmp_path / "results" / "model.pkl"))
    assert ck["env_push"]["prob"] == 0.05 and ck["env_push"]["sigma"] == [0.5] * 3
