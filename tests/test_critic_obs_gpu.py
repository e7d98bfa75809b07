"""Privileged critic rows behind the fused env step on the GPU (include/roboy_sim.h: rb_env_critic_obs_*; csrc/env_critic.hpp;
DESIGN.md §20).  Everything compares bit for bit; no tolerance anywhere.

MsjRobot with randomization, a delay range (0, 3) redrawn on reset and K = 2 action rows; episodes of 3 steps with auto-reset over 5
steps, so every env resets at least once.  Sizes: 1 (a lone lane), 64 (one full wave), 65 (a full wave plus one lane), 333 (a partial
last wave behind full ones), 1024 (several workgroups).  What each block is compared with:
    state    q, qd read back from the handle (rb_read_state) and the goal columns of the observation row (never noised)
    age      float32(step_num) / float32(max_len), the step counter kept on the host from the done flags
    params   get_params() in plane order
    delay    get_action_delay()
    actions  the observation row's columns from `lead` on"""
import itertools

import numpy as np
import pytest

from gym_roboy_amd import _native as nat

pytestmark = pytest.mark.gpu

MAX_LEN, STEPS = 3, 5
SIZES = (1, 64, 65, 333, 1024)
RANGES = dict(force_scale=(0.8, 1.2), setpoint_offset=(-0.01, 0.01), mass_scale=(0.8, 1.25), damping_scale=(0.5, 2.0))
ALL = ("state", "age", "params", "delay", "actions")
K = 2


def _env(n, critic_obs, seed=5, robot=None, randomization=True, action_delay=(0, 3), action_obs=K, **kw):
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    return RoboyVecEnv(robot or MsjRobot(), n, seed=seed, max_episode_length=MAX_LEN, randomization=ParamRanges(**RANGES) if randomization else None,
                       action_delay=action_delay, action_obs=action_obs, critic_obs=critic_obs, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _blocks(env, cobs):
    """the row's blocks by name"""
    nq, nt = env.n_q, env.n_t
    width = {"state": 3 * nq, "age": 1, "params": 2 * nt + 4, "delay": 1, "actions": env.action_obs * nt}
    out, c = {}, 0
    for name in env.critic_obs_names:
        out[name] = cobs[:, c:c + width[name]]
        c += width[name]
    assert c == env.critic_obs_dim == cobs.shape[1]
    return out


def _param_rows(env):
    p = env.get_params()
    return np.concatenate((p["force_scale"], p["setpoint_offset"], p["mass_scale"][:, None], p["damping_scale"]), axis=1)


def _check_rows(env, cobs, obs, step_num, what):
    """every block of the rows against what the handle holds now"""
    n = env.num_envs
    assert cobs.shape == (n, env.critic_obs_dim) and cobs.dtype == np.float32, what
    b = _blocks(env, cobs)
    q, qd, _ = env.sim.read_state()
    assert _same(b["state"][:, 0:3], q) and _same(b["state"][:, 3:6], qd) and _same(b["state"][:, 6:9], obs[:, 6:9]), what
    if "age" in b:
        assert _same(b["age"][:, 0], step_num.astype(np.float32) / np.float32(MAX_LEN)), what
    if "params" in b:
        assert _same(b["params"], _param_rows(env)), what
    if "delay" in b:
        assert _same(b["delay"][:, 0], env.get_action_delay().astype(np.float32)), what
    if "actions" in b:
        lead = env.obs_dim - env.action_obs * env.n_t
        assert _same(b["actions"], obs[:, lead:]), what
    return b


def _walk(env, seed, steps=STEPS):
    """reset and `steps` steps, every row checked; returns [(obs, reward, done, q, qd, feasible)], the rows of every step and the
    number of episode ends per env"""
    n = env.num_envs
    rng = np.random.default_rng(seed)
    obs = env.reset()
    step_num = np.ones(n, np.int64)
    rows = [env.critic_obs()]
    prev = _check_rows(env, rows[0], obs, step_num, "reset")
    assert not prev["state"][:, :6].any() and ("actions" not in prev or not prev["actions"].any())
    out, n_done, delay_moved = [], np.zeros(n, int), 0
    for t in range(steps):
        act = rng.uniform(-2, 2, (n, env.n_t)).astype(np.float32)
        obs, rew, done, _ = env.step(act)
        step_num = np.where(done, 1, step_num + 1)
        cobs = env.critic_obs()
        b = _check_rows(env, cobs, obs, step_num, "step %d" % t)
        if done.any():                              # an auto-reset lane shows what its NEXT episode starts from
            d = done
            assert not b["state"][d, :6].any() and (b["state"][d, 6:9] != prev["state"][d, 6:9]).any(axis=1).all()
            if "age" in b:
                assert (b["age"][d, 0] == np.float32(1) / np.float32(MAX_LEN)).all()
            if "params" in b:
                assert (b["params"][d] != prev["params"][d]).any(axis=1).all()
            if "delay" in b:
                delay_moved += int((b["delay"][d, 0] != prev["delay"][d, 0]).sum())
            if "actions" in b:
                assert not b["actions"][d].any()
        if "actions" in b and (~done).any():        # a live lane's newest block is the handed row, clamped
            assert _same(b["actions"][~done, :env.n_t], np.clip(act, -1, 1)[~done])
        n_done += done
        prev = b
        rows.append(cobs)
        out.append((obs, rew, done) + tuple(env.sim.read_state()))
    assert n_done.min() >= 1
    if "delay" in prev and n >= 64:
        assert delay_moved > 0                      # (a redraw from {0..3} repeats the old value one time in four)
    return out, rows, n_done


# ---- 1. the rows ----
@pytest.mark.parametrize("n", SIZES)
def test_every_block_is_what_the_handle_holds_bit_for_bit(n):
    env = _env(n, ALL)
    try:
        assert env.critic_obs_names == ALL and env.critic_obs_dim == 9 + 1 + 20 + 1 + K * 8
        _walk(env, n)
    finally:
        env.close()


def test_every_legal_subset_of_blocks():
    n = 333
    for r in range(5):
        for extra in itertools.combinations(ALL[1:], r):
            env = _env(n, ("state",) + extra)
            try:
                assert env.critic_obs_names == ("state",) + extra, extra
                _walk(env, 7)
            finally:
                env.close()
    # "state" is part of the row whether named or not, and the order of the names does not matter
    env = _env(n, ("delay", "age"))
    try:
        assert env.critic_obs_names == ("state", "age", "delay") and env.critic_obs_dim == 11
    finally:
        env.close()


def test_blocks_follow_the_options_the_env_has():
    """no randomization, no delay, no action rows: state and age alone, 10 columns - and the torch step's rows are a tensor"""
    import torch
    env = _env(65, ("state", "age"), randomization=False, action_delay=None, action_obs=None)
    try:
        assert env.critic_obs_dim == 10
        _walk(env, 3)
        obs, _, done, _ = env.step(torch.zeros(65, 8, device="cuda"))
        cobs = env.critic_obs()
        assert cobs.is_cuda and tuple(cobs.shape) == (65, 10)
        torch.cuda.synchronize()
        assert _same(cobs.cpu().numpy()[:, :9], obs.cpu().numpy())
    finally:
        env.close()


def test_the_state_block_is_exact_under_sensor_noise():
    env = _env(333, ALL, sensor_noise={"q": 0.01, "qd": 0.05})
    try:
        env.reset()
        rng = np.random.default_rng(1)
        for t in range(2):                          # (before any auto-reset: the state is not zero)
            obs, _, done, _ = env.step(rng.uniform(-1, 1, (333, 8)).astype(np.float32))
            cobs = env.critic_obs()
            q, qd, _ = env.sim.read_state()
            assert _same(cobs[:, 0:3], q) and _same(cobs[:, 3:6], qd) and _same(cobs[:, 6:9], obs[:, 6:9])
            assert (obs[:, 0:3] != q).mean() > 0.9 and (obs[:, 3:6] != qd).mean() > 0.9
            assert _same(cobs[:, -K * 8:], obs[:, -K * 8:])
    finally:
        env.close()


# ---- 2. nothing else moved ----
@pytest.mark.parametrize("report_truncation", [False, True])
def test_a_twin_without_the_option_steps_identically(report_truncation):
    n = 333
    res = []
    for critic_obs in (None, ALL):
        env = _env(n, critic_obs, sensor_noise={"q": 0.01}, report_truncation=report_truncation)
        try:
            rng = np.random.default_rng(9)
            obs0, out = env.reset(), []
            for t in range(STEPS):
                o, r, d, _ = env.step(rng.uniform(-2, 2, (n, 8)).astype(np.float32))
                out.append((o, r, d) + tuple(env.sim.read_state()) + ((env.truncated(),) if report_truncation else ()))
            res.append((obs0, out, env.stats(), _param_rows(env), env.get_action_delay()))
        finally:
            env.close()
    a, b = res
    assert _same(a[0], b[0]) and a[2] == b[2] and _same(a[3], b[3]) and np.array_equal(a[4], b[4])
    for t, (x, y) in enumerate(zip(a[1], b[1])):
        for u, v in zip(x, y):
            assert np.array_equal(u, v), t
        assert _same(x[0], y[0]) and _same(x[1], y[1]), t
    assert sum(x[2].sum() for x in a[1]) >= n
    if report_truncation:
        assert sum(x[-1].sum() for x in a[1]) > 0


# ---- 3. sub-ranges, and rows through the caller's pointer ----
def test_two_ranges_on_two_streams_write_the_rows_of_the_whole_batch():
    import torch
    n, half = 1024, 512
    whole, split = _env(n, ALL), _env(n, ALL)
    try:
        assert split.range_capable()
        dc, od = whole.critic_obs_dim, whole.obs_dim
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        rng = np.random.default_rng(4)
        whole.reset()
        split.reset()
        assert _same(whole.critic_obs(), split.critic_obs())
        obs = torch.empty(n, od, device="cuda")
        rew, done = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        # rows at an address off the float4 grid too: a [T, n, Dc] tensor's slices are wherever n Dc puts them
        slab = torch.zeros(n * dc + 1, device="cuda")
        for t in range(STEPS):
            a = rng.uniform(-2, 2, (n, 8)).astype(np.float32)
            o_w, r_w, d_w, _ = whole.step(a)                     # the old entry point: rows into the handle's plane
            c_w = whole.critic_obs()
            act = torch.from_numpy(a).cuda()
            cobs = slab[t % 2:t % 2 + n * dc].view(n, dc)
            assert cobs.data_ptr() % 16 == (4 if t % 2 else 0)
            torch.cuda.synchronize()
            for first, st in ((0, s1), (half, s2)):
                split.step_range_dev(first, half, st.cuda_stream, act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), cobs.data_ptr())
            torch.cuda.synchronize()
            assert _same(obs.cpu().numpy(), o_w) and _same(rew.cpu().numpy(), r_w) and np.array_equal(done.cpu().numpy() != 0, d_w), t
            assert _same(cobs.cpu().numpy(), c_w), t
        # the pointer form of the whole-batch entry against the plane form, on twins in the same state
        a = rng.uniform(-2, 2, (n, 8)).astype(np.float32)
        whole.step(a)
        act = torch.from_numpy(a).cuda()
        mine = torch.empty(n, dc, device="cuda")
        torch.cuda.synchronize()
        split.step_dev(act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), mine.data_ptr())
        split.sim.synchronize()
        torch.cuda.synchronize()
        assert _same(mine.cpu().numpy(), whole.critic_obs())
    finally:
        whole.close()
        split.close()


# ---- 4. refusals ----
def test_a_joint_tree_is_refused_and_leaves_no_handle_behind(monkeypatch):
    import gym_roboy_amd.envs.vec_env as vec_env
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    made = []

    class Recorded(vec_env.HipBatchSimulation):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(vec_env, "HipBatchSimulation", Recorded)
    with pytest.raises(nat.NativeError, match="ball-joint"):
        vec_env.RoboyVecEnv(UpperBodyRobot(), 64, critic_obs=("state",))
    assert len(made) == 1 and made[0]._h is None


def test_library_refusals_and_the_off_state():
    import ctypes
    env = _env(64, None, randomization=False, action_delay=None, action_obs=None)
    try:
        lib, h = env.sim._lib, env.sim.handle
        dim, rows = ctypes.c_int32(-1), ctypes.c_void_p()
        assert lib.rb_env_critic_obs_dim(h, ctypes.byref(dim)) == nat.RB_OK and dim.value == 0
        assert lib.rb_env_critic_obs_ptr(h, ctypes.byref(rows)) == nat.RB_EINVAL
        for bit in (nat.RB_CRITIC_PARAMS, nat.RB_CRITIC_DELAY, nat.RB_CRITIC_ACTIONS, 32):
            assert lib.rb_env_critic_obs_configure(h, nat.RB_CRITIC_STATE | bit) == nat.RB_EINVAL, bit
        with pytest.raises(RuntimeError):
            env.critic_obs()
        with pytest.raises(ValueError, match="not enabled"):
            env.step_dev(env._d_act, env._d_obs, env._d_rew, env._d_done, env._d_obs)
        # on, then off again: the handle launches what it launched before
        assert lib.rb_env_critic_obs_configure(h, nat.RB_CRITIC_AGE) == nat.RB_OK
        assert lib.rb_env_critic_obs_dim(h, ctypes.byref(dim)) == nat.RB_OK and dim.value == 10
        assert lib.rb_env_critic_obs_configure(h, 0) == nat.RB_OK
        assert lib.rb_env_critic_obs_dim(h, ctypes.byref(dim)) == nat.RB_OK and dim.value == 0
        env.reset()
        env.step(np.zeros((64, 8), np.float32))
    finally:
        env.close()
    # a row wider than the gradient kernels' input: K = 8 action rows make 31 + 64 columns (the library's own refusal)
    env = _env(64, None, action_obs=8)
    try:
        assert env.sim._lib.rb_env_critic_obs_configure(env.sim.handle, 31) == nat.RB_EINVAL
        assert b"63" in env.sim._lib.rb_last_error()
        assert env.sim._lib.rb_env_critic_obs_configure(env.sim.handle, 15) == nat.RB_OK      # without the action blocks: 31 columns
    finally:
        env.close()
