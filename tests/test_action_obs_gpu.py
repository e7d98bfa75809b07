"""The last K commanded actions as observation columns of the fused env step on the GPU (include/roboy_sim.h: rb_env_action_obs_*;
csrc/env_hist.hpp).  Twin handles: B has the option, A has not, same seed and configuration - the leading columns and
every other output bit for bit, B's action columns against tests/action_obs_util.HistoryBook fed with the handed rows and A's done.
Everything compares exactly; no tolerance anywhere.

Shapes: 1 env, 65 (a whole wave plus one lane), 257 (a second workgroup with one lane), 320; action rows from U[-2, 2] so that the
clamp shows; episodes of 5 steps with auto-reset over 13 steps: every env resets twice.  MsjRobot with K = 3 and mask 9 writes 49
columns (staged through LDS), with K = 8 and mask 15 it writes 105 (per lane); ball12's widths are no multiple of 4; ball16 (the
widest robot of the class) with K = 8 and mask 15 writes 201 columns."""
import ctypes

import numpy as np
import pytest

from action_obs_util import HistoryBook, ring_slots
from env_obs_util import channels_of
from gym_roboy_amd import _native as nat
from test_env_io_gpu import SIGMA, _io_cfg, _plane, _run, _start
from test_env_obs_gpu import ROBOTS as _ROBOTS, _state, _vec
from test_env_params_gpu import _msj

pytestmark = pytest.mark.gpu



def _ball16():
    from random_robots import random_ball_joint_robot
    return random_ball_joint_robot(11, n_t=16)[0]


ROBOTS = dict(_ROBOTS, ball16=_ball16)
SIZES = (1, 65, 257, 320)
STEPS, MAX_LEN = 13, 5


def _inputs(which, n, seed, steps=STEPS):
    desc = ROBOTS[which]().get_description()
    rng = np.random.default_rng(seed)
    q, qd = _state(desc, n, rng)
    return desc, q, qd, rng.uniform(-2, 2, (steps, n, desc.n_t)).astype(np.float32)


def _make(which, n, integ, form, mask, rows=0, scale=None, seed=5, **kw):
    env = _vec(ROBOTS[which](), n, integ, tendon_obs=channels_of(mask) or None, scale=scale, seed=seed, max_len=MAX_LEN,
               randomization=True if form == "randomized" else None, action_obs=rows or None, **kw)
    assert env.action_obs == rows and env.sim.action_obs_rows() == rows
    return env


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_twin(desc, n, lead, rows, acts, res_a, res_b):
    """res_*: _run's (reset rows, [(obs, reward, done, q, qd, feasible)], stats) of the handle without / with the option"""
    (a0, a, a_stats), (b0, b, b_stats) = res_a, res_b
    od = lead + rows * desc.n_t
    assert a0.shape == (n, lead) and b0.shape == (n, od)
    assert np.array_equal(_bits(a0), _bits(b0[:, :lead])) and not _bits(b0[:, lead:]).any()          # reset rows: K zero blocks
    book = HistoryBook(n, desc.n_t, rows)
    n_done = np.zeros(n, int)
    for t, (ra, rb) in enumerate(zip(a, b)):
        assert rb[0].shape == (n, od)
        assert np.array_equal(_bits(ra[0]), _bits(rb[0][:, :lead])), t
        for x, y in zip(ra[1:], rb[1:]):                                   # reward, done, q, qd, feasible
            assert np.array_equal(x, y), t
        want = book.blocks(acts[t], ra[2])
        assert np.array_equal(_bits(rb[0][:, lead:]), _bits(want)), (t, np.argwhere(rb[0][:, lead:] != want)[:4])
        if t == 0:                                                         # the first step after reset(): block 0 is the handed row
            on = ~ra[2]                                                    # (an env that ended its episode there: zeros, as above)
            assert np.array_equal(rb[0][on, lead:lead + desc.n_t], np.clip(acts[0], -1, 1)[on]) and not rb[0][:, lead + desc.n_t:].any()
        n_done += ra[2]
    assert n_done.min() >= 2 and a_stats == b_stats
    assert max(np.abs(rb[0][:, lead:]).max() for rb in b) == 1.0           # the clamp showed


def _twin(which, n, integ, form, mask, rows, seed, cfg=None, scale=None):
    desc, q, qd, acts = _inputs(which, n, seed)
    res = []
    for k in (0, rows):
        env = _make(which, n, integ, form, mask, k, scale=scale, seed=seed)
        try:
            if form == "nominal" and not mask and cfg is None:
                env.sim.select_kernel(1)          # A runs its env-per-lane row: the step text the history kernel expands
                if not k:
                    assert "/env_per_lane/" in env.sim.dispatch("env_step")["id"]
            if cfg is not None:
                env.sim.configure_io(cfg)
            if k:
                p = env.sim.io_ptrs()
                assert p["history"] is not None and p["slots"] == ring_slots(k, cfg.delay_hi if cfg is not None else 0)
            res.append(_run(env, q, qd, acts))
            if cfg is not None:
                res[-1] += tuple(_plane(env, name) for name in ("delay", "delay_draws", "rows"))
        finally:
            env.close()
    lead = 9 + len(channels_of(mask)) * desc.n_t
    _check_twin(desc, n, lead, rows, acts, res[0][:3], res[1][:3])
    for x, y in zip(res[0][3:], res[1][3:]):                               # delay redraws and noise counters
        assert np.array_equal(x, y)


# ---- 1. the grid ----
GRID = [(which, integ, form) for which in ("baked", "kernarg", "ball12") for integ in ("euler", "rk4") for form in ("nominal", "randomized")]


@pytest.mark.parametrize("mask", [0, 9, 15])
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("which,integ,form", GRID)
def test_leading_columns_and_every_other_output_are_the_twins_and_the_blocks_are_the_handed_rows(which, integ, form, rows, mask, monkeypatch):
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    n = SIZES[(GRID.index((which, integ, form)) + rows + mask) % 4]
    _twin(which, n, integ, form, mask, rows, seed=11 + rows)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("which,integ,form,rows,mask", [("baked", "rk4", "nominal", 3, 9),         # 49 columns, staged
                                                        ("baked", "euler", "randomized", 8, 15),    # 105 columns, per lane
                                                        ("baked", "rk4", "nominal", 8, 0),          # the 64-thread instance, 73 columns
                                                        ("kernarg", "euler", "nominal", 3, 0),
                                                        ("ball12", "rk4", "randomized", 3, 0),      # 45 columns
                                                        ("ball12", "euler", "nominal", 1, 15),      # 69 columns
                                                        ("ball16", "euler", "randomized", 1, 0),    # 25 columns, staged
                                                        ("ball16", "rk4", "nominal", 3, 9),         # 89 columns
                                                        ("ball16", "euler", "nominal", 8, 15)])     # 201 columns
def test_every_batch_size_on_every_row_path(which, integ, form, rows, mask, n, monkeypatch):
    monkeypatch.setenv("ROBOY_SIM_JIT", "0")
    _twin(which, n, integ, form, mask, rows, seed=n)


# ---- 2. with the delay, with noise ----
@pytest.mark.parametrize("which,integ,form,mask,n", [("baked", "rk4", "nominal", 0, 257), ("kernarg", "euler", "randomized", 9, 320),
                                                     ("ball12", "euler", "nominal", 15, 65)])
def test_delay_and_history_share_the_ring_and_the_blocks_hold_the_handed_rows(which, integ, form, mask, n):
    """delay (0, 3) redrawn on reset, K = 2: S = 4 comes from the delay.  The twin with the delay alone steps identically (state,
    reward, done, delay planes); the blocks are what was handed, not what the delay applied."""
    _twin(which, n, integ, form, mask, 2, seed=31, cfg=_io_cfg(delay=(0, 3), resample=True))


@pytest.mark.parametrize("which,integ,form,mask,n", [("baked", "euler", "nominal", 9, 320), ("kernarg", "rk4", "randomized", 15, 65),
                                                     ("ball12", "rk4", "nominal", 0, 257)])
def test_noise_reaches_the_leading_columns_only(which, integ, form, mask, n):
    """noise on q, qd and force, K = 3: the leading columns are, bit for bit, those of the twin with the same noise and no history
    (the same Philox blocks by row position), the row counters agree, the action columns hold the exact clamps."""
    sigma = {k: v for k, v in SIGMA.items() if k in ("q", "qd", "force")}
    _twin(which, n, integ, form, mask, 3, seed=37, cfg=_io_cfg(sigma, channels_of(mask)), scale={"force": 1 / 400} if mask else None)


@pytest.mark.parametrize("which,form,n", [("ball12", "nominal", 65), ("ball16", "randomized", 257)])
def test_noise_on_the_widest_rows_stops_in_front_of_the_action_blocks(which, form, n):
    """mask 15 and K = 8: rows of 153 and 201 columns, more than the 32 Philox blocks the noise's block mask can name and more than
    its per-column sigmas cover.  Reset rows and step rows: the leading columns are the twin's with the same noise, the blocks exact."""
    _twin(which, n, "euler", form, 15, 8, seed=43, cfg=_io_cfg(SIGMA, channels_of(15)))


def test_noise_delay_channels_and_parameters_together():
    _twin("baked", 321, "rk4", "randomized", 9, 8, seed=41, cfg=_io_cfg(SIGMA, channels_of(9), delay=(0, 7), resample=True))


# ---- 3. reset rows, without auto-reset ----
def test_reset_rows_and_the_first_step_behind_a_reset():
    n, rows = 257, 3
    desc, q, qd, acts = _inputs("baked", n, 43, steps=4)
    env = _make("baked", n, "euler", "nominal", 9, rows)
    try:
        lead = 25
        for _ in range(2):                        # the second reset comes with three steps of history in the ring
            obs0 = _start(env, q, qd)
            assert obs0.shape == (n, 49) and not _bits(obs0[:, lead:]).any()
            for t in range(3):
                obs = env.step(acts[t])[0]
                for j in range(rows):
                    blk = obs[:, lead + 8 * j:lead + 8 * (j + 1)]
                    assert np.array_equal(blk, np.clip(acts[t - j], -1, 1) if j <= t else np.zeros((n, 8), np.float32)), (t, j)
    finally:
        env.close()


def test_without_auto_reset_counter_and_history_run_on():
    n, rows = 65, 3
    desc, q, qd, acts = _inputs("ball12", n, 47, steps=8)
    env = _make("ball12", n, "euler", "nominal", 0, rows, auto_reset=False)
    try:
        _start(env, q, qd)
        book = HistoryBook(n, desc.n_t, rows)
        seen_done = False
        for t in range(8):
            obs, _, done, _ = env.step(acts[t])
            assert np.array_equal(_bits(obs[:, 9:]), _bits(book.blocks(acts[t], done, auto_reset=False)))
            seen_done |= bool(done.any())
        assert seen_done and obs[:, 9:].all()
    finally:
        env.close()


# ---- 4. sub-ranges, a captured graph ----
@pytest.mark.parametrize("which,form,mask,rows", [("baked", "nominal", 9, 3), ("ball12", "randomized", 0, 8)])
def test_sub_ranges_give_the_whole_batch_rows(which, form, mask, rows):
    import torch
    n, h = 577, 256
    desc, q, qd, acts = _inputs(which, n, 53, steps=7)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for mode in ("whole", "split"):
        env = _make(which, n, "euler", form, mask, rows, seed=3, env_id_offset=1000)
        try:
            env.sim.configure_io(_io_cfg(delay=(0, 3), resample=True))
            assert env.range_capable()
            _start(env, q, qd)
            od = env.obs_dim
            d_act, d_obs, d_rew, d_done = env.sim.malloc(acts[0].nbytes), env.sim.malloc(n * od * 4), env.sim.malloc(n * 4), env.sim.malloc(n * 4)
            out = []
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
                out.append((env.sim.download(d_obs, (n, od)), env.sim.download(d_rew, (n,)), env.sim.download(d_done, (n,), np.uint32)))
            res.append(out)
        finally:
            env.close()
    whole, split = res
    lead = od - rows * desc.n_t
    book = HistoryBook(n, desc.n_t, rows)
    for t in range(len(acts)):
        for x, y in zip(whole[t], split[t]):
            assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y), t
        assert np.array_equal(_bits(split[t][0][:, lead:]), _bits(book.blocks(acts[t], split[t][2])))
    assert sum(w[2] for w in whole).min() >= 1


def test_a_captured_graph_of_six_steps_replays_with_counters_and_ring_on_the_device():
    import torch
    n, T, rows = 321, 6, 3
    kw = dict(tendon_obs=("length", "force"), randomization=True, seed=4, max_len=MAX_LEN, action_obs=rows)
    env, ref = _vec(_msj(), n, "rk4", **kw), _vec(_msj(), n, "rk4", **kw)
    try:
        for e in (env, ref):
            e.sim.configure_io(_io_cfg(SIGMA, ("length", "force"), delay=(0, 3), resample=True))
        dev = torch.device("cuda", 0)
        acts = torch.rand((2, T, n, 8), device=dev) * 4 - 2
        slab = torch.zeros((T, n, 8), device=dev)
        obs = torch.zeros((T, n, env.obs_dim), device=dev)
        rew, done = torch.zeros((T, n), device=dev), torch.zeros((T, n), dtype=torch.int32, device=dev)
        assert env.obs_dim == 49 and np.array_equal(env.reset(), ref.reset())
        side = torch.cuda.Stream(device=dev)
        env.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for t in range(T):
                env.step_dev(slab[t].data_ptr(), obs[t].data_ptr(), rew[t].data_ptr(), done[t].data_ptr())
        book = HistoryBook(n, 8, rows)
        n_done = np.zeros(n, int)
        for r in range(2):                       # 12 steps: the ring and the counters carry over from replay to replay
            slab.copy_(acts[r])
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            for t in range(T):
                a = acts[r, t].cpu().numpy()
                o, w, dn, _ = ref.step(a)
                got = obs[t].cpu().numpy()
                assert np.array_equal(_bits(got), _bits(o)) and np.array_equal(rew[t].cpu().numpy(), w), (r, t)
                assert np.array_equal(done[t].cpu().numpy().astype(bool), dn)
                assert np.array_equal(_bits(got[:, 25:]), _bits(book.blocks(a, dn))), (r, t)
                n_done += dn
        assert n_done.min() >= 2
        env.set_stream(0)
    finally:
        env.close(); ref.close()


# ---- 5. configure order, switching off, refusals ----
def _dev_run(env, od, q, qd, acts):
    """reset, the state, the steps - through buffers of the handle's CURRENT row width (freed with the handle)"""
    n = env.num_envs
    d_act, d_obs, d_rew, d_done = env.sim.malloc(acts[0].nbytes), env.sim.malloc(n * od * 4), env.sim.malloc(n * 4), env.sim.malloc(n * 4)
    if env.randomization is not None:
        env.sim.sample_params()
    nat.check(env.sim._lib.rb_env_reset_dev(env.sim.handle, ctypes.c_void_p(d_obs)))
    env.sim.synchronize()
    out = [env.sim.download(d_obs, (n, od))]
    env.sim.set_state(q, qd)
    for a in acts:
        env.sim.upload(d_act, a)
        env.step_dev(d_act, d_obs, d_rew, d_done)
        env.sim.synchronize()
        out.append(np.concatenate((env.sim.download(d_obs, (n, od)), env.sim.download(d_rew, (n, 1)),
                                   env.sim.download(d_done, (n, 1), np.uint32).astype(np.float32)), axis=1))
    return out


def _obs_dim(env):
    dim = ctypes.c_int32()
    nat.check(env.sim._lib.rb_env_obs_dim(env.sim.handle, ctypes.byref(dim)))
    return int(dim.value)


@pytest.mark.parametrize("delay,rows", [((0, 3), 2), ((0, 1), 3)])          # S stays 4 / S goes 2 -> 4 -> 2
def test_configure_order_and_switching_off(delay, rows):
    n = 257
    desc, q, qd, acts = _inputs("baked", n, 59, steps=7)
    cfg = lambda: _io_cfg({"q": 0.01, "force": 2.0}, ("length", "force"), delay=delay, resample=True)
    envs = [_make("baked", n, "euler", "randomized", 9, seed=23) for _ in range(3)]
    io_first, hist_first, io_only = envs
    try:
        io_first.sim.configure_io(cfg())
        io_first.sim.configure_action_obs(rows)
        hist_first.sim.configure_action_obs(rows)
        assert hist_first.sim.io_ptrs()["slots"] == ring_slots(rows, 0) and hist_first.sim.io_ptrs()["delay"] is None
        hist_first.sim.configure_io(cfg())
        io_only.sim.configure_io(cfg())
        od = 25 + 8 * rows
        for e in (io_first, hist_first):
            assert _obs_dim(e) == od and e.sim.io_ptrs()["slots"] == ring_slots(rows, delay[1])
        assert _obs_dim(io_only) == 25 and io_only.sim.io_ptrs()["slots"] == ring_slots(0, delay[1])
        a, b, c = _dev_run(io_first, od, q, qd, acts), _dev_run(hist_first, od, q, qd, acts), _dev_run(io_only, 25, q, qd, acts)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(_bits(x), _bits(y))
            assert np.array_equal(_bits(x[:, :25]), _bits(z[:, :25])) and np.array_equal(x[:, od:], z[:, 25:])
        # off again: the io handle's rows.  Where S changed the io planes and counters are a fresh configuration's - the twin is
        # configured again too; where it did not they run on, as the twin's do
        io_first.sim.configure_action_obs(0)
        assert _obs_dim(io_first) == 25 and io_first.sim.action_obs_rows() == 0
        assert io_first.sim.io_ptrs()["slots"] == ring_slots(0, delay[1])
        if ring_slots(rows, delay[1]) != ring_slots(0, delay[1]):
            io_only.sim.configure_io(cfg())
        for name in ("delay", "delay_draws", "rows"):
            assert np.array_equal(_plane(io_first, name), _plane(io_only, name))
        for x, z in zip(_dev_run(io_first, 25, q, qd, acts), _dev_run(io_only, 25, q, qd, acts)):
            assert np.array_equal(_bits(x), _bits(z))
    finally:
        for e in envs:
            e.close()


def test_switching_off_without_io_restores_the_plain_handle():
    n = 320
    desc, q, qd, acts = _inputs("kernarg", n, 61, steps=7)
    env, plain = _make("kernarg", n, "rk4", "nominal", 0, seed=29), _make("kernarg", n, "rk4", "nominal", 0, seed=29)
    try:
        for e in (env, plain):
            e.sim.select_kernel(1)                # the env-per-lane row: the step text the history kernel expands
        row = env.sim.dispatch("env_step")["id"]
        env.sim.configure_action_obs(4)
        with pytest.raises(nat.NativeError, match="action rows"):
            env.sim.dispatch("env_step")
        assert env.sim.dispatch("step")["id"]                                                      # the step entry is untouched
        hist = _dev_run(env, 9 + 32, q, qd, acts)
        assert np.abs(hist[-1][:, 9:41]).max() == 1.0
        env.sim.configure_action_obs(0)
        assert env.sim.dispatch("env_step")["id"] == row
        assert env.sim._lib.rb_env_io_ptr(env.sim.handle, None, None, None, None, None) == nat.RB_EINVAL      # the ring is gone
        _dev_run(plain, 9, q, qd, acts)
        for x, z in zip(_dev_run(env, 9, q, qd, acts), _dev_run(plain, 9, q, qd, acts)):
            assert np.array_equal(_bits(x), _bits(z))
    finally:
        env.close(); plain.close()


def test_refusals():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    env = _vec(_msj(), 256)
    try:
        lib, h = env.sim._lib, env.sim.handle
        for bad in (-1, 9, 1 << 20):
            assert lib.rb_env_action_obs_configure(h, bad) == nat.RB_EINVAL and b"RB_ACTION_OBS_MAX" in lib.rb_last_error()
        assert lib.rb_env_action_obs_rows(h, None) == nat.RB_EINVAL
        assert env.sim.action_obs_rows() == 0 and _obs_dim(env) == 9                               # a refused call leaves the handle as it was
        assert lib.rb_env_io_ptr(h, None, None, None, None, None) == nat.RB_EINVAL
        env.sim.configure_action_obs(8)
        assert env.sim.action_obs_rows() == 8 and _obs_dim(env) == 73 == lib.rb_env_action_obs_count(3, 8, 0, 8)
        assert env.sim.io_ptrs()["slots"] == 8
    finally:
        env.close()
    bare = HipBatchSimulation(_msj(), 64)
    try:
        assert bare._lib.rb_env_action_obs_configure(bare.handle, 2) == nat.RB_EINVAL               # no rb_env_configure yet
        assert b"rb_env_configure" in bare._lib.rb_last_error()
    finally:
        bare.close()
    tree = _vec(UpperBodyRobot(), 64)
    try:
        assert tree.sim._lib.rb_env_action_obs_configure(tree.sim.handle, 2) == nat.RB_EUNSUPPORTED
        assert b"ball-joint" in tree.sim._lib.rb_last_error()
        assert tree.sim._lib.rb_env_action_obs_configure(tree.sim.handle, 0) == nat.RB_OK
        with pytest.raises(nat.NativeError):
            _vec(UpperBodyRobot(), 64, action_obs=1)
    finally:
        tree.close()
    with pytest.raises(ValueError):
        _vec(_msj(), 64, action_obs=9)


# ---- 6. the consumers ----
def test_vec_env_numpy_and_torch_paths():
    import torch
    n, rows = 512, 3
    env = _vec(_msj(), n, "rk4", action_obs=rows, action_delay=(0, 3), seed=21, max_len=MAX_LEN)
    plain = _vec(_msj(), n, "rk4", seed=21, max_len=MAX_LEN)
    try:
        assert env.action_obs == 3 and plain.action_obs == 0 and env.obs_dim == 33 and env.observation_space.shape == (33,)
        assert np.array_equal(env.observation_space.low[:9], plain.observation_space.low)
        assert np.array_equal(env.observation_space.high[:9], plain.observation_space.high)
        assert np.all(env.observation_space.low[9:] == -1) and np.all(env.observation_space.high[9:] == 1)
        obs0 = env.reset()
        assert obs0.shape == (n, 33) and not obs0[:, 9:].any()
        book = HistoryBook(n, 8, rows)
        acts = torch.rand((STEPS, n, 8), device="cuda") * 4 - 2
        n_done = np.zeros(n, int)
        for t in range(STEPS):
            a = acts[t].cpu().numpy()
            obs, rew, done, _ = env.step(acts[t]) if t % 2 else env.step(a)
            if t % 2:
                obs, done = obs.cpu().numpy(), done.cpu().numpy()
            assert obs.shape == (n, 33) and np.array_equal(_bits(obs[:, 9:]), _bits(book.blocks(a, done))), t
            assert env.observation_space.low[9:].min() <= obs[:, 9:].min() and obs[:, 9:].max() <= 1.0
            n_done += done
        assert n_done.min() >= 2
    finally:
        env.close(); plain.close()


def test_ppo_iteration_in_graph_mode_checkpoint_and_playback(tmp_path, capsys):
    import torch
    from gym_roboy_amd import visualize_agent
    from gym_roboy_amd.ppo import PPO
    env = _vec(_msj(), 512, action_delay=(0, 3), action_obs=3, seed=2, max_len=MAX_LEN)
    try:
        agent = PPO(env, n_steps=16, use_graphs=True, seed=3, normalize_obs=True)
        assert agent._fused is not None and agent._fused.obs_dim == 33
        roll = agent.collect()
        obs, act = roll["obs"], roll["act"]
        assert tuple(obs.shape[1:]) == (512, 33) and torch.isfinite(obs).all() and torch.isfinite(act).all()
        assert float(obs[..., 9:].abs().max()) <= 1.0 and bool((obs[..., 9:] != 0).any())
        stats = agent.update(roll)
        assert all(np.isfinite(v) for v in stats.values()) and all(torch.isfinite(p).all() for p in agent.policy.parameters())
        path = str(tmp_path / "model.pkl")
        agent.save(path)
        ck = torch.load(path, map_location="cpu")
        assert ck["env_io"] == {"sensor_noise": {}, "action_delay": [0, 3], "action_obs": 3}
        assert ck["policy"]["pi.0.weight"].shape[1] == 33 and ck["obs_norm"] is not None
        again = PPO(env, n_steps=16, use_graphs=True, seed=4, normalize_obs=True)
        again.load(path)
        for p, r in zip(again.policy.parameters(), agent.policy.parameters()):
            assert torch.equal(p, r)
    finally:
        env.close()
    total = visualize_agent.main([path, "--steps", "5", "--pause", "0"])
    assert np.isfinite(total) and capsys.readouterr().out.count("reward") == 5
