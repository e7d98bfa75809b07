"""The env layer's host code seen through the C entry points (gym_roboy_amd/csrc/env_host.hpp): handles with every option
switched on, stepped by the raw rb_env_step*_dev calls, and every plane a getter exposes read back - shared by
tests/test_env_host_gpu.py, and the generator of tests/golden/env_host_parent.npz (record_golden)."""
import ctypes
import hashlib
import os

import numpy as np

import goal_stats_util as gs
from gym_roboy_amd import _native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_host_parent.npz")
SEED, MAX_LEN, STEPS = 7, 5, 12
CRITIC = ("state", "age", "delay", "actions")
SIGMA = {"q": 0.01, "qd": 0.05}
CURRICULUM = dict(levels=4, up=1, down=1, start=1)
HEAD = 16          # envs whose rows of a wide float plane the golden file keeps verbatim; the whole plane goes in as a SHA-256
VP = ctypes.c_void_p


def msj():
    from gym_roboy_amd.envs.robots import MsjRobot
    return MsjRobot()


def make(n, integrator, critic=True, params=False, seed=SEED):
    """MsjRobot, every option of the env layer: goal pool + curriculum + row counts, action delay and sensor noise, two action rows,
    episode-end codes and (critic) the critic rows; params: per-env parameters too"""
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = msj()
    ranges = ParamRanges(force_scale=(0.7, 1.3), setpoint_offset=(-0.02, 0.02), mass_scale=(0.6, 1.6), damping_scale=(0.5, 2.0))
    return RoboyVecEnv(robot, n, seed=seed, max_episode_length=MAX_LEN, integrator=integrator, goals=gs.mixed_pool(robot.get_description()),
                       goal_curriculum=dict(CURRICULUM), goal_row_stats=True, critic_obs=CRITIC if critic else None, action_delay=(0, 3),
                       action_obs=2, sensor_noise=dict(SIGMA), report_truncation=True, randomization=ranges if params else None)


def actions(n, n_t, steps=STEPS, seed=SEED):
    """random actions for the odd envs, zero actions (which reach the pool's zero pose from rest) for the even ones"""
    a = np.random.default_rng(seed).uniform(-1, 1, (steps, n, n_t)).astype(np.float32)
    a[:, ::2] = 0.0
    return a


class Raw:
    """A RoboyVecEnv's handle driven through the C entry points: buffers of its own, whole-batch or two-range steps"""

    def __init__(self, env, stream=None):
        self.env, self.sim, self.lib, self.h = env, env.sim, env.sim._lib, env.sim.handle
        self.n, self.n_t, self.od, self.dc = env.num_envs, env.n_t, env.obs_dim, env.critic_obs_dim
        m = self.sim.malloc
        self.d_act, self.d_obs, self.d_rew, self.d_done = m(4 * self.n * self.n_t), m(4 * self.n * self.od), m(4 * self.n), m(4 * self.n)
        self.d_cobs = m(4 * self.n * self.dc) if self.dc else None
        self.stream = stream                                        # a torch.cuda.Stream: step in two ranges on it

    def sync(self):
        if self.stream is not None:
            self.stream.synchronize()
        self.sim.synchronize()

    def reset(self):
        if self.env.randomization is not None:
            self.sim.sample_params()
        nat.check(self.lib.rb_env_reset_dev(self.h, VP(self.d_obs)))
        self.sync()

    def step(self, act):
        self.sim.upload(self.d_act, act)
        args = [VP(self.d_act), VP(self.d_obs), VP(self.d_rew), VP(self.d_done)]
        if self.stream is None:
            rc = self.lib.rb_env_step_critic_dev(self.h, *args, VP(self.d_cobs)) if self.dc else self.lib.rb_env_step_dev(self.h, *args)
            nat.check(rc)
        else:
            for first, cnt in ((0, 256), (256, self.n - 256)):
                head = [self.h, first, cnt, VP(self.stream.cuda_stream)] + args
                nat.check(self.lib.rb_env_step_range_critic_dev(*head, VP(self.d_cobs)) if self.dc else self.lib.rb_env_step_range_dev(*head))
        self.sync()

    def outputs(self):
        dl = self.sim.download
        out = {"obs": dl(self.d_obs, (self.n, self.od)), "reward": dl(self.d_rew, (self.n,)), "done": dl(self.d_done, (self.n,), np.uint32)}
        if self.dc:
            out["critic_arg"] = dl(self.d_cobs, (self.n, self.dc))
        return out

    def stats(self, reset=False):
        out = (ctypes.c_double * 8)()
        nat.check(self.lib.rb_env_stats(self.h, out, int(reset)))
        return np.array(out[:], np.float64)

    def planes(self):
        """every plane a getter of the env layer exposes, as the device holds it"""
        self.sync()
        dl, n = self.sim.download, self.n
        io = self.sim.io_ptrs()
        out = {"io_delay": dl(io["delay"], (n,), np.uint32), "io_draws": dl(io["delay_draws"], (n,), np.uint32),
               "io_rows": dl(io["rows"], (n,), np.uint32), "io_slots": np.array([io["slots"]]),
               "ring": dl(io["history"], (io["slots"], n, self.n_t))}
        p = VP()
        nat.check(self.lib.rb_env_done_kind_ptr(self.h, ctypes.byref(p)))
        out["done_kind"] = dl(p.value, (n,), np.uint32)
        if self.dc:
            nat.check(self.lib.rb_env_critic_obs_ptr(self.h, ctypes.byref(p)))
            out["critic"] = dl(p.value, (n, self.dc))
        nat.check(self.lib.rb_env_goal_level_ptr(self.h, ctypes.byref(p)))
        out["level"] = dl(p.value, (n,), np.uint32)
        nat.check(self.lib.rb_env_goal_index_ptr(self.h, ctypes.byref(p)))
        out["index"] = dl(p.value, (n,), np.uint32)
        m = ctypes.c_int64()
        nat.check(self.lib.rb_env_goal_row_stats_ptr(self.h, ctypes.byref(p), ctypes.byref(m)))
        out["row_counts"] = dl(p.value, (2, m.value), np.uint64)
        nat.check(self.lib.rb_env_goal_pool_ptr(self.h, ctypes.byref(p), ctypes.byref(m)))
        out["pool"] = dl(p.value, (m.value, self.env.n_q))
        hist = np.zeros(CURRICULUM["levels"], np.uint64)
        nat.check(self.lib.rb_env_goal_level_hist(self.h, hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        out["level_hist"] = hist
        if self.env.randomization is not None:
            out["params"] = self.sim.get_param_planes()
            out["param_draws"] = self.sim.get_param_draws()
        return out


# ---- case b: reset, statistics reset and re-issued configure calls ----
def reconfigure(raw):
    """every *_configure of the handle's options once more with the arguments it was configured with; -> the return codes and messages
    of the two that are once per handle"""
    env, lib, h = raw.env, raw.lib, raw.h
    pool = gs.mixed_pool(env.robot.get_description())
    nat.check(lib.rb_env_configure(h, ctypes.byref(env._cfg)))
    nat.check(lib.rb_env_goal_pool_set(h, nat.fptr(pool), pool.shape[0]))
    refused = []
    for call in (lambda: lib.rb_env_goal_curriculum_configure(h, CURRICULUM["levels"], CURRICULUM["up"], CURRICULUM["down"], CURRICULUM["start"]),
                 lambda: lib.rb_env_goal_row_stats_enable(h)):
        refused.append((call(), lib.rb_last_error().decode()))
    nat.check(lib.rb_env_obs_configure(h, 0, None))
    if env.randomization is not None:
        raw.sim.enable_params()
        raw.sim.set_param_ranges(env.randomization, resample_on_reset=True)
    io = nat.EnvIoConfig()
    io.sigma_q, io.sigma_qd = SIGMA["q"], SIGMA["qd"]
    io.delay_lo, io.delay_hi, io.resample_on_reset = 0, 3, 1
    raw.sim.configure_io(io)
    raw.sim.configure_action_obs(2)
    nat.check(lib.rb_env_done_kind_configure(h, 1))
    nat.check(lib.rb_env_critic_obs_configure(h, sum(1 << nat.CRITIC_OBS_BLOCKS.index(c) for c in CRITIC)))
    return refused


def scenario(integrator, n=300):
    """-> {"<stage>/<plane>": array}: the planes after STEPS steps, then after rb_env_reset_dev, after two more steps and
    rb_env_stats(reset=1), and after every configure call was issued again; and the refusals of the once-per-handle calls"""
    env = make(n, integrator, params=True)
    try:
        raw = Raw(env)
        acts = actions(n, env.n_t, STEPS + 2)
        out = {}

        def snap(stage, **more):
            for k, v in dict(raw.planes(), **more).items():
                out["%s/%s" % (stage, k)] = v
        raw.reset()
        for a in acts[:STEPS]:
            raw.step(a)
        snap("stepped", stats=raw.stats(), **raw.outputs())
        raw.reset()
        snap("reset", stats=raw.stats(), obs=raw.outputs()["obs"])
        for a in acts[STEPS:]:
            raw.step(a)
        before = raw.stats(reset=True)
        snap("stats_reset", stats_before=before, stats=raw.stats())
        refused = reconfigure(raw)
        snap("reconfigured", stats=raw.stats())
        return out, refused
    finally:
        env.close()


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def compact(planes):
    """what the golden file keeps of a scenario: small planes verbatim; of a float plane with rows per env the first HEAD envs' rows
    and the SHA-256 of the whole"""
    out = {}
    for k, v in planes.items():
        v = np.asarray(v)
        if v.dtype == np.float32 and v.nbytes > 4096:
            env_axis = 1 if k.endswith(("/ring", "/params")) else 0
            out[k + "@head"] = np.take(v, np.arange(HEAD), axis=env_axis)
            out[k + "@sha256"] = np.array(digest(v))
        else:
            out[k] = v
    return out


def record_golden(path=GOLDEN):
    """Write the golden file from the library that is loaded (the build BEFORE a change to the env layer's host code): run once on a
    GPU, `python -c "import sys; sys.path.insert(0, 'tests'); import env_host_util as u; u.record_golden()"`."""
    out = {}
    for integrator in ("rk4", "euler"):
        planes, _ = scenario(integrator)
        for k, v in compact(planes).items():
            out["%s/%s" % (integrator, k)] = v
    np.savez_compressed(path, **out)
    return out
