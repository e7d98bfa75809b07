"""The env layer's host code (gym_roboy_amd/csrc/env_host.hpp) held to what it did before it was gathered there: the four
rb_env_step*_dev entry points agree bit for bit, a reset / a statistics reset / re-issued configure calls leave every plane as the
recorded build left it (tests/golden/env_host_parent.npz, env_host_util.record_golden), every refusal keeps its code and text, and a
handle with every option gives its memory back."""
import ctypes

import numpy as np
import pytest

import env_host_util as u
from gym_roboy_amd import _native as nat

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
EINVAL, EUNSUP = nat.RB_EINVAL, nat.RB_EUNSUPPORTED


# ---- a. four entry points, one step ----
@pytest.mark.parametrize("n,integrator", [(512, "rk4"), (512, "euler"), (300, "rk4"), (300, "euler")])
def test_four_entry_points_one_step(n, integrator):
    """whole-batch against two ranges ([0, 256) and the rest: 256 envs, or a ragged block of 44) on a caller's stream, with and
    without the critic-row argument: after every step the outputs, after the last one every plane and the statistics are bit-equal"""
    import torch
    acts = u.actions(n, 8)
    for critic in (True, False):
        envs = [u.make(n, integrator, critic=critic), u.make(n, integrator, critic=critic)]
        try:
            whole, ranged = u.Raw(envs[0]), u.Raw(envs[1], stream=torch.cuda.Stream())
            for r in (whole, ranged):
                r.reset()
            ends = np.zeros(3, np.int64)
            for t, a in enumerate(acts):
                whole.step(a)
                ranged.step(a)
                ow, orr = whole.outputs(), ranged.outputs()
                assert set(ow) == {"obs", "reward", "done"} | ({"critic_arg"} if critic else set())
                for k in ow:
                    assert np.array_equal(ow[k], orr[k]), (critic, t, k)
                ends += np.bincount(ow["done"], minlength=3)[:3]
                if critic:                                           # the goal plane: the critic row's third block, exact
                    assert np.array_equal(ow["critic_arg"][:, 6:9], orr["critic_arg"][:, 6:9])
            assert ends[nat.RB_DONE_TERMINATED] > 0 and ends[nat.RB_DONE_TRUNCATED] > 0, ends
            pw, pr = whole.planes(), ranged.planes()
            assert set(pw) == set(pr) and {"level", "index", "row_counts", "done_kind", "ring"} <= set(pw)
            for k in pw:
                assert np.array_equal(pw[k], pr[k]), (critic, k)
            assert pw["row_counts"][0].sum() == ends[1] + ends[2] and pw["row_counts"][1].sum() > 0
            sw, sr = whole.stats(), ranged.stats()
            assert np.array_equal(sw, sr) and sw[6] == n * u.STEPS and sw[2] == ends[1] + ends[2] and sw[4] == ends[1]
        finally:
            for e in envs:
                e.close()


# ---- b. reset and reconfigure against the recorded build ----
@pytest.mark.parametrize("integrator", ["rk4", "euler"])
def test_reset_stats_reset_and_reconfigure_leave_the_recorded_planes(integrator):
    golden = np.load(u.GOLDEN)
    planes, refused = u.scenario(integrator)
    got = u.compact(planes)
    want = {k[len(integrator) + 1:]: golden[k] for k in golden.files if k.startswith(integrator + "/")}
    assert set(got) == set(want)
    stages = {k.split("/")[0] for k in got}
    assert stages == {"stepped", "reset", "stats_reset", "reconfigured"}
    bad = [k for k in sorted(got) if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    assert not bad, bad
    # the scenario did something: episodes ended both ways, the statistics reset cleared, the reconfigured handle starts over
    assert planes["stepped/stats"][2] > planes["stepped/stats"][4] > 0 and planes["stepped/row_counts"].sum() > 0
    assert planes["stats_reset/stats_before"][6] == 300 * (u.STEPS + 2) and not planes["stats_reset/stats"][:7].any()
    assert not planes["reconfigured/io_rows"].any() and not planes["reconfigured/done_kind"].any()
    assert np.array_equal(planes["reconfigured/row_counts"], planes["stats_reset/row_counts"])
    # once per handle, both of them
    assert refused == [(EINVAL, "goal curriculum: already configured (once per handle: a captured graph holds the arguments by value)"),
                       (EINVAL, "goal row stats: already enabled (once per handle: a captured graph holds the kernel it was captured with)")]


# ---- c. the refusals ----
NOT_CONFIGURED = "rb_env_configure has not been called"
NULL = "null argument"
ALIGN = "action slab must be 16-byte aligned"
NO_CURR = "no goal curriculum is configured (rb_env_goal_curriculum_configure)"
NO_STATS = "goal row stats are not enabled (rb_env_goal_row_stats_enable)"
NO_POOL = "no goal pool is set (rb_env_goal_pool_set)"
NO_IO = "no io configuration (rb_env_io_configure)"
NO_PARAMS = "per-env parameters are not enabled (rb_params_enable)"
NO_CRITIC = "critic rows are not enabled (rb_env_critic_obs_configure)"


class _Handles:
    """the handles the table's rows are tried on, made on first use and closed with the module"""

    def __init__(self):
        self.made = {}

    def get(self, state):
        if state not in self.made:
            self.made[state] = getattr(self, "_" + state)()
        return self.made[state]

    def close(self):
        for _, closer, _ in self.made.values():
            closer()

    @staticmethod
    def _bufs(sim, n, n_t, width=64):
        # (one slab serves every array argument: a refused call touches none of them)
        return sim.malloc(4 * n * max(n_t, width) + 64)

    def _sim(self, robot, n=256):
        from gym_roboy_amd.envs.simulations import HipBatchSimulation
        sim = HipBatchSimulation(robot, n, integrator="euler", seed=3)
        return sim, sim.close, self._bufs(sim, n, sim.n_t)

    def _vec(self, robot, n=256, **kw):
        from gym_roboy_amd.envs.vec_env import RoboyVecEnv
        env = RoboyVecEnv(robot, n, seed=3, max_episode_length=u.MAX_LEN, **kw)
        return env.sim, env.close, self._bufs(env.sim, n, env.n_t)

    def _fresh(self):                  # no rb_env_configure
        return self._sim(u.msj())

    def _env(self):                    # the env layer, no option
        return self._vec(u.msj(), 512)

    def _tree(self):                   # a joint tree with the env layer
        from gym_roboy_amd.envs.robots import UpperBodyRobot
        return self._vec(UpperBodyRobot())

    def _full(self):                   # every option
        env = u.make(512, "euler", params=True)
        return env.sim, env.close, self._bufs(env.sim, 512, env.n_t)

    def _pool(self):                   # a goal pool, no curriculum
        import goal_stats_util as gs
        robot = u.msj()
        return self._vec(robot, goals=gs.mixed_pool(robot.get_description()))

    def _curriculum(self):             # a curriculum, no row counts
        import goal_stats_util as gs
        robot = u.msj()
        return self._vec(robot, goals=gs.mixed_pool(robot.get_description()), goal_curriculum=2)

    def _critic_lost_params(self):     # critic rows with the parameter block, then rb_params_disable
        from gym_roboy_amd.envs.params import ParamRanges
        sim, closer, d = self._vec(u.msj(), randomization=ParamRanges(mass_scale=(0.9, 1.1)), critic_obs=("state", "params"))
        sim.disable_params()
        return sim, closer, d


@pytest.fixture(scope="module")
def handles():
    h = _Handles()
    yield h
    h.close()


def _io_cfg(**kw):
    cfg = nat.EnvIoConfig()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _env_cfg(**kw):
    cfg = nat.EnvConfig()
    cfg.max_episode_length = 5
    cfg.angle_lo, cfg.angle_hi, cfg.vel_lo, cfg.vel_hi, cfg.action_lo, cfg.action_hi = -1.0, 1.0, -1.0, 1.0, 0.0, 1.0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _step(lib, h, d, critic=False, rng=None, act=None, null=None):
    """one of the four env-step entry points with d for every array (act: another action pointer; null: that argument as NULL)"""
    args = [VP(d if act is None else act), VP(d), VP(d), VP(d)] + ([VP(d)] if critic else [])
    if null is not None:
        args[null] = None
    head = [h] + ([rng[0], rng[1], None] if rng else [])
    name = "rb_env_step%s%s_dev" % ("_range" if rng else "", "_critic" if critic else "")
    return getattr(lib, name)(*(head + args))


_u32 = ctypes.POINTER(ctypes.c_uint32)
_u64 = ctypes.POINTER(ctypes.c_uint64)
_out, _out2, _m = VP(), VP(), ctypes.c_int64()
_ref = ctypes.byref
_levels_too_high = np.full(256, 9, np.uint32)
_counts_bad = np.concatenate((np.zeros(7, np.uint64), np.ones(7, np.uint64)))
_order_twice = np.zeros(7, np.uint32)
_order_far = np.full(7, 7, np.uint32)
_row = np.zeros((1, 3), np.float32)
_rows_nan = np.full((7, 3), np.nan, np.float32)
_f4 = np.ones(4, np.float32)
_f_inf = np.full(4, np.inf, np.float32)
_lo = np.ones(20, np.float32)
_hi_low = np.zeros(20, np.float32)

# (name, state of the handle, call(lib, handle, device slab), code, text of rb_last_error)
REFUSALS = [
    # before rb_env_configure
    ("reset", "fresh", lambda L, h, d: L.rb_env_reset_dev(h, VP(d)), EINVAL, NOT_CONFIGURED),
    ("obs", "fresh", lambda L, h, d: L.rb_env_obs_configure(h, 1, None), EINVAL, NOT_CONFIGURED),
    ("io", "fresh", lambda L, h, d: L.rb_env_io_configure(h, _ref(_io_cfg())), EINVAL, NOT_CONFIGURED),
    ("action_obs", "fresh", lambda L, h, d: L.rb_env_action_obs_configure(h, 1), EINVAL, NOT_CONFIGURED),
    ("done_kind", "fresh", lambda L, h, d: L.rb_env_done_kind_configure(h, 1), EINVAL, NOT_CONFIGURED),
    ("critic", "fresh", lambda L, h, d: L.rb_env_critic_obs_configure(h, 1), EINVAL, NOT_CONFIGURED),
    ("curriculum", "fresh", lambda L, h, d: L.rb_env_goal_curriculum_configure(h, 2, 1, 1, 0), EINVAL, NOT_CONFIGURED),
    ("set_goal", "fresh", lambda L, h, d: L.rb_env_set_goal(h, nat.fptr(np.zeros((256, 3), np.float32)), None), EINVAL, NOT_CONFIGURED),
    ("step", "fresh", lambda L, h, d: _step(L, h, d), EINVAL, NOT_CONFIGURED),
    ("step_critic", "fresh", lambda L, h, d: _step(L, h, d, critic=True), EINVAL, NOT_CONFIGURED),
    ("step_range", "fresh", lambda L, h, d: _step(L, h, d, rng=(0, 256)), EINVAL, NOT_CONFIGURED),
    ("step_range_critic", "fresh", lambda L, h, d: _step(L, h, d, critic=True, rng=(0, 256)), EINVAL, NOT_CONFIGURED),
    # rb_env_configure's own
    ("configure_null", "fresh", lambda L, h, d: L.rb_env_configure(h, None), EINVAL, NULL),
    ("configure_length", "fresh", lambda L, h, d: L.rb_env_configure(h, _ref(_env_cfg(max_episode_length=0))), EINVAL,
     "max_episode_length must be >= 1"),
    ("configure_box", "fresh", lambda L, h, d: L.rb_env_configure(h, _ref(_env_cfg(angle_hi=-1.0))), EINVAL, "empty box in env config"),
    # unknown mask bits, values out of range
    ("obs_bits", "env", lambda L, h, d: L.rb_env_obs_configure(h, 0x10, None), EINVAL,
     "unknown bits in the channel mask (RB_OBS_LENGTH | RB_OBS_RATE | RB_OBS_ACTIVATION | RB_OBS_FORCE)"),
    ("obs_scale", "env", lambda L, h, d: L.rb_env_obs_configure(h, 1, nat.fptr(_f_inf)), EINVAL, "channel scales must be finite"),
    ("critic_bits", "env", lambda L, h, d: L.rb_env_critic_obs_configure(h, 0x20), EINVAL,
     "unknown bits in the critic-row mask (RB_CRITIC_STATE | _AGE | _PARAMS | _DELAY | _ACTIONS)"),
    ("io_sigma", "env", lambda L, h, d: L.rb_env_io_configure(h, _ref(_io_cfg(sigma_q=-1.0))), EINVAL,
     "sensor-noise standard deviations must be finite and >= 0"),
    ("io_delay", "env", lambda L, h, d: L.rb_env_io_configure(h, _ref(_io_cfg(delay_lo=2, delay_hi=1))), EINVAL,
     "action delay: 0 <= delay_lo <= delay_hi <= RB_IO_MAX_DELAY"),
    ("action_rows", "env", lambda L, h, d: L.rb_env_action_obs_configure(h, 9), EINVAL,
     "action rows in the observation: 0 <= rows <= RB_ACTION_OBS_MAX"),
    ("pool_m", "env", lambda L, h, d: L.rb_env_goal_pool_set(h, nat.fptr(_row), 0), EINVAL, "goal pool: m must be >= 1 (and below 2^32)"),
    ("pool_nan", "env", lambda L, h, d: L.rb_env_goal_pool_set(h, nat.fptr(_rows_nan), 7), EINVAL,
     "goal pool: row 0, joint 0 is not finite or outside the angle box"),
    ("pool_other_m", "pool", lambda L, h, d: L.rb_env_goal_pool_set(h, nat.fptr(_row), 1), EINVAL,
     "goal pool: the handle's pool has 7 rows, fixed by the first call; got 1"),
    ("curriculum_levels", "pool", lambda L, h, d: L.rb_env_goal_curriculum_configure(h, 8, 1, 1, 0), EINVAL,
     "goal curriculum: levels must be in 1..7 (at most the pool's rows and RB_GOAL_LEVELS_MAX = 256), got 8"),
    ("curriculum_moves", "pool", lambda L, h, d: L.rb_env_goal_curriculum_configure(h, 2, -1, 1, 0), EINVAL,
     "goal curriculum: up and down must be >= 0"),
    ("curriculum_level0", "pool", lambda L, h, d: L.rb_env_goal_curriculum_configure(h, 2, 1, 1, 2), EINVAL,
     "goal curriculum: level0 must be in 0..levels - 1"),
    ("levels_high", "curriculum", lambda L, h, d: L.rb_env_goal_levels_set(h, _levels_too_high.ctypes.data_as(_u32)), EINVAL,
     "goal levels: env 0 has level 9, the curriculum has 2 levels"),
    ("counts_bad", "full", lambda L, h, d: L.rb_env_goal_row_stats_set(h, _counts_bad.ctypes.data_as(_u64)), EINVAL,
     "goal row stats: row 0 has reached 1 > attempts 0"),
    ("permute_twice", "pool", lambda L, h, d: L.rb_env_goal_pool_permute(h, _order_twice.ctypes.data_as(_u32)), EINVAL,
     "goal pool permute: row 0 occurs twice (not a permutation)"),
    ("permute_far", "pool", lambda L, h, d: L.rb_env_goal_pool_permute(h, _order_far.ctypes.data_as(_u32)), EINVAL,
     "goal pool permute: entry 0 is 7, the pool has 7 rows"),
    ("ranges_lo_hi", "full", lambda L, h, d: L.rb_params_set_ranges(h, nat.fptr(_lo), nat.fptr(_hi_low), 1), EINVAL, "parameter 0: lo > hi"),
    # joint trees
    ("obs_tree", "tree", lambda L, h, d: L.rb_env_obs_configure(h, 1, None), EUNSUP,
     "tendon channels in the observation are built for ball-joint robots (1-16 tendons); a joint tree's readout is rb_tendon_state_dev"),
    ("io_tree", "tree", lambda L, h, d: L.rb_env_io_configure(h, _ref(_io_cfg())), EUNSUP,
     "action latency and sensor noise are built for ball-joint robots (1-16 tendons); joint trees have none"),
    ("action_obs_tree", "tree", lambda L, h, d: L.rb_env_action_obs_configure(h, 1), EUNSUP,
     "action columns in the observation are built for ball-joint robots (1-16 tendons); joint trees have none"),
    ("critic_tree", "tree", lambda L, h, d: L.rb_env_critic_obs_configure(h, 1), EUNSUP,
     "critic rows are built for ball-joint robots (1-16 tendons); joint trees have none"),
    ("params_tree", "tree", lambda L, h, d: L.rb_params_enable(h, None), EUNSUP,
     "per-env parameters are built for ball-joint robots (the closed-form kernels); joint trees have none"),
    ("step_critic_tree", "tree", lambda L, h, d: _step(L, h, d, critic=True), EINVAL, NO_CRITIC),
    # needs X first
    ("critic_params", "env", lambda L, h, d: L.rb_env_critic_obs_configure(h, nat.RB_CRITIC_PARAMS), EINVAL,
     "critic rows: RB_CRITIC_PARAMS needs per-env parameters (rb_params_enable first)"),
    ("critic_delay", "env", lambda L, h, d: L.rb_env_critic_obs_configure(h, nat.RB_CRITIC_DELAY), EINVAL,
     "critic rows: RB_CRITIC_DELAY needs an io configuration (rb_env_io_configure first)"),
    ("critic_actions", "env", lambda L, h, d: L.rb_env_critic_obs_configure(h, nat.RB_CRITIC_ACTIONS), EINVAL,
     "critic rows: RB_CRITIC_ACTIONS needs action rows in the observation (rb_env_action_obs_configure first)"),
    ("curriculum_pool", "env", lambda L, h, d: L.rb_env_goal_curriculum_configure(h, 2, 1, 1, 0), EINVAL,
     "goal curriculum: no goal pool is set (rb_env_goal_pool_set first)"),
    ("stats_enable", "pool", lambda L, h, d: L.rb_env_goal_row_stats_enable(h), EINVAL, NO_CURR),
    ("level_ptr", "pool", lambda L, h, d: L.rb_env_goal_level_ptr(h, _ref(_out)), EINVAL, NO_CURR),
    ("index_ptr", "env", lambda L, h, d: L.rb_env_goal_index_ptr(h, _ref(_out)), EINVAL, NO_CURR),
    ("levels_set", "env", lambda L, h, d: L.rb_env_goal_levels_set(h, _levels_too_high.ctypes.data_as(_u32)), EINVAL, NO_CURR),
    ("level_hist", "env", lambda L, h, d: L.rb_env_goal_level_hist(h, _counts_bad.ctypes.data_as(_u64)), EINVAL, NO_CURR),
    ("level_hist_dev", "env", lambda L, h, d: L.rb_env_goal_level_hist_dev(h, VP(d), None), EINVAL, NO_CURR),
    ("stats_ptr", "curriculum", lambda L, h, d: L.rb_env_goal_row_stats_ptr(h, _ref(_out), _ref(_m)), EINVAL, NO_STATS),
    ("stats_read", "curriculum", lambda L, h, d: L.rb_env_goal_row_stats_read(h, _counts_bad.ctypes.data_as(_u64), 0), EINVAL, NO_STATS),
    ("stats_set", "env", lambda L, h, d: L.rb_env_goal_row_stats_set(h, _counts_bad.ctypes.data_as(_u64)), EINVAL, NO_STATS),
    ("pool_ptr", "env", lambda L, h, d: L.rb_env_goal_pool_ptr(h, _ref(_out), _ref(_m)), EINVAL, NO_POOL),
    ("permute", "env", lambda L, h, d: L.rb_env_goal_pool_permute(h, _order_twice.ctypes.data_as(_u32)), EINVAL, NO_POOL),
    ("done_kind_ptr", "env", lambda L, h, d: L.rb_env_done_kind_ptr(h, _ref(_out)), EINVAL,
     "episode-end codes are not enabled (rb_env_done_kind_configure)"),
    ("critic_ptr", "env", lambda L, h, d: L.rb_env_critic_obs_ptr(h, _ref(_out)), EINVAL, NO_CRITIC),
    ("step_critic_none", "env", lambda L, h, d: _step(L, h, d, critic=True), EINVAL, NO_CRITIC),
    ("step_range_critic_none", "env", lambda L, h, d: _step(L, h, d, critic=True, rng=(0, 256)), EINVAL, NO_CRITIC),
    ("io_ptr", "env", lambda L, h, d: L.rb_env_io_ptr(h, _ref(_out), None, None, None, None), EINVAL, NO_IO),
    ("io_sample", "env", lambda L, h, d: L.rb_env_io_sample_delay_dev(h, None), EINVAL, NO_IO),
    ("params_ptr", "env", lambda L, h, d: L.rb_params_ptr(h, _ref(_out), _ref(_out2)), EINVAL, NO_PARAMS),
    ("params_ranges", "env", lambda L, h, d: L.rb_params_set_ranges(h, nat.fptr(_lo), nat.fptr(_lo), 0), EINVAL, NO_PARAMS),
    ("params_sample", "env", lambda L, h, d: L.rb_params_sample_dev(h, None), EINVAL, NO_PARAMS),
    # already configured / enabled
    ("curriculum_again", "full", lambda L, h, d: L.rb_env_goal_curriculum_configure(h, 4, 1, 1, 1), EINVAL,
     "goal curriculum: already configured (once per handle: a captured graph holds the arguments by value)"),
    ("stats_again", "full", lambda L, h, d: L.rb_env_goal_row_stats_enable(h), EINVAL,
     "goal row stats: already enabled (once per handle: a captured graph holds the kernel it was captured with)"),
    # an option the critic rows depend on is gone
    ("critic_lost_step", "critic_lost_params", lambda L, h, d: _step(L, h, d), EINVAL,
     "an option the critic rows depend on changed after rb_env_critic_obs_configure: configure the rows again"),
    ("critic_lost_step_range_critic", "critic_lost_params", lambda L, h, d: _step(L, h, d, critic=True, rng=(0, 256)), EINVAL,
     "an option the critic rows depend on changed after rb_env_critic_obs_configure: configure the rows again"),
    ("critic_lost_reset", "critic_lost_params", lambda L, h, d: L.rb_env_reset_dev(h, VP(d)), EINVAL,
     "an option the critic rows depend on changed after rb_env_critic_obs_configure: configure the rows again"),
    # ranges
    ("range_outside", "env", lambda L, h, d: _step(L, h, d, rng=(256, 512)), EINVAL, "range outside the batch"),
    ("range_negative", "env", lambda L, h, d: _step(L, h, d, rng=(-256, 256)), EINVAL, "range outside the batch"),
    ("range_empty", "full", lambda L, h, d: _step(L, h, d, critic=True, rng=(256, 0)), EINVAL, "range outside the batch"),
    ("range_start", "env", lambda L, h, d: _step(L, h, d, rng=(128, 256)), EINVAL, "a range starts at a multiple of 256 envs"),
    ("range_start_critic", "full", lambda L, h, d: _step(L, h, d, critic=True, rng=(255, 1)), EINVAL, "a range starts at a multiple of 256 envs"),
    # unaligned action slabs
    ("align", "env", lambda L, h, d: _step(L, h, d, act=d + 4), EINVAL, ALIGN),
    ("align_range", "env", lambda L, h, d: _step(L, h, d, act=d + 8, rng=(0, 256)), EINVAL, ALIGN),
    ("align_critic", "full", lambda L, h, d: _step(L, h, d, critic=True, act=d + 4), EINVAL, ALIGN),
    ("align_range_critic", "full", lambda L, h, d: _step(L, h, d, critic=True, act=d + 12, rng=(256, 256)), EINVAL, ALIGN),
    # null arguments
    ("null_act", "env", lambda L, h, d: _step(L, h, d, null=0), EINVAL, NULL),
    ("null_done", "env", lambda L, h, d: _step(L, h, d, null=3, rng=(0, 256)), EINVAL, NULL),
    ("null_cobs", "full", lambda L, h, d: _step(L, h, d, critic=True, null=4), EINVAL, NULL),
    ("null_cobs_range", "full", lambda L, h, d: _step(L, h, d, critic=True, null=4, rng=(0, 256)), EINVAL, NULL),
    ("null_handle", "env", lambda L, h, d: _step(L, None, d), EINVAL, NULL),
    ("null_handle_obs", "env", lambda L, h, d: L.rb_env_obs_configure(None, 1, None), EINVAL, "null simulation handle"),
    ("null_handle_curriculum", "env", lambda L, h, d: L.rb_env_goal_curriculum_configure(None, 2, 1, 1, 0), EINVAL, "null simulation handle"),
    ("null_handle_counts", "env", lambda L, h, d: L.rb_env_goal_row_stats_set(None, _counts_bad.ctypes.data_as(_u64)), EINVAL,
     "null simulation handle"),
    ("null_handle_params", "env", lambda L, h, d: L.rb_params_disable(None), EINVAL, "null simulation handle"),
    ("null_stats", "env", lambda L, h, d: L.rb_env_stats(h, None, 0), EINVAL, NULL),
    ("null_stats_dev", "env", lambda L, h, d: L.rb_env_stats_dev(h, None, 0), EINVAL, NULL),
    ("null_obs_dim", "env", lambda L, h, d: L.rb_env_obs_dim(h, None), EINVAL, NULL),
    ("null_pool", "env", lambda L, h, d: L.rb_env_goal_pool_set(h, None, 7), EINVAL, NULL),
    ("null_pool_ptr", "pool", lambda L, h, d: L.rb_env_goal_pool_ptr(h, None, _ref(_m)), EINVAL, NULL),
    ("null_level_ptr", "curriculum", lambda L, h, d: L.rb_env_goal_level_ptr(h, None), EINVAL, NULL),
    ("null_levels", "curriculum", lambda L, h, d: L.rb_env_goal_levels_set(h, None), EINVAL, NULL),
    ("null_counts", "full", lambda L, h, d: L.rb_env_goal_row_stats_read(h, None, 0), EINVAL, NULL),
    ("null_order", "pool", lambda L, h, d: L.rb_env_goal_pool_permute(h, None), EINVAL, NULL),
    ("null_kind_ptr", "full", lambda L, h, d: L.rb_env_done_kind_ptr(h, None), EINVAL, NULL),
    ("null_critic_ptr", "full", lambda L, h, d: L.rb_env_critic_obs_ptr(h, None), EINVAL, NULL),
    ("null_ranges", "full", lambda L, h, d: L.rb_params_set_ranges(h, None, nat.fptr(_lo), 0), EINVAL, NULL),
]


@pytest.mark.parametrize("name,state,call,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_keeps_its_code_and_text(handles, name, state, call, code, text):
    sim, _, d = handles.get(state)
    lib = sim._lib
    assert call(lib, sim.handle, d) == code
    assert lib.rb_last_error().decode() == text


def test_refused_handles_still_step(handles):
    """behind the whole table: the handle with every option steps, resets and reports as if nothing had been asked of it"""
    sim, _, d = handles.get("full")
    lib, h, n = sim._lib, sim.handle, 512
    bufs = [sim.malloc(4 * n * 64) for _ in range(5)]
    nat.check(lib.rb_env_reset_dev(h, VP(bufs[1])))
    sim.upload(bufs[0], np.zeros((n, 8), np.float32))
    for _ in range(u.MAX_LEN):
        nat.check(lib.rb_env_step_critic_dev(h, *[VP(b) for b in bufs]))
    out = (ctypes.c_double * 8)()
    nat.check(lib.rb_env_stats(h, out, 0))
    assert out[2] >= n and out[6] >= n * u.MAX_LEN


# ---- d. release ----
def test_a_handle_with_every_option_gives_its_memory_back():
    """20 handles with every option, one after the other: what the device has free after the last is what it had after the first,
    within what the first one itself left behind (code objects, the runtime's pools: the allocation granule, read off, not assumed)"""
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def once():
        env = u.make(512, "rk4", params=True)
        try:
            raw = u.Raw(env)
            raw.reset()
            raw.step(np.zeros((512, 8), np.float32))
        finally:
            env.close()

    before = free()
    once()
    first = free()
    granule = abs(before - first)
    for _ in range(19):
        once()
    last = free()
    print("free bytes: before %d, after the first handle %d, after the 20th %d (granule %d)" % (before, first, last, granule))
    assert abs(last - first) <= granule
