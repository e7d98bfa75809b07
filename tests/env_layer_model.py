"""TEST HELPER: ONE host model of the fused env layer with several options on at once - ``EnvLayerModel``, driven by
(seed, options, actions) alone.  It is ``host_env_model.HostEnvModel`` (the env-step and reset kernels: physics from a plain stepper,
box goals from oracle/philox_np.py, reward and done from envs/reward.py in float64) plus one block per line of §6's order, each block
built from the option's own restatement (push_util, shaping_util, goal_pool_util, goal_curriculum_util, start_pose_util,
episode_log_util).  Hold this file against the list in csrc/env_host.hpp ("what runs behind an env step and behind a reset"): the
stage numbers in the comments are that list's.

What the model never does: read the env under test.  ONE device value is adopted, behind a check against the model's own float64
value: the push impulse plane (``step(actions, impulse=...)``; the device's fp32 Box-Muller differs from sigma z64 in the last bits and
the velocity feeds back into the state).  Goal rows, start rows, levels, counters and every decision are the model's own.

Options the model states: goals (pool), goal_curriculum, goal_row_stats, report_truncation, critic_obs ("state", "age", "params",
"delay", "actions"), reward_shaping, push, episode_log, start_poses, randomization, action_delay, sensor_noise (q, qd),
action_obs.  The drawn parameters are the model's own: tests/test_env_params_gpu.py holds the device's draw to the restatement bit
for bit, so nothing is adopted.  tendon_obs: the columns are env_obs_util.expected_columns at the state the row reports, within the
readout's tolerances (plus the noise's where both are set).  A new option adds a stage block here and a key to CASES."""
import numpy as np

import env_io_util as iu
import env_obs_util as ou
import env_params_util as epu
import episode_log_util as eu
import goal_curriculum_util as gc
import goal_pool_util as gp
import push_util as pu
import shaping_util as shu
import start_pose_util as su
from action_obs_util import HistoryBook, clip_action
from env_io_util import NOISE_TOL as SENSOR_NOISE_TOL      # with 4 ulp of the reported value (tests/test_env_io_gpu.py: _check_noise)
from host_env_model import REWARD_ATOL, REWARD_RTOL, HostEnvModel
from push_util import NOISE_TOL as PUSH_NOISE_TOL          # relative to sigma (tests/test_push_gpu.py)

MARGIN = 1e-5                             # the done test's distance from its thresholds below which fp32 and float64 may differ
STEP_STAGES = ("0", "1", "1a", "2", "3", "4")


# ---- steppers: step(sp), reset(mask), state(), set_state(mask, q, qd), add_velocity(mask, dv), set_params(mask, par) ----
class _StepperRules:
    """the two rules every stepper shares, in float32 as the kernels state them"""

    def set_state(self, mask, q, qd):
        """the masked envs take the pose q [n, n_q] and the velocity qd, and are feasible"""
        sq, sqd, sf = self.state()
        sq[mask], sqd[mask], sf[mask] = q[mask], qd[mask], True
        self._write(sq, sqd, sf)

    def add_velocity(self, mask, dv):
        """qd <- clamp(fl32(qd + dv), -qd_max, qd_max) for the masked envs -> [n, n_q] bool: the joints the clamp changed"""
        sq, sqd, sf = self.state()
        moved = (sqd + np.asarray(dv, np.float32)).astype(np.float32)
        new = np.clip(moved, -self.qd_max, self.qd_max).astype(np.float32)
        sqd[mask] = new[mask]
        self._write(sq, sqd, sf)
        return (new != moved) & np.asarray(mask, bool)[:, None]


class OracleStepper(_StepperRules):
    """the fp32 C oracle (host_env_model.COracleStepper with an integrator and the two rules)"""

    def __init__(self, robot, n, integrator="euler"):
        from oracle.c_oracle import COracle
        desc = robot.get_description()
        self.orc, self.integ = COracle(desc, "f32"), 0 if integrator == "euler" else 1
        self.qd_max = np.asarray(desc.qd_max, np.float32)
        self.q, self.qd = np.zeros((n, desc.n_q), np.float32), np.zeros((n, desc.n_q), np.float32)
        self.f = np.ones(n, np.uint8)

    def step(self, sp):
        self.orc.step_inplace(self.q, self.qd, np.ascontiguousarray(sp, dtype=np.float32), self.f, integrator=self.integ)
        return self.state()

    def reset(self, mask):
        self.q[mask] = 0; self.qd[mask] = 0; self.f[mask] = 1

    def state(self):
        return self.q.copy(), self.qd.copy(), self.f.astype(bool)

    def _write(self, q, qd, f):
        self.q[:], self.qd[:], self.f[:] = q, qd, f

    def close(self):
        pass


class ParamOracleStepper(_StepperRules, epu.PerEnvOracle):
    """env_params_util.PerEnvOracle - the C oracle with each env on its own description, the base of that module's own stepper -
    nominal until the model hands its draws in (set_params): the model owns the draws"""

    def __init__(self, robot, n, integrator="euler"):
        desc = robot.get_description()
        nominal = np.concatenate([np.ones(desc.n_t), np.zeros(desc.n_t), np.ones(4)]).astype(np.float32)
        epu.PerEnvOracle.__init__(self, robot, n, np.tile(nominal, (n, 1)), integrator)
        self.qd_max = np.asarray(desc.qd_max, np.float32)

    def reset(self, mask):
        self.zero(mask)

    def state(self):
        return self.q.copy(), self.qd.copy(), self.f.copy()

    def _write(self, q, qd, f):
        self.q[:], self.qd[:], self.f[:] = q, qd, f

    def close(self):
        pass


class PlainKernelStepper(_StepperRules):
    """a plain HipBatchSimulation in the kernel form the fused env step takes (host_env_model.HipStepper): the state planes then
    compare without a tolerance.  (So this handle's own offset planes are never non-zero: tests/test_env_params_gpu.py covers
    those.)  With parameters the two kernels state the activation offset differently: the env step
    (RB_MSJ_PARAMS_ENV_STEP_BODY) rounds (set-point + offset) and multiplies by ksg, the plain step (msj_params_step) adds
    set-point ksg and offset ksg.  So this stepper keeps the handle's offset planes at zero and adds the offsets to the set-points
    itself, in float32 - the plain kernel's fl32(sp' ksg + 0 ksg) is then the env step's fl32(fl32(sp + offset) ksg)."""

    def __init__(self, robot, n, seed, env_id_offset=0, integrator="euler", kernel=1, params=False, tree_kernel=None, batch=None):
        from host_env_model import HipStepper
        # ``batch``: the handle's own env count where it has to differ from n - the env step with tendon channels runs the
        # large-batch env-per-lane text at every size, which a plain handle of a kernarg 8-tendon robot takes above
        # 65 536 envs only; the model's envs are the first n of such a handle, the others rest at the zero pose
        self.n, self.batch = n, batch or n
        self.inner = HipStepper(robot, self.batch, seed, env_id_offset, integrator, kernel)
        self.sim = self.inner.sim
        if tree_kernel is not None:      # a joint tree in a form the batch size would not choose (the env under test selects it too)
            self.sim.select_kernel(tree_kernel)
        if params:                       # the parameter kernels, every env nominal until set_params
            self.sim.enable_params()
        desc = robot.get_description()
        self.qd_max = np.asarray(desc.qd_max, np.float32)
        self.nt, self.offset = desc.n_t, np.zeros((n, desc.n_t), np.float32)

    def _padded(self, x, fill=0):
        x = np.asarray(x)
        if self.batch == self.n:
            return x
        out = np.full((self.batch,) + x.shape[1:], fill, x.dtype)
        out[:self.n] = x
        return out

    def step(self, sp):
        self.inner.step(self._padded((np.asarray(sp, np.float32) + self.offset).astype(np.float32)))
        return self.state()

    def reset(self, mask):
        self.inner.reset(self._padded(np.asarray(mask, bool)))

    def state(self):
        return tuple(x[:self.n].copy() for x in self.sim.read_state())

    def _write(self, q, qd, f):
        self.sim.set_state(self._padded(q), self._padded(qd), self._padded(f, 1))

    def set_params(self, mask, par):
        assert self.batch == self.n
        planes = self.sim.get_param_planes()
        planes[:, mask] = np.asarray(par, np.float32)[mask].T
        self.offset[mask] = np.asarray(par, np.float32)[mask, self.nt:2 * self.nt]
        planes[self.nt:2 * self.nt] = 0.0
        self.sim.upload(self.sim.params_ptr()[0], np.ascontiguousarray(planes))
        self.sim.synchronize()

    def close(self):
        self.inner.close()


# ---- the model ----
class EnvLayerModel(HostEnvModel):
    """``RoboyVecEnv``'s keywords; ``stepper`` as above.  ``behind_step_order``: TEST-ONLY, a permutation of STEP_STAGES - the order
    sensitivity test swaps neighbours to show that the cases can see §6's order."""

    def __init__(self, robot, stepper, n, seed, env_id_offset=0, max_episode_length=400, auto_reset=True, joint_vel_penalty=False,
                 is_agent_getting_bonus_for_reaching_goal=True, report_truncation=False, critic_obs=None, goals=None,
                 goal_curriculum=None, goal_row_stats=False, reward_shaping=None, push=None, episode_log=None, start_poses=None,
                 start_prob=1.0, randomization=None, action_delay=None, sensor_noise=None, action_obs=None, tendon_obs=None,
                 tendon_obs_scale=None, behind_step_order=STEP_STAGES):
        assert sorted(behind_step_order) == sorted(STEP_STAGES)
        self.order = tuple(behind_step_order)
        super().__init__(robot, stepper, n, seed, max_episode_length, joint_vel_penalty, is_agent_getting_bonus_for_reaching_goal,
                         auto_reset, env_id_offset)
        nq, nt = self.desc.n_q, self.desc.n_t
        self.gid0 = int(env_id_offset)
        self.reached_count = np.zeros(n, np.uint32)      # the statistics' goals-reached counter per env (d_ep_cnt's third plane)
        self.margin_min = np.inf
        self.obs = None
        self.ep_tol = np.zeros(n)                        # the running return's tolerance (the statistics add up the step's own reward)
        self.stats_tol = np.zeros(3)                     # of all rewards handed out, of stats()' sum_return and sum_return_sq
        # goal pool / curriculum / row counts (rb_env_goal_pool_set, rb_env_goal_curriculum_configure: goal number 0 becomes its row)
        self.pool = None if goals is None else np.ascontiguousarray(goals, np.float32)
        self.curriculum = None if goal_curriculum is None else dict(goal_curriculum)
        self.row_stats = bool(goal_row_stats)
        if self.pool is not None:
            m = len(self.pool)
            self.level = np.full(n, self.curriculum["start"] if self.curriculum else 0, np.int64)
            self.goal_index = self._goal_row(np.ones(n, bool))
            self.goal = self.pool[self.goal_index].copy()
            self.goal_seen = np.zeros(n, np.uint32)
            self.attempts, self.row_reached = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
            self.promotions = self.demotions = 0
        # episode-end codes
        self.truncation = bool(report_truncation)
        self.done_seen, self.kind = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        # per-env parameters (rb_params_enable: nominal, no draw made; reset() draws number 0)
        self.par = None
        if randomization is not None:
            self.par_lo, self.par_hi = randomization.to_arrays(nt)
            self.par = np.tile(np.concatenate([np.ones(nt), np.zeros(nt), np.ones(4)]).astype(np.float32), (n, 1))
            self.par_draws = np.zeros(n, np.uint32)
        # action latency (rb_env_io_configure: draw 0 of every env), sensor noise (the row counters start at 0), action rows
        self.delay = None
        if action_delay is not None:
            ranged = not np.isscalar(action_delay)
            self.delay_lo, self.delay_hi = (int(action_delay[0]), int(action_delay[1])) if ranged else (int(action_delay), int(action_delay))
            self.delay_resample = ranged
            self.delay = iu.delay_draw(seed, self.ids, 0, self.delay_lo, self.delay_hi)
            self.delay_draws = np.ones(n, np.uint32)
            self.delay_book = iu.DelayBook(n, nt)
            self.delays_seen = set(int(d) for d in self.delay)
        self.action_rows = int(action_obs or 0)
        self.history = HistoryBook(n, nt, self.action_rows) if self.action_rows else None
        # tendon channels: the row is [q, qd, goal | n_t columns per channel, in CHANNELS' order | K action blocks]
        self.channels = tuple(c for c in ou.CHANNELS if c in (tendon_obs or ()))
        self.chan_scale = dict(tendon_obs_scale or {})
        assert not self.channels or start_poses is None, "start_poses does not combine with tendon_obs (DESIGN §30)"
        n_chan = len(self.channels) * nt
        self.obs_dim = 3 * nq + n_chan + self.action_rows * nt
        self.chan_cols = np.zeros(self.obs_dim, bool)
        self.chan_cols[3 * nq:3 * nq + n_chan] = True
        self.base_tol = np.zeros(self.obs_dim)           # the fp32 tendon columns against float64: the readout's own tolerances
        if self.channels:
            from oracle.physics_np import TendonRobotOracle
            self.base_tol[self.chan_cols] = ou.column_tolerances(TendonRobotOracle(self.desc), self.channels, self.chan_scale)
        self.colsig = np.zeros(self.obs_dim)
        if sensor_noise:
            assert not set(sensor_noise) - {"q", "qd"} - set(self.channels)
            self.colsig[:3 * nq + n_chan] = iu.column_sigmas(nq, nt, self.channels, sensor_noise, self.chan_scale)
        self.tol_cols = self.chan_cols | (self.colsig != 0)      # the columns compared within self.obs_tol; every other one exactly
        self.noise_rows = np.zeros(n, np.uint32)
        self.obs_tol = np.zeros((n, self.obs_dim))
        # critic rows
        self.critic_names = None
        if critic_obs is not None:
            self.critic_names = tuple(b for b in ("state", "age", "params", "delay", "actions") if b == "state" or b in critic_obs)
            assert "params" not in self.critic_names or self.par is not None
            assert ("delay" not in self.critic_names or self.delay is not None) and ("actions" not in self.critic_names or self.history)
            self.action_blocks = np.zeros((n, self.action_rows * nt), np.float32)
            self.critic_rows = self._critic()
        # reward shaping
        self.shaping = None
        if reward_shaping is not None and any(shu.weights_of(reward_shaping)):
            self.shaping = dict(reward_shaping)
            self.prev_action = np.zeros((n, nt), np.float32)
            self.cost, self.cost_tol = np.zeros(n), np.zeros(n)
            self.run_cost = np.zeros(n)
            self.shaping_sums = np.zeros(4)              # sum_episode_cost, n_episodes, sum_step_cost, n_steps
            self.shaping_sums_tol = np.zeros(2)          # of the two cost sums
            self.run_tol = np.zeros(n)
            self.rate_zero_beside_live = self.rate_zero_seen = self.rate_live_seen = False
        # random pushes
        self.push = None
        if push is not None:
            self.push = {"threshold": pu.threshold_of(push["prob"]),
                         "sigma": np.broadcast_to(np.asarray(push["sigma"], np.float32), (nq,)).astype(np.float64)}
            self.push_book = pu.Book(seed, n, self.push["threshold"], self.gid0)
            self.impulse = np.zeros((n, nq), np.float32)
            self.pushed = np.zeros(n, bool)
            self.push_clamped = self.push_free = self.pushed_and_done = 0
        # episode log
        self.log = None
        if episode_log:
            self.log = eu.EpisodeLogModel(n, episode_log)
            self.log_tol_acc = np.zeros(n)               # the running return's tolerance: the sum of its steps' reward tolerances
            self.log_tol = np.zeros((episode_log, n))
            self.log_overflow = np.zeros(n, bool)        # a full log saw a further episode end
        # start poses
        self.start_pool = None
        if start_poses is not None:
            self.start_pool = np.ascontiguousarray(start_poses, np.float32)
            self.start_book = su.Book(seed, n, su.threshold_of(start_prob), len(self.start_pool), self.gid0)
            self.starts_from_pool = self.starts_at_rest = 0

    # -- the rules of the goal options, as functions of (seed, gids, counters) --
    def _goal_row(self, mask):
        """the pool row of the masked envs' goal number draws - 1 at their level (the plain pool: the whole pool)"""
        gids, draw = self.ids[mask], (self.draws[mask] - np.uint32(1)).astype(np.uint32)
        if self.curriculum:
            return gc.row(self.seed, gids, draw, self.level[mask], len(self.pool), self.curriculum["levels"])
        return gp.pool_row(self.seed, gids, draw, len(self.pool))

    def _critic(self):
        q, qd, _ = self.stepper.state()
        cols = [q, qd, self.goal]
        if "age" in self.critic_names:
            cols.append((self.step_num.astype(np.float32) / np.float32(self.max_len))[:, None])
        if "params" in self.critic_names:
            cols.append(self.par)
        if "delay" in self.critic_names:
            cols.append(self.delay.astype(np.float32)[:, None])
        if "actions" in self.critic_names:
            cols.append(self.action_blocks)
        return np.concatenate(cols, axis=1).astype(np.float32)

    # ------------------------------------------------------------------
    def reset(self):
        n, nq = self.n, self.desc.n_q
        everyone = np.ones(n, bool)
        # in front (RoboyVecEnv.reset): every env draws its parameters
        if self.par is not None:
            self._draw_params(everyone)
        # the reset kernel: zero pose, step counter 1, running return 0, a fresh box goal (goal counter + 1)
        self.stepper.reset(everyone)
        self.step_num[:] = 1
        self.ep_ret[:], self.ep_tol[:] = 0.0, 0.0
        self.goal = self.draw(everyone)
        obs = np.concatenate([np.zeros((n, 2 * nq), np.float32), self.goal], axis=1)
        if self.delay is not None:
            self.delay_book.k[:] = 1                        # (the delays stand: a reset draws none)
        # 0. start poses - every env's zero pose becomes a pool row or stays
        if self.start_pool is not None:
            self._start(everyone, obs)
        # 1. observation rows - the tendon columns at the zero pose, every set-point 0 (plus the env's offset); the action blocks
        #    zero (4. writes the zeros behind the noise)
        if self.channels:
            obs = np.concatenate([obs, self._tendon_columns(obs, None)], axis=1)
        if self.history:
            self.history.reset()
            self.action_blocks = self.history.reset_blocks()
            obs = np.concatenate([obs, self.action_blocks], axis=1)
        # 2. the done-seen re-base: a reset is no episode end, no code is reported; the log's `seen` follows the counter too
        if self.log is not None:
            self.log.seen[:] = self.reached_count
        self.done_seen[:] = self.reached_count
        self.kind[:] = 0
        # 3. sensor noise on the rows, 4. zero action blocks: the noise is additive on the q and qd columns whatever 0. put there and
        #    never touches the blocks, so it is applied where the row is finished (_noised, below)
        # 5. goal pool / curriculum - the goal the reset kernel drew becomes its pool row; the level stands, `seen` is re-based,
        #    nothing is counted
        if self.pool is not None:
            self.goal_seen[:] = self.reached_count
            self.goal_index = self._goal_row(everyone)
            self.goal = self.pool[self.goal_index].copy()
            obs[:, 2 * nq:3 * nq] = self.goal
        # 6. critic rows
        if self.critic_names:
            self.critic_rows = self._critic()
        # 7. shaping - the running episode costs and the cost plane to zero
        if self.shaping:
            self.cost[:], self.cost_tol[:], self.run_cost[:], self.run_tol[:] = 0.0, 0.0, 0.0, 0.0
        # 8. episode log - the running return and age to zero; records and counts stay
        if self.log is not None:
            self.log.acc[:], self.log.age[:], self.log_tol_acc[:] = 0, 0, 0.0
        self.obs = self._noised(obs)
        return self.obs

    def _tendon_columns(self, obs, applied):
        """[n, C n_t] float64: the channels at the state the row reports (its q and qd columns), under the set-points of the
        action rows `applied` held (None: every set-point 0) and the parameters the env's next step will use - env_obs_util"""
        nq = self.desc.n_q
        return ou.expected_columns(self.robot, self.desc, obs[:, :nq], obs[:, nq:2 * nq], applied, self.channels, self.chan_scale, self.par)[0]

    def _noised(self, obs):
        """the finished row as reported: value + colsig z of the env's row number on the noised columns (float64), the tendon
        columns in float64; the tolerance of the fp32 row against it in self.obs_tol (the tendon columns' own plus the noise's);
        every other column the exact float32 value; with noise the row is counted"""
        if not self.tol_cols.any():
            return obs
        out = obs.astype(np.float64)
        tol = np.tile(self.base_tol, (self.n, 1))
        if self.colsig.any():
            z = iu.sensor_noise64(self.seed, self.ids, self.noise_rows, self.obs_dim)
            self.noise_rows = self.noise_rows + np.uint32(1)
            out = out + self.colsig[None, :] * z
            tol += (np.abs(self.colsig)[None, :] * SENSOR_NOISE_TOL + 4 * np.spacing(np.abs(out).astype(np.float32)).astype(np.float64)) * (self.colsig != 0)[None, :]
        self.obs_tol = tol
        return out

    def step(self, actions, impulse=None):
        """-> (obs, reward float64, done bool, reward tolerance).  ``impulse``: the device's impulse plane [n, n_q] behind the same
        step (the ONE adoption) - checked against sigma z64 within PUSH_NOISE_TOL, then used; None: fl32(sigma z64)."""
        act = clip_action(actions)
        first = self.step_num == 1
        # in front: the random push - it makes the state s_t the step really starts from
        if self.push:
            self._push(impulse)
        # in front: the shaping cost of (s_t, a_t)
        if self.shaping:
            q, qd, _ = self.stepper.state()
            args = (self.desc, self.robot, q.astype(np.float64), qd.astype(np.float64), act, self.prev_action, first, self.shaping)
            self.cost, self.cost_tol = shu.cost64(*args), shu.cost_tolerance(*args)
            if shu.weights_of(self.shaping)[0]:
                rate = shu.terms64(*args[:-1])[0][0]
                assert not rate[first].any()
                self.rate_zero_seen |= bool(first.any())
                self.rate_live_seen |= bool((rate[~first] > 0).any())
                self.rate_zero_beside_live |= bool(first.any() and (rate[~first] > 0).any())
                self.prev_action = act.copy()
        # the env-step kernel (HostEnvModel): physics, reward, done, statistics, the box goal, the auto-reset
        ep_before = self.ep_ret.copy()
        applied = act
        if self.delay is not None:                          # the row handed in d steps earlier in the same episode, or the rest command
            assert not self.robot.get_action_space().low[0] + self.robot.get_action_space().high[0], "rest = action 0 needs a symmetric box"
            applied, _ = self.delay_book.shifted(act, self.delay)
        obs, reward, done, margin = super().step(applied)
        if self.delay is not None:
            self.delay_book.advance(done, self.auto_reset)
            if self.auto_reset and self.delay_resample:     # the episode-end hook: a done env draws its next delay
                self.delay[done] = iu.delay_draw(self.seed, self.ids[done], self.delay_draws[done], self.delay_lo, self.delay_hi)
                self.delay_draws[done] += np.uint32(1)
                self.delays_seen |= set(int(d) for d in self.delay[done])
        if self.par is not None and self.auto_reset:        # the episode-end hook: the parameters are redrawn where the goal is
            self._draw_params(done)
        if self.channels:                                   # at the reported state (a done env's zero pose), under the APPLIED command, held, and
            obs = np.concatenate([obs, self._tendon_columns(obs, applied)], axis=1)      # the parameters as the hook left them
        if self.history:                                    # the K blocks: the rows handed in this episode, newest first
            self.action_blocks = self.history.blocks(act, done, self.auto_reset)
            obs = np.concatenate([obs, self.action_blocks], axis=1)
        base_tol = REWARD_ATOL + REWARD_RTOL * np.abs(reward)
        ret = ep_before + reward
        self.ep_tol += base_tol + 2.0 ** -24 * np.abs(ret)          # (the device's running return is an fp32 sum: one rounding per step)
        self.stats_tol += (base_tol.sum(), self.ep_tol[done].sum(), ((2.0 * np.abs(ret) + self.ep_tol) * self.ep_tol)[done].sum())
        self.ep_tol[done] = 0.0
        self.margin_min = min(self.margin_min, float(margin.min()))
        reached = self.last_reached
        self.reached_count += reached.astype(np.uint32)
        c = {"obs": obs, "reward": reward, "tol": base_tol, "done": done.astype(np.uint32)}
        if self.push:
            self.pushed_and_done += int((self.pushed & done).sum())
        for stage in self.order:
            getattr(self, "_stage_" + stage)(c)
        self.obs = self._noised(c["obs"])
        return self.obs, c["reward"], c["done"] != 0, c["tol"]

    def _draw_params(self, mask):
        self.par[mask] = epu.draw(self.seed, self.ids[mask], self.par_draws[mask], self.par_lo, self.par_hi)
        self.par_draws[mask] += np.uint32(1)
        self.stepper.set_params(mask, self.par)

    # -- in front of the step --
    def _push(self, adopted):
        pushed, m = self.push_book.step()
        own = self.push["sigma"][None, :] * pu.z64(self.seed, self.push_book.gids[pushed], m[pushed], self.desc.n_q)
        if adopted is None:
            self.impulse[pushed] = own.astype(np.float32)
        else:
            adopted = np.asarray(adopted, np.float32)
            assert np.array_equal(adopted[~pushed], self.impulse[~pushed]), "an env that was not pushed must keep its impulse row"
            err = np.abs(adopted[pushed].astype(np.float64) - own)
            assert np.all(err <= self.push["sigma"][None, :] * PUSH_NOISE_TOL), "impulse off sigma z64: %g" % err.max()
            self.impulse[pushed] = adopted[pushed]
        changed = self.stepper.add_velocity(pushed, self.impulse)
        self.pushed = pushed
        self.push_clamped += int(changed.sum())
        self.push_free += int(pushed.sum()) * self.desc.n_q - int(changed.sum())

    def _start(self, who, obs):
        nq = self.desc.n_q
        started = self.start_book.start(who)
        pose = np.zeros((self.n, nq), np.float32)
        pose[started] = self.start_pool[self.start_book.index[started].astype(np.int64)]
        self.stepper.set_state(started, pose, np.zeros_like(pose))
        obs[started, :nq], obs[started, nq:2 * nq] = pose[started], 0.0
        self.starts_from_pool += int(started.sum())
        self.starts_at_rest += int(who.sum() - started.sum())

    # -- behind the step: one block per line of §6 --
    def _stage_0(self, c):
        # 0. shaping apply - reward -= cost, the cost statistics; reads the done words as flags
        if not self.shaping:
            return
        done = c["done"] != 0
        c["reward"] = c["reward"] - self.cost
        c["tol"] = c["tol"] + self.cost_tol
        self.run_cost += self.cost
        self.run_tol += self.cost_tol
        s, t = self.shaping_sums, self.shaping_sums_tol
        s[2] += self.cost.sum(); s[3] += self.n; t[1] += self.cost_tol.sum()
        s[0] += self.run_cost[done].sum(); s[1] += done.sum(); t[0] += self.run_tol[done].sum()
        self.run_cost[done], self.run_tol[done] = 0.0, 0.0

    def _stage_1(self, c):
        # 1. goal pool / curriculum / row counts - the done envs' new goal becomes a pool row, in the plane and in the row
        if self.pool is None:
            return
        done = c["done"] != 0
        if not done.any():
            return
        hit = (self.reached_count != self.goal_seen)[done]
        if self.row_stats:              # counted against the row the env was aimed at, before the index moves
            k0 = self.goal_index[done]
            np.add.at(self.attempts, k0, np.uint64(1))
            np.add.at(self.row_reached, k0[hit], np.uint64(1))
        if self.curriculum:             # the level moves first, the draw is made at the new level
            cur = self.curriculum
            new = gc.next_level(self.level[done], hit, cur["up"], cur["down"], cur["levels"])
            self.promotions += int((new > self.level[done]).sum())
            self.demotions += int((new < self.level[done]).sum())
            self.level[done] = new
        self.goal_seen[done] = self.reached_count[done]
        self.goal_index[done] = self._goal_row(done)
        self.goal[done] = self.pool[self.goal_index[done]]
        nq = self.desc.n_q
        c["obs"][done, 2 * nq:3 * nq] = self.goal[done]

    def _stage_1a(self, c):
        # 1a. start poses (auto_reset only) - the done envs' zero pose becomes a pool row or stays, in the planes and in the row
        if self.start_pool is None or not self.auto_reset:
            return
        self._start(c["done"] != 0, c["obs"])

    def _stage_2(self, c):
        # 2. critic rows - from the planes as 1. and 1a. left them
        if self.critic_names:
            self.critic_rows = self._critic()

    def _stage_3(self, c):
        # 3. episode log - the reward as 0. left it (what the caller receives), the done words read as flags
        if self.log is None:
            return
        done = c["done"] != 0
        count = self.log.count.copy()
        self.log_overflow |= done & (count >= self.log.E)
        self.log_tol_acc += c["tol"] + 2.0 ** -24 * np.abs(self.log.acc.astype(np.float64) + c["reward"])      # (an fp32 running sum)
        write = done & (count < self.log.E)
        self.log_tol[count[write], np.nonzero(write)[0]] = self.log_tol_acc[write]
        self.log_tol_acc[done] = 0.0
        self.log.step(c["reward"].astype(np.float32), done, self.reached_count)

    def _stage_4(self, c):
        # 4. episode-end codes - last: it turns the done words, which 0., 1. and 3. read as flags, into codes
        done = c["done"] != 0
        kind = np.where(self.reached_count != self.done_seen, eu.TERMINATED, eu.TRUNCATED).astype(np.uint32)
        self.kind = np.where(done, kind, 0).astype(np.uint32)
        self.done_seen[done] = self.reached_count[done]
        if self.truncation:
            c["done"] = self.kind.copy()

    # -- what RoboyVecEnv exposes --
    def truncated(self):
        return self.kind == eu.TRUNCATED

    def state(self):
        return self.stepper.state()

    def stats_dict(self):
        keys = ("sum_return", "sum_return_sq", "n_episodes", "sum_length", "n_goal_reached", "n_infeasible_steps", "n_env_steps", "sum_reward")
        out = dict(zip(keys, (float(v) for v in self.stats)))
        # the library's sum_reward is the finished plus the RUNNING returns (stats_reduce_kernel): what an episode that a reset()
        # abandoned had collected is in neither.  HostEnvModel's own sum counts every reward handed out; they agree until a reset
        # in mid-episode
        out["sum_reward"] = float(self.stats[0] + self.ep_ret.sum())
        return out

    def stats_tolerance(self):
        """of stats(): (sum_reward, sum_return, sum_return_sq)"""
        return self.stats_tol[1] + self.ep_tol.sum(), self.stats_tol[1], self.stats_tol[2]

    def shaping_stats(self):
        return dict(zip(("sum_episode_cost", "n_episodes", "sum_step_cost", "n_steps"), (float(v) for v in self.shaping_sums)))

    def goal_level_histogram(self):
        return np.bincount(self.level, minlength=self.curriculum["levels"]).astype(np.int64)

    def push_count(self):
        return int(self.push_book.n_pushes.astype(np.int64).sum())

    def last_push(self):
        b = self.push_book
        return (b.count == b.last) & (b.count != 0), self.impulse

    def episode_log(self):
        return self.log.log()

    def episode_log_tolerance(self):
        """[n, E]: per record, the sum of its steps' reward tolerances (0 where there is no record)"""
        live = np.arange(self.log.E)[None, :] < self.log.count.astype(np.int64)[:, None]
        return np.where(live, self.log_tol.T, 0.0)


# ---- the cases: shared by tests/test_env_layer_model_cpu.py and tests/test_env_layer_model_gpu.py ----
MAX_LEN, LEG1, LEG2 = 5, 14, 8
GOAL_ROWS, LEVELS, START_LEVEL = 8, 4, 1          # the start level's window: rows [0, 4) - one planted row per episode step 2..5
ALL_TERMS = {"action_rate": 0.1, "tension": 0.05, "activation": 0.02}
MSJ_SEED, WIDE_SEED, RANGES_SEED, TENDON_SEED, BALL12_SEED = 14, 7, 13, 7, 18


def _msj():
    from gym_roboy_amd.envs.robots import MsjRobot
    return MsjRobot()


def _upper():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    return UpperBodyRobot()


def _ranges():
    from gym_roboy_amd.envs.params import ParamRanges
    return ParamRanges(force_scale=(0.8, 1.2), setpoint_offset=(-0.01, 0.01), mass_scale=(0.8, 1.25), damping_scale=(0.5, 2.0))


def case_stepper(name, gpu=False):
    """a factory of the case's stepper: the C oracle, or (gpu) the plain kernel in the env's form"""
    make, integ, n, seed, options, id0 = CASES[name]
    params = "randomization" in options(make().get_description())
    if not gpu:
        return lambda: (ParamOracleStepper if params else OracleStepper)(make(), n, integ)
    return lambda: PlainKernelStepper(make(), n, seed, id0, integ, 1, params, TREE_LANE if name in TREE_LANE_CASES else None,
                                      LARGE_BATCH if name in LARGE_BATCH_CASES else None)


def _common(desc, shaping, log):
    return dict(goal_curriculum=dict(levels=LEVELS, up=1, down=1, start=START_LEVEL), goal_row_stats=True, report_truncation=True,
                reward_shaping=shaping, push={"prob": 0.25, "sigma": pu.sigma_of(desc)}, episode_log=log,
                start_poses=su.pool_of(desc), start_prob=0.5)


def _msj_all(d):
    return dict(_common(d, {"action_rate": 0.1}, 2), randomization=_ranges(), critic_obs=("state", "age", "params", "delay", "actions"),
                joint_vel_penalty=True, action_delay=(0, 3), sensor_noise={"q": 0.01, "qd": 0.05}, action_obs=2)


def _kernarg_msj():
    from test_env_params_gpu import _kernarg_msj as make
    return make()


def _ball12():
    from test_env_params_gpu import _ball12 as make
    return make()


def _msj_tendon(d):
    return dict(tendon_obs=("length", "force"), tendon_obs_scale={"force": 1 / 400}, sensor_noise={"q": 0.01, "length": 5e-4, "force": 2.0},
                action_obs=3, critic_obs=("state", "age", "actions"), report_truncation=True, reward_shaping=ALL_TERMS,
                push={"prob": 0.25, "sigma": pu.sigma_of(d)}, episode_log=4)


def _ball12_mix(d):
    return dict(randomization=_ranges(), action_delay=2, tendon_obs=("rate", "activation"), action_obs=1, goal_row_stats=True,
                goal_curriculum=dict(levels=1, up=1, down=1, start=0), episode_log=1, report_truncation=True)


# name: (robot factory, integrator, n, seed, options without the goal pool: case_goals makes it, env_id_offset).  Under its seed a
# case qualifies (qualify(), below) on the fp32 C oracle for both auto_reset values, with the done margin above 4e-5 - four times
# what the comparison needs, for the last bits between the oracle's states and the kernel's.
CASES = {
    "msj_all": (_msj, "rk4", 300, MSJ_SEED, _msj_all, 0),
    # the kernarg MsjRobot (run with ROBOY_SIM_JIT=0 on the device: its kernarg instances), a pool without curriculum; no delay
    # range, no parameters, no start poses: what the shaping terms and the tendon channels refuse
    "msj_tendon": (_kernarg_msj, "euler", 300, TENDON_SEED, _msj_tendon, 0),
    # twelve tendons (the run-time tendon count), a fixed delay, a curriculum of one level
    "ball12_mix": (_ball12, "euler", 257, BALL12_SEED, _ball12_mix, 0),
    "upper_all": (_upper, "euler", 130, 2, lambda d: _common(d, ALL_TERMS, 2), 0),
    # msj_all with global ids 2^32 - 100 .. 2^32 + 199: they cross the 32-bit word every draw is keyed by
    "msj_all_wide_ids": (_msj, "rk4", 300, WIDE_SEED, _msj_all, 2 ** 32 - 100),
    # upper_all with a second group of 256 envs, ragged: the library starts a sub-range at a multiple of 256 envs, so this is the
    # smallest batch of the joint-tree class that two streams can share (256 + 66)
    "upper_ranges": (_upper, "euler", 322, RANGES_SEED, lambda d: _common(d, ALL_TERMS, 2), 0),
}
TREE_LANE, TREE_LANE_CASES = 1, ("upper_ranges",)      # RB_KERNEL_ENV_PER_LANE: for joint trees the one-wave-per-64-envs form, the one
#                                                         that takes sub-ranges; at 322 envs the batch size alone chooses the split form
LARGE_BATCH, LARGE_BATCH_CASES = 66819, ("msj_tendon",)   # (PlainKernelStepper's ``batch``)
JIT_OFF_CASES = ("msj_tendon",)                           # run with ROBOY_SIM_JIT=0 on the device
BOTH_WAYS = ("msj_all", "msj_tendon", "ball12_mix", "upper_all")         # run with auto_reset and without; the other two are variants of these, run with it


def case_actions(name):
    from action_box_util import wide_actions
    make, _, n, seed, _, _ = CASES[name]
    return wide_actions(n, make().get_description().n_t, LEG1 + LEG2, seed + 1)


def case_model(name, stepper, auto_reset, goals, **kw):
    make, _, n, seed, options, id0 = CASES[name]
    robot = make()
    return EnvLayerModel(robot, stepper, n, seed, env_id_offset=id0, max_episode_length=MAX_LEN, auto_reset=auto_reset,
                         goals=goals, **options(robot.get_description()), **kw)


def case_goals(name, make_stepper):
    """The case's goal pool [GOAL_ROWS, n_q].  Rows beyond the start level's window [0, 4) are goal_pool_util.small_pool's, which
    no env reaches.  A row of the window becomes the pose that some env which draws this row at the first reset is in after episode
    step 5 (its last permitted step; this one must be found), 4, 3 or 2 of its first episode - a row per step as far as such envs
    exist - slowly enough for the goal test's velocity bound (within 0.95 of it).  Found by a scout run of THIS model over a stepper
    of its own, without auto_reset and under the unreachable pool: the motion of an env's first episode depends on its start pose,
    its pushes and its actions, not on its goal."""
    make = CASES[name][0]
    pool = gp.small_pool(make().get_description(), m=GOAL_ROWS).copy()
    cur = CASES[name][4](make().get_description()).get("goal_curriculum")
    window = int(gc.hi(cur["start"], GOAL_ROWS, cur["levels"])) if cur else GOAL_ROWS      # the rows the first goals are drawn from
    stepper = make_stepper()
    try:
        scout = case_model(name, stepper, False, pool)
        scout.reset()
        rows = scout.goal_index.copy()
        acts = case_actions(name)
        seen = []
        for t in range(MAX_LEN):
            scout.step(acts[t])
            q, qd, feas = scout.state()
            seen.append((q, feas & (np.linalg.norm(qd.astype(np.float64), axis=1) < 0.95 * scout.max_dv / 5)))
    finally:
        stepper.close()
    free = set(range(window))
    for t in range(MAX_LEN - 1, 0, -1):                   # episode steps 5, 4, 3, 2
        q, ok = seen[t]
        cand = [e for e in np.nonzero(ok)[0] if rows[e] in free]
        assert cand or t < MAX_LEN - 1, "no env to plant the last permitted step with"
        if cand:
            pool[rows[cand[0]]] = q[cand[0]]
            free.discard(int(rows[cand[0]]))
    return pool


class Record:
    """what a scenario leaves for the qualification: per step the done flags, the codes, who was pushed and who was in an episode's
    first step; the legs' boundaries"""

    def __init__(self):
        self.done, self.kind, self.pushed, self.first, self.resets = [], [], [], [], []


def run_scenario(model, actions, device=None):
    """reset(), LEG1 steps, a second reset() in mid-episode, LEG2 more steps.  Without auto_reset the caller resets as a training
    loop without it would: whenever every env's episode is over - by the MODEL's step counters.
    ``device``: the env under test behind three methods - reset() -> rows; step(act) -> (what it returned, the impulse plane or
    None); compare(where, device_out, model_out) - every call is made in front of the model's, so the model is never fed but the
    impulse plane.  -> Record"""
    rec = Record()

    def reset(where):
        dev = device.reset() if device else None
        obs = model.reset()
        rec.resets.append(len(rec.done))
        if device:
            device.compare(where, dev, (obs,))

    reset("reset")
    for t, act in enumerate(actions):
        if t == LEG1:
            reset("the reset in mid-episode")
        first = model.step_num == 1
        dev, impulse = device.step(act) if device else (None, None)
        out = model.step(act, impulse=impulse)
        rec.done.append(out[2]); rec.kind.append(model.kind.copy()); rec.first.append(first)
        rec.pushed.append(model.pushed.copy() if model.push else np.zeros(model.n, bool))
        if device:
            device.compare("step %d" % t, dev, out)
        if not model.auto_reset and t + 1 < len(actions) and t + 1 != LEG1 and (model.step_num > model.max_len).all():
            reset("the reset behind step %d" % t)
    return rec


def qualify(model, rec):
    """The scenario made every path run (ISSUE part 3), as far as the model's options exist; asserted on the model's own planes, so
    the GPU test - where the device has been held to them - asserts it on what the device did."""
    done, kind = np.array(rec.done), np.array(rec.kind)
    assert model.margin_min > MARGIN, model.margin_min
    if model.auto_reset:
        assert done[:LEG1].sum(axis=0).min() >= 2 and done[LEG1:].sum(axis=0).min() >= 1
    assert (kind == eu.TERMINATED).any() and (kind == eu.TRUNCATED).any()
    # some env reaches its goal on its last permitted step: terminated in a step that began with the counter at max_len
    ages = np.zeros_like(done, dtype=np.int64)
    age = np.zeros(model.n, np.int64)
    for t in range(len(done)):
        if t in rec.resets[1:]:
            age[:] = 0
        age += 1
        ages[t] = age
        if model.auto_reset:
            age[done[t]] = 0
    assert ((kind == eu.TERMINATED) & (ages == model.max_len)).any()
    if model.pool is not None and model.curriculum and model.curriculum["levels"] > 1:
        assert model.promotions > 0 and model.demotions > 0
    if model.pool is not None and model.row_stats:
        assert ((model.row_reached > 0) & (model.row_reached < model.attempts)).any()
    if model.start_pool is not None:
        assert model.starts_from_pool > 0 and model.starts_at_rest > 0
    if model.push:
        assert model.push_clamped > 0 and model.push_free > 0 and model.pushed_and_done > 0
    if model.log is not None:
        # a full log with a further episode behind it.  The time limit alone ends three episodes per env in this scenario (steps 5
        # and 10 of the first leg, step 5 of the second), so a log of 1 or 2 records fills and overflows on every env; one of 4 needs
        # five ends of ONE env, i.e. two goals reached by it beside the planted one - the scenario cannot promise that, so there the
        # other path is asserted: records written at positions beyond the first two, and logs of different fill
        if model.log.E <= 2 or not model.auto_reset:
            assert (model.log.count == model.log.E).any() and model.log_overflow.any()
        else:
            assert model.log.count.max() >= 3 and model.log.count.min() < model.log.count.max()
    if model.delay is not None and model.delay_resample:
        assert model.delays_seen == set(range(model.delay_lo, model.delay_hi + 1))
    if model.shaping and shu.weights_of(model.shaping)[0]:
        assert model.rate_zero_seen and model.rate_live_seen          # (without auto_reset every episode starts at a reset, together)
        assert model.rate_zero_beside_live or not model.auto_reset
