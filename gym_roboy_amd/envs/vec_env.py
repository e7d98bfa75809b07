"""``RoboyVecEnv``: N ``RoboyEnv``s advanced by one fused kernel per step.

The reference vectorises by running one OS process, one ROS client and one
simulator instance per env under stable_baselines' ``SubprocVecEnv``
(``/root/reference/gym_roboy/train_parallel.py:19-29``); every env step costs
two process boundaries plus ~150 us of Python.  Here the whole env layer of
``RoboyEnv.step`` (``roboy_env.py:51-70``: action rescale, simulator step,
observation, reward, done, goal resampling) runs on the GPU next to the
physics, for all envs at once, and ``auto_reset`` reproduces what the
``SubprocVecEnv`` worker does on ``done`` (``env.reset()``, i.e. simulator
reset, step counter back to 1, a fresh goal, and the reset observation is the
one returned).

``step`` takes actions ``[N, n_t]`` in ``[-1, 1]`` either as a numpy array
(copied to the device) or as a CUDA ``torch.Tensor`` (used in place), and
returns ``(obs [N, obs_dim], reward [N], done [N], infos)`` of the same kind;
``obs_dim`` is ``3 n_q``, or ``3 n_q + C n_t`` with ``tendon_obs`` (C channels), plus ``K n_t`` with ``action_obs=K``.
"""
import ctypes
import warnings

import numpy as np

from .. import _native as nat
from .._gymcompat import spaces
from . import goals as envgoals
from . import reward as rw
from .options import (SENSOR_NOISE_KEYS, TENDON_OBS_CHANNELS, _TENDON_OBS_BOUNDS, action_delay_range, action_obs_bounds,  # noqa: F401
                      action_obs_rows, critic_obs_spec, episode_log_capacity, episode_log_figures, parse_push, parse_reward_shaping, push_spec, reward_shaping_weights,
                      sensor_noise_sigmas, start_pose_spec, tendon_obs_mask, tendon_obs_scales)
from .robots import RoboyRobot
from .simulations.hip_simulation_client import HipBatchSimulation

_IN_SLAB = object()      # RoboyVecEnv._last_actions: the last step's numpy actions, uploaded into the action slab


class RoboyVecEnv:

    def __init__(self, robot: RoboyRobot, num_envs: int, seed: int = 0,
                 joint_vel_penalty: bool = False,
                 is_agent_getting_bonus_for_reaching_goal: bool = True,
                 auto_reset: bool = True, integrator="euler", n_substeps: int = 1,
                 device: int = 0, env_id_offset: int = 0, max_episode_length: int = 400,
                 randomization=None, tendon_obs=None, tendon_obs_scale=None, sensor_noise=None, action_delay=None,
                 report_truncation: bool = False, action_obs=None, critic_obs=None, goals=None, goal_curriculum=None,
                 goal_row_stats: bool = False, reward_shaping=None, push=None, episode_log=None,
                 start_poses=None, start_prob=1.0):
        """``randomization``: an ``envs.params.ParamRanges`` - every env gets its own physical parameters, drawn from these ranges by
        ``reset()`` and again whenever the env auto-resets (ball-joint robots).  None: every env is the robot itself.
        ``tendon_obs``: channel names out of ``("length", "rate", "activation", "force")`` - the observation row becomes
        ``[q, qd, goal, then n_t values per channel in that fixed order]``, the tendons' state at the reported state under the actions
        just applied (ball-joint robots); ``tendon_obs_scale``: ``{channel: factor}``, default 1 (m, m/s, [0, 1], N).
        Combines with ``randomization``.
        ``sensor_noise``: ``{"q": 0.01, "qd": 0.05, "length": 5e-4, "force": 2.0}`` - Gaussian noise on the reported columns, standard
        deviations in physical units (rad, rad/s, m, m/s, activation, N; a channel must be in ``tendon_obs``); the goal columns,
        reward, done and the state are exact, and nothing is clipped to ``observation_space``, which is unchanged.
        ``action_delay``: an int ``d`` - every step is driven by the action handed in ``d`` steps earlier in the same episode (the rest
        command, every set-point 0, before that) - or a pair ``(lo, hi)``: each env draws its own delay, again at every auto-reset.
        At most 7.  Both combine with ``randomization`` and ``tendon_obs``; ball-joint robots.
        ``action_obs``: an int ``K`` (1..8) - the row grows by ``K n_t`` columns behind everything else: the last K actions the env was
        handed in this episode, newest first, clamped to [-1, 1] as the step clamps them, zeros where the episode is younger (every
        block behind a reset or an auto-reset).  What a memoryless policy needs under ``action_delay``: the commands still on
        their way.  Never noised; ``observation_space`` grows by columns within [-1, 1]; ball-joint robots.
        ``report_truncation``: tell the episodes that ended at ``max_episode_length`` from those that reached their goal (DESIGN.md
        §17; every robot, every kernel form, every option above).  ``step()`` returns ``done`` as bools as before, and
        ``truncated()`` gives the last step's ``[N]`` bools: True where the time limit alone ended the episode (an env that
        reaches its goal on its last permitted step is not truncated).  ``step_dev`` and ``step_range_dev`` then leave episode-end
        CODES in ``d_done`` - 0 not done, 1 terminated, 2 truncated (``_native.RB_DONE_*``) - so ``done != 0`` is the done of an env
        without the option.  The ``info`` dicts stay empty: a dict per env does not scale to 262 144 envs, so there is no
        ``TimeLimit.truncated`` key.
        ``critic_obs``: block names out of ``("state", "age", "params", "delay", "actions")`` - every step and reset also writes a
        PRIVILEGED row per env for an asymmetric critic (ball-joint robots): ``[q, qd, goal`` exactly as the planes hold
        them, without noise ``| episode age / max_episode_length | the env's parameters (needs randomization) | its action delay (needs
        action_delay) | the K action blocks of the observation (needs action_obs)]``, ``critic_obs_dim`` columns, ``"state"``
        always.  The row belongs to the observation row returned with it (an auto-reset env shows its reset state, new goal and redrawn
        parameters).  ``critic_obs()`` returns the last rows; observations, rewards, dones and statistics are unchanged.
        ``goals``: an ``envs.goals.GoalPool`` (``reachable_goals(robot, m)``) or an array ``[m, n_q]`` inside the angle box - every goal
        the env draws, at a reset and at every episode end, is a row of this pool instead of a point uniform in the goal box: row
        ``k(seed, global env id, draw number)`` (every robot, every kernel form, every option above).  Reward and done of
        the step that ends an episode use the old goal as before; ``set_goal`` still overrides.  ``goal_pool()`` returns the rows,
        ``set_goal_pool(rows)`` replaces them in place by as many others.  None: the env launches exactly what it launched before.
        ``goal_curriculum``: an int ``L`` or ``dict(levels=L, up=1, down=1, start=0)`` - a difficulty level per env over the pool's
        rows taken from easiest to hardest (needs ``goals``): an env at level ``l`` draws from the first
        ``(l + 1) m / L`` rows, moves ``up`` levels when an episode ends at its goal and ``down`` when it ends otherwise, and draws its
        next goal at the new level.  A ``GoalPool`` whose recipe is not marked ordered is ordered by ``GoalPool.ordered()`` (distance
        from the rest pose) with a warning; bare row arrays are taken as ordered.  ``goal_levels()``, ``goal_index()`` and
        ``goal_level_histogram()`` read the levels, the rows held and the envs per level; ``set_goal_levels(levels)`` writes the levels.
        At the top level an env draws exactly what it draws without the option.
        ``goal_row_stats``: count per pool row how many episodes were aimed at it and how many of them reached it (DESIGN.md §24;
        needs ``goal_curriculum`` - ``goal_curriculum=1`` counts without a staircase).  ``goal_row_stats()`` reads the counts,
        ``set_goal_row_stats`` writes them, ``permute_goal_pool(order)`` re-orders the live pool (any env with ``goals``) and
        ``reorder_goals_by_reach_rate()`` re-orders it by the measured reach rate.  False: the env launches exactly what it launched
        before.
        ``reward_shaping``: ``{"action_rate": w_r, "tension": w_f, "activation": w_a}`` (finite, >= 0, a missing key is 0) - the reward
        becomes ``r_step - (w_r c_rate + w_f c_tension + w_a c_activation)`` with the costs of the state before the step and the
        action handed to it: the mean squared change of the clamped action against the same episode's previous step (0 on an
        episode's first step), the mean squared tendon force over its maximum, the mean squared activation (every
        robot, every kernel form).  Observations, dones, the state and ``stats()`` are those of an env without the option.
        ``shaping_cost()`` returns the last step's costs, ``shaping_stats()`` their sums.  ``tension`` and ``activation`` do not
        combine with ``randomization`` nor with an ``action_delay`` above 0; ``action_rate`` does.  None or all zeros: the env
        launches exactly what it launched before.
        ``push``: ``{"prob": p, "sigma": s}`` - random velocity pushes, an external disturbance: in front of every env step each env
        is pushed with probability ``round(p * 2**24) / 2**24``; a pushed env's joint velocities get ``sigma_j z_j`` added (``z``
        standard normal, ``s`` a scalar or ``n_q`` entries in rad/s) and are clamped to the robot's velocity bounds; the step then
        runs from that state as it always did (every robot, every kernel form, every option above).  ``push`` holds
        the record (None without the option), ``last_push()`` returns who was pushed in the last step and by how much,
        ``push_count()`` the number of pushes so far.  None, ``prob`` 0 or all-zero sigmas: the env launches exactly what it launched
        before.
        ``episode_log``: an int ``E`` (1..64) - the device keeps each env's first E finished episodes since the log was last cleared:
        return (the sum of the rewards ``step`` returned, so with ``reward_shaping`` the shaped ones, added up in fp32 in step order),
        length and outcome (``_native.RB_DONE_TERMINATED``: the goal was reached, ``RB_DONE_TRUNCATED``: the time limit alone ended
        it), written by one small kernel behind every env step (every robot, every kernel form, every option above,
        sub-ranges and captured graphs).  Every env contributes exactly its first E episodes, so the figures are not biased towards
        short episodes as totals over whatever ended are.  ``reset()`` drops the episode under way without recording it.
        ``episode_log()`` reads the records, ``episode_log_summary(first_k)`` their sums and rates, ``episode_log_full()`` how many
        envs have all E, ``clear_episode_log()`` starts over; ``episode_log_capacity`` holds E (0 without the option).  None: the env
        launches exactly what it launched before.
        ``start_poses``: an ``envs.goals.GoalPool`` (``reachable_goals(robot, m)``) or an array ``[m, n_q]`` inside the joint limits -
        an episode, at ``reset()`` and at every auto-reset inside a step, begins at a row of this pool with zero velocity instead of
        the zero pose: with probability ``round(start_prob * 2**24) / 2**24`` at row ``k(seed, global env id, start number)``,
        otherwise at the zero pose as before (every robot, every kernel form, every option above but ``tendon_obs``).
        The observation row returned for a started env reports the pose (under ``sensor_noise`` with the row's own noise), critic
        rows the true pose; reward and done of the step that ended the previous episode are untouched.  ``start_pose_pool()``
        returns the rows, ``set_start_poses(rows)`` replaces them in place by as many others, ``start_index()`` the row every env's
        running episode began at (``_native.RB_START_INDEX_REST``: the zero pose); ``start_poses_size`` and ``start_prob`` hold the
        pool's size (0 without the option) and the probability.  None: the env launches exactly what it launched before."""
        desc = robot.get_description()
        # 1. every ValueError of a bad option, before anything is allocated
        crit_names, crit_mask, crit_dim = critic_obs_spec(critic_obs, desc.n_q, desc.n_t, randomization is not None, action_delay, action_obs)
        obs_names = tuple(c for c in TENDON_OBS_CHANNELS if tendon_obs and tendon_obs_mask(tendon_obs) >> TENDON_OBS_CHANNELS.index(c) & 1)
        obs_scale = tendon_obs_scales(tendon_obs_scale)
        sig = sensor_noise_sigmas(sensor_noise, obs_names)
        delay = action_delay_range(action_delay)
        n_action_rows = action_obs_rows(action_obs)
        shaping = reward_shaping_weights(reward_shaping)
        push_rec = push_spec(push, desc.n_q)
        log_capacity = episode_log_capacity(episode_log)
        start = start_pose_spec(start_poses, start_prob, desc.n_q, desc.q_lo, desc.q_hi)      # (the joint limits, per joint: not the angle box)
        if start is not None and obs_names:
            raise ValueError("start_poses does not combine with tendon_obs: a started env's tendon columns would have to be evaluated at "
                             "the new pose under the held command, and no readout does that yet")
        curriculum = envgoals.goal_curriculum_spec(goal_curriculum)
        if curriculum is not None:
            if goals is None:
                raise ValueError("goal_curriculum needs goals= (a pool whose row order it takes for difficulty order)")
            if isinstance(goals, envgoals.GoalPool) and not goals.recipe.get("ordered"):
                warnings.warn("goal_curriculum: the goal pool's recipe is not marked ordered; ordering it by rest_distance (GoalPool.ordered())")
                goals = goals.ordered()
        if goal_row_stats and curriculum is None:
            raise ValueError("goal_row_stats needs goal_curriculum= (the counts are kept by the row each env holds, the curriculum's index "
                             "plane; goal_curriculum=1 is the plain pool plus that plane)")
        # 2. the simulation and the plain env layer (rb_env_configure)
        self.robot, self.num_envs, self.max_episode_length = robot, int(num_envs), int(max_episode_length)
        self.sim = HipBatchSimulation(robot, num_envs, integrator=integrator, n_substeps=n_substeps, device=device, seed=seed, env_id_offset=env_id_offset)
        angles, vels, acts = robot.get_joint_angles_space(), robot.get_joint_vels_space(), robot.get_action_space()
        self.n_q, self.n_t, self.obs_dim = self.sim.n_q, self.sim.n_t, 3 * self.sim.n_q
        self.action_space = spaces.Box(low=-1, high=1, shape=acts.shape, dtype="float32")
        self.observation_space = spaces.Box(low=np.concatenate((angles.low, vels.low, angles.low)),
                                            high=np.concatenate((angles.high, vels.high, angles.high)), dtype="float32")
        cfg = self._cfg = nat.EnvConfig()
        cfg.joint_vel_penalty, cfg.goal_bonus = int(bool(joint_vel_penalty)), int(bool(is_agent_getting_bonus_for_reaching_goal))
        cfg.max_episode_length, cfg.auto_reset = int(max_episode_length), int(bool(auto_reset))
        cfg.penalty_boundary, cfg.bonus_goal = 1.0, 1000.0
        cfg.angle_lo, cfg.angle_hi, cfg.vel_lo, cfg.vel_hi = float(angles.low[0]), float(angles.high[0]), float(vels.low[0]), float(vels.high[0])
        cfg.action_lo, cfg.action_hi = float(acts.low[0]), float(acts.high[0])
        # thresholds exactly as the reference forms them (roboy_env.py:24-25,127,130)
        cfg.goal_angle_tol, cfg.goal_vel_tol = float(rw.l2_distance(angles.low, angles.high) / 200), float(rw.l2_distance(vels.low, vels.high) / 5)
        for box in (angles, vels, acts):
            if not (np.all(box.low == box.low[0]) and np.all(box.high == box.high[0])):
                raise NotImplementedError("fused env layer expects uniform per-joint boxes")
        # (bad rows: before anything is configured)
        pool_rows = None if goals is None else self._or_close(lambda: envgoals.goal_rows(goals, self.n_q, angles.low, angles.high))
        self.goal_recipe = dict(goals.recipe) if isinstance(goals, envgoals.GoalPool) else {}
        nat.check(self.sim._lib.rb_env_configure(self.sim.handle, ctypes.byref(cfg)))
        # 3. the options, in the one order they take (a call puts its kernels in the place of, in front of or behind those of the calls before
        # it): pool, curriculum, row counts, tendon channels, action rows, buffers, randomization, io, start poses, truncation, critic rows, shaping,
        # pushes, episode log
        self._configure_goal_pool(pool_rows)
        self._configure_goal_curriculum(curriculum)
        self._configure_goal_row_stats(goal_row_stats)
        self._configure_tendon_obs(obs_names, obs_scale)
        self._configure_action_obs(n_action_rows)
        self._allocate_buffers(seed)
        self._configure_randomization(randomization)
        self._configure_io(sensor_noise, action_delay, sig, *delay)
        self._configure_start_poses(start)
        self._configure_truncation(report_truncation)
        self._configure_critic_obs(crit_names, crit_mask, crit_dim)
        self._configure_shaping(shaping)
        self._configure_push(push_rec)
        self._configure_episode_log(log_capacity)

    def _configure_goal_pool(self, pool_rows):
        self.goal_pool_size = 0               # the pool's number of rows m; 0: the env draws its goals from the box
        if pool_rows is not None:
            # before anything is captured into a graph: every env-step launch and reset is followed by the small kernel that puts the
            # pool's rows in place of the box goals (the first call also turns the goal rb_env_configure's reset drew, draw 0, into its
            # pool row: the draw counters stay those of an env without a pool)
            self._or_close(lambda: self._set_goal_pool_rows(pool_rows))

    def _configure_goal_curriculum(self, curriculum):
        self.goal_curriculum = None if curriculum is None else dict(curriculum)
        if curriculum is not None:
            # directly behind the pool, before anything is captured into a graph: from here on the curriculum's kernel stands in the
            # pool kernel's place (the call also redraws every env's goal inside its window; the draw counters stay as they are)
            self._or_close(lambda: envgoals.goal_curriculum_spec(curriculum, m=self.goal_pool_size))
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_goal_curriculum_configure(
                self.sim.handle, curriculum["levels"], curriculum["up"], curriculum["down"], curriculum["start"])))

    def _configure_goal_row_stats(self, goal_row_stats):
        self.goal_row_stats_enabled = bool(goal_row_stats)
        if goal_row_stats:
            # directly behind the curriculum, before anything is captured into a graph: the counting kernel stands in its kernel's place
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_goal_row_stats_enable(self.sim.handle)))

    def _configure_tendon_obs(self, obs_names, obs_scale):
        self.tendon_obs, self.tendon_obs_scale = obs_names, obs_scale
        if self.tendon_obs:
            # before anything is captured into a graph: the extended kernels replace the handle's env-step kernels from here on
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_obs_configure(self.sim.handle, tendon_obs_mask(self.tendon_obs),
                                                                                nat.fptr(self.tendon_obs_scale))))
            lo, hi = [self.observation_space.low], [self.observation_space.high]
            for c in self.tendon_obs:
                b = np.sort(np.float32(_TENDON_OBS_BOUNDS[c]) * self.tendon_obs_scale[TENDON_OBS_CHANNELS.index(c)]) \
                    if self.tendon_obs_scale[TENDON_OBS_CHANNELS.index(c)] != 0 else np.zeros(2, np.float32)
                lo.append(np.full(self.n_t, b[0], np.float32))
                hi.append(np.full(self.n_t, b[1], np.float32))
            self._grow_observation(np.concatenate(lo), np.concatenate(hi))

    def _configure_action_obs(self, n_action_rows):
        self.action_obs = n_action_rows
        if self.action_obs:
            # before anything is captured into a graph: the history kernels replace the env-step kernels from here on
            self._or_close(lambda: self.sim.configure_action_obs(self.action_obs))
            self._grow_observation(*action_obs_bounds(self.observation_space.low, self.observation_space.high, self.n_t, self.action_obs))

    def _grow_observation(self, low, high):
        """an option has widened the row: ``obs_dim`` is read back from the library, and the caller's box has to be as wide"""
        dim = ctypes.c_int32()
        nat.check(self.sim._lib.rb_env_obs_dim(self.sim.handle, ctypes.byref(dim)))
        self.obs_dim = int(dim.value)
        self.observation_space = spaces.Box(low=low, high=high, dtype="float32")
        assert self.observation_space.shape == (self.obs_dim,)

    def _allocate_buffers(self, seed):
        n = self.num_envs                  # (behind the options that set obs_dim)
        self._d_act, self._d_obs = self.sim.malloc(4 * n * self.n_t), self.sim.malloc(4 * n * self.obs_dim)
        self._d_rew, self._d_done = self.sim.malloc(4 * n), self.sim.malloc(4 * n)
        self._slabs_live = 0           # state_dict(): 0 = nothing of this env has written its slabs, 1 = a reset (obs), 2 = a numpy step (all)
        self._pending_actions = None
        self._last_actions = None      # tendon_state(): the last step's actions - _IN_SLAB (numpy: in _d_act) or the torch tensor
        self._d_ts = None              # tendon_state(): device outputs of the numpy path (4 x [N, n_t], first use)
        self._seed, self._replayed_env_steps = int(seed), 0.0
        self._stream = None            # the simulation's own stream

    def _configure_randomization(self, randomization):
        self.randomization = randomization
        if randomization is not None:
            # before anything is captured into a graph: the parameter kernels replace the handle's step kernels from here on
            self._or_close(self.sim.enable_params)
            self._or_close(lambda: self.sim.set_param_ranges(randomization, resample_on_reset=True))

    def _configure_io(self, sensor_noise, action_delay, sig, d_lo, d_hi, ranged):
        self.sensor_noise = dict(sensor_noise or {})
        self.action_delay = None if action_delay is None else ((d_lo, d_hi) if ranged else d_lo)
        self._io = bool(sig.any() or d_hi > 0)
        if self._io:
            # after tendon_obs and randomization, before anything is captured into a graph: the io kernels replace the env-step kernels
            io = nat.EnvIoConfig()
            io.sigma_q, io.sigma_qd = float(sig[0]), float(sig[1])
            for c in range(4):
                io.sigma_tendon[c] = float(sig[2 + c])
            io.delay_lo, io.delay_hi, io.resample_on_reset = d_lo, d_hi, int(ranged)
            self._or_close(lambda: self.sim.configure_io(io))

    def _configure_start_poses(self, start):
        self.start_poses_size = 0             # the pool's number of rows m; 0: every episode begins at the zero pose
        self.start_prob, self.start_recipe = (1.0, {}) if start is None else (start["prob"], dict(start["recipe"]))
        if start is not None:
            # behind the io configuration (the kernel restates the noise of the columns it replaces) and behind the tendon channels, which
            # the library refuses beside it; before anything is captured into a graph: every reset kernel and every env-step launch is
            # followed by the small kernel that puts the pool's rows in place of the zero pose
            rows = start["q"]
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_start_poses_configure(self.sim.handle, nat.fptr(rows), rows.shape[0],
                                                                                        float(start["prob"]))))
            self.start_poses_size = int(rows.shape[0])

    def _configure_truncation(self, report_truncation):
        self.report_truncation = bool(report_truncation)
        self._last_done_codes = None   # truncated(): the last torch step's int32 codes (None: the last step was not a torch step)
        if self.report_truncation:
            # before anything is captured into a graph: every env-step launch is followed by the small kernel that writes the codes
            nat.check(self.sim._lib.rb_env_done_kind_configure(self.sim.handle, 1))

    def _configure_critic_obs(self, crit_names, crit_mask, crit_dim):
        self.critic_obs_names, self.critic_obs_dim = crit_names, 0
        self._last_cobs = None         # critic_obs(): the last torch step's rows (None: the handle's plane holds the last rows)
        if crit_mask:
            # after the options the row reads, before anything is captured into a graph: every env-step launch and reset is followed
            # by the small kernel that writes the rows
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_critic_obs_configure(self.sim.handle, crit_mask)))
            dim = ctypes.c_int32()
            nat.check(self.sim._lib.rb_env_critic_obs_dim(self.sim.handle, ctypes.byref(dim)))
            self.critic_obs_dim = int(dim.value)
            assert self.critic_obs_dim == crit_dim

    def _configure_shaping(self, shaping):
        self.reward_shaping = shaping
        if shaping is not None:
            # after the options it has to agree with, before anything is captured into a graph: every env-step launch gets the cost
            # kernel in front of it and the kernel that applies the cost behind it
            cfg = nat.EnvShapingConfig(shaping["action_rate"], shaping["tension"], shaping["activation"], 0.0)
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_shaping_configure(self.sim.handle, ctypes.byref(cfg))))

    def _configure_push(self, push_rec):
        self.push = push_rec
        if push_rec is not None:
            # before anything is captured into a graph: every env-step launch gets the push kernel in front of it
            pcfg = nat.EnvPushConfig()
            pcfg.threshold = push_rec["threshold"]
            for j, v in enumerate(push_rec["sigma"]):
                pcfg.sigma[j] = v
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_push_configure(self.sim.handle, ctypes.byref(pcfg))))

    def _configure_episode_log(self, capacity):
        self.episode_log_capacity = capacity
        if capacity:
            # last, before anything is captured into a graph: every env-step launch is followed by the small kernel that keeps the
            # records (behind the shaping apply, whose reward it adds up; in front of the kernel that writes the episode-end codes)
            self._or_close(lambda: nat.check(self.sim._lib.rb_env_episode_log_configure(self.sim.handle, capacity)))

    def _or_close(self, configure):
        """an option the library refuses (a joint tree asked for a ball-joint option) must not leave the simulation's handle behind"""
        try:
            return configure()
        except Exception:
            self.sim.close()
            raise

    @staticmethod
    def _need(has_option, message):             # the guard of every accessor that belongs to an option
        if not has_option:
            raise RuntimeError(message)

    # -- goal pool (rb_env_goal_pool_*) -------------------
    def _set_goal_pool_rows(self, rows):
        nat.check(self.sim._lib.rb_env_goal_pool_set(self.sim.handle, nat.fptr(rows), rows.shape[0]))
        self.goal_pool_size = int(rows.shape[0])

    def goal_pool(self) -> np.ndarray:
        """The pool's rows ``[m, n_q]`` as the device holds them; needs ``goals``."""
        self._need(self.goal_pool_size, "this RoboyVecEnv draws its goals from the box (goals=None)")
        d_pool, m = ctypes.c_void_p(), ctypes.c_int64()
        nat.check(self.sim._lib.rb_env_goal_pool_ptr(self.sim.handle, ctypes.byref(d_pool), ctypes.byref(m)))
        self.sim.synchronize()
        return self.sim.download(d_pool.value, (int(m.value), self.n_q))

    def set_goal_pool(self, goals):
        """Replace the pool's rows in place by as many others (a ``GoalPool`` or an array ``[m, n_q]``), between steps: goals drawn from
        now on - also by a captured graph's next replay, the device rows do not move - are rows of the new pool; goals already drawn
        stay until their env draws again.  Needs ``goals``; ``ValueError`` for another size."""
        self._need(self.goal_pool_size, "this RoboyVecEnv draws its goals from the box (goals=None): a pool is given at construction")
        angles = self.robot.get_joint_angles_space()
        rows = envgoals.goal_rows(goals, self.n_q, angles.low, angles.high, m=self.goal_pool_size)
        self._set_goal_pool_rows(rows)
        self.goal_recipe = dict(goals.recipe) if isinstance(goals, envgoals.GoalPool) else {}

    # -- goal curriculum (rb_env_goal_curriculum_*) --------
    def _curriculum_plane(self, getter):
        """a uint32 plane [N] of the curriculum: numpy, or a CUDA int64 tensor when the last step was a torch step"""
        self._need(self.goal_curriculum is not None, "this RoboyVecEnv has no goal curriculum (goal_curriculum=None)")
        ptr = ctypes.c_void_p()
        nat.check(getter(self.sim.handle, ctypes.byref(ptr)))
        self.sim.synchronize()
        plane = self.sim.download(ptr.value, (self.num_envs,), np.uint32)
        if _is_cuda_tensor(self._last_actions):
            import torch
            return torch.from_numpy(plane.astype(np.int64)).to(self._last_actions.device)
        return plane

    def goal_levels(self):
        """``[N]``: every env's level, 0 (the easiest rows only) to ``levels - 1`` (the whole pool).  Needs ``goal_curriculum``."""
        return self._curriculum_plane(self.sim._lib.rb_env_goal_level_ptr)

    def goal_index(self):
        """``[N]``: the pool row every env's goal is; ``_native.RB_GOAL_INDEX_NONE`` behind ``set_goal``.  Needs ``goal_curriculum``."""
        return self._curriculum_plane(self.sim._lib.rb_env_goal_index_ptr)

    def set_goal_levels(self, levels):
        """Write every env's level ``[N]`` (ints below ``levels``), between steps: goals already drawn stay until their env draws
        again.  ``ValueError`` for a level out of range, and nothing has changed then."""
        self._need(self.goal_curriculum is not None, "this RoboyVecEnv has no goal curriculum (goal_curriculum=None)")
        if _is_cuda_tensor(levels):
            levels = levels.cpu().numpy()
        lv = np.asarray(levels)
        if lv.shape != (self.num_envs,) or lv.dtype.kind not in "iu":
            raise ValueError("levels must be %d ints" % self.num_envs)
        if np.any(lv < 0) or np.any(lv >= self.goal_curriculum["levels"]):
            raise ValueError("levels must lie in 0..%d" % (self.goal_curriculum["levels"] - 1))
        lv = np.ascontiguousarray(lv, dtype=np.uint32)
        nat.check(self.sim._lib.rb_env_goal_levels_set(self.sim.handle, lv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))

    def goal_level_histogram(self):
        """``[levels]`` counts: how many envs sit at each level (one small kernel; numpy int64, or a CUDA tensor after a torch step)."""
        self._need(self.goal_curriculum is not None, "this RoboyVecEnv has no goal curriculum (goal_curriculum=None)")
        n_levels = self.goal_curriculum["levels"]
        if _is_cuda_tensor(self._last_actions):
            import torch
            device = self._last_actions.device
            out = torch.empty((n_levels,), dtype=torch.int64, device=device)
            nat.check(self.sim._lib.rb_env_goal_level_hist_dev(self.sim.handle, ctypes.c_void_p(out.data_ptr()),
                                                               ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
            return out
        out = np.empty(n_levels, np.uint64)
        nat.check(self.sim._lib.rb_env_goal_level_hist(self.sim.handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out.astype(np.int64)

    # -- outcome counts per pool row (rb_env_goal_row_stats_*, rb_env_goal_pool_permute) --------
    def goal_row_stats(self, reset: bool = False):
        """``{"attempts": uint64 [m], "reached": uint64 [m]}``: per pool row, the episodes that ended while aimed at it and those of
        them that reached it, since the counts were last cleared (``reset=True`` clears them behind the read).  Needs
        ``goal_row_stats``."""
        self._need(self.goal_row_stats_enabled, "this RoboyVecEnv keeps no goal row stats (goal_row_stats=False)")
        out = np.empty((2, self.goal_pool_size), np.uint64)
        nat.check(self.sim._lib.rb_env_goal_row_stats_read(self.sim.handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(bool(reset))))
        return {"attempts": out[0].copy(), "reached": out[1].copy()}

    def set_goal_row_stats(self, attempts, reached):
        """Write the counts ``[m]`` each (non-negative ints, ``reached <= attempts``), between steps.  ``ValueError`` otherwise, and
        nothing has changed then."""
        self._need(self.goal_row_stats_enabled, "this RoboyVecEnv keeps no goal row stats (goal_row_stats=False)")
        planes = []
        for name, x in (("attempts", attempts), ("reached", reached)):
            a = np.asarray(x.cpu().numpy() if _is_cuda_tensor(x) else x)
            if a.shape != (self.goal_pool_size,) or a.dtype.kind not in "iu":
                raise ValueError("%s must be %d ints" % (name, self.goal_pool_size))
            if a.dtype.kind == "i" and np.any(a < 0):
                raise ValueError("%s must be >= 0" % name)
            planes.append(a.astype(np.uint64))
        if np.any(planes[1] > planes[0]):
            raise ValueError("reached must not exceed attempts")
        both = np.ascontiguousarray(np.stack(planes))
        nat.check(self.sim._lib.rb_env_goal_row_stats_set(self.sim.handle, both.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))

    def permute_goal_pool(self, order):
        """Re-order the live pool, between steps: new row ``j`` is old row ``order[j]`` (a permutation of ``0..m-1``, ``ValueError``
        otherwise and nothing has changed).  The device rows are permuted in place, so a captured graph's next replay reads the new
        order; every env keeps the goal it holds, ``goal_index()`` follows the rows, and the row counts travel with them.  Levels
        stay.  Needs ``goals``; the recipe's ``"ordered"`` mark becomes ``"custom"``."""
        self._need(self.goal_pool_size, "this RoboyVecEnv draws its goals from the box (goals=None)")
        a = np.asarray(order.cpu().numpy() if _is_cuda_tensor(order) else order)
        m = self.goal_pool_size
        if a.shape != (m,) or a.dtype.kind not in "iu":
            raise ValueError("order must be %d ints, a permutation of 0..%d" % (m, m - 1))
        if np.any(a < 0) or np.any(a >= m) or np.unique(a).size != m:
            raise ValueError("order must be a permutation of 0..%d" % (m - 1))
        a = np.ascontiguousarray(a, dtype=np.uint32)
        nat.check(self.sim._lib.rb_env_goal_pool_permute(self.sim.handle, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        if self.goal_recipe.get("ordered"):
            self.goal_recipe["ordered"] = "custom"

    def reorder_goals_by_reach_rate(self, attempts=None, reached=None, prior=(1, 2), halve: bool = True):
        """Re-order the live pool from the most often reached row to the least (``envs.goals.reach_rate_order``) and return the order
        applied.  The rates come from this env's counts, or from ``attempts`` / ``reached`` where given (a multi-rank run passes the
        sums over its ranks, so that every rank applies the same order).  ``halve``: afterwards every count of this env is shifted
        right by one, so an older policy's outcomes fade by a fixed rule.  Needs ``goal_row_stats``."""
        self._need(self.goal_row_stats_enabled, "this RoboyVecEnv keeps no goal row stats (goal_row_stats=False)")
        if (attempts is None) != (reached is None):
            raise ValueError("give both attempts and reached, or neither")
        if attempts is None:
            own = self.goal_row_stats()
            attempts, reached = own["attempts"], own["reached"]
        order = envgoals.reach_rate_order(attempts, reached, prior)
        if order.shape != (self.goal_pool_size,):
            raise ValueError("the pool has %d rows, the counts have %d" % (self.goal_pool_size, order.shape[0]))
        self.permute_goal_pool(order)
        self.goal_recipe["ordered"] = "reach_rate"
        if halve:
            own = self.goal_row_stats()
            self.set_goal_row_stats(own["attempts"] >> np.uint64(1), own["reached"] >> np.uint64(1))
        return order

    # ------------------------------------------------------------------
    def reset(self):
        if self.randomization is not None:
            self.sim.sample_params()
        nat.check(self.sim._lib.rb_env_reset_dev(self.sim.handle, ctypes.c_void_p(self._d_obs)))
        self._last_cobs = None
        self._slabs_live = max(self._slabs_live, 1)
        self.sim.synchronize()
        return self.sim.download(self._d_obs, (self.num_envs, self.obs_dim))

    def set_goal(self, goal_q, step_num=None):
        """Overwrite every env's goal ``[N, n_q]`` (and episode step counter ``[N]``): the
        batched form of assigning ``RoboyEnv._goal_state`` / ``.step_num`` as the reference's
        tests do (``gym_roboy/envs/tests/test_roboy_env.py:62-66,172-176``)."""
        g = nat.as_f32(goal_q, (self.num_envs, self.n_q), "goal_q")
        sn = None
        if step_num is not None:
            sn = np.ascontiguousarray(step_num, dtype=np.uint32)
            if sn.shape != (self.num_envs,):
                raise ValueError("step_num must have shape (%d,)" % self.num_envs)
        nat.check(self.sim._lib.rb_env_set_goal(
            self.sim.handle, nat.fptr(g), None if sn is None else sn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))

    def step(self, actions):
        if _is_cuda_tensor(actions):
            return self._step_torch(actions)
        a = nat.as_f32(actions, (self.num_envs, self.n_t), "actions")
        self.sim.upload(self._d_act, a)
        self.step_dev(self._d_act, self._d_obs, self._d_rew, self._d_done)
        self._last_actions = _IN_SLAB
        self._last_done_codes = None
        self._last_cobs = None
        self._slabs_live = 2
        self.sim.synchronize()
        n = self.num_envs
        return (self.sim.download(self._d_obs, (n, self.obs_dim)),
                self.sim.download(self._d_rew, (n,)),
                self.sim.download(self._d_done, (n,), np.uint32).astype(bool), [{}] * n)

    def step_dev(self, d_act, d_obs, d_rew, d_done, d_cobs=None):
        """Raw device-pointer form: asynchronous on the simulation's stream.  ``d_obs`` holds ``num_envs * obs_dim`` floats.
        ``d_done``: ``num_envs`` uint32, 0 / 1 - with ``report_truncation`` the codes 0 / 1 (terminated) / 2 (truncated).
        ``d_cobs`` (needs ``critic_obs``): ``num_envs * critic_obs_dim`` floats that take the step's critic rows; None leaves them
        in the handle's own plane (``critic_obs()``)."""
        if d_cobs is None:
            nat.check(self.sim._lib.rb_env_step_dev(
                self.sim.handle, ctypes.c_void_p(d_act), ctypes.c_void_p(d_obs),
                ctypes.c_void_p(d_rew), ctypes.c_void_p(d_done)))
        else:
            nat.check(self.sim._lib.rb_env_step_critic_dev(
                self.sim.handle, ctypes.c_void_p(d_act), ctypes.c_void_p(d_obs),
                ctypes.c_void_p(d_rew), ctypes.c_void_p(d_done), ctypes.c_void_p(d_cobs)))

    def step_range_dev(self, first_env, n_envs, stream_ptr, d_act, d_obs, d_rew, d_done, d_cobs=None):
        """``step_dev`` for envs [first_env, first_env + n_envs) on the stream ``stream_ptr`` (None: the simulation's); the
        pointers are those of the WHOLE batch's arrays.  Disjoint ranges may be stepped concurrently on different streams
        (``rb_env_step_range_dev``): how a closed-loop caller overlaps one half's launch gaps and memory phases with the
        other half's arithmetic (``gym_roboy_amd/ppo.py``).  With ``report_truncation`` the range's ``d_done`` words are the codes
        0 / 1 / 2 as ``step_dev`` leaves them, written on the same stream.  ``d_cobs`` (needs ``critic_obs``): the WHOLE batch's
        ``[num_envs, critic_obs_dim]`` array, whose rows of the range are written on the same stream; None: the handle's plane."""
        if d_cobs is None:
            nat.check(self.sim._lib.rb_env_step_range_dev(
                self.sim.handle, int(first_env), int(n_envs), ctypes.c_void_p(int(stream_ptr or 0)), ctypes.c_void_p(d_act),
                ctypes.c_void_p(d_obs), ctypes.c_void_p(d_rew), ctypes.c_void_p(d_done)))
        else:
            nat.check(self.sim._lib.rb_env_step_range_critic_dev(
                self.sim.handle, int(first_env), int(n_envs), ctypes.c_void_p(int(stream_ptr or 0)), ctypes.c_void_p(d_act),
                ctypes.c_void_p(d_obs), ctypes.c_void_p(d_rew), ctypes.c_void_p(d_done), ctypes.c_void_p(d_cobs)))

    def range_capable(self) -> bool:
        return self.sim.range_capable(env_layer=True)

    def _step_torch(self, actions):
        import torch
        n = self.num_envs
        if actions.dtype != torch.float32 or tuple(actions.shape) != (n, self.n_t) or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous float32 CUDA tensor of shape (%d, %d)" % (n, self.n_t))
        # run on torch's current stream so the policy's kernels and the env
        # step are ordered without a host sync
        self.set_stream(torch.cuda.current_stream(actions.device).cuda_stream)
        obs = torch.empty((n, self.obs_dim), dtype=torch.float32, device=actions.device)
        rew = torch.empty((n,), dtype=torch.float32, device=actions.device)
        done = torch.empty((n,), dtype=torch.int32, device=actions.device)
        cobs = torch.empty((n, self.critic_obs_dim), dtype=torch.float32, device=actions.device) if self.critic_obs_dim else None
        self.step_dev(actions.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None if cobs is None else cobs.data_ptr())
        self._last_cobs = cobs
        self._last_actions = actions
        self._last_done_codes = done if self.report_truncation else None
        return obs, rew, done.bool(), [{}] * n

    def truncated(self):
        """``[N]`` bools of the last step: True where the episode ended at the time limit without reaching its goal.  numpy after a
        numpy step (or ``step_dev`` / ``step_range_dev``, read from the handle's code plane after a synchronisation), a CUDA tensor
        after a torch step.  Needs ``report_truncation=True``."""
        self._need(self.report_truncation, "this RoboyVecEnv does not report truncation (report_truncation=False)")
        if self._last_done_codes is not None:
            return self._last_done_codes == nat.RB_DONE_TRUNCATED
        kind = ctypes.c_void_p()
        nat.check(self.sim._lib.rb_env_done_kind_ptr(self.sim.handle, ctypes.byref(kind)))
        self.sim.synchronize()
        return self.sim.download(kind.value, (self.num_envs,), np.uint32) == nat.RB_DONE_TRUNCATED

    def mirror_map(self):
        """``(obs_src int32[obs_dim], obs_sign float32[obs_dim], act_src int32[n_t])``: the mirror image of this env's observation and
        action rows as configured (``envs.symmetry.row_mirror_map`` on the library's ``rb_mirror_info``) - the twin
        ``(obs[:, obs_src] * obs_sign, act[:, act_src])`` of a transition is a transition of the mirrored env.  Raises the library's
        error for a robot without a mirror plane."""
        from .symmetry import row_mirror_map
        info = self.sim.mirror_info()
        return row_mirror_map(self.n_q, self.n_t, info["joint_sign"], info["tendon_image"], self.tendon_obs, self.action_obs)

    def critic_obs(self):
        """``[N, critic_obs_dim]``: the privileged rows that belong to the observation rows last returned.  A CUDA tensor after a torch
        step; otherwise numpy, read from the handle's plane after a synchronisation (a reset, a numpy step, ``step_dev`` /
        ``step_range_dev`` without ``d_cobs``).  Needs ``critic_obs``."""
        self._need(self.critic_obs_dim, "this RoboyVecEnv writes no critic rows (critic_obs=None)")
        if self._last_cobs is not None:
            return self._last_cobs
        rows = ctypes.c_void_p()
        nat.check(self.sim._lib.rb_env_critic_obs_ptr(self.sim.handle, ctypes.byref(rows)))
        self.sim.synchronize()
        return self.sim.download(rows.value, (self.num_envs, self.critic_obs_dim))

    # -- reward shaping (rb_env_shaping_*) -----------------
    def _shaping_plane(self):
        self._need(self.reward_shaping is not None, "this RoboyVecEnv has no reward shaping (reward_shaping=None)")
        ptr = ctypes.c_void_p()
        nat.check(self.sim._lib.rb_env_shaping_cost_ptr(self.sim.handle, ctypes.byref(ptr)))
        return ptr.value

    def shaping_cost(self):
        """``[N]``: the cost the last step subtracted from every env's reward (zeros behind a reset).  numpy after a numpy step, read
        from the handle's plane after a synchronisation; after a torch step a CUDA tensor VIEW of that plane - the next step
        overwrites it, clone it to keep it.  Needs ``reward_shaping``."""
        d_cost = self._shaping_plane()
        if _is_cuda_tensor(self._last_actions):
            return _device_view_f32(d_cost, self.num_envs, self._last_actions.device)
        self.sim.synchronize()
        return self.sim.download(d_cost, (self.num_envs,))

    def shaping_stats(self, reset: bool = False) -> dict:
        """``{"sum_episode_cost", "n_episodes", "sum_step_cost", "n_steps"}``: the summed shaping costs of the episodes that ended and
        their number, the sum of all step costs and the number of env steps, since these sums were last cleared (``reset=True``
        clears them behind the read; ``stats(reset=True)`` does not).  Counted on the device, so steps replayed from a captured
        graph are in.  Needs ``reward_shaping``."""
        self._shaping_plane()
        out = (ctypes.c_double * 4)()
        nat.check(self.sim._lib.rb_env_shaping_stats(self.sim.handle, out, int(bool(reset))))
        return dict(zip(("sum_episode_cost", "n_episodes", "sum_step_cost", "n_steps"), list(out)))

    # -- random pushes (rb_env_push_*) ----------------------
    def _push_planes(self):
        self._need(self.push is not None, "this RoboyVecEnv has no random pushes (push=None)")
        p = [ctypes.c_void_p() for _ in range(4)]
        nat.check(self.sim._lib.rb_env_push_ptr(self.sim.handle, *[ctypes.byref(x) for x in p]))
        return [x.value for x in p]            # count, last, n_pushes, impulse

    def last_push(self):
        """``(pushed [N] bool, impulse [N, n_q])``: the envs the last step pushed, and every env's impulse row (rad/s, exactly what
        was added before the clamp) - an env that was not pushed keeps the row of its last push, zeros before its first.  numpy
        after a numpy step, read after a synchronisation; after a torch step CUDA tensors, ``impulse`` a VIEW of the handle's plane
        that the next step overwrites (clone it to keep it).  Before the first step behind the configuration nobody was pushed (the
        step counter is 0).  Needs ``push``."""
        d_count, d_last, _, d_imp = self._push_planes()
        n = self.num_envs
        if _is_cuda_tensor(self._last_actions):
            import torch
            dev = self._last_actions.device
            count, last = (_device_view_f32(p, n, dev).view(torch.int32) for p in (d_count, d_last))
            return (count == last) & (count != 0), _device_view_f32(d_imp, n * self.n_q, dev).view(n, self.n_q)
        self.sim.synchronize()
        count, last = (self.sim.download(p, (n,), np.uint32) for p in (d_count, d_last))
        return (count == last) & (count != 0), self.sim.download(d_imp, (n, self.n_q))

    def push_count(self, reset: bool = False) -> int:
        """The number of pushes over all envs since the count was last cleared (``reset=True`` clears it behind the read).  Counted
        on the device, so steps replayed from a captured graph are in.  Needs ``push``."""
        self._push_planes()
        out = ctypes.c_uint64()
        nat.check(self.sim._lib.rb_env_push_count(self.sim.handle, ctypes.byref(out), int(bool(reset))))
        return int(out.value)

    # -- start poses (rb_env_start_poses_*) ------------------
    def _start_planes(self):
        self._need(self.start_poses_size, "this RoboyVecEnv starts every episode at the zero pose (start_poses=None)")
        p = [ctypes.c_void_p() for _ in range(3)]
        m = ctypes.c_int64()
        nat.check(self.sim._lib.rb_env_start_poses_ptr(self.sim.handle, ctypes.byref(p[0]), ctypes.byref(m), ctypes.byref(p[1]), ctypes.byref(p[2])))
        assert m.value == self.start_poses_size
        return [x.value for x in p]            # pool, count, index

    def start_pose_pool(self) -> np.ndarray:
        """The pool's rows ``[m, n_q]`` as the device holds them; needs ``start_poses``."""
        d_pool = self._start_planes()[0]
        self.sim.synchronize()
        return self.sim.download(d_pool, (self.start_poses_size, self.n_q))

    def set_start_poses(self, rows):
        """Replace the pool's rows in place by as many others (a ``GoalPool`` or an array ``[m, n_q]``), between steps: episodes that
        start from now on - also in a captured graph's next replay, the device rows do not move - start at rows of the new pool; poses
        already started from stay.  Needs ``start_poses``; ``ValueError`` for another size or a row outside the joint limits."""
        self._start_planes()
        desc = self.robot.get_description()
        start = start_pose_spec(rows, self.start_prob, self.n_q, desc.q_lo, desc.q_hi, m=self.start_poses_size)
        nat.check(self.sim._lib.rb_env_start_poses_set(self.sim.handle, nat.fptr(start["q"]), start["q"].shape[0]))
        self.start_recipe = dict(start["recipe"])

    def start_index(self):
        """``[N]``: the pool row every env's running episode began at, ``_native.RB_START_INDEX_REST`` for the zero pose.  numpy
        (uint32) after a numpy step, read after a synchronisation; after a torch step a CUDA int32 tensor VIEW of the handle's plane
        (the rest pose reads -1) that the next step overwrites - clone it to keep it.  Needs ``start_poses``."""
        d_index = self._start_planes()[2]
        if _is_cuda_tensor(self._last_actions):
            import torch
            return _device_view_f32(d_index, self.num_envs, self._last_actions.device).view(torch.int32)
        self.sim.synchronize()
        return self.sim.download(d_index, (self.num_envs,), np.uint32)

    def start_count(self) -> np.ndarray:
        """``[N]`` uint32: the starts every env has made since the option was configured (numpy, read after a synchronisation)."""
        d_count = self._start_planes()[1]
        self.sim.synchronize()
        return self.sim.download(d_count, (self.num_envs,), np.uint32)

    # -- episode log (rb_env_episode_log_*) ------------------
    def _episode_log_planes(self):
        self._need(self.episode_log_capacity, "this RoboyVecEnv keeps no episode log (episode_log=None)")
        p = [ctypes.c_void_p() for _ in range(5)]
        capacity = ctypes.c_int32()
        nat.check(self.sim._lib.rb_env_episode_log_ptr(self.sim.handle, *[ctypes.byref(x) for x in p], ctypes.byref(capacity)))
        assert capacity.value == self.episode_log_capacity
        return [x.value for x in p]            # count, ret, len, kind, full

    def episode_log(self) -> dict:
        """``{"count": [N], "return": [N, E], "length": [N, E], "kind": [N, E]}`` (numpy; int64, float32, int64, int64), read after a
        synchronisation: env ``i``'s record ``k < count[i]`` is its ``k``-th episode that ended since the log was last cleared; entries
        at or beyond ``count`` are zero.  Needs ``episode_log``."""
        d_count, d_ret, d_len, d_kind, _ = self._episode_log_planes()
        n, E = self.num_envs, self.episode_log_capacity
        self.sim.synchronize()
        count = self.sim.download(d_count, (n,), np.uint32).astype(np.int64)
        live = np.arange(E)[None, :] < count[:, None]
        planes = (self.sim.download(d_ret, (E, n)), self.sim.download(d_len, (E, n), np.uint32).astype(np.int64),
                  self.sim.download(d_kind, (E, n), np.uint32).astype(np.int64))
        ret, length, kind = (np.where(live, np.ascontiguousarray(x.T), x.dtype.type(0)) for x in planes)
        return {"count": count, "return": ret, "length": length, "kind": kind}

    def episode_log_summary(self, first_k=None) -> dict:
        """The records ``k < min(count[i], first_k)`` of every env, reduced on the device in a fixed order (the same planes give the
        same bits; the counts are exact): ``{"n_records", "sum_return", "sum_return_sq", "sum_length", "n_terminated", "n_truncated",
        "n_complete"}`` - the last the number of envs with at least ``first_k`` records - and from them ``mean_return``, ``std_return``
        (population), ``mean_length``, ``success_rate`` (terminated over records), ``truncated_rate`` and ``complete`` (every env has
        its ``first_k``); the means and rates are NaN without a record.  ``first_k=None``: the capacity.  Needs ``episode_log``."""
        self._need(self.episode_log_capacity, "this RoboyVecEnv keeps no episode log (episode_log=None)")
        k = self.episode_log_capacity if first_k is None else first_k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("first_k: an int >= 1, got %r" % (first_k,))
        out = (ctypes.c_double * 8)()
        nat.check(self.sim._lib.rb_env_episode_log_summary(self.sim.handle, int(k), out))
        return episode_log_figures(list(out), self.num_envs)

    def episode_log_full(self) -> int:
        """The number of envs that have all ``episode_log`` records: one 4-byte read behind a synchronisation.  Needs ``episode_log``."""
        d_full = self._episode_log_planes()[4]
        self.sim.synchronize()
        return int(self.sim.download(d_full, (1,), np.uint32)[0])

    def clear_episode_log(self):
        """No records, no episode under way: every env records its next E episodes that START from here - an episode under way is
        dropped from its return and length, so call it behind a ``reset()`` (or accept a first record that is the tail of an episode).
        Enqueued on the env's stream; between replays of a captured graph it needs no new capture.  Needs ``episode_log``."""
        self._need(self.episode_log_capacity, "this RoboyVecEnv keeps no episode log (episode_log=None)")
        nat.check(self.sim._lib.rb_env_episode_log_clear(self.sim.handle))

    def tendon_state(self, actions=None):
        """Per-tendon state of every env at its current state (``HipBatchSimulation.tendon_state``), the set-points formed
        from ``actions`` ``[N, n_t]`` in [-1, 1] as ``step`` forms them (``RB_SP_ENV``): ``{'length', 'rate', 'activation',
        'force'}``, each ``[N, n_t]``.  ``actions=None``: the actions of the last ``step`` (a torch input is read again as it
        is now, not copied), or all set-points 0 before the first step.  numpy in (or a numpy last step) gives numpy out;
        a CUDA tensor gives tensors, on torch's current stream.
        Auto-reset caveat: an env that was done in the last step and reset by it (``auto_reset``) reports its RESET state,
        i.e. the tendons of the zero pose under the last actions, not the state the episode ended in."""
        if actions is None:
            actions = self._last_actions
        if actions is None:
            return self.sim._tendon_state(None, nat.RB_SP_ENV, 1.0)
        if _is_cuda_tensor(actions):
            import torch
            self.set_stream(torch.cuda.current_stream(actions.device).cuda_stream)
            return self.sim._tendon_state(actions, nat.RB_SP_ENV, 1.0)
        if actions is _IN_SLAB:                 # the last numpy step's actions, already on the device
            return self._tendon_state_slab()
        return self.sim._tendon_state(actions, nat.RB_SP_ENV, 1.0)

    def _tendon_state_slab(self):
        from .simulations.hip_simulation_client import TENDON_STATE_KEYS
        n, slab = self.num_envs, 4 * self.num_envs * self.n_t
        if self._d_ts is None:
            self._d_ts = [self.sim.malloc(slab) for _ in TENDON_STATE_KEYS]
        self.sim.tendon_state_dev(self._d_act, nat.RB_SP_ENV, 1.0, *self._d_ts)
        self.sim.synchronize()
        return {k: self.sim.download(d, (n, self.n_t)) for k, d in zip(TENDON_STATE_KEYS, self._d_ts)}

    # -- the rest of stable_baselines' VecEnv surface (what PPO2 / wrappers call on the
    #    reference's SubprocVecEnv, train_parallel.py:29) ---------------------------------
    def step_async(self, actions):
        self._pending_actions = actions

    def step_wait(self):
        actions, self._pending_actions = self._pending_actions, None
        if actions is None:
            raise RuntimeError("step_wait() without step_async()")
        return self.step(actions)

    def seed(self, seed=None):
        """The random streams are keyed at construction (seed, global env id); a VecEnv
        cannot be re-seeded in place.  Returns one entry per env like SubprocVecEnv."""
        if seed is not None and int(seed) != self._seed:
            raise NotImplementedError("construct RoboyVecEnv(seed=%d) instead of re-seeding" % int(seed))
        return [None] * self.num_envs

    def get_attr(self, attr_name, indices=None):
        n = self.num_envs if indices is None else len(list(indices))
        return [getattr(self, attr_name)] * n

    def env_method(self, method_name, *args, indices=None, **kwargs):
        raise NotImplementedError("the envs of a RoboyVecEnv are not separate Python objects (no %s)" % method_name)

    def render(self, mode="human"):
        pass        # RoboyEnv.render is a no-op too (roboy_env.py:89-90)

    def set_stream(self, stream_ptr):
        """Stream of every later launch of this env (``HipBatchSimulation.set_stream``: 0 = the
        device's default stream).  A change drains the previous stream, so it is only forwarded
        when the stream really changes."""
        if stream_ptr != self._stream:
            self.sim.set_stream(stream_ptr)
            self._stream = stream_ptr

    def stats(self, reset: bool = False) -> dict:
        """The task's statistics.  With ``reward_shaping`` they are untouched: returns and ``sum_reward`` are those of the step's own
        reward, without the shaping cost, so the weights change them only through the policy and runs with different weights stay
        comparable (the costs: ``shaping_stats()``).  ``sum_reward`` is the finished episodes' returns plus the running ones: the
        rewards of an episode that ``reset()`` abandoned in mid-episode are in neither."""
        out = (ctypes.c_double * 8)()
        nat.check(self.sim._lib.rb_env_stats(self.sim.handle, out, int(reset)))
        keys = ("sum_return", "sum_return_sq", "n_episodes", "sum_length", "n_goal_reached",
                "n_infeasible_steps", "n_env_steps", "sum_reward")
        stats = dict(zip(keys, list(out)))
        stats["n_env_steps"] += self._replayed_env_steps    # steps replayed from a captured graph
        if reset:
            self._replayed_env_steps = 0.0
        return stats

    def note_replayed_steps(self, n_steps: int):
        """n_env_steps is counted where launches are issued; a caller that replays a
        captured graph of `n_steps` env steps (ppo.py) reports them here."""
        self._replayed_env_steps += float(n_steps) * self.num_envs

    def stats_dev(self, d_out8: int, reset: bool = False):
        nat.check(self.sim._lib.rb_env_stats_dev(self.sim.handle, ctypes.c_void_p(d_out8), int(reset)))

    def get_action_delay(self) -> np.ndarray:
        """Every env's action delay ``[N]`` (steps); needs ``sensor_noise`` or ``action_delay``."""
        self._need(self._io, "this RoboyVecEnv has no action delay (action_delay=None)")
        self.sim.synchronize()
        return self.sim.download(self.sim.io_ptrs()["delay"], (self.num_envs,), np.uint32).astype(np.int64)

    def set_action_delay(self, delay):
        """Overwrite every env's delay ``[N]``: integers in ``[0, hi]`` of the configured ``action_delay``."""
        self._need(self._io, "this RoboyVecEnv has no action delay (action_delay=None)")
        d = np.asarray(delay)
        hi = action_delay_range(self.action_delay)[1]
        if d.shape != (self.num_envs,) or np.any(d < 0) or np.any(d > hi) or np.any(d != np.floor(d)):
            raise ValueError("delay must be %d integers in [0, %d]" % (self.num_envs, hi))
        self.sim.synchronize()
        self.sim.upload(self.sim.io_ptrs()["delay"], np.ascontiguousarray(d, dtype=np.uint32))

    def get_params(self) -> dict:
        """Every env's physical parameters (``HipBatchSimulation.get_params``); needs ``randomization``."""
        self._need(self.randomization is not None, "this RoboyVecEnv has no per-env parameters (randomization=None)")
        return self.sim.get_params()

    # -- snapshot and restore (rb_env_state_*) ---------------
    def _state_identity(self) -> dict:
        info = self.sim.info()
        return {"n_envs": int(info["n_envs"]), "n_q": int(info["n_q"]), "n_t": int(info["n_t"]), "seed": self._seed,
                "env_id_offset": int(info["env_id_offset"]), "integrator": int(info["integrator"]), "n_substeps": int(info["n_substeps"]),
                "step_size": float(info["step_size"])}

    def state_dict(self, dict_view: bool = False) -> dict:
        """Everything a later ``step``, ``reset``, statistic or accessor of this env reads that an earlier one wrote, as a plain dict
        ``torch.save`` takes: ``load_state_dict`` of it into an env constructed with the same arguments continues this env bit for bit
        (every random draw is keyed by seed, global env id and a counter that is part of the state).  Keys: ``"identity"`` (batch
        size, robot sizes, seed, env id offset, integrator, substeps, step size), ``"segments"`` (the library's table of state planes:
        tuples ``(name, dtype, rows, cols, offset)``), ``"blob"`` (those planes, one ``uint8`` numpy array), ``"host"`` (the env-step
        count kept on the host: the library's and the steps replayed from captured graphs as ONE number, as ``stats()`` reports them -
        ``stats_dev`` of the restored env counts the replayed ones too), ``"env"`` (``options.env_checkpoint_record`` - the options in readable form), ``"slabs"`` (the env's
        own action / observation / reward / done buffers) and ``"markers"``.  Taken on the env's stream behind whatever is in flight
        there; work a caller put on another stream (a captured graph on a side stream) must have finished.
        The markers say where the last step's actions, done codes and critic rows are.  A marker that named a CALLER's tensor - after
        a torch step - comes back as None, so in the restored env, until its next step, ``tendon_state()`` without arguments reads
        all set-points 0 and ``critic_obs()`` reads the handle's own plane (the rows of the last reset or numpy step), and the
        accessors answer in numpy.  ``truncated()`` reads the handle's code plane, which is part of the state.
        ``dict_view=True`` adds ``"views"``: every segment as a named numpy view ``[rows, cols]`` of the blob (tests, debugging)."""
        if not isinstance(dict_view, (bool, np.bool_)):
            raise ValueError("state_dict: dict_view must be a bool, got %r" % (dict_view,))
        if getattr(self, "_pending_actions", None) is not None:
            raise RuntimeError("state_dict() between step_async() and step_wait(): the pending actions are no part of a state")
        from .options import ENV_STATE_VERSION, env_checkpoint_record, env_state_views
        record = env_checkpoint_record(self)           # (reads through the accessors: before the snapshot, it changes no plane)
        segments = self.sim.state_segments()
        blob, host = self.sim.save_state()
        host["env_steps"] += float(self._replayed_env_steps)      # one count: stats() adds the two, a captured rollout moves between them
        n = self.num_envs
        # (a slab nothing of this env has written yet holds whatever the allocation held: zeros stand for it, so that the same run gives
        # the same bytes - torch steps and captured rollouts never touch them)
        live = self._slabs_live
        slabs = {"act": self.sim.download(self._d_act, (n, self.n_t)) if live > 1 else np.zeros((n, self.n_t), np.float32),
                 "obs": self.sim.download(self._d_obs, (n, self.obs_dim)) if live > 0 else np.zeros((n, self.obs_dim), np.float32),
                 "rew": self.sim.download(self._d_rew, (n,)) if live > 1 else np.zeros((n,), np.float32),
                 "done": self.sim.download(self._d_done, (n,), np.uint32) if live > 1 else np.zeros((n,), np.uint32)}
        sd = {"version": ENV_STATE_VERSION, "identity": self._state_identity(), "segments": segments, "blob": blob, "host": host,
              "env": record, "slabs": slabs,
              "markers": {"last_actions": "slab" if self._last_actions is _IN_SLAB else None, "last_done_codes": None, "last_cobs": None}}
        if dict_view:
            sd["views"] = env_state_views(segments, blob)
        return sd

    def load_state_dict(self, sd):
        """Continue from ``sd`` (``state_dict()`` of an env constructed with the same arguments).  Identity and segment table are
        compared first: ``ValueError`` naming the first field or segment that differs - another batch size or seed, an option this
        env does not run or the saved one did not, another ring size or log capacity - and nothing has been copied then.  Every plane
        is written in place, so a captured graph of this env's steps continues from the restored state at its next replay.  The pools'
        recipes (``goal_recipe``, ``start_recipe``) come back with their rows; an action handed to ``step_async`` and not yet waited
        for is dropped (``state_dict()`` refuses to be taken in that place)."""
        from .options import ENV_STATE_SLABS, check_env_state_dict, compare_env_state
        check_env_state_dict(sd)                       # (the dict alone: before any library call)
        compare_env_state(self._state_identity(), self.sim.state_segments(), sd)
        n = self.num_envs
        shapes = {"act": (n, self.n_t), "obs": (n, self.obs_dim), "rew": (n,), "done": (n,)}
        for name in ENV_STATE_SLABS:
            if sd["slabs"][name].shape != shapes[name]:
                raise ValueError("load_state_dict: the %s slab has shape %s, this env's has %s" % (name, sd["slabs"][name].shape, shapes[name]))
        self.sim.load_state(sd["blob"], {"env_steps": sd["host"]["env_steps"]})
        for name, d_ptr, dtype in (("act", self._d_act, np.float32), ("obs", self._d_obs, np.float32), ("rew", self._d_rew, np.float32),
                                   ("done", self._d_done, np.uint32)):
            self.sim.upload(d_ptr, np.ascontiguousarray(sd["slabs"][name], dtype=dtype))
        self._slabs_live = 2
        self._replayed_env_steps = 0.0                 # (the state's count holds the replayed steps: the library's counter has them now)
        self._last_actions = _IN_SLAB if sd["markers"].get("last_actions") == "slab" else None
        self._last_done_codes = self._last_cobs = None
        self._pending_actions = None
        # what set_goal_pool / set_start_poses / permute_goal_pool move beside the rows: the recipes a later checkpoint records
        if self.goal_pool_size and "goals" in sd["env"]:
            self.goal_recipe = dict(sd["env"]["goals"].get("recipe") or {})
        if self.start_poses_size and "env_start_poses" in sd["env"]:
            self.start_recipe = dict(sd["env"]["env_start_poses"].get("recipe") or {})

    def close(self):
        self.sim.close()


def _device_view_f32(ptr: int, n: int, device):
    """a float32 CUDA tensor [n] over device memory this library owns (no copy; the memory outlives the tensor's use by contract)"""
    import torch

    class _Plane:
        __cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f4", "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(_Plane(), device=device)


def _is_cuda_tensor(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)
