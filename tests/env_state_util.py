"""TEST HELPER of tests/test_env_state_gpu.py and tests/test_ppo_resume_gpu.py: the option sets a snapshot is taken under, the scenario's
legs, and the bit-for-bit comparison.  Nothing here knows what the planes should hold: every statement of the tests is "the resumed run
is the continuous run", and the continuous run is held to the host model elsewhere (tests/test_env_layer_model_gpu.py)."""
import numpy as np

import goal_pool_util as gp
import push_util as pu
import start_pose_util as su

MAX_LEN, POOL_ROWS, LEG, OTHER = 6, 37, 13, 7      # 13 steps wrap a ring of 4 slots three times and end two episodes of 6 steps
ALL_TERMS = {"action_rate": 0.1, "tension": 0.05, "activation": 0.02}


def _msj():
    from gym_roboy_amd.envs.robots import MsjRobot
    return MsjRobot()


def _upper():
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    return UpperBodyRobot()


def _ball12():
    from random_robots import random_ball_joint_robot
    return random_ball_joint_robot(7, n_t=12)[0]


def _ranges():
    from gym_roboy_amd.envs.params import ParamRanges
    return ParamRanges(force_scale=(0.8, 1.2), setpoint_offset=(-0.01, 0.01), mass_scale=(0.8, 1.25), damping_scale=(0.5, 2.0))


def goal_rows(desc):
    return gp.small_pool(desc, m=POOL_ROWS, base=0.5, step=0.012)


def _common(d, shaping):
    return dict(goals=goal_rows(d), goal_curriculum=dict(levels=4, up=1, down=1, start=2), goal_row_stats=True, report_truncation=True,
                reward_shaping=shaping, push={"prob": 0.25, "sigma": pu.sigma_of(d)}, episode_log=2,
                start_poses=su.pool_of(d, m=POOL_ROWS), start_prob=0.5)


def _ball_all(d):
    """everything a ball-joint robot takes beside start poses (tendon channels exclude them, the tendon terms exclude parameters and delays)"""
    return dict(_common(d, {"action_rate": 0.1}), randomization=_ranges(), critic_obs=("state", "age", "params", "delay", "actions"),
                joint_vel_penalty=True, action_delay=(0, 3), sensor_noise={"q": 0.01, "qd": 0.05}, action_obs=2)


def _ball_tendon(d):
    """the tendon channels, the shaping's tendon terms, a pool without curriculum"""
    return dict(goals=goal_rows(d), tendon_obs=("length", "force"), tendon_obs_scale={"force": 1 / 400},
                sensor_noise={"q": 0.01, "length": 5e-4, "force": 2.0}, action_obs=3, critic_obs=("state", "age", "actions"),
                report_truncation=True, reward_shaping=ALL_TERMS, push={"prob": 0.25, "sigma": pu.sigma_of(d)}, episode_log=2)


# name: (robot factory, integrator, envs, seed, options).  Between them every option is on for every robot class that takes it: the
# ball-joint classes (8 tendons: the ahead-of-time table; 12: the run-time tendon count) everything, joint trees what _common holds.
# 300 and 66 envs: neither a multiple of 256 nor of 64, so the rows of the [k][n] planes are unaligned
SETS = {
    "msj_all": (_msj, "rk4", 300, 14, _ball_all),
    "msj_tendon": (_msj, "euler", 300, 7, _ball_tendon),
    "ball12_all": (_ball12, "euler", 300, 18, _ball_all),
    "ball12_tendon": (_ball12, "rk4", 300, 5, _ball_tendon),
    "upper_all": (_upper, "euler", 66, 2, lambda d: _common(d, ALL_TERMS)),
}


def make_env(name, n=None, seed=None, **override):
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    make, integ, n0, seed0, options = SETS[name]
    robot = make()
    kw = dict(options(robot.get_description()), **override)
    return RoboyVecEnv(robot, n0 if n is None else n, seed=seed0 if seed is None else seed, integrator=integ, max_episode_length=MAX_LEN, **kw)


def actions(name, steps, seed):
    """[steps, n, n_t] float32 from U(-2, 2): some outside the box [-1, 1]"""
    make, _, n, _, _ = SETS[name]
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (steps, n, make().get_description().n_t)).astype(np.float32)


def to_np(x):
    if isinstance(x, dict):
        return {k: to_np(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [to_np(v) for v in x]
    if type(x).__module__.startswith("torch"):
        return x.detach().cpu().numpy().copy()
    return x


def first_difference(a, b, where=""):
    """None where a and b are the same bit for bit (arrays by their bytes, shape and type; floats by their bytes), else where they differ"""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)) or list(a) != list(b):
            return where + ": keys"
        for k in a:
            d = first_difference(a[k], b[k], "%s[%r]" % (where, k))
            if d:
                return d
        return None
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        if not (isinstance(a, (tuple, list)) and isinstance(b, (tuple, list))) or len(a) != len(b):
            return where + ": length"
        for k, (x, y) in enumerate(zip(a, b)):
            d = first_difference(x, y, "%s[%d]" % (where, k))
            if d:
                return d
        return None
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s: %s %s against %s %s" % (where, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)):
            return "%s: %d of %d entries differ" % (where, int((a != b).sum()), a.size)
        return None
    if isinstance(a, float) and isinstance(b, float):
        return None if np.float64(a).tobytes() == np.float64(b).tobytes() else "%s: %r against %r" % (where, a, b)
    return None if type(a) is type(b) and a == b else "%s: %r against %r" % (where, a, b)


def step_outputs(env, out):
    """everything a step returns or leaves behind an accessor, as numpy copies"""
    rec = {"obs": out[0], "reward": out[1], "done": out[2]}
    if env.report_truncation:
        rec["truncated"] = env.truncated()
    if env.critic_obs_dim:
        rec["critic_obs"] = env.critic_obs()
    if env.reward_shaping is not None:
        rec["shaping_cost"] = env.shaping_cost()
    if env.push is not None:
        rec["last_push"] = env.last_push()
    return to_np(rec)


def final_accessors(env, probe_actions):
    """every accessor at the end of a run; ``probe_actions``: what tendon_state() is asked under (numpy or a CUDA tensor)"""
    rec = {"stats": env.stats()}
    if env.randomization is None:             # (the readout has no per-env-parameter form: the library refuses it beside randomization)
        rec["tendon_state"] = env.tendon_state(probe_actions)
    if env.episode_log_capacity:
        rec["episode_log"] = env.episode_log()
        rec["episode_log_summary"] = env.episode_log_summary()
        rec["episode_log_full"] = env.episode_log_full()
    if env.goal_curriculum is not None:
        rec["goal_levels"], rec["goal_index"], rec["goal_level_histogram"] = env.goal_levels(), env.goal_index(), env.goal_level_histogram()
    if env.goal_row_stats_enabled:
        rec["goal_row_stats"] = env.goal_row_stats()
    if env.goal_pool_size:
        rec["goal_pool"] = env.goal_pool()
    if env.start_poses_size:
        rec["start_index"], rec["start_count"], rec["start_pose_pool"] = env.start_index(), env.start_count(), env.start_pose_pool()
    if env.push is not None:
        rec["push_count"] = env.push_count()
    if env.reward_shaping is not None:
        rec["shaping_stats"] = env.shaping_stats()
    if env._io:
        rec["action_delay"] = env.get_action_delay()
    if env.randomization is not None:
        rec["params"] = env.get_params()
    return to_np(rec)


def run_steps(env, acts, cuda):
    """one env.step per row block of ``acts`` (numpy, or CUDA tensors on the current stream) -> the list of step_outputs"""
    recs = []
    for a in acts:
        if cuda:
            import torch
            a = torch.from_numpy(a).cuda()
        recs.append(step_outputs(env, env.step(a)))
    return recs


def state_views(env):
    """(segment table, {name: plane}, the rest of the dict without blob and views) of env.state_dict(dict_view=True)"""
    sd = env.state_dict(dict_view=True)
    rest = {k: to_np(v) for k, v in sd.items() if k not in ("blob", "views", "segments")}
    return sd["segments"], sd["views"], rest
