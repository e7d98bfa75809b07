"""The surface of ``RoboyVecEnv``'s options in one place: the validators the constructor runs before anything is allocated, the one
``KEY=VALUE,...`` parser, ``train_parallel``'s env flags and the keyword arguments they become, what a checkpoint records about the env,
checks at ``load()`` and replays in ``visualize_agent``.  No torch at import, no library load.  A new option: NEXT.md, "an env option"."""
import numpy as np

from .. import _native as nat

# tendon channels of the observation, in row order, with their bits (rb_obs_channel) and physical bounds
TENDON_OBS_CHANNELS = ("length", "rate", "activation", "force")
_TENDON_OBS_BOUNDS = {"length": (0.0, np.inf), "rate": (-np.inf, np.inf), "activation": (0.0, 1.0), "force": (0.0, np.inf)}
SENSOR_NOISE_KEYS = ("q", "qd") + TENDON_OBS_CHANNELS
DEFAULT_GOAL_POOL = 16384                        # --goals reachable
DEFAULT_START_POOL = 4096                        # --start-poses reachable
ENV_INTEGRATOR = "euler"                         # RoboyVecEnv's default: the pool is settled with the integrator the env steps with
GOAL_ORDERS = ("rest_distance", "reach_rate")


def tendon_obs_mask(channels) -> int:
    """Channel names (any order, no repeats) -> the mask of ``rb_env_obs_configure``."""
    names = [channels] if isinstance(channels, str) else list(channels)
    unknown = [c for c in names if c not in TENDON_OBS_CHANNELS]
    if unknown or len(set(names)) != len(names):
        raise ValueError("tendon_obs takes distinct names out of %s, got %r" % (TENDON_OBS_CHANNELS, channels))
    return sum(1 << TENDON_OBS_CHANNELS.index(c) for c in names)


def tendon_obs_scales(scale) -> np.ndarray:
    """``{"force": 1/400, ...}`` (or None) -> the four finite fp32 scales in channel order, 1 where not given."""
    out = np.ones(4, np.float32)
    for k, v in dict(scale or {}).items():
        if k not in TENDON_OBS_CHANNELS:
            raise ValueError("tendon_obs_scale: unknown channel %r" % (k,))
        out[TENDON_OBS_CHANNELS.index(k)] = v
    if not np.all(np.isfinite(out)):
        raise ValueError("tendon_obs_scale must be finite")
    return out


def sensor_noise_sigmas(sensor_noise, tendon_obs=()) -> np.ndarray:
    """``{"q": 0.01, "force": 2.0, ...}`` (or None) -> six fp32 standard deviations ``[q, qd, length, rate, activation, force]``
    in physical units, 0 where not given.  Keys: ``q``, ``qd`` and the channel names; a channel must be one of ``tendon_obs``."""
    out = np.zeros(6, np.float32)
    for k, v in dict(sensor_noise or {}).items():
        if k not in SENSOR_NOISE_KEYS:
            raise ValueError("sensor_noise: unknown key %r (takes %s)" % (k, SENSOR_NOISE_KEYS))
        if k in TENDON_OBS_CHANNELS and k not in tuple(tendon_obs or ()):
            raise ValueError("sensor_noise: channel %r is not in tendon_obs" % (k,))
        if not np.isfinite(v) or v < 0:
            raise ValueError("sensor_noise[%r] must be finite and >= 0" % (k,))
        out[SENSOR_NOISE_KEYS.index(k)] = v
    return out


def action_delay_range(action_delay):
    """``2`` -> ``(2, 2, False)``, ``(0, 3)`` -> ``(0, 3, True)`` (a range is redrawn on auto-reset), None -> ``(0, 0, False)``"""
    if action_delay is None:
        return 0, 0, False
    if isinstance(action_delay, (int, np.integer)):
        lo = hi = int(action_delay)
        ranged = False
    else:
        lo, hi = (int(x) for x in action_delay)
        ranged = True
    if not 0 <= lo <= hi <= nat.RB_IO_MAX_DELAY:
        raise ValueError("action_delay: 0 <= lo <= hi <= %d, got %r" % (nat.RB_IO_MAX_DELAY, action_delay))
    return lo, hi, ranged


def action_obs_rows(action_obs) -> int:
    """None -> 0, K -> K: the number of action rows behind the observation, 0 <= K <= 8"""
    if action_obs is None:
        return 0
    if isinstance(action_obs, bool) or not isinstance(action_obs, (int, np.integer)) or not 0 <= int(action_obs) <= nat.RB_ACTION_OBS_MAX:
        raise ValueError("action_obs: an int, 0 <= K <= %d, got %r" % (nat.RB_ACTION_OBS_MAX, action_obs))
    return int(action_obs)


def action_obs_bounds(low, high, n_t: int, rows: int):
    """The observation box with K = ``rows`` action rows behind it: ``rows * n_t`` more columns, each within [-1, 1] (the clamp
    the env step applies to an action).  Returns ``(low, high)`` as float32 arrays."""
    extra = int(rows) * int(n_t)
    return (np.concatenate((np.asarray(low, np.float32), np.full(extra, -1.0, np.float32))),
            np.concatenate((np.asarray(high, np.float32), np.full(extra, 1.0, np.float32))))


def critic_obs_spec(critic_obs, n_q: int, n_t: int, randomization: bool = False, action_delay=None, action_obs=None):
    """Block names of a privileged critic row (``RoboyVecEnv(critic_obs=...)``; any order, no repeats; ``"state"`` is always part of the
    row, named or not) -> ``(names in row order, the mask of rb_env_critic_obs_configure, Dc)`` for a ball-joint robot with ``n_q``
    joints and ``n_t`` tendons.  None or an empty list: ``((), 0, 0)``.  ``ValueError`` for an unknown name, for a block whose option
    the env does not have (``params``: ``randomization``; ``delay``: an ``action_delay`` above 0; ``actions``: ``action_obs=K``) and
    for a row wider than 63 columns, the PPO gradient kernels' input limit."""
    if critic_obs is None:
        return (), 0, 0
    names = [critic_obs] if isinstance(critic_obs, str) else list(critic_obs)
    unknown = [c for c in names if c not in nat.CRITIC_OBS_BLOCKS]
    if unknown or len(set(names)) != len(names):
        raise ValueError("critic_obs takes distinct names out of %s, got %r" % (nat.CRITIC_OBS_BLOCKS, critic_obs))
    if not names:
        return (), 0, 0
    rows = action_obs_rows(action_obs)
    needs = {"params": (bool(randomization), "randomization"), "delay": (action_delay_range(action_delay)[1] > 0, "an action_delay above 0"),
             "actions": (rows > 0, "action_obs=K")}
    for c in names:
        if c in needs and not needs[c][0]:
            raise ValueError("critic_obs: %r needs %s" % (c, needs[c][1]))
    names = tuple(c for c in nat.CRITIC_OBS_BLOCKS if c == "state" or c in names)
    width = {"state": 3 * n_q, "age": 1, "params": 2 * n_t + 4, "delay": 1, "actions": rows * n_t}
    dim = sum(width[c] for c in names)
    if dim > nat.RB_CRITIC_OBS_MAX_DIM:
        raise ValueError("critic_obs: %s is %d columns wide, at most %d (the PPO gradient kernels' input limit)"
                         % (names, dim, nat.RB_CRITIC_OBS_MAX_DIM))
    return names, sum(1 << nat.CRITIC_OBS_BLOCKS.index(c) for c in names), dim


def reward_shaping_weights(reward_shaping):
    """``{"action_rate": 0.05, "tension": 0.01}`` (or None) -> the dict with all three keys of ``_native.REWARD_SHAPING_TERMS`` as
    floats, 0 where not given - or None where every weight is 0 (the option is off).  ``ValueError`` for an unknown key and for a
    weight that is negative or not finite."""
    if reward_shaping is None:
        return None
    out = dict.fromkeys(nat.REWARD_SHAPING_TERMS, 0.0)
    for k, v in dict(reward_shaping).items():
        if k not in nat.REWARD_SHAPING_TERMS:
            raise ValueError("reward_shaping: unknown term %r (takes %s)" % (k, nat.REWARD_SHAPING_TERMS))
        if isinstance(v, bool) or not np.isfinite(v) or v < 0:
            raise ValueError("reward_shaping[%r] must be finite and >= 0, got %r" % (k, v))
        out[k] = float(np.float32(v))
    return out if any(out.values()) else None


def push_spec(push, n_q: int):
    """``{"prob": p, "sigma": s}`` (or None) -> ``{"prob": p, "sigma": [n_q floats], "threshold": round(p * 2**24)}`` - or None where
    the option is off (``prob`` rounds to a threshold of 0, or every sigma is 0).  ``sigma``: a scalar or ``n_q`` entries, rad/s, as
    the library holds them (float32).  ``ValueError`` for an unknown or missing key, a ``prob`` outside [0, 1], a sigma that is negative
    or not finite, or a sigma vector of another length."""
    if push is None:
        return None
    push = dict(push)
    for k in push:
        if k not in ("prob", "sigma"):
            raise ValueError("push: unknown key %r (takes 'prob' and 'sigma')" % (k,))
    if "prob" not in push or "sigma" not in push:
        raise ValueError("push: needs both 'prob' and 'sigma', got %r" % (sorted(push),))
    p = push["prob"]
    if isinstance(p, bool) or not np.isscalar(p) or not np.isfinite(p) or p < 0 or p > 1:
        raise ValueError("push['prob'] must be in [0, 1], got %r" % (p,))
    sig = np.asarray(push["sigma"], dtype=np.float64)
    if sig.ndim == 0:
        sig = np.full(n_q, float(sig))
    if sig.shape != (n_q,):
        raise ValueError("push['sigma'] must be a scalar or have %d entries (one per joint), got shape %r" % (n_q, sig.shape))
    if not np.all(np.isfinite(sig)) or np.any(sig < 0):
        raise ValueError("push['sigma'] must be finite and >= 0, got %r" % (push["sigma"],))
    sig = sig.astype(np.float32)
    threshold = int(round(float(p) * 2 ** 24))
    if threshold == 0 or not sig.any():
        return None
    return {"prob": float(p), "sigma": [float(v) for v in sig], "threshold": threshold}


def start_pose_spec(start_poses, start_prob, n_q: int, low, high, m=None):
    """``RoboyVecEnv(start_poses=pool, start_prob=p)`` -> ``{"q": float32 rows [m, n_q], "prob": p, "threshold": round(p * 2**24),
    "recipe": dict}`` - or None without a pool (the option is off; ``start_prob`` must then be left at 1).  ``start_poses``: an
    ``envs.goals.GoalPool`` (its recipe is kept) or an array ``[m, n_q]``, every value finite and inside ``[low, high]``, the robot's
    joint limits (``goals.goal_rows``); ``m`` given: the size of the pool the env already holds.  ``start_prob`` 0 keeps the option on
    (every episode starts at rest, the planes are kept).  ``ValueError`` for bad rows and for a ``start_prob`` outside [0, 1]."""
    from . import goals as envgoals
    p = start_prob
    if isinstance(p, (bool, str)) or not np.isscalar(p) or not np.isfinite(p) or p < 0 or p > 1:
        raise ValueError("start_prob must be in [0, 1], got %r" % (p,))
    if start_poses is None:
        if float(p) != 1.0:
            raise ValueError("start_prob needs start_poses= (a pool of poses to start from)")
        return None
    try:
        rows = envgoals.goal_rows(start_poses, n_q, low, high, m=m)
    except ValueError as e:
        raise ValueError("start_poses: %s" % e) from None
    recipe = dict(start_poses.recipe) if isinstance(start_poses, envgoals.GoalPool) else {}
    return {"q": rows, "prob": float(p), "threshold": int(round(float(p) * 2 ** 24)), "recipe": recipe}


def episode_log_capacity(episode_log) -> int:
    """None -> 0 (the option is off), E -> E: the number of finished episodes the env records per env, 1 <= E <= 64.  ``ValueError``
    for anything else (0 too: an env without the option is ``episode_log=None``)."""
    if episode_log is None:
        return 0
    if isinstance(episode_log, bool) or not isinstance(episode_log, (int, np.integer)) or not 1 <= int(episode_log) <= nat.RB_EPISODE_LOG_MAX:
        raise ValueError("episode_log: an int, 1 <= E <= %d, got %r" % (nat.RB_EPISODE_LOG_MAX, episode_log))
    return int(episode_log)


EPISODE_LOG_SUMS = ("n_records", "sum_return", "sum_return_sq", "sum_length", "n_terminated", "n_truncated", "n_complete")


def episode_log_figures(sums, num_envs: int) -> dict:
    """the eight sums of ``rb_env_episode_log_summary`` (over one env batch, or added up over several of ``num_envs`` envs in all) ->
    ``episode_log_summary``'s dict"""
    out = {key: float(v) for key, v in zip(EPISODE_LOG_SUMS, sums)}
    n = out["n_records"]
    nan = float("nan")
    out["mean_return"] = out["sum_return"] / n if n else nan
    out["std_return"] = max(out["sum_return_sq"] / n - out["mean_return"] ** 2, 0.0) ** 0.5 if n else nan
    out["mean_length"] = out["sum_length"] / n if n else nan
    out["success_rate"] = out["n_terminated"] / n if n else nan
    out["truncated_rate"] = out["n_truncated"] / n if n else nan
    out["complete"] = bool(out["n_complete"] == num_envs)
    return out


# ---- the command line (train_parallel) ----
def parse_key_values(text, name, form="KEY=VALUE", check=lambda values: None):
    """``key=1.5,other=2`` -> ``{"key": 1.5, "other": 2.0}`` ('' -> None); ``ValueError`` in the option's ``name`` for a malformed item"""
    out = {}
    for item in filter(None, (text or "").split(",")):
        if "=" not in item:
            raise ValueError("%s: expected %s, got %r" % (name, form, item))
        k, v = item.split("=", 1)
        if k in out:
            raise ValueError("%s: %r given twice" % (name, k))
        out[k] = float(v)
    check(out or None)                           # (a caller's validator: raises, or lets the dict pass as it is)
    return out or None


def parse_reward_shaping(text):
    """The command line's ``action_rate=0.05,tension=0.01`` -> the dict ``reward_shaping_weights`` takes ('' -> None)."""
    return parse_key_values(text, "reward shaping", "TERM=WEIGHT", check=reward_shaping_weights)


def parse_push(text):
    """The command line's ``prob=0.02,sigma=0.5`` -> the dict ``RoboyVecEnv(push=...)`` takes ('' -> None); one sigma for every joint."""
    return parse_key_values(text, "push", check=lambda push: push_spec(push, 1))


def parse_goals(text):
    """``--goals``: "" -> 0 (box goals), "reachable" -> 16384, "reachable:M" -> M"""
    if not text:
        return 0
    kind, _, m = text.partition(":")
    if kind != "reachable" or (m and (not m.isdigit() or int(m) < 1)):
        raise SystemExit("--goals takes reachable or reachable:M with M >= 1, got %r" % text)
    return int(m) if m else DEFAULT_GOAL_POOL


def parse_start_poses(text, prob=None):
    """``--start-poses reachable[:M] --start-prob P``: ``(0, 1.0)`` without ``--start-poses``, else ``(M, P)`` with M the pool's size
    (default 4096) and P in [0, 1] (default 1); ``--start-prob`` needs ``--start-poses``"""
    if not text:
        if prob is not None:
            raise SystemExit("--start-prob needs --start-poses")
        return 0, 1.0
    kind, _, m = text.partition(":")
    if kind != "reachable" or (m and (not m.isdigit() or int(m) < 1)):
        raise SystemExit("--start-poses takes reachable or reachable:M with M >= 1, got %r" % text)
    prob = 1.0 if prob is None else prob
    if not 0.0 <= prob <= 1.0:               # (NaN too)
        raise SystemExit("--start-prob takes P in [0, 1], got %r" % (prob,))
    return (int(m) if m else DEFAULT_START_POOL), float(prob)


def parse_goal_curriculum(levels, up, down, goals_m):
    """``--goal-levels L --goal-up U --goal-down D``: None without ``--goal-levels``, else RoboyVecEnv's ``goal_curriculum`` dict;
    needs ``--goals`` (``goals_m``: its pool size, 0 without) and ``1 <= L <= min(M, 256)``, ``U, D >= 0``"""
    if not levels:
        if up is not None or down is not None:
            raise SystemExit("--goal-up and --goal-down need --goal-levels")
        return None
    if not goals_m:
        raise SystemExit("--goal-levels needs --goals (a curriculum runs over a goal pool)")
    up, down = 1 if up is None else up, 1 if down is None else down
    if not 1 <= levels <= min(goals_m, 256) or up < 0 or down < 0:
        raise SystemExit("--goal-levels takes 1..min(M, 256), --goal-up and --goal-down take >= 0; got %d, %d, %d with a pool of %d"
                         % (levels, up, down, goals_m))
    return {"levels": levels, "up": up, "down": down, "start": 0}


def parse_goal_order(order, reorder_every, goal_curriculum):
    """``--goal-order KEY --goal-reorder-every R``: ``reach_rate`` re-orders the pool by the measured reach rate per row after every
    R-th round and needs ``--goal-levels`` (the counts are kept by the curriculum's index plane); R >= 1"""
    if order not in GOAL_ORDERS:
        raise SystemExit("--goal-order takes %s, got %r" % (" or ".join(GOAL_ORDERS), order))
    if reorder_every < 1:
        raise SystemExit("--goal-reorder-every takes R >= 1, got %d" % reorder_every)
    if order == "reach_rate" and goal_curriculum is None:
        raise SystemExit("--goal-order reach_rate needs --goal-levels (the counts per row are kept by the curriculum)")
    if order != "reach_rate" and reorder_every != 1:
        raise SystemExit("--goal-reorder-every needs --goal-order reach_rate")
    return order == "reach_rate"


# the env's flags: (flag, type, default, metavar, help).  Two groups, because --help lists flags in the order they were declared and the
# agent's own stand between the env's (--bootstrap-timeouts is the agent's flag; the env follows it, env_kwargs_from_args)
ENV_FLAGS = (
    ("--tendon-obs", str, "", "CHANNELS", "comma-separated tendon channels appended to the observation, out of length,rate,activation,force "
     "(e.g. length,force: 25 columns for MsjRobot); stored in the checkpoint"),
    ("--tendon-obs-scale", str, "", "CHANNEL=FACTOR,...", "factor per channel, default 1 (m, m/s, [0,1], N), e.g. force=0.0025,length=4"),
    ("--sensor-noise", str, "", "KEY=SIGMA,...", "Gaussian noise on the observation: standard deviations in physical units for q, qd and the "
     "selected tendon channels, e.g. q=0.01,qd=0.05,force=2; stored in the checkpoint"),
    ("--action-delay", str, "", "D | LO:HI", "steps by which every action acts late (at most 7): one number, or a range each env draws from at "
     "every episode start, e.g. 0:3; stored in the checkpoint"),
    ("--action-obs", int, 0, "K", "append the last K commanded actions (at most 8, newest first, zeros where the episode is younger) to the "
     "observation: what the policy needs to compensate --action-delay; stored in the checkpoint"),
    ("--critic-obs", str, "", "BLOCK,...", "an asymmetric critic: the value net is trained on privileged rows the env writes beside the "
     "observation - state (exact q, qd, goal; always part of the row), age, params, delay (needs --action-delay), actions (needs --action-obs), "
     "e.g. state,age,delay,actions; only the actor is deployed; recorded in the checkpoint"),
    ("--goals", str, "", "reachable[:M]", "draw every goal from a pool of M poses (default 16384) the robot holds under constant set-points, "
     "made once at start with the run's seed and integrator (envs.goals.reachable_goals; every rank makes the same pool) instead of uniformly in "
     "the goal box; rows and recipe are stored in the checkpoint"),
    ("--goal-levels", int, 0, "L", "a goal curriculum over the pool ordered by distance from the rest pose (needs --goals): every env starts at "
     "level 0 of L, draws its goals from the nearest (level + 1) / L of the pool, and moves with its episodes' outcomes; levels are stored in "
     "the checkpoint"),
    ("--goal-up", int, None, "U", "levels up after an episode that reached its goal (default 1)"),
    ("--goal-down", int, None, "D", "levels down after an episode that did not (default 1)"),
    ("--goal-order", str, "rest_distance", "KEY", "what the curriculum takes for difficulty: rest_distance (default: the pool stays ordered by "
     "distance from the rest pose) or reach_rate (needs --goal-levels: the run starts from that order, counts per pool row how many episodes "
     "aimed at it and how many reached it, and re-orders the live pool by the measured rate, summed over the ranks, after every R-th round; the "
     "counts are stored in the checkpoint)"),
    ("--goal-reorder-every", int, 1, "R", "rounds between re-orderings (default 1)"),
    # behind the agent's flags (add_env_arguments(ap, late=True)):
    ("--reward-shaping", str, "", "TERM=WEIGHT,...", "regularising reward terms, subtracted from the step's reward on the device: action_rate "
     "(mean squared change of the clamped action within an episode), tension (mean squared tendon force over its maximum), activation (mean "
     "squared muscle activation), e.g. action_rate=0.05,tension=0.01; the round's statistics then show shaping_cost_per_step, while return and "
     "goals reached stay the task's; recorded in the checkpoint"),
    ("--push", str, "", "prob=P,sigma=S", "random velocity pushes, an external disturbance on the device: in front of every env step each env is "
     "pushed with probability P, a pushed env's joint velocities get S * z added (z standard normal, S in rad/s) and are clamped to the robot's "
     "bounds, e.g. prob=0.02,sigma=0.5; the round's statistics then show pushes_per_step; recorded in the checkpoint"),
    ("--episode-log", int, 0, "E", "record every env's first E finished episodes (at most 64) on the device: return, length and whether the goal "
     "was reached (RoboyVecEnv.episode_log, episode_log_summary); a condition of the run, recorded in the checkpoint and not replayed"),
    ("--start-poses", str, "", "reachable[:M]", "begin episodes, at a reset and at every auto-reset, at a pose out of a pool of M poses (default "
     "4096) the robot holds under constant set-points, with zero velocity, instead of the zero pose; the pool is made once at start with the "
     "run's seed + 1 (so it is not the goal pool; every rank makes the same one); the round's statistics then show start_pool_share; rows and "
     "recipe are recorded in the checkpoint"),
    ("--start-prob", float, None, "P", "the probability that an episode begins at a pool pose (default 1; otherwise it begins at the zero "
     "pose); needs --start-poses"),
)

N_LATE_ENV_FLAGS = 5                             # ENV_FLAGS' last rows: declared behind the agent's flags


def add_env_arguments(ap, late: bool = False):
    """Declare the env's flags on ``ap``: the observation and goal flags, or (``late=True``) the reward and disturbance flags."""
    for flag, kind, default, metavar, text in (ENV_FLAGS[-N_LATE_ENV_FLAGS:] if late else ENV_FLAGS[:-N_LATE_ENV_FLAGS]):
        ap.add_argument(flag, type=kind, default=default, metavar=metavar, help=text)


def env_kwargs_from_args(args) -> dict:
    """The parsed command line -> ``RoboyVecEnv``'s keyword arguments, all but what only the running process knows (``goals``, the pool
    ``--goals`` asks for; ``device``; ``env_id_offset``).  An option that is off is None, or absent (``goal_row_stats``, ``reward_shaping``, ``push``,
    ``episode_log``, ``start_poses``: here ``{"m": M, "prob": P}``, what the running process makes the pool from - ``start_pose_pool``)."""
    noise = parse_key_values(args.sensor_noise, "sensor noise", "KEY=SIGMA")         # (a bad flag is reported in this order)
    delay = [int(x) for x in args.action_delay.split(":")] if args.action_delay else None
    scale = parse_key_values(args.tendon_obs_scale, "tendon obs scale", "CHANNEL=FACTOR")
    curriculum = parse_goal_curriculum(args.goal_levels, args.goal_up, args.goal_down, parse_goals(args.goals))
    kw = dict(seed=args.seed, integrator=ENV_INTEGRATOR, tendon_obs=tuple(c for c in args.tendon_obs.split(",") if c) or None,
              tendon_obs_scale=scale, sensor_noise=noise, action_delay=delay and (delay[0] if len(delay) == 1 else (delay[0], delay[1])),
              report_truncation=args.bootstrap_timeouts, action_obs=args.action_obs or None,
              critic_obs=tuple(c for c in args.critic_obs.split(",") if c) or None, goal_curriculum=curriculum)
    late = {"goal_row_stats": parse_goal_order(args.goal_order, args.goal_reorder_every, curriculum),
            "reward_shaping": parse_reward_shaping(args.reward_shaping), "push": parse_push(args.push),
            "episode_log": episode_log_capacity(getattr(args, "episode_log", 0) or None)}
    start_m, start_prob = parse_start_poses(getattr(args, "start_poses", ""), getattr(args, "start_prob", None))
    if start_m:
        late["start_poses"] = {"m": start_m, "prob": start_prob}
    return dict(kw, **{key: value for key, value in late.items() if value})


def start_pose_pool(robot, request, seed: int, device: int = 0):
    """``env_kwargs_from_args``' ``start_poses`` request ``{"m", "prob"}`` -> ``RoboyVecEnv``'s ``(start_poses, start_prob)``: the pool
    ``reachable_goals`` makes with the run's seed + 1 - not the goal pool's rows, and every rank makes the same one."""
    from .goals import reachable_goals
    return reachable_goals(robot, int(request["m"]), seed=int(seed) + 1, integrator=ENV_INTEGRATOR, device=device), float(request["prob"])


# ---- the checkpoint (PPO.save / PPO.load, visualize_agent) ----
def tendon_obs_record(env):
    """a checkpoint's record of the observation's tendon channels and their scales; none for an env without the option (or None)"""
    channels = tuple(getattr(env, "tendon_obs", ()) or ())
    scale = [float(x) for x in getattr(env, "tendon_obs_scale", (1.0, 1.0, 1.0, 1.0))] if channels else [1.0] * 4
    return {"channels": list(channels), "scale": scale}


def env_io_record(env):
    """a checkpoint's record of sensor_noise, action_delay and action_obs (K n_t more columns of the row): visualize_agent reads them back"""
    delay = getattr(env, "action_delay", None)
    out = {"sensor_noise": {k: float(v) for k, v in dict(getattr(env, "sensor_noise", None) or {}).items()},
           "action_delay": list(delay) if isinstance(delay, tuple) else delay}
    if getattr(env, "action_obs", 0):          # (an env without the option records what it always recorded)
        out["action_obs"] = int(env.action_obs)
    return out


def env_checkpoint_record(env, critic=None) -> dict:
    """The env's keys of a checkpoint; an env without an option (any env that is no RoboyVecEnv) writes what it always wrote.  ``critic``:
    whether the agent's value net reads the env's critic rows (PPO's asymmetric_critic; None: whether the env writes any)."""
    import torch                               # (a checkpoint holds tensors; torch comes in here, never with this module)
    ck = {"tendon_obs": tendon_obs_record(env), "env_io": env_io_record(env)}
    names = list(getattr(env, "critic_obs_names", ()) or ())
    if bool(names) if critic is None else critic:
        ck["critic_obs"] = names
    if getattr(env, "goal_pool_size", 0):
        ck["goals"] = {"q": torch.from_numpy(env.goal_pool()), "recipe": dict(getattr(env, "goal_recipe", {}) or {})}
    if (curriculum := getattr(env, "goal_curriculum", None)) is not None:
        level = env.goal_levels()
        ck["goal_curriculum"] = {"levels": curriculum["levels"], "up": curriculum["up"], "down": curriculum["down"],
                                 "level": (level if torch.is_tensor(level) else torch.from_numpy(level.astype("int64"))).cpu()}
    if getattr(env, "goal_row_stats_enabled", False):
        counts = env.goal_row_stats()          # per row of ck["goals"]["q"], which is the pool in its current order
        ck["goal_row_stats"] = {k: torch.from_numpy(counts[k].astype("int64")) for k in ("attempts", "reached")}
    if (shaping := getattr(env, "reward_shaping", None)) is not None:
        ck["reward_shaping"] = {k: float(v) for k, v in shaping.items()}
    if (push := getattr(env, "push", None)) is not None:
        ck["env_push"] = {"prob": float(push["prob"]), "sigma": [float(v) for v in push["sigma"]], "threshold": int(push["threshold"])}
    if (capacity := getattr(env, "episode_log_capacity", 0)):
        ck["episode_log"] = int(capacity)
    if getattr(env, "start_poses_size", 0):
        ck["env_start_poses"] = {"q": torch.from_numpy(env.start_pose_pool()), "prob": float(env.start_prob),
                                 "threshold": int(round(float(env.start_prob) * 2 ** 24)), "recipe": dict(getattr(env, "start_recipe", {}) or {})}
    return ck


def check_env_checkpoint(env, ck, critic_dim=None) -> dict:
    """``load()``'s env side.  ``ValueError`` where the checkpoint's rows are not this env's (tendon channels; with ``critic_dim``, the width an
    asymmetric agent reads, the critic rows); a warning where the reward-shaping weights differ (the env's hold); the curriculum's levels go into
    an env with as many levels and envs.  Returns what the env does not take over: ``{"goals", "goal_row_stats", "goal_curriculum", "env_push"}`` and, where the
    checkpoint has it, ``"env_start_poses"`` (a condition of the run like the pushes).  ``episode_log`` (the
    capacity of the run that wrote the checkpoint) is a condition of that run, never a layout: it must be a capacity (``ValueError`` otherwise), is
    neither taken over nor kept, and this env's own capacity holds, whatever it is."""
    old, own = ck.get("tendon_obs", tendon_obs_record(None)), tendon_obs_record(env)
    if old != own:
        raise ValueError("the checkpoint was trained on the observation %r, this env gives %r (RoboyVecEnv's tendon_obs / tendon_obs_scale)" % (old, own))
    names = list(getattr(env, "critic_obs_names", ()) or ())
    if critic_dim is not None and "critic_obs" in ck and (ck["critic_obs"] != names or int(ck["critic_obs_dim"]) != critic_dim):
        raise ValueError("the checkpoint's critic was trained on the rows %r (%d columns), this env writes %r (%d; RoboyVecEnv's "
                         "critic_obs)" % (ck["critic_obs"], int(ck["critic_obs_dim"]), names, critic_dim))
    if ck.get("reward_shaping") != getattr(env, "reward_shaping", None):
        import warnings
        warnings.warn("the checkpoint was trained with reward_shaping=%r, this env runs reward_shaping=%r"
                      % (ck.get("reward_shaping"), getattr(env, "reward_shaping", None)))
    if "episode_log" in ck:
        episode_log_capacity(ck["episode_log"])
    kept = {k: ck.get(k) for k in ("goals", "goal_row_stats", "goal_curriculum", "env_push")}
    if "env_start_poses" in ck:                  # (absent when off: a checkpoint without the option returns exactly what it did)
        kept["env_start_poses"] = ck["env_start_poses"]
    saved, own = kept["goal_curriculum"], getattr(env, "goal_curriculum", None)
    if saved is not None and own is not None and own["levels"] == int(saved["levels"]) and int(saved["level"].numel()) == env.num_envs:
        env.set_goal_levels(saved["level"].cpu().numpy())
        kept["goal_curriculum"] = None
    return kept


# ---- the env's state (RoboyVecEnv.state_dict / load_state_dict) ----
ENV_STATE_VERSION = 1
ENV_STATE_IDENTITY = ("n_envs", "n_q", "n_t", "seed", "env_id_offset", "integrator", "n_substeps", "step_size")
ENV_STATE_KEYS = ("version", "identity", "segments", "blob", "host", "env", "slabs", "markers")
ENV_STATE_SLABS = ("act", "obs", "rew", "done")
_STATE_ITEM_BYTES = {"float32": 4, "uint32": 4, "float64": 8, "uint64": 8}


def check_env_state_dict(sd) -> None:
    """``ValueError`` where ``sd`` is no ``RoboyVecEnv.state_dict()``: not a dict, a key missing, another version, a segment table
    that is no list of ``(name, dtype, rows, cols, offset)``, or a blob that is no ``uint8`` array as long as the table says.  Looks
    at ``sd`` alone: no env, no library."""
    if not isinstance(sd, dict):
        raise ValueError("load_state_dict: a dict from RoboyVecEnv.state_dict(), got %s" % type(sd).__name__)
    for key in ENV_STATE_KEYS:
        if key not in sd:
            raise ValueError("load_state_dict: the dict has no %r (not a RoboyVecEnv.state_dict())" % key)
    if sd["version"] != ENV_STATE_VERSION:
        raise ValueError("load_state_dict: state version %r, this package reads version %d" % (sd["version"], ENV_STATE_VERSION))
    end = 0
    for seg in sd["segments"]:
        if not (isinstance(seg, (tuple, list)) and len(seg) == 5 and isinstance(seg[0], str) and seg[1] in _STATE_ITEM_BYTES
                and all(isinstance(v, (int, np.integer)) and v >= 0 for v in seg[2:])):
            raise ValueError("load_state_dict: %r is no segment (name, dtype, rows, cols, offset)" % (seg,))
        if seg[4] % 16 or seg[4] < end:
            raise ValueError("load_state_dict: segment %r lies at offset %d, behind a table that ends at %d" % (seg[0], seg[4], end))
        end = seg[4] + _STATE_ITEM_BYTES[seg[1]] * seg[2] * seg[3]
    blob = sd["blob"]
    if not isinstance(blob, np.ndarray) or blob.dtype != np.uint8 or blob.ndim != 1:
        raise ValueError("load_state_dict: the blob must be a one-dimensional uint8 numpy array")
    if blob.nbytes != (end + 15) // 16 * 16:
        raise ValueError("load_state_dict: the blob has %d bytes, its segment table describes %d" % (blob.nbytes, (end + 15) // 16 * 16))
    for name in ENV_STATE_SLABS:
        if not isinstance(sd["slabs"].get(name), np.ndarray):
            raise ValueError("load_state_dict: the dict has no %r slab" % name)
    if "env_steps" not in sd["host"]:
        raise ValueError("load_state_dict: the host record has no env_steps")


def compare_env_state(identity, segments, sd) -> None:
    """Is ``sd`` (a ``state_dict()``) the state of an env like this one - ``identity`` (``{field: value}`` over ``ENV_STATE_IDENTITY``)
    and ``segments`` (``HipBatchSimulation.state_segments()``)?  ``ValueError`` naming the FIRST identity field, then the first segment
    that differs: one this env has and the dict lacks (or the other way round), another dtype, another shape, another place in the
    blob.  A pure function of its arguments: nothing is copied before it has passed."""
    theirs = sd["identity"]
    for field in ENV_STATE_IDENTITY:
        if field not in theirs:
            raise ValueError("load_state_dict: the state's identity has no %r" % field)
        if theirs[field] != identity[field]:
            raise ValueError("load_state_dict: the state was taken from an env with %s = %r, this env has %s = %r"
                             % (field, theirs[field], field, identity[field]))
    own, other = [tuple(s) for s in segments], [tuple(s) for s in sd["segments"]]
    own_names, other_names = [s[0] for s in own], [s[0] for s in other]
    for k in range(max(len(own), len(other))):
        a, b = own[k] if k < len(own) else None, other[k] if k < len(other) else None
        if a == b:
            continue
        if a is None or (b is not None and a[0] != b[0] and b[0] not in own_names):
            raise ValueError("load_state_dict: the state has the segment %r, this env has none (an option it does not run)" % b[0])
        if b is None or a[0] != b[0]:
            if a[0] not in other_names:
                raise ValueError("load_state_dict: this env has the segment %r, the state has none (an option the saved env did not run)" % a[0])
            raise ValueError("load_state_dict: segment %r stands at another place in the state's table (%r there)" % (a[0], b[0]))
        if a[1] != b[1]:
            raise ValueError("load_state_dict: segment %r is %s in the state, %s in this env" % (a[0], b[1], a[1]))
        if a[2:4] != b[2:4]:
            raise ValueError("load_state_dict: segment %r has shape [%d][%d] in the state, [%d][%d] in this env" % (a[0], b[2], b[3], a[2], a[3]))
        raise ValueError("load_state_dict: segment %r lies at offset %d in the state, %d in this env" % (a[0], b[4], a[4]))


def env_state_views(segments, blob) -> dict:
    """``{name: array [rows, cols]}``: every segment as a numpy VIEW of the blob (no copy)"""
    return {name: blob[offset:offset + _STATE_ITEM_BYTES[dtype] * rows * cols].view(dtype).reshape(rows, cols)
            for name, dtype, rows, cols, offset in segments}


def env_kwargs_from_checkpoint(ck):
    """A checkpoint -> ``(kwargs, needs_vec_env)``: the arguments of a one-env ``RoboyVecEnv`` that gives the policy's row under the conditions it
    was trained under, and whether playback needs one - ``RoboyEnv`` takes ``kwargs["goals"]`` and has no channels, noise, delay, action rows, pushes."""
    channels = ck.get("tendon_obs", {}).get("channels", [])
    env_io, goals, push, delay = ck.get("env_io", {}), ck.get("goals"), ck.get("env_push"), ck.get("env_io", {}).get("action_delay")
    kw = dict(tendon_obs=channels or None, tendon_obs_scale=dict(zip(TENDON_OBS_CHANNELS, ck["tendon_obs"]["scale"])) if channels else None,
              sensor_noise=env_io.get("sensor_noise") or None, action_delay=tuple(delay) if isinstance(delay, list) else delay,
              action_obs=int(env_io.get("action_obs") or 0) or None,
              goals=None if goals is None else np.asarray(goals["q"], dtype=np.float32),      # the stored rows; the recipe is not needed
              push=None if push is None else {"prob": push["prob"], "sigma": push["sigma"]})  # (the threshold follows from prob)
    if (start := ck.get("env_start_poses")) is not None:      # (absent when off)
        kw["start_poses"], kw["start_prob"] = np.asarray(start["q"], dtype=np.float32), float(start["prob"])
    # not replayed, each on purpose - critic_obs: only the actor is played back, and no critic row is needed
    # goal_curriculum: playback draws from the whole pool, the top level's draw
    # goal_row_stats: counts of the training run, nothing a step reads
    # reward_shaping: shapes the reward the trainer saw; playback prints the task's reward
    # episode_log: a condition of the run that wrote the checkpoint, no layout; whoever evaluates asks for the capacity it needs
    return kw, any(kw[k] for k in ("tendon_obs", "sensor_noise", "action_delay", "action_obs", "push"))
