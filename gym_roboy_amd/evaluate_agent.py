"""Evaluate a trained agent on a fresh batch of environments and print per-episode figures.

``python -m gym_roboy_amd.evaluate_agent model.pkl [--envs N --episodes E --seed S --max-episode-length L --json out.json] [env flags]``:
the checkpoint's deterministic policy (the action mean) runs on ``N`` envs until every one of them has finished exactly ``E``
episodes (``ppo.evaluate_policy`` over the env's episode log), so short episodes are not over-represented as they are in
totals over whatever ended.  The env is built under the conditions the checkpoint records (``envs.options.env_kwargs_from_checkpoint``);
every env flag given on the command line (``envs.options.ENV_FLAGS``) REPLACES the checkpoint's condition: pushes, sensor noise, an
action delay, the goal pool, the start poses may change - that is what "evaluated under pushes it was not trained with" takes - while the row's
layout (``--tendon-obs``, ``--action-obs``) may not: the policy reads the columns it was trained on.  One line with the summary is printed;
``--json`` also writes it, with the conditions used, to a file.  Where ``visualize_agent`` plays one env at 30 ms per step, this plays
thousands at a few microseconds per step."""
import argparse
import json

from .envs.options import ENV_FLAGS, add_env_arguments, env_kwargs_from_args, env_kwargs_from_checkpoint, parse_goals

# the keyword arguments of RoboyVecEnv an env flag decides (env_kwargs_from_args' keys), per flag; a flag that is given replaces them
FLAG_KEYS = {"--tendon-obs": ("tendon_obs",), "--tendon-obs-scale": ("tendon_obs_scale",), "--sensor-noise": ("sensor_noise",),
             "--action-delay": ("action_delay",), "--action-obs": ("action_obs",), "--critic-obs": ("critic_obs",), "--goals": ("goals",),
             "--goal-levels": ("goal_curriculum",), "--goal-up": ("goal_curriculum",), "--goal-down": ("goal_curriculum",),
             "--goal-order": ("goal_row_stats",), "--goal-reorder-every": ("goal_row_stats",), "--reward-shaping": ("reward_shaping",),
             "--push": ("push",), "--episode-log": (), "--start-poses": ("start_poses", "start_prob"),
             "--start-prob": ("start_poses", "start_prob")}
LAYOUT_FLAGS = ("--tendon-obs", "--action-obs")      # they change the observation row's width


def parser():
    ap = argparse.ArgumentParser(description="evaluate a checkpoint's deterministic policy for exactly E episodes of each of N envs")
    ap.add_argument("model", help="model.pkl written by gym_roboy_amd.train_parallel")
    ap.add_argument("--envs", type=int, default=4096, metavar="N", help="environments (default 4096)")
    ap.add_argument("--episodes", type=int, default=1, metavar="E", help="episodes per env, at most 64 (default 1)")
    ap.add_argument("--seed", type=int, default=1, help="the env batch's seed (default 1; training's default is 0)")
    ap.add_argument("--max-episode-length", type=int, default=400, metavar="L", help="the time limit in steps (default 400, the trainer's)")
    ap.add_argument("--json", default=None, metavar="FILE", help="also write the summary and the conditions used to FILE")
    ap.add_argument("--device", type=int, default=0, help="the GPU (default 0)")
    add_env_arguments(ap)
    add_env_arguments(ap, late=True)
    return ap


def given_flags(argv):
    """the env flags that stand on the command line (``--push x`` or ``--push=x``), in ENV_FLAGS' order"""
    words = [w.split("=", 1)[0] for w in argv if w.startswith("--")]
    return [row[0] for row in ENV_FLAGS if row[0] in words]


def env_conditions(ck, args, argv):
    """``(kwargs, given)``: RoboyVecEnv's keyword arguments for the evaluation - the checkpoint's conditions, each replaced where its
    flag stands on the command line (``goals``: True where ``--goals`` asks for a pool that still has to be made, ``start_poses``: the
    request ``{"m", "prob"}`` where ``--start-poses`` does; the episode log is
    the evaluation's own: ``--episodes``) - and the env flags that were given."""
    args.bootstrap_timeouts = False              # (the trainer's flag: evaluation needs no truncation codes)
    given = given_flags(argv)
    from_args = env_kwargs_from_args(args)
    kw = env_kwargs_from_checkpoint(ck)[0]
    kw.update(seed=args.seed, integrator=from_args["integrator"], max_episode_length=args.max_episode_length, episode_log=args.episodes)
    for flag in given:
        for key in FLAG_KEYS[flag]:
            if key == "goals":
                kw["goals"] = True if parse_goals(args.goals) else None
            elif key in from_args:
                kw[key] = from_args[key]
            else:
                kw.pop(key, None)
    if kw.get("goal_curriculum") is not None and kw.get("goals") is None:
        raise SystemExit("--goal-levels needs a goal pool: the checkpoint has none, give --goals")
    kw.pop("critic_obs", None)                   # only the actor is evaluated, and no critic row is needed
    return kw, given


def printable(kw):
    """the conditions as JSON takes them: arrays become their shape"""
    return {k: ({"rows": list(v.shape)} if hasattr(v, "shape") else list(v) if isinstance(v, tuple) else v) for k, v in sorted(kw.items())}


def main(argv=None):
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parser().parse_args(argv)
    if not 1 <= args.episodes <= 64 or args.envs < 1 or args.max_episode_length < 1:
        raise SystemExit("--episodes takes 1..64, --envs and --max-episode-length take >= 1")

    import torch
    from .envs.robots import MsjRobot
    from .envs.vec_env import RoboyVecEnv
    from .ppo import FusedPolicyStep, MlpPolicy, ObsNorm, _fused_kernels_apply, evaluate_policy

    ck = torch.load(args.model, map_location="cpu")
    kw, given = env_conditions(ck, args, argv)
    if kw.get("goals") is True:                  # --goals reachable[:M]: a pool made for this evaluation, as the trainer makes its own
        from .envs.goals import reachable_goals
        kw["goals"] = reachable_goals(MsjRobot(), parse_goals(args.goals), seed=args.seed, integrator=kw["integrator"], device=args.device)
        if kw.get("goal_curriculum") is not None:
            kw["goals"] = kw["goals"].ordered()
    if isinstance(kw.get("start_poses"), dict):      # --start-poses reachable[:M]: a pool made for this evaluation (the seed + 1: not the goal pool)
        from .envs.options import start_pose_pool
        pool, kw["start_prob"] = start_pose_pool(MsjRobot(), kw["start_poses"], args.seed, device=args.device)
        kw["start_poses"] = pool.q
    torch.cuda.set_device(args.device)
    env = RoboyVecEnv(MsjRobot(), args.envs, device=args.device, **kw)
    try:
        n_obs, n_act = env.observation_space.shape[0], env.action_space.shape[0]
        trained_on = ck["policy"]["pi.0.weight"].shape[1]
        if trained_on != n_obs:
            layout = [f for f in given if f in LAYOUT_FLAGS]
            raise SystemExit("%s holds a policy over %d observation columns, this env gives %d: %s" % (
                args.model, trained_on, n_obs, "drop %s (the row's layout is the checkpoint's)" % " and ".join(layout) if layout
                else "it was not written by this train_parallel"))
        device = torch.device("cuda", args.device)
        policy = MlpPolicy(n_obs, n_act, critic_obs_dim=ck.get("critic_obs_dim"))
        policy.load_state_dict(ck["policy"])
        policy.to(device)
        norm = cnorm = None
        if ck.get("obs_norm") is not None:       # trained with PPO's normalize_obs: the policy reads the observation through them
            norm = ObsNorm(n_obs, device)
            norm.load_state_dict(ck["obs_norm"])
            if ck.get("critic_obs_norm") is not None:
                cnorm = ObsNorm(int(ck["critic_obs_dim"]), device)
                cnorm.load_state_dict(ck["critic_obs_norm"])
            policy.set_obs_norm(norm, cnorm)
        fused = FusedPolicyStep(policy) if _fused_kernels_apply(policy, n_obs, n_act) else None
        summary = evaluate_policy(policy, env, args.episodes, fused=fused, obs_norm=norm, cobs_norm=cnorm, device=device)
    finally:
        env.close()
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"summary": summary, "conditions": printable(kw), "flags": given, "model": args.model, "envs": args.envs,
                       "episodes": args.episodes, "timesteps": int(ck.get("num_timesteps", 0))}, f, indent=1)
    return summary


if __name__ == "__main__":
    main()
