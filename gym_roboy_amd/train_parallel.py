"""Training driver: PPO over a GPU-resident batch of RoboyEnvs.

Counterpart of ``/root/reference/gym_roboy/train_parallel.py`` (same CLI:
``python -m gym_roboy_amd.train_parallel <num_envs> [results_dir]``): where the
reference builds ``num_cpu`` ROS-backed envs in ``num_cpu`` processes (:19-29),
this builds one ``RoboyVecEnv`` of ``num_envs`` envs per GPU; like the
reference it trains in rounds of 100 000 timesteps and saves ``model.pkl``
after each (:16,33-35; the reference loops forever, here ``--rounds`` bounds it).
Launch with ``python -m torch.distributed.run --nproc-per-node N ...`` for N
GPUs: env shards by ``env_id_offset``; every rank replays its own captured
rollout graph (policy step, env step, GAE are rank-local), the gradient
vector is averaged over RCCL once per minibatch and the episode statistics are
summed over the ranks (``sharding.allreduce_stats``) before rank 0 prints them.
"""
import argparse
import os

from .envs.options import (DEFAULT_GOAL_POOL, ENV_INTEGRATOR, GOAL_ORDERS, add_env_arguments, env_kwargs_from_args,  # noqa: F401
                           parse_goal_curriculum, parse_goal_order, parse_goals)

TRAINING_STEPS_BETWEEN_BACKUPS = 100000
EVAL_SEED_OFFSET = 7919                         # --eval-every: the evaluation env's seed is the run's plus this


def log_line(stats):
    """An update's statistics as they are printed: four decimals, and three significant digits for the small ones (the approximate KL
    and the learning rate of --lr-schedule, which four decimals would print as 0.0003 or 0)."""
    return {k: float("%.3g" % v) if k in ("approx_kl", "lr", "symmetry_loss") else round(v, 4) for k, v in stats.items()}


def reach_rate_summary(attempts, reached, first_level_rows):
    """the summed row counts as they are logged: the share of the episodes that reached their goal among those aimed at the first
    level's rows, and at any row (0 where nothing was attempted)"""
    a, r = [int(x) for x in attempts], [int(x) for x in reached]
    k = int(first_level_rows)
    return {"reach_rate_first_level": sum(r[:k]) / max(sum(a[:k]), 1), "reach_rate_whole_pool": sum(r) / max(sum(a), 1)}


def level_summary(hist):
    """the level histogram (summed over the ranks) as it is logged: the mean level and the share of envs at the top level"""
    h = [float(x) for x in hist]
    n = max(sum(h), 1.0)
    return {"mean_level": sum(l * c for l, c in enumerate(h)) / n, "top_level_share": h[-1] / n}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("num_envs", type=int, help="environments per GPU (the reference's num_cpu)")
    ap.add_argument("results_dir", nargs="?", default="./training_results")
    ap.add_argument("--rounds", type=int, default=1, help="rounds of 100 000 timesteps (reference: unbounded)")
    ap.add_argument("--steps-per-round", type=int, default=TRAINING_STEPS_BETWEEN_BACKUPS)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-graphs", action="store_true",
                    help="launch every kernel from Python instead of replaying HIP graphs")
    ap.add_argument("--n-steps", type=int, default=128, help="rollout length per update (stable_baselines' default)")
    ap.add_argument("--backend", default=os.environ.get("ROBOY_TRAIN_BACKEND", "nccl"), choices=("nccl", "gloo"),
                    help="nccl = RCCL over xGMI, one rank per GPU; gloo = rehearsal with the ranks sharing the visible GPUs")
    ap.add_argument("--torch-policy", action="store_true",
                    help="policy step and minibatch gradient through torch (autograd, rocBLAS) instead of the fused "
                         "matrix-core kernels of include/roboy_policy.h")
    add_env_arguments(ap)
    ap.add_argument("--normalize-obs", action="store_true",
                    help="running mean / variance normalisation of the observation inside the policy kernels (what "
                         "stable-baselines calls VecNormalize); the statistics are stored in the checkpoint")
    ap.add_argument("--clip-obs", type=float, default=10.0, metavar="X", help="clamp of the normalised observation (default 10)")
    ap.add_argument("--normalize-reward", action="store_true",
                    help="divide the (scaled) reward by the running standard deviation of the discounted return (what "
                         "stable-baselines calls VecNormalize(norm_reward=True)); the statistics are stored in the checkpoint")
    ap.add_argument("--clip-reward", type=float, default=10.0, metavar="X", help="clamp of the normalised reward (default 10)")
    ap.add_argument("--bootstrap-timeouts", action="store_true",
                    help="episodes that end at the time limit bootstrap the value of their last observation in GAE instead of "
                         "ending the return there (the env then reports truncation); recorded in the checkpoint")
    ap.add_argument("--lr-schedule", default=None, choices=("adaptive",),
                    help="adaptive = move the learning rate by the update's approximate KL, minibatch by minibatch (cut above twice "
                         "--desired-kl, raised below half of it); the log line then shows approx_kl, clip_frac and lr; stored in the "
                         "checkpoint")
    ap.add_argument("--desired-kl", type=float, default=0.01, metavar="KL", help="the KL the adaptive schedule steers to (default 0.01)")
    ap.add_argument("--lr-min", type=float, default=1e-5, metavar="LR", help="lower bound of the scheduled learning rate (default 1e-5)")
    ap.add_argument("--lr-max", type=float, default=1e-2, metavar="LR", help="upper bound of the scheduled learning rate (default 1e-2)")
    ap.add_argument("--symmetry", default=None, choices=("augment", "loss"),
                    help="augment = every update runs on the rollout's samples and their images in the robot's mirror plane (twice the "
                         "samples per env step, no more simulation; not with --critic-obs); loss = every minibatch's loss gains "
                         "--symmetry-coef x the mean squared distance of the action mean from the symmetry (the action net only: works "
                         "with --critic-obs); the round's statistics then show symmetry_gap_action, the policy's distance from the "
                         "symmetry, and with loss symmetry_loss, the last minibatch's term; recorded in the checkpoint")
    ap.add_argument("--symmetry-coef", type=float, default=1.0, metavar="C",
                    help="the weight of --symmetry loss's term (>= 0, default 1)")
    add_env_arguments(ap, late=True)
    ap.add_argument("--eval-every", type=int, default=0, metavar="R",
                    help="after every R-th round the deterministic policy is evaluated on a second env batch under the training conditions "
                         "(another seed; exactly --eval-episodes episodes of each of --eval-envs envs per rank, PPO.evaluate); the round's "
                         "statistics then show eval_success_rate, eval_mean_return and eval_mean_length; 0 (default): no second env")
    ap.add_argument("--eval-envs", type=int, default=4096, metavar="N", help="evaluation envs per rank (default 4096)")
    ap.add_argument("--eval-episodes", type=int, default=1, metavar="E", help="episodes per evaluation env, at most 64 (default 1)")
    ap.add_argument("--exact-resume", action="store_true",
                    help="every backup also carries what continues the run: each rank writes resume.rank<R>.pt beside model.pkl - its env "
                         "shard's state, its agent's carries and its evaluation env's state - and a start that finds model.pkl and these files "
                         "continues where the backup was taken instead of restarting the envs (the same ranks and batch sizes); the count of "
                         "completed rounds travels too, so --eval-every and --goal-reorder-every keep their cadence; files are written under a "
                         "temporary name and renamed, so a stop in the middle of a backup leaves the previous one")
    args = ap.parse_args(argv)
    env_kw = env_kwargs_from_args(args)         # (bad values: before torch is imported or a GPU is touched)
    if args.eval_every < 0 or (args.eval_every and (args.eval_envs < 1 or not 1 <= args.eval_episodes <= 64)):
        raise SystemExit("--eval-every takes R >= 0, --eval-envs N >= 1 and --eval-episodes 1..64")
    goals_m, goal_curriculum, by_reach_rate = parse_goals(args.goals), env_kw["goal_curriculum"], "goal_row_stats" in env_kw

    import numpy as np
    import torch
    from .envs.robots import MsjRobot
    from .envs.vec_env import RoboyVecEnv
    from .ppo import PPO

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if args.backend == "gloo":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")
    results = os.path.abspath(args.results_dir)
    model_file = os.path.join(results, "model.pkl")
    if rank == 0:
        os.makedirs(results, exist_ok=True)

    goals = None
    if goals_m:
        from .envs.goals import reachable_goals
        goals = reachable_goals(MsjRobot(), goals_m, seed=args.seed, integrator=ENV_INTEGRATOR, device=local_rank)
        if goal_curriculum is not None:
            goals = goals.ordered()
        if rank == 0:
            print("goal pool:", goals.recipe)
    if "start_poses" in env_kw:                 # the request becomes the pool: the run's seed + 1, so it is not the goal pool
        from .envs.options import start_pose_pool
        env_kw["start_poses"], env_kw["start_prob"] = start_pose_pool(MsjRobot(), env_kw["start_poses"], args.seed, device=local_rank)
        if rank == 0:
            print("start poses:", env_kw["start_poses"].recipe, "start_prob", env_kw["start_prob"])
    env = RoboyVecEnv(MsjRobot(), args.num_envs, goals=goals, device=local_rank, env_id_offset=rank * args.num_envs, **env_kw)
    more_exploration = 0.1                      # train_parallel.py:30
    agent = PPO(env, n_steps=args.n_steps, ent_coef=more_exploration, device="cuda", dist=dist, seed=args.seed,
                reward_scale=0.01, use_graphs=not args.no_graphs, fused_policy=not args.torch_policy,
                fused_update=not args.torch_policy, normalize_obs=args.normalize_obs, clip_obs=args.clip_obs,
                normalize_reward=args.normalize_reward, clip_reward=args.clip_reward,
                bootstrap_timeouts=args.bootstrap_timeouts, lr_schedule=args.lr_schedule, desired_kl=args.desired_kl,
                lr_min=args.lr_min, lr_max=args.lr_max, asymmetric_critic=bool(env_kw["critic_obs"]),
                symmetry=args.symmetry, symmetry_coef=args.symmetry_coef)
    eval_env = None
    if args.eval_every:
        # the training conditions on a batch of its own: a seed apart from training's, this rank's shard of the evaluation's global env
        # ids, and a log of exactly the episodes asked for (the training env's own --episode-log, if any, stays the training env's)
        eval_env = RoboyVecEnv(MsjRobot(), args.eval_envs, goals=goals, device=local_rank, env_id_offset=rank * args.eval_envs,
                               **dict(env_kw, seed=args.seed + EVAL_SEED_OFFSET, episode_log=args.eval_episodes, goal_row_stats=False))
    resume_file = os.path.join(results, "resume.rank%d.pt" % rank)
    push_steps_seen = 0.0                       # (--push: the env steps counted up to the last round's end)
    rounds_done = 0                             # (--exact-resume: the rounds completed before this start - what the cadences count from)
    if os.path.exists(model_file):
        agent.load(model_file, resume=False)    # resume from the last backup
        if args.exact_resume and os.path.exists(resume_file):
            # ... exactly: this rank's envs, carries and evaluation env as the backup left them (PPO.resume_record)
            own = torch.load(resume_file, map_location="cpu")
            if int(own["num_timesteps"]) != int(agent.num_timesteps) and os.path.exists(resume_file + ".prev"):
                # the run was stopped between this file and model.pkl: the backup before it is whole
                own = torch.load(resume_file + ".prev", map_location="cpu")
            if (int(own["num_timesteps"]), int(own["world"])) != (int(agent.num_timesteps), world):
                raise SystemExit("%s was written at %d timesteps by %d ranks, model.pkl holds %d and this run has %d: not one backup"
                                 % (resume_file, own["num_timesteps"], own["world"], agent.num_timesteps, world))
            agent.load_resume_record(own["resume"])
            if eval_env is not None and own["eval_env"] is not None:
                from .ppo import unpack_arrays
                eval_env.load_state_dict(unpack_arrays(own["eval_env"]))
            push_steps_seen = float(env.stats()["n_env_steps"])
            rounds_done = int(own["rounds_done"])
        elif args.exact_resume:
            print("rank %d: %s is missing beside model.pkl - the policy is loaded, the envs start over" % (rank, resume_file))
    last_stats = {}
    for round_no in range(rounds_done, rounds_done + args.rounds):
        agent.learn(total_timesteps=args.steps_per_round,
                    log=(lambda s: (last_stats.update(s), print(log_line(s)))) if rank == 0 else None)
        # episode statistics of ALL ranks' envs, summed (RCCL; gloo: through the host): the env's 8 doubles, then a named segment per option
        from .sharding import STAT_KEYS, allreduce_stats, join_segments, split_segments, summarize
        local = env.stats()
        segments = [("statistics", [local[k] for k in STAT_KEYS])]
        if goal_curriculum is not None:         # the envs per level: L counts
            segments.append(("levels", env.goal_level_histogram()))
        if by_reach_rate:                       # the counts per row: m attempts, m reached, exact below 2^53
            counts = env.goal_row_stats()
            segments.append(("row_counts", np.concatenate((counts["attempts"], counts["reached"])).astype(np.float64)))
        if env.push is not None:                # the round's pushes and its env steps
            steps_now = float(local["n_env_steps"])
            segments.append(("pushes", [env.push_count(reset=True), steps_now - push_steps_seen]))
            push_steps_seen = steps_now
        if env.reward_shaping is not None:      # the round's sum of step costs and its steps
            cost = env.shaping_stats(reset=True)
            segments.append(("shaping", [cost["sum_step_cost"], cost["n_steps"]]))
        if env.start_poses_size:                # the envs whose running episode began at a pool row, and the envs
            index = env.start_index()           # (a CUDA view reads the rest pose as -1, numpy as 0xFFFFFFFF)
            index = (index.cpu().numpy() if torch.is_tensor(index) else index).astype(np.uint32)
            segments.append(("start_poses", [float(np.count_nonzero(index != 0xFFFFFFFF)), float(env.num_envs)]))
        if eval_env is not None and (round_no + 1) % args.eval_every == 0:      # the evaluation's eight sums (every rank evaluates its shard)
            from .envs.options import EPISODE_LOG_SUMS
            figures = agent.evaluate(eval_env, episodes_per_env=args.eval_episodes)
            segments.append(("eval", [figures[k] for k in EPISODE_LOG_SUMS] + [0.0]))
        block, layout = join_segments(segments, "cuda" if (dist is not None and args.backend == "nccl") else "cpu")
        total = split_segments(allreduce_stats(block, dist).cpu(), layout)
        row_counts = total["row_counts"].numpy().astype(np.uint64).reshape(2, goals_m) if by_reach_rate else None
        if by_reach_rate and (round_no + 1) % args.goal_reorder_every == 0:      # every rank orders by the same sums: all ranks keep the same pool
            env.reorder_goals_by_reach_rate(attempts=row_counts[0], reached=row_counts[1])
        if args.exact_resume:                    # every rank: its own shard (before model.pkl, which names the backup they belong to)
            from .ppo import pack_arrays
            os.makedirs(results, exist_ok=True)
            torch.save({"resume": agent.resume_record(), "eval_env": None if eval_env is None else pack_arrays(eval_env.state_dict()),
                        "num_timesteps": int(agent.num_timesteps), "world": world, "rank": rank, "rounds_done": round_no + 1},
                       resume_file + ".tmp")
            if os.path.exists(resume_file):                    # (kept until the next backup: model.pkl is replaced last, and a stop
                os.replace(resume_file, resume_file + ".prev")  # between the two leaves model.pkl with the file it belongs to)
            os.replace(resume_file + ".tmp", resume_file)
            if world > 1:
                dist.barrier()
        if rank == 0 and args.exact_resume:
            agent.save(model_file + ".tmp")
            os.replace(model_file + ".tmp", model_file)
        elif rank == 0:
            agent.save(model_file)
        if rank == 0:
            summary = summarize(total["statistics"])
            if goal_curriculum is not None:
                summary.update(level_summary(total["levels"]))
            if row_counts is not None:          # (by the order the round ran with: the first level's rows as they were)
                summary.update(reach_rate_summary(row_counts[0], row_counts[1], goals_m // goal_curriculum["levels"]))
            if args.symmetry and agent.last_rollout is not None:      # (rank 0's policy on rank 0's last rollout: the policy is shared)
                summary["symmetry_gap_action"] = float("%.3g" % agent.symmetry_gap(agent.last_rollout)["action"])
                if "symmetry_loss" in last_stats:                     # (symmetry="loss": the term of the round's last minibatch)
                    summary["symmetry_loss"] = float("%.3g" % last_stats["symmetry_loss"])
            for name, key in (("pushes", "pushes_per_step"), ("shaping", "shaping_cost_per_step")):
                if name in total:                # (a sum of the round over its env steps)
                    summary[key] = float("%.4g" % (float(total[name][0]) / max(float(total[name][1]), 1.0)))
            if "start_poses" in total:           # (a share of the envs as they stand at the round's end)
                summary["start_pool_share"] = float("%.4g" % (float(total["start_poses"][0]) / max(float(total["start_poses"][1]), 1.0)))
            if "eval" in total:                  # (exactly --eval-episodes episodes of every evaluation env of every rank)
                from .envs.options import episode_log_figures
                figures = episode_log_figures([float(x) for x in total["eval"]], args.eval_envs * world)
                summary.update({"eval_" + k: float("%.6g" % figures[k]) for k in ("success_rate", "mean_return", "mean_length")})
            print("episode statistics (all ranks):", summary)
    if world > 1:
        dist.destroy_process_group()
    return agent


if __name__ == "__main__":
    main()
