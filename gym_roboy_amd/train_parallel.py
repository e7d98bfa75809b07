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

TRAINING_STEPS_BETWEEN_BACKUPS = 100000


def log_line(stats):
    """An update's statistics as they are printed: four decimals, and three significant digits for the small ones (the approximate KL
    and the learning rate of --lr-schedule, which four decimals would print as 0.0003 or 0)."""
    return {k: float("%.3g" % v) if k in ("approx_kl", "lr", "symmetry_loss") else round(v, 4) for k, v in stats.items()}


DEFAULT_GOAL_POOL = 16384
ENV_INTEGRATOR = "euler"                         # RoboyVecEnv's default: the pool is settled with the integrator the env steps with


def parse_goals(text):
    """``--goals``: "" -> 0 (box goals), "reachable" -> 16384, "reachable:M" -> M"""
    if not text:
        return 0
    kind, _, m = text.partition(":")
    if kind != "reachable" or (m and (not m.isdigit() or int(m) < 1)):
        raise SystemExit("--goals takes reachable or reachable:M with M >= 1, got %r" % text)
    return int(m) if m else DEFAULT_GOAL_POOL


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


GOAL_ORDERS = ("rest_distance", "reach_rate")


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
    ap.add_argument("--tendon-obs", default="", metavar="CHANNELS",
                    help="comma-separated tendon channels appended to the observation, out of length,rate,activation,force "
                         "(e.g. length,force: 25 columns for MsjRobot); stored in the checkpoint")
    ap.add_argument("--tendon-obs-scale", default="", metavar="CHANNEL=FACTOR,...",
                    help="factor per channel, default 1 (m, m/s, [0,1], N), e.g. force=0.0025,length=4")
    ap.add_argument("--sensor-noise", default="", metavar="KEY=SIGMA,...",
                    help="Gaussian noise on the observation: standard deviations in physical units for q, qd and the selected tendon "
                         "channels, e.g. q=0.01,qd=0.05,force=2; stored in the checkpoint")
    ap.add_argument("--action-delay", default="", metavar="D | LO:HI",
                    help="steps by which every action acts late (at most 7): one number, or a range each env draws from at every "
                         "episode start, e.g. 0:3; stored in the checkpoint")
    ap.add_argument("--action-obs", type=int, default=0, metavar="K",
                    help="append the last K commanded actions (at most 8, newest first, zeros where the episode is younger) to the "
                         "observation: what the policy needs to compensate --action-delay; stored in the checkpoint")
    ap.add_argument("--critic-obs", default="", metavar="BLOCK,...",
                    help="an asymmetric critic: the value net is trained on privileged rows the env writes beside the observation - state "
                         "(exact q, qd, goal; always part of the row), age, params, delay (needs --action-delay), actions (needs "
                         "--action-obs), e.g. state,age,delay,actions; only the actor is deployed; recorded in the checkpoint")
    ap.add_argument("--goals", default="", metavar="reachable[:M]",
                    help="draw every goal from a pool of M poses (default 16384) the robot holds under constant set-points, made once "
                         "at start with the run's seed and integrator (envs.goals.reachable_goals; every rank makes the same pool) "
                         "instead of uniformly in the goal box; rows and recipe are stored in the checkpoint")
    ap.add_argument("--goal-levels", type=int, default=0, metavar="L",
                    help="a goal curriculum over the pool ordered by distance from the rest pose (needs --goals): every env starts at "
                         "level 0 of L, draws its goals from the nearest (level + 1) / L of the pool, and moves with its episodes' "
                         "outcomes; levels are stored in the checkpoint")
    ap.add_argument("--goal-up", type=int, default=None, metavar="U", help="levels up after an episode that reached its goal (default 1)")
    ap.add_argument("--goal-down", type=int, default=None, metavar="D", help="levels down after an episode that did not (default 1)")
    ap.add_argument("--goal-order", default="rest_distance", metavar="KEY",
                    help="what the curriculum takes for difficulty: rest_distance (default: the pool stays ordered by distance from "
                         "the rest pose) or reach_rate (needs --goal-levels: the run starts from that order, counts per pool row how "
                         "many episodes aimed at it and how many reached it, and re-orders the live pool by the measured rate, summed "
                         "over the ranks, after every R-th round; the counts are stored in the checkpoint)")
    ap.add_argument("--goal-reorder-every", type=int, default=1, metavar="R", help="rounds between re-orderings (default 1)")
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
    ap.add_argument("--reward-shaping", default="", metavar="TERM=WEIGHT,...",
                    help="regularising reward terms, subtracted from the step's reward on the device: action_rate (mean squared change "
                         "of the clamped action within an episode), tension (mean squared tendon force over its maximum), activation "
                         "(mean squared muscle activation), e.g. action_rate=0.05,tension=0.01; the round's statistics then show "
                         "shaping_cost_per_step, while return and goals reached stay the task's; recorded in the checkpoint")
    ap.add_argument("--push", default="", metavar="prob=P,sigma=S",
                    help="random velocity pushes, an external disturbance on the device: in front of every env step each env is pushed "
                         "with probability P, a pushed env's joint velocities get S * z added (z standard normal, S in rad/s) and are "
                         "clamped to the robot's bounds, e.g. prob=0.02,sigma=0.5; the round's statistics then show pushes_per_step; "
                         "recorded in the checkpoint")
    args = ap.parse_args(argv)
    sensor_noise = {k: float(v) for k, v in (item.split("=", 1) for item in args.sensor_noise.split(",") if item)}
    action_delay = None
    if args.action_delay:
        parts = [int(x) for x in args.action_delay.split(":")]
        action_delay = parts[0] if len(parts) == 1 else (parts[0], parts[1])
    tendon_obs = tuple(c for c in args.tendon_obs.split(",") if c)
    critic_obs = tuple(c for c in args.critic_obs.split(",") if c)
    tendon_obs_scale = {k: float(v) for k, v in (item.split("=", 1) for item in args.tendon_obs_scale.split(",") if item)}
    goals_m = parse_goals(args.goals)
    goal_curriculum = parse_goal_curriculum(args.goal_levels, args.goal_up, args.goal_down, goals_m)
    by_reach_rate = parse_goal_order(args.goal_order, args.goal_reorder_every, goal_curriculum)
    from .envs.vec_env import parse_reward_shaping
    reward_shaping = parse_reward_shaping(args.reward_shaping)
    from .envs.vec_env import parse_push
    push = parse_push(args.push)

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
    env = RoboyVecEnv(MsjRobot(), args.num_envs, seed=args.seed, device=local_rank, integrator=ENV_INTEGRATOR, goals=goals,
                      env_id_offset=rank * args.num_envs, tendon_obs=tendon_obs or None, tendon_obs_scale=tendon_obs_scale or None,
                      sensor_noise=sensor_noise or None, action_delay=action_delay,
                      report_truncation=args.bootstrap_timeouts, action_obs=args.action_obs or None,
                      critic_obs=critic_obs or None, goal_curriculum=goal_curriculum, **({"goal_row_stats": True} if by_reach_rate else {}),
                      **({"reward_shaping": reward_shaping} if reward_shaping else {}), **({"push": push} if push else {}))
    more_exploration = 0.1                      # train_parallel.py:30
    agent = PPO(env, n_steps=args.n_steps, ent_coef=more_exploration, device="cuda", dist=dist, seed=args.seed,
                reward_scale=0.01, use_graphs=not args.no_graphs, fused_policy=not args.torch_policy,
                fused_update=not args.torch_policy, normalize_obs=args.normalize_obs, clip_obs=args.clip_obs,
                normalize_reward=args.normalize_reward, clip_reward=args.clip_reward,
                bootstrap_timeouts=args.bootstrap_timeouts, lr_schedule=args.lr_schedule, desired_kl=args.desired_kl,
                lr_min=args.lr_min, lr_max=args.lr_max, asymmetric_critic=bool(critic_obs),
                symmetry=args.symmetry, symmetry_coef=args.symmetry_coef)
    if os.path.exists(model_file):
        agent.load(model_file)                  # resume from the last backup
    last_stats = {}
    push_steps_seen = 0.0                       # (--push: the env steps counted up to the last round's end)
    for round_no in range(args.rounds):
        agent.learn(total_timesteps=args.steps_per_round,
                    log=(lambda s: (last_stats.update(s), print(log_line(s)))) if rank == 0 else None)
        # episode statistics of ALL ranks' envs: the 8-double block of every rank, summed (RCCL; gloo: through the host)
        from .sharding import STAT_KEYS, allreduce_stats, summarize
        local = env.stats()
        block = torch.tensor([local[k] for k in STAT_KEYS], dtype=torch.float64,
                             device="cuda" if (dist is not None and args.backend == "nccl") else "cpu")
        if goal_curriculum is not None:         # the envs per level ride along: [8 statistics | L counts]
            hist = env.goal_level_histogram()
            hist = hist if torch.is_tensor(hist) else torch.from_numpy(hist)
            block = torch.cat((block, hist.to(block)))
        n_head = block.numel()
        if by_reach_rate:                       # the counts per row ride along as well: [... | m attempts | m reached], exact below 2^53
            counts = env.goal_row_stats()
            rows = torch.from_numpy(np.concatenate((counts["attempts"], counts["reached"])).astype(np.float64))
            block = torch.cat((block, rows.to(block)))
        i_push = block.numel()
        if env.push is not None:                # the round's pushes ride along: [... | pushes | env steps of the round]
            steps_now = float(local["n_env_steps"])
            block = torch.cat((block, torch.tensor([env.push_count(reset=True), steps_now - push_steps_seen], dtype=torch.float64).to(block)))
            push_steps_seen = steps_now
        if env.reward_shaping is not None:      # the round's shaping costs ride along at the end: [... | sum of step costs | steps]
            cost = env.shaping_stats(reset=True)
            block = torch.cat((block, torch.tensor([cost["sum_step_cost"], cost["n_steps"]], dtype=torch.float64).to(block)))
        allreduce_stats(block, dist)
        row_counts = None
        if by_reach_rate:
            row_counts = block[n_head:n_head + 2 * goals_m].cpu().numpy().astype(np.uint64).reshape(2, goals_m)
            if (round_no + 1) % args.goal_reorder_every == 0:      # every rank orders by the same sums: all ranks keep the same pool
                env.reorder_goals_by_reach_rate(attempts=row_counts[0], reached=row_counts[1])
        if rank == 0:
            agent.save(model_file)
            summary = summarize(block[:len(STAT_KEYS)].cpu())
            if goal_curriculum is not None:
                summary.update(level_summary(block[len(STAT_KEYS):n_head].cpu()))
            if row_counts is not None:          # (by the order the round ran with: the first level's rows as they were)
                summary.update(reach_rate_summary(row_counts[0], row_counts[1], goals_m // goal_curriculum["levels"]))
            if args.symmetry and agent.last_rollout is not None:      # (rank 0's policy on rank 0's last rollout: the policy is shared)
                summary["symmetry_gap_action"] = float("%.3g" % agent.symmetry_gap(agent.last_rollout)["action"])
                if "symmetry_loss" in last_stats:                     # (symmetry="loss": the term of the round's last minibatch)
                    summary["symmetry_loss"] = float("%.3g" % last_stats["symmetry_loss"])
            if env.push is not None:
                summary["pushes_per_step"] = float("%.4g" % (float(block[i_push]) / max(float(block[i_push + 1]), 1.0)))
            if env.reward_shaping is not None:
                summary["shaping_cost_per_step"] = float("%.4g" % (float(block[-2]) / max(float(block[-1]), 1.0)))
            print("episode statistics (all ranks):", summary)
    if world > 1:
        dist.destroy_process_group()
    return agent


if __name__ == "__main__":
    main()
