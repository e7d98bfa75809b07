#!/usr/bin/env python3
"""What the asymmetric critic costs, each item against a handle or agent without the option - which launches exactly
the kernels of a build without the feature (tools/compare_code_objects.py: every pre-existing function identical) - taken twice, so
that the spread between two identical variants is visible next to the difference.  One process, the variants replayed alternately
from captured graphs, HIP events on torch's stream after warm-up, medians of the rounds (tools/rollout_tail_bench.py: alternate).

    python tools/critic_obs_bench.py [--steps 32] [--reps 10] [--rounds 9] [--iter-rounds 5]

At 4 096 and at 262 144 envs, one JSON line each:
  * the critic row per env step (Euler): Dc = 10 (state, age) on a plain env, and the full row (Dc = 47: state, age, params, delay,
    K = 2 action blocks) on an env with randomization, a delay range and action_obs=2 - rows written through the caller's pointer;
  * the asymmetric policy step (rp_act_asym_dev, Da = 25, Dc = 47) against rp_act_dev at Da = 25;
  * a full PPO iteration (collect + update, two-chain graphs where PPO picks them, host clock around a device synchronise) with and
    without asymmetric_critic on the env with every option."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rollout_tail_bench import alternate  # noqa: E402

FULL = ("state", "age", "params", "delay", "actions")


def _env(n, options, critic_obs):
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    kw = {}
    if options:
        kw = dict(randomization=ParamRanges(force_scale=(0.8, 1.2), mass_scale=(0.8, 1.25)), sensor_noise={"q": 0.01, "qd": 0.05},
                  action_delay=(0, 3), action_obs=2)
    return RoboyVecEnv(MsjRobot(), n, max_episode_length=400, critic_obs=critic_obs, **kw)


def _med(times, per):
    return [float(np.median(t)) / per for t in times]


def row_cost(n, options, names, K, reps, rounds):
    import torch
    envs, fns, keep = [], [], []
    for critic in (None, names, None):                      # the plain handle twice: what separates the two is the spread
        env = _env(n, options, critic)
        env.reset()
        act = torch.rand(K, n, env.n_t, device="cuda") * 2.0 - 1.0
        obs, rew = torch.empty(n, env.obs_dim, device="cuda"), torch.empty(n, device="cuda")
        done = torch.zeros(n, dtype=torch.int32, device="cuda")
        cobs = torch.empty(n, env.critic_obs_dim, device="cuda") if critic else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        env.set_stream(side.cuda_stream)
        env.sim.specialization()

        def run(env=env, act=act, obs=obs, rew=rew, done=done, cobs=cobs):
            for t in range(K):
                env.step_dev(act[t].data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None if cobs is None else cobs.data_ptr())
        with torch.cuda.stream(side):
            run()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        env.set_stream(torch.cuda.current_stream().cuda_stream)
        envs.append(env); fns.append(g.replay); keep.append((act, obs, rew, done, cobs, g))
    times = alternate(fns, reps, rounds)
    med = _med(times, K)
    print(json.dumps({"what": "critic row per env step, graph replay", "envs": n, "steps_per_graph": K, "Dc": envs[1].critic_obs_dim,
                      "obs_dim": envs[1].obs_dim, "form": envs[0].sim.dispatch("env_step")["id"] if not options else "extension kernels",
                      "plain_a_us": round(med[0], 3), "with_rows_us": round(med[1], 3), "plain_b_us": round(med[2], 3),
                      "rows_cost_us": round(med[1] - 0.5 * (med[0] + med[2]), 3),
                      "row_bytes_per_step": 4 * n * envs[1].critic_obs_dim,
                      "min_max_us": [[round(min(t) / K, 3), round(max(t) / K, 3)] for t in times]}), flush=True)
    for env in envs:
        env.close()


def step_cost(n, da, dc, act_dim, K, reps, rounds):
    import torch
    from gym_roboy_amd.ppo import FusedPolicyStep, MlpPolicy
    from rollout_tail_bench import captured
    torch.manual_seed(0)
    obs, cobs = torch.randn(n, da, device="cuda"), torch.randn(n, dc, device="cuda")
    fns, keep = [], []
    for asym in (False, True, False):
        f = FusedPolicyStep(MlpPolicy(da, act_dim, critic_obs_dim=dc if asym else None).cuda(), seed=1)
        a, lp, v = torch.empty(n, act_dim, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        packed = f.pack()

        def run(f=f, a=a, lp=lp, v=v, packed=packed, asym=asym):
            for t in range(K):
                f.act_into(obs, a, lp, v, step=t, packed=packed, cobs=cobs if asym else None)
        fns.append(captured(run)); keep.append((f, a, lp, v, packed))
    times = alternate(fns, reps, rounds)
    med = _med(times, K)
    print(json.dumps({"what": "policy step, graph replay", "samples": n, "Da": da, "Dc": dc, "act_dim": act_dim, "steps_per_graph": K,
                      "rp_act_dev_a_us": round(med[0], 3), "rp_act_asym_dev_us": round(med[1], 3), "rp_act_dev_b_us": round(med[2], 3),
                      "asym_cost_us": round(med[1] - 0.5 * (med[0] + med[2]), 3),
                      "min_max_us": [[round(min(t) / K, 3), round(max(t) / K, 3)] for t in times]}), flush=True)


def iteration_cost(n, n_steps, rounds):
    import torch
    from gym_roboy_amd.ppo import PPO
    envs, agents = [], []
    for asym in (False, True, False):
        env = _env(n, True, FULL if asym else None)         # (the symmetric agents' env writes no rows: the launches of a build without the feature)
        agent = PPO(env, n_steps=n_steps, noptepochs=4, use_graphs=True, seed=3, reward_scale=0.01, asymmetric_critic=asym)
        agent.update(agent.collect())                       # capture, first launches
        agent.update(agent.collect())
        envs.append(env); agents.append(agent)
    times = [[] for _ in agents]
    for _ in range(rounds):
        for k, agent in enumerate(agents):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            roll = agent.collect()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            agent.update(roll)
            torch.cuda.synchronize()
            times[k].append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
    med = [[float(np.median([x[j] for x in t])) for j in (0, 1)] for t in times]
    print(json.dumps({"what": "PPO iteration (collect, update), ms", "envs": n, "n_steps": n_steps, "chains": [a.rollout_chains for a in agents],
                      "obs_dim": envs[1].obs_dim, "Dc": envs[1].critic_obs_dim,
                      "symmetric_a_ms": [round(x, 3) for x in med[0]], "asymmetric_ms": [round(x, 3) for x in med[1]],
                      "symmetric_b_ms": [round(x, 3) for x in med[2]],
                      "cost_ms": [round(med[1][j] - 0.5 * (med[0][j] + med[2][j]), 3) for j in (0, 1)],
                      "min_max_total_ms": [[round(min(sum(x) for x in t), 3), round(max(sum(x) for x in t), 3)] for t in times]}), flush=True)
    for env in envs:
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iter-rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=32, help="rollout length of the PPO iteration")
    ap.add_argument("--envs", type=int, nargs="*", default=[4096, 262144])
    args = ap.parse_args()
    import torch
    for n in args.envs:
        row_cost(n, False, ("state", "age"), args.steps, args.reps, args.rounds)
        torch.cuda.empty_cache()
        row_cost(n, True, FULL, args.steps, args.reps, args.rounds)
        torch.cuda.empty_cache()
        step_cost(n, 25, 47, 8, args.steps, args.reps, args.rounds)
        torch.cuda.empty_cache()
        iteration_cost(n, args.n_steps, args.iter_rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
