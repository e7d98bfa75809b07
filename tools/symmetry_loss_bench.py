#!/usr/bin/env python3
"""What the mirror-symmetry loss costs (PPO(symmetry="loss")).

    python tools/symmetry_loss_bench.py [--kernel] [--ppo] [--rounds 5] [--launches 10] [--iterations 3] [--sizes 131072,8388608]
    python tools/symmetry_loss_bench.py --summarize DIR        # a rocprofv3 --kernel-trace directory of a --kernel run

--kernel: rp_sym_grad_dev on B pairs (its gradient kernel + the small reduction) against rp_ppo_grad_dev on 2 B rows of the same
widths - the action net's kernel on as many columns, the same matrix work, plus the value net's kernel and two reductions, which the
entry point cannot leave out: the per-kernel split is what --summarize prints from a kernel trace of the same run (per kernel name:
dispatches, median, min and max microseconds), and that is where mlp_sym_kernel stands beside mlp_grad_kernel<0, ...>.  Widths
9 / 25 / 33 x 8 actions (small form x 2, general form), B = 131 072 and 8 388 608, indexed as the update addresses them.  HIP events
around `launches` back-to-back calls, `rounds` times per variant, the order rotated from round to round; median and min / max.

--ppo: one PPO iteration (rollout, update) at 4 096 and 262 144 envs x 128 steps in graph mode with the fused kernels for
symmetry=None, "augment" and "loss", the agents taking turns: host clock around work that ends in a device synchronisation, the median
of `iterations`.

One JSON line per measurement."""
import argparse
import ctypes
import glob
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
WIDTHS = ((9, 8), (25, 8), (33, 8))
PPO_SIZES = (4096, 262144)
STEPS = 128


def bench_kernel(args):
    import numpy as np
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad, MlpPolicy
    lib = pn.load()
    for obs_dim, act_dim in WIDTHS:
        torch.manual_seed(obs_dim)
        policy = MlpPolicy(obs_dim, act_dim).cuda()
        with torch.no_grad():
            for p in policy.parameters():
                p.add_(0.3 * torch.randn_like(p))
        fg = FusedPolicyGrad(policy)
        act_src = list(range(act_dim))[::-1]
        for B in args.sizes:
            g = torch.Generator(device="cuda").manual_seed(B % 1000)
            rows = 2 * B
            obs = torch.rand(rows, obs_dim, device="cuda", generator=g) * 4 - 2
            image = torch.rand(B, obs_dim, device="cuda", generator=g) * 4 - 2
            act = torch.randn(rows, act_dim, device="cuda", generator=g)
            adv, logp, val, ret = (torch.randn(rows, device="cuda", generator=g) for _ in range(4))
            logp -= 8.0
            idx_pairs = torch.randperm(B, device="cuda", generator=g)
            idx_rows = torch.randperm(rows, device="cuda", generator=g)
            stats = fg.minibatch_adv_stats(adv, idx_rows).clone()

            def sym():
                fg.sym_run(obs[:B], image, act_src, 1.0, index=idx_pairs, accumulate=True, repack=False)

            def ppo():
                fg.run(obs, act, adv, logp, val, ret, 0.2, 0.5, 0.0, index=idx_rows, adv_stats=stats, entropy_grad=False)
            variants = [("sym_B_pairs", sym), ("ppo_2B_rows", ppo)]
            ppo(); sym()
            torch.cuda.synchronize()
            us = {name: [] for name, _ in variants}
            for r in range(args.rounds):
                for name, fn in variants[r % 2:] + variants[:r % 2]:
                    fn()
                    torch.cuda.synchronize()
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(args.launches):
                        fn()
                    stop.record()
                    stop.synchronize()
                    us[name].append(1e3 * start.elapsed_time(stop) / args.launches)
            line = {"kernel": True, "obs_dim": obs_dim, "act_dim": act_dim, "pairs": B, "form": int(lib.rp_sym_grad_form(obs_dim, act_dim)),
                    "ppo_form": int(lib.rp_grad_form(obs_dim, act_dim)), "prefetch_env": os.environ.get("ROBOY_POLICY_PREFETCH", "")}
            for name in us:
                line[name + "_us"] = round(float(np.median(us[name])), 1)
                line[name + "_us_min_max"] = [round(min(us[name]), 1), round(max(us[name]), 1)]
            line["sym_over_ppo_entry"] = round(line["sym_B_pairs_us"] / line["ppo_2B_rows_us"], 3)
            print(json.dumps(line), flush=True)
            del obs, image, act, adv, logp, val, ret, idx_pairs, idx_rows
            torch.cuda.empty_cache()


def summarize(directory):
    """per (kernel, grid) of a rocprofv3 kernel trace: dispatches and the median / min / max microseconds"""
    import csv
    import re
    import numpy as np
    by = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = re.sub(r"\(anonymous namespace\)::", "", row["Kernel_Name"])
            name = re.sub(r"^void ", "", name)
            name = name.split("(")[0]
            if not re.match(r"mlp_(sym|grad)|reduce_", name):
                continue
            by.setdefault((name, int(row["Grid_Size_X"])), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    for (name, grid), us in sorted(by.items()):
        print(json.dumps({"trace": True, "kernel_name": name, "grid": grid, "dispatches": len(us), "median_us": round(float(np.median(us)), 1),
                          "min_us": round(min(us), 1), "max_us": round(max(us), 1)}), flush=True)


def bench_ppo(args):
    import numpy as np
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    for n_envs in PPO_SIZES:
        agents = []
        for symmetry in (None, "augment", "loss"):
            env = RoboyVecEnv(MsjRobot(), n_envs, seed=0)
            agents.append((symmetry, env, PPO(env, n_steps=STEPS, device="cuda", seed=0, use_graphs=True, reward_scale=0.01,
                                              symmetry=symmetry)))
        ms = {s: {"rollout": [], "update": []} for s, _, _ in agents}
        for it in range(args.iterations + 1):                  # (the first one warms up: graph capture, buffers)
            k = it % len(agents)
            for symmetry, _, agent in agents[k:] + agents[:k]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                roll = agent.collect()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                agent.update(roll)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if it:
                    ms[symmetry]["rollout"].append(1e3 * (t1 - t0)); ms[symmetry]["update"].append(1e3 * (t2 - t1))
        line = {"ppo": True, "n_envs": n_envs, "n_steps": STEPS}
        for s in ms:
            for k in ("rollout", "update"):
                line["%s_%s_ms" % (s or "plain", k)] = round(float(np.median(ms[s][k])), 2)
                line["%s_%s_ms_all" % (s or "plain", k)] = [round(v, 2) for v in ms[s][k]]
        line["augment_update_ratio"] = round(line["augment_update_ms"] / line["plain_update_ms"], 3)
        line["loss_update_ratio"] = round(line["loss_update_ms"] / line["plain_update_ms"], 3)
        print(json.dumps(line), flush=True)
        for _, env, _ in agents:
            env.close()
        del agents, agent, roll
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--ppo", action="store_true")
    ap.add_argument("--summarize", metavar="DIR", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--sizes", default="131072,8388608")
    args = ap.parse_args()
    args.sizes = [int(x) for x in args.sizes.split(",") if x]
    if args.summarize:
        return summarize(args.summarize)
    if not (args.kernel or args.ppo):
        args.kernel = args.ppo = True
    if args.kernel:
        bench_kernel(args)
    if args.ppo:
        bench_ppo(args)


if __name__ == "__main__":
    main()
