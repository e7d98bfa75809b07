#!/usr/bin/env python3
"""What the outcome counts per pool row cost per env step (rb_env_goal_row_stats_enable), against the parent commit and
against this build with the counts off, with the same pool and curriculum: reachable_goals(MsjRobot(), 16384, seed=0).ordered(), 8
levels, max_episode_length = 1 - every env ends its episode in every step and, timing out, sits at level 0, so every lane of every
step adds into the first m / L = 2 048 rows: the shape at which the accumulation is busiest.

    python tools/goal_stats_bench.py --parent PARENT_TREE [--alt-lib LIB] [--rounds 3] [--repeats 7] [--steps 400] [--episode-length 1]

--episode-length E gives the other end: the envs, in lock-step, end together every E-th step and hardly otherwise.

PARENT_TREE: a built checkout of the parent commit (its package and its library are used as they are).  --alt-lib: another build of
this tree's libroboy_sim.so with another accumulation form (loaded through ROBOY_SIM_LIB).  Every variant - parent / counts off /
counts on (/ counts on, alt) - runs in a process of its own, in that order within each round; inside it, at 4 096 and at 262 144 envs,
`steps` env steps are captured in a HIP graph as a PPO rollout captures them and the graph is replayed `repeats` times between HIP
events after warm-up.  One JSON line per (round, variant, size): the median, smallest and largest microseconds per env step, the
envs that were done in the last step and the level histogram; then one summary line per size: the parent's spread between rounds,
whether counts-off lies inside it, and the microseconds per step each counting form costs over counts-off."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 262144)


def child(args):
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    from gym_roboy_amd.envs.goals import reachable_goals
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    pool = reachable_goals(MsjRobot(), 16384, seed=0).ordered()
    K = args.steps
    for n in SIZES:
        env = RoboyVecEnv(MsjRobot(), n, seed=0, max_episode_length=args.episode_length, goals=pool, goal_curriculum=8,
                          **({"goal_row_stats": True} if args.counts else {}))
        env.reset()
        act = torch.rand(n, env.n_t, device="cuda") * 2.0 - 1.0
        obs, rew = torch.empty(n, env.obs_dim, device="cuda"), torch.empty(n, device="cuda")
        done = torch.zeros(n, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        env.set_stream(side.cuda_stream)
        env.sim.specialization()

        def run():
            for _ in range(K):
                env.step_dev(act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr())
        with torch.cuda.stream(side):
            run()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        env.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            g.replay()
            stop.record()
            stop.synchronize()
            us.append(1e3 * start.elapsed_time(stop) / K)
        line = {"build": args.label, "counts": bool(args.counts), "n_envs": n, "steps_per_repeat": K, "episode_length": args.episode_length,
                "us_per_step_median": round(float(np.median(us)), 3), "min": round(min(us), 3), "max": round(max(us), 3),
                "dones_last_step": int((done != 0).sum().item()), "levels": [int(x) for x in env.goal_level_histogram().tolist()]}
        if args.counts:
            counts = env.goal_row_stats()
            line["attempts"] = int(counts["attempts"].sum())
            line["rows_attempted"] = int((counts["attempts"] != 0).sum())
        print(json.dumps(line), flush=True)
        env.close()
        del g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--alt-lib", action="append", default=[], metavar="LIB",
                    help="a libroboy_sim.so of this tree with another accumulation form; may be given several times")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--episode-length", type=int, default=1, help="the envs' time limit (default 1: every step ends every episode)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="repo", help=argparse.SUPPRESS)
    ap.add_argument("--counts", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent:
        ap.error("--parent PARENT_TREE is needed")
    variants = [("parent", os.path.abspath(args.parent), 0, ""), ("repo", HERE, 0, ""), ("repo", HERE, 1, "")]
    for lib in args.alt_lib:                    # labelled by file name: lib_plain.so -> "lib_plain"
        variants.append((os.path.splitext(os.path.basename(lib))[0], HERE, 1, os.path.abspath(lib)))
    rows = []
    for _ in range(args.rounds):
        for label, tree, counts, lib in variants:
            env = dict(os.environ)
            env.pop("ROBOY_SIM_LIB", None)
            if lib:
                env["ROBOY_SIM_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", label, "--counts", str(counts),
                   "--repeats", str(args.repeats), "--steps", str(args.steps), "--episode-length", str(args.episode_length)]
            out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=600).stdout
            for text in out.splitlines():
                if text.startswith("{"):
                    print(text, flush=True)
                    rows.append(json.loads(text))
    for n in SIZES:
        def med(label, counts):
            return [r["us_per_step_median"] for r in rows if r["build"] == label and r["counts"] == bool(counts) and r["n_envs"] == n]
        parent, off = med("parent", 0), med("repo", 0)
        mid = sorted(off)[len(off) // 2]
        summary = {"summary": n, "parent_us": parent, "counts_off_us": off,
                   "counts_off_median_inside_parent_spread": min(parent) <= mid <= max(parent),
                   "counts_off_median_minus_parent_median_us": round(mid - sorted(parent)[len(parent) // 2], 3),
                   "counts_on_cost_us": {"repo": round(sorted(med("repo", 1))[args.rounds // 2] - mid, 3)}}
        for label, _, _, lib in variants[3:]:
            summary["counts_on_cost_us"][label] = round(sorted(med(label, 1))[args.rounds // 2] - mid, 3)
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
