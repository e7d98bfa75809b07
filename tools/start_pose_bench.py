#!/usr/bin/env python3
"""What the start poses cost per env step (rb_env_start_poses_configure).

    python tools/start_pose_bench.py --parent PARENT_TREE [--rounds 3] [--repeats 7] [--steps 100] [--out profiles/start_poses/bench.log]

Five variants, each in a process of its own that measures MsjRobot at 4 096 and 262 144 envs and the upper body at 8 192 and 65 536:
    parent      a built checkout of the parent commit (its package and its libroboy_sim.so), no option, episodes of 50 steps
    off_long    this tree, no option, episodes that never end within the measurement (max_episode_length 10^6): launches what the
                parent launches (tools/compare_code_objects.py: every pre-existing kernel is identical)
    off_50      the same with episodes of 50 steps (every env auto-resets twice per 100 captured steps)
    start_long  start_poses = 4 096 rows, start_prob 1, long episodes: the kernel is launched behind every step and every lane leaves
                after its done word
    start_50    the same with episodes of 50 steps: two steps in a hundred every lane draws, reads its row and writes its state
Per (variant, robot, batch) `steps` env steps are captured in a HIP graph as a PPO rollout captures them; the figure is the median
over `repeats` replays between HIP events after two warm-up replays.  The variants run `rounds` times, in an order rotated by one per
round.  One JSON line per (round, variant, robot, batch), then one summary line per (robot, batch): per variant the median over the
rounds with the smallest and largest round, what the option costs over `off` at either episode length, `off`'s own spread between
rounds beside it, and `off_50` against the parent."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (("msj", 4096), ("msj", 262144), ("upper", 8192), ("upper", 65536))
VARIANTS = ("parent", "off_long", "off_50", "start_long", "start_50")
LONG, POOL_ROWS = 1000000, 4096


def child(args):
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robots = {"msj": MsjRobot, "upper": UpperBodyRobot}
    K = args.steps
    for which, n in SIZES:
        robot = robots[which]()
        kw = {}
        if args.start:
            desc = robot.get_description()
            kw = {"start_poses": np.random.default_rng(3).uniform(0.5 * desc.q_lo, 0.5 * desc.q_hi, (POOL_ROWS, desc.n_q)).astype(np.float32),
                  "start_prob": 1.0}
        env = RoboyVecEnv(robot, n, seed=0, max_episode_length=args.episode, **kw)
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
        line = {"variant": args.label, "robot": which, "n_envs": n, "steps_per_repeat": K, "us_per_step": round(statistics.median(us), 3),
                "min": round(min(us), 3), "max": round(max(us), 3)}
        if args.start:
            line["starts_per_env_step"] = round(float(env.start_count().astype(np.float64).sum()) / (float(n) * K * (3 + args.repeats)), 5)
        print(json.dumps(line), flush=True)
        env.close()
        del g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "start_poses", "bench.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="off_50", help=argparse.SUPPRESS)
    ap.add_argument("--start", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--episode", type=int, default=50, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent:
        ap.error("--parent PARENT_TREE is needed")
    setup = {"parent": (os.path.abspath(args.parent), 0, 50), "off_long": (HERE, 0, LONG), "off_50": (HERE, 0, 50),
             "start_long": (HERE, 1, LONG), "start_50": (HERE, 1, 50)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines, rows = [], []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    for r in range(args.rounds):
        for v in VARIANTS[r % len(VARIANTS):] + VARIANTS[:r % len(VARIANTS)]:
            tree, start, episode = setup[v]
            env = dict(os.environ)
            env.pop("ROBOY_SIM_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", v, "--start", str(start),
                   "--episode", str(episode), "--repeats", str(args.repeats), "--steps", str(args.steps)]
            out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=600).stdout
            for text in out.splitlines():
                if text.startswith("{"):
                    rec = dict(json.loads(text), round=r)
                    rows.append(rec)
                    emit(rec)
    for which, n in SIZES:
        per = {v: [x["us_per_step"] for x in rows if x["variant"] == v and x["robot"] == which and x["n_envs"] == n] for v in VARIANTS}
        med = {v: statistics.median(per[v]) for v in VARIANTS}
        emit({"summary": "%s:%d" % (which, n),
              **{v: {"median": round(med[v], 3), "min": round(min(per[v]), 3), "max": round(max(per[v]), 3)} for v in VARIANTS},
              "off_long_spread_between_rounds": round(max(per["off_long"]) - min(per["off_long"]), 3),
              "off_50_spread_between_rounds": round(max(per["off_50"]) - min(per["off_50"]), 3),
              "off_50_minus_parent": round(med["off_50"] - med["parent"], 3),
              "start_long_over_off_long": round(med["start_long"] - med["off_long"], 3),
              "start_50_over_off_50": round(med["start_50"] - med["off_50"], 3)})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
