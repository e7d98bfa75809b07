#!/usr/bin/env python3
"""What the episode log costs per env step (rb_env_episode_log_configure).

    python tools/episode_log_bench.py --parent PARENT_TREE [--rounds 3] [--repeats 7] [--steps 100] [--out profiles/episode_log/bench.log]

Three variants, each in a process of its own that measures MsjRobot at 4 096 and 262 144 envs and the upper body at 8 192 and 65 536,
each with long episodes (max_episode_length 400: few episode ends per step, the lanes read and write two words) and with
max_episode_length 4 (a quarter of the lanes writes a record per step):
    parent    a built checkout of the parent commit (its package and its libroboy_sim.so), no option
    off       this tree, no option: launches what the parent launches (tools/compare_code_objects.py: every pre-existing kernel is
              identical)
    log       episode_log=32: one more launch per env step
Per (variant, robot, batch, length) `steps` env steps are captured in a HIP graph as a PPO rollout captures them; the figure is the
median over `repeats` replays between HIP events after two warm-up replays.  In front of every replay, outside the timed span, the log
is cleared, so that records are written through the whole replay (100 steps of 4-step episodes: 25 records per env, below the
capacity).  The variants run `rounds` times, in an order rotated by one per round.  One JSON line per (round, variant, robot, batch,
length), then one summary line per (robot, batch, length): per variant the median over the rounds with the smallest and largest
round, what the log costs over `off` and over `parent`, and `off`'s own spread between rounds beside them."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (("msj", 4096), ("msj", 262144), ("upper", 8192), ("upper", 65536))
LENGTHS = (400, 4)
VARIANTS = ("parent", "off", "log")
CAPACITY = 32


def child(args):
    sys.path.insert(0, args.tree)
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robots = {"msj": MsjRobot, "upper": UpperBodyRobot}
    K = args.steps
    for which, n in SIZES:
        for length in LENGTHS:
            kw = {"episode_log": CAPACITY} if args.log else {}
            env = RoboyVecEnv(robots[which](), n, seed=0, max_episode_length=length, **kw)
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
            us, records = [], 0.0
            for rep in range(2 + args.repeats):
                if args.log:
                    env.clear_episode_log()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                g.replay()
                stop.record()
                stop.synchronize()
                if rep >= 2:
                    us.append(1e3 * start.elapsed_time(stop) / K)
                    if args.log:
                        records = env.episode_log_summary()["n_records"]
            line = {"variant": args.label, "robot": which, "n_envs": n, "max_episode_length": length, "steps_per_repeat": K,
                    "us_per_step": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}
            if args.log:
                line["records_per_env_step"] = round(records / (float(n) * K), 5)
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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "episode_log", "bench.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="off", help=argparse.SUPPRESS)
    ap.add_argument("--log", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent:
        ap.error("--parent PARENT_TREE is needed")
    setup = {"parent": (os.path.abspath(args.parent), 0), "off": (HERE, 0), "log": (HERE, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines, rows = [], []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    for r in range(args.rounds):
        for v in VARIANTS[r % len(VARIANTS):] + VARIANTS[:r % len(VARIANTS)]:
            tree, log = setup[v]
            env = dict(os.environ)
            env.pop("ROBOY_SIM_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", v, "--log", str(log),
                   "--repeats", str(args.repeats), "--steps", str(args.steps)]
            out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=600).stdout
            for text in out.splitlines():
                if text.startswith("{"):
                    rec = dict(json.loads(text), round=r)
                    rows.append(rec)
                    emit(rec)
    for which, n in SIZES:
        for length in LENGTHS:
            per = {v: [x["us_per_step"] for x in rows if x["variant"] == v and x["robot"] == which and x["n_envs"] == n
                       and x["max_episode_length"] == length] for v in VARIANTS}
            med = {v: statistics.median(per[v]) for v in VARIANTS}
            emit({"summary": "%s:%d:len%d" % (which, n, length),
                  **{v: {"median": round(med[v], 3), "min": round(min(per[v]), 3), "max": round(max(per[v]), 3)} for v in VARIANTS},
                  "off_spread_between_rounds": round(max(per["off"]) - min(per["off"]), 3),
                  "off_minus_parent": round(med["off"] - med["parent"], 3),
                  "log_over_off": round(med["log"] - med["off"], 3), "log_over_parent": round(med["log"] - med["parent"], 3)})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
