#!/usr/bin/env python3
"""What reward shaping costs per env step (rb_env_shaping_configure), and what the fused cost kernel saves against the
same cost composed from what existed before it.

    python tools/reward_shaping_bench.py [--rounds 3] [--repeats 7] [--steps 100] [--out profiles/reward_shaping/bench.log]

One process.  Per (robot, batch) - MsjRobot at 4 096 and 262 144 envs, the upper body at 8 192 and 65 536 - four variants, each an env
of its own whose `steps` env steps are captured in a HIP graph as a PPO rollout captures them:
    off       no option: the env step as the parent commit launches it (tools/compare_code_objects.py: every pre-existing kernel is
              identical, and an env without the option launches nothing else)
    rate      reward_shaping={"action_rate": 0.05}
    all       all three terms
    composed  the cost of `all` from rb_tendon_state_dev (RB_SP_ENV: two [N, n_t] arrays written and read back), torch arithmetic and
              a reward update, in front of and behind an env step without the option
In every round the variants run in an order rotated by one; a variant's figure in a round is the median over `repeats` replays
between HIP events after a warm-up replay.  One JSON line per (round, robot, batch, variant), then one summary line per (robot,
batch): per variant the median over the rounds with the smallest and largest round, `off`'s own spread between rounds beside them,
and the microseconds per step each variant costs over `off`."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
VARIANTS = ("off", "rate", "all", "composed")
WEIGHTS = {"action_rate": 0.05, "tension": 0.01, "activation": 0.01}


def build(robot, n, variant, steps):
    """(graph, env): `steps` env steps of the variant, captured"""
    import torch
    from gym_roboy_amd import _native as nat
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    shaping = {"rate": {"action_rate": WEIGHTS["action_rate"]}, "all": WEIGHTS}.get(variant)
    env = RoboyVecEnv(robot, n, seed=0, max_episode_length=50, reward_shaping=shaping)
    env.reset()
    nt = env.n_t
    act = torch.rand(n, nt, device="cuda") * 2.0 - 1.0
    obs, rew = torch.empty(n, env.obs_dim, device="cuda"), torch.empty(n, device="cuda")
    done = torch.zeros(n, dtype=torch.int32, device="cuda")
    if variant == "composed":
        force, activation = torch.empty(n, nt, device="cuda"), torch.empty(n, nt, device="cuda")
        prev, cost = torch.zeros(n, nt, device="cuda"), torch.empty(n, device="cuda")
        fmax = torch.tensor(robot.get_description().f_max, dtype=torch.float32, device="cuda")
        first = torch.ones(n, dtype=torch.bool, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    env.set_stream(side.cuda_stream)
    env.sim.specialization()

    def run():
        for _ in range(steps):
            if variant == "composed":
                env.sim.tendon_state_dev(act.data_ptr(), nat.RB_SP_ENV, 1.0, 0, 0, activation.data_ptr(), force.data_ptr())
                clamped = act.clamp(-1.0, 1.0)
                rate = torch.where(first, torch.zeros_like(cost), ((clamped - prev) ** 2).mean(1))
                torch.add(WEIGHTS["action_rate"] * rate, WEIGHTS["tension"] * ((force / fmax) ** 2).mean(1)
                          + WEIGHTS["activation"] * (activation ** 2).mean(1), out=cost)
                prev.copy_(clamped)
            env.step_dev(act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr())
            if variant == "composed":
                rew.sub_(cost)
                first.copy_(done != 0)
    with torch.cuda.stream(side):
        run()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    return g, env


def measure(g, steps, repeats):
    import torch
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        g.replay()
        t1.record()
        t1.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / steps)
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "reward_shaping", "bench.log"))
    ap.add_argument("--sizes", default="", help="robot:n,... (default msj:4096,msj:262144,upper:8192,upper:65536)")
    args = ap.parse_args()
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    robots = {"msj": MsjRobot, "upper": UpperBodyRobot}
    sizes = [(r, int(n)) for r, n in (item.split(":") for item in (args.sizes or "msj:4096,msj:262144,upper:8192,upper:65536").split(","))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        lines.append(line)
        print(line, flush=True)
    for which, n in sizes:
        built = {v: build(robots[which](), n, v, args.steps) for v in VARIANTS}
        rounds = {v: [] for v in VARIANTS}
        for r in range(args.rounds):
            for v in VARIANTS[r % len(VARIANTS):] + VARIANTS[:r % len(VARIANTS)]:
                med, lo, hi = measure(built[v][0], args.steps, args.repeats)
                rounds[v].append(med)
                emit({"round": r, "robot": which, "n_envs": n, "variant": v, "us_per_step": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)})
        for _, env in built.values():
            env.close()
        off = statistics.median(rounds["off"])
        emit({"summary": "%s:%d" % (which, n),
              **{v: {"median": round(statistics.median(rounds[v]), 3), "min": round(min(rounds[v]), 3), "max": round(max(rounds[v]), 3),
                     "over_off": round(statistics.median(rounds[v]) - off, 3)} for v in VARIANTS},
              "off_spread_between_rounds": round(max(rounds["off"]) - min(rounds["off"]), 3)})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
