#!/usr/bin/env python3
"""Time the rollout's tail as one launch (rp_rollout_tail_dev) against the tail it replaces - the scale copy, the done
conversion and rp_gae_dev as PPO._rollout_tail issues them - each captured in a HIP graph as the rollout captures them, replayed in
one process, alternating, with HIP events on torch's stream after warm-up.

    python tools/rollout_tail_bench.py [--reps 10] [--rounds 7] [--iteration]

Variants per shape (262 144 x 128 and 4 096 x 128): the parent's tail TWICE (two graphs over buffers of their own: what separates them
is the run-to-run spread the new launch is judged against), the one launch with identity statistics (null pointers) and with real
ones (an rstd, a clamp, a shift), and the bootstrapping instance (rp_rollout_tail_boot_dev; half of the dones truncated)
with identity statistics - what PPO(bootstrap_timeouts=True) runs without normalize_reward - and with real ones.  One JSON line per shape: per variant the median, the smallest and the largest of the rounds'
microseconds per replay, and the bytes per second of the nine array passes each variant makes (read rew_raw and done_i twice, val
once; write rew, done, adv, ret) against the chip's 8 TB/s.  --iteration adds a whole PPO iteration (rollout + update) at 262 144 envs with
the option off and on, timed as tools/policy_bench.py times it."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12
GAMMA, LAM, SCALE = 0.99, 0.95, 0.01


def _time(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def alternate(fns, reps, rounds):
    for f in fns:
        for _ in range(3):
            f()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            times[k].append(_time(f, reps))
    return times


def captured(fn):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                                   # first use outside the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    return g.replay


def tail_shapes(args):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import gae_fused
    lib = pn.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for N, T in ((262144, 128), (4096, 128)):
        g = torch.Generator(device="cuda").manual_seed(N)
        rew_raw = torch.randn(T, N, device="cuda", generator=g) * 2.0 - 1.0
        done_i = (torch.rand(T, N, device="cuda", generator=g) < 0.01).to(torch.int32)
        val, last = torch.randn(T, N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)

        def parent():
            b = {k: torch.empty(T, N, device="cuda") for k in ("rew", "done", "adv", "ret")}

            def run():                                         # PPO._rollout_tail's statements
                b["rew"].copy_(rew_raw * SCALE)
                b["done"].copy_(done_i.to(torch.float32))
                gae_fused(b["rew"], val, b["done"], last, GAMMA, LAM, b["adv"], b["ret"])
            return captured(run)

        code_i = torch.where((done_i != 0) & (torch.rand(T, N, device="cuda", generator=g) < 0.5), 2, done_i).to(torch.int32)

        def fused(norm2, shift, clip, boot=False):
            b = {k: torch.empty(T, N, device="cuda") for k in ("rew", "done", "adv", "ret")}
            carry, sums = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
            scratch = torch.zeros(int(lib.rp_rollout_tail_scratch_doubles()), dtype=torch.float64, device="cuda")

            def run():
                fn = lib.rp_rollout_tail_boot_dev if boot else lib.rp_rollout_tail_dev
                pn.check(fn(ptr(rew_raw), ptr(code_i if boot else done_i), ptr(val), ptr(last), SCALE, ptr(norm2), clip, ptr(shift), GAMMA,
                            LAM, ptr(carry), ptr(b["rew"]), ptr(b["done"]), ptr(b["adv"]), ptr(b["ret"]), ptr(sums),
                            ptr(scratch), T, N, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return captured(run)

        norm2 = torch.tensor([[-0.4], [2.5]], device="cuda")
        shift = torch.tensor([-0.4], dtype=torch.float64, device="cuda")
        names = ["parent_a", "parent_b", "one_launch_identity", "one_launch_statistics", "boot_identity", "boot_statistics"]
        fns = [parent(), parent(), fused(None, None, float("inf")), fused(norm2, shift, 0.05), fused(None, None, float("inf"), True),
               fused(norm2, shift, 0.05, True)]
        times = alternate(fns, args.reps, args.rounds)
        passes = {name: 9 * T * N * 4 for name in names}
        out = {"what": "rollout tail", "shape": "%d x %d" % (N, T), "blocks": int(lib.rp_rollout_tail_blocks(T, N))}
        for name, t in zip(names, times):
            med = float(np.median(t))
            out[name] = {"median_us": round(med, 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
                         "TB_per_s": round(passes[name] / med / 1e6, 3), "of_hbm_peak": round(passes[name] / med / 1e6 / (HBM_PEAK / 1e12), 3)}
        pa, pb = out["parent_a"]["median_us"], out["parent_b"]["median_us"]
        out["parent_spread_us"] = round(max(max(times[0]), max(times[1])) - min(min(times[0]), min(times[1])), 2)
        out["one_launch_over_parent"] = round(out["one_launch_statistics"]["median_us"] / (0.5 * (pa + pb)), 4)
        out["boot_identity_over_parent"] = round(out["boot_identity"]["median_us"] / (0.5 * (pa + pb)), 4)
        out["boot_over_one_launch"] = round(out["boot_statistics"]["median_us"] / out["one_launch_statistics"]["median_us"], 4)
        print(json.dumps(out), flush=True)
        del fns


def iteration(args):
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    n = 262144
    for on in (False, True, False, True):
        env = RoboyVecEnv(MsjRobot(), n)
        agent = PPO(env, ent_coef=0.1, device="cuda", reward_scale=SCALE, use_graphs=True, fused_policy=True, fused_update=True,
                    normalize_reward=on)
        roll = agent.collect(); agent.update(roll); torch.cuda.synchronize()
        tc, tu = [], []
        for _ in range(3):
            t0 = time.perf_counter(); roll = agent.collect(); torch.cuda.synchronize(); t1 = time.perf_counter()
            agent.update(roll); torch.cuda.synchronize(); t2 = time.perf_counter()
            tc.append(t1 - t0); tu.append(t2 - t1)
        print(json.dumps({"what": "PPO iteration", "envs": n, "normalize_reward": on, "rollout_ms": [round(1e3 * t, 2) for t in tc],
                          "update_ms": [round(1e3 * t, 2) for t in tu]}), flush=True)
        env.close()
        del agent, env, roll
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iteration", action="store_true", help="also time a whole PPO iteration at 262 144 envs, option off and on")
    args = ap.parse_args()
    tail_shapes(args)
    if args.iteration:
        iteration(args)


if __name__ == "__main__":
    main()
