#!/usr/bin/env python3
"""What the mirror-symmetry augmentation costs (PPO(symmetry="augment")).

    python tools/symmetry_bench.py [--pass] [--ppo] [--rounds 5] [--launches 20] [--iterations 3]

--pass: the streaming pass alone.  rp_mirror_rows_dev (both halves of a [2 rows, width] buffer from a [rows, width] source) against
the torch statement on the same tensors, torch.cat([x, x[:, src] * sign]) - what a build without the kernel would run - at
4 096 x 128 and 262 144 x 128 rows for widths 9 (the bare observation), 25 (length and force channels) and 8 (the action).  HIP events
around `launches` back-to-back calls, `rounds` times per variant with the order of the variants rotated from round to round; the
median microseconds per call and the bytes per second the algorithm needs (read rows x width floats once, write them twice) over it.
The outputs are compared bit for bit first.

--ppo: one PPO iteration (rollout, update) at 4 096 and 262 144 envs x 128 steps in graph mode with the fused kernels, with and without
the option, the two agents taking turns: host clock around work that ends in a device synchronisation, median of `iterations`.

One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SIZES = (4096, 262144)
STEPS = 128


def bench_pass(args):
    import numpy as np
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.envs.symmetry import row_mirror_map
    lib = pn.load()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    image = np.arange(8)[::-1].copy()
    maps = {9: row_mirror_map(3, 8, (-1, 1, -1), image)[:2], 25: row_mirror_map(3, 8, (-1, 1, -1), image, ("length", "force"))[:2],
            8: (image.astype(np.int32), np.ones(8, np.float32))}
    for n_envs in SIZES:
        rows = n_envs * STEPS
        for width, (src, sign) in maps.items():
            x = torch.randn(rows, width, device="cuda")
            out = torch.empty(2 * rows, width, device="cuda")
            src32, src64 = torch.from_numpy(src.astype(np.int32)).cuda(), torch.from_numpy(src.astype(np.int64)).cuda()
            sgn = torch.from_numpy(sign).cuda()

            def kernel():
                pn.check(lib.rp_mirror_rows_dev(ptr(x), ptr(out), ptr(out[rows:]), rows, width, ptr(src32), ptr(sgn), stream()))

            def statement():
                return torch.cat([x, x[:, src64] * sgn])
            kernel()
            want = statement()
            torch.cuda.synchronize()
            same = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            del want
            variants = [("kernel", kernel), ("torch", statement)]
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
            needed = 3 * rows * width * 4                      # bytes the algorithm needs: one read, two writes
            line = {"pass": True, "n_envs": n_envs, "rows": rows, "width": width, "bit_equal": same, "bytes_needed": needed}
            for name in us:
                med = float(np.median(us[name]))
                line[name + "_us"] = round(med, 1)
                line[name + "_us_min_max"] = [round(min(us[name]), 1), round(max(us[name]), 1)]
                line[name + "_TB_per_s"] = round(needed / med * 1e-6, 3)
            line["torch_over_kernel"] = round(line["torch_us"] / line["kernel_us"], 2)
            print(json.dumps(line), flush=True)
            del x, out
            torch.cuda.empty_cache()


def bench_ppo(args):
    import numpy as np
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    for n_envs in SIZES:
        agents = []
        for symmetry in (None, "augment"):
            env = RoboyVecEnv(MsjRobot(), n_envs, seed=0)
            agents.append((symmetry, env, PPO(env, n_steps=STEPS, device="cuda", seed=0, use_graphs=True, reward_scale=0.01,
                                              symmetry=symmetry)))
        ms = {s: {"rollout": [], "update": []} for s, _, _ in agents}
        for it in range(args.iterations + 1):                  # (the first one warms up: graph capture, buffers)
            for symmetry, _, agent in agents[it % 2:] + agents[:it % 2]:
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
        # the pass alone, as augment() runs it on the last rollout
        agent = agents[1][2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            agent.augment(roll)
        torch.cuda.synchronize()
        aug = 1e3 * (time.perf_counter() - t0) / 5
        line = {"ppo": True, "n_envs": n_envs, "n_steps": STEPS, "augment_ms": round(aug, 3)}
        for s in ms:
            for k in ("rollout", "update"):
                line["%s_%s_ms" % (s or "plain", k)] = round(float(np.median(ms[s][k])), 2)
                line["%s_%s_ms_all" % (s or "plain", k)] = [round(v, 2) for v in ms[s][k]]
        line["update_ratio"] = round(line["augment_update_ms"] / line["plain_update_ms"], 3)
        line["rest_ms"] = round(line["augment_update_ms"] - 2 * line["plain_update_ms"] - aug, 2)
        print(json.dumps(line), flush=True)
        for _, env, _ in agents:
            env.close()
        del agents, agent, roll
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass", dest="do_pass", action="store_true")
    ap.add_argument("--ppo", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=3)
    args = ap.parse_args()
    if not (args.do_pass or args.ppo):
        args.do_pass = args.ppo = True
    if args.do_pass:
        bench_pass(args)
    if args.ppo:
        bench_ppo(args)


if __name__ == "__main__":
    main()
