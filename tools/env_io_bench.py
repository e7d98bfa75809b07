#!/usr/bin/env python3
"""Time the fused env step with action latency and sensor noise (rb_env_io_*) against the same handle shape without
the io configuration, in one process, the handles stepped in turn, with HIP events on torch's stream.

    python tools/env_io_bench.py [--reps 50] [--rounds 5]

MsjRobot, Euler at 2 097 152 and at 4 096 envs, RK4 at 262 144 envs.  Per batch: noise alone on rows of 9 columns (q, qd) and of 25
(q, qd, length, force), a delay range (0, 3) alone on 9 columns, and both on 25 columns - each beside a handle of the same row width
that never configured io (RB_KERNEL_AUTO's kernel, or the tendon-channel kernel).  --rounds times --reps launches each; one JSON line
per pair with the median microseconds per launch of each, their ratio, and the ratio of the algorithmic bytes per env step."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CASES = (("noise", 9, {"q": 0.01, "qd": 0.05}, None),
         ("noise", 25, {"q": 0.01, "qd": 0.05, "length": 5e-4, "force": 2.0}, None),
         ("delay", 9, None, (0, 3)),
         ("both", 25, {"q": 0.01, "qd": 0.05, "length": 5e-4, "force": 2.0}, (0, 3)))


def _time(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def bench(what, cols, sigma, delay, integ, n, reps, rounds):
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = MsjRobot()
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream().cuda_stream
    act = torch.from_numpy(rng.uniform(-1, 1, (n, 8)).astype(np.float32)).cuda()
    channels = ("length", "force") if cols == 25 else None
    fns, envs = [], []
    for io in (False, True):
        env = RoboyVecEnv(robot, n, seed=1, integrator=integ, tendon_obs=channels, tendon_obs_scale={"force": 1 / 400} if channels else None,
                          sensor_noise=sigma if io else None, action_delay=delay if io else None)
        env.reset()
        env.sim.set_stream(stream)
        outs = [torch.empty(s, dtype=torch.float32, device="cuda") for s in ((n, cols), (n,), (n,))]
        fns.append(lambda env=env, outs=outs: env.step_dev(act.data_ptr(), *[o.data_ptr() for o in outs]))
        envs.append(env)
    for f in fns:
        for _ in range(5):
            f()
    times = [[], []]
    for _ in range(rounds):
        for k in (0, 1):
            times[k].append(_time(fns[k], reps))
    for env in envs:
        env.close()
    plain, io_us = float(np.median(times[0])), float(np.median(times[1]))
    base = 156 - 36 + 4 * cols                            # the nominal env step's 156 bytes hold a row of 36
    extra = (8 if sigma else 0) + (4 + 32 + 32 if delay else 0)
    return {"what": what, "columns": cols, "integrator": integ, "n_envs": n, "plain_us": round(plain, 2), "io_us": round(io_us, 2),
            "ratio": round(io_us / plain, 3), "bytes_per_env_plain": base, "bytes_per_env_io": base + extra,
            "byte_ratio": round((base + extra) / base, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    for integ, n in (("euler", 2097152), ("euler", 4096), ("rk4", 262144)):
        for what, cols, sigma, delay in CASES:
            print(json.dumps(bench(what, cols, sigma, delay, integ, n, args.reps, args.rounds)), flush=True)


if __name__ == "__main__":
    main()
