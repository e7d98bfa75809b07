#!/usr/bin/env python3
"""Time the fused env step with the last K actions in the observation (rb_env_action_obs_*) against a handle of the
same shape with K = 0, in one process, the handles stepped in turn, with HIP events on torch's stream.

    python tools/action_obs_bench.py [--reps 50] [--rounds 5]

MsjRobot at 2 097 152 and at 4 096 envs, Euler and RK4, rows of 9 leading columns and of 25 (length, force), K = 1, 3, 8.  The K = 0
handle launches what it launched before the option existed (RB_KERNEL_AUTO's row, or the tendon-channel kernel).  --rounds times
--reps launches each; one JSON line per (batch, integrator, columns, K) with the median microseconds per launch of each, their ratio,
and the ratio of the algorithmic bytes per env step: the option adds 4 K n_t bytes of row, 4 (K - 1) n_t bytes of ring reads and
4 n_t bytes of ring store (no ring exists without it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N_T = 8


def _time(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def bench(cols, integ, n, ks, reps, rounds):
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = MsjRobot()
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream().cuda_stream
    act = torch.from_numpy(rng.uniform(-2, 2, (n, N_T)).astype(np.float32)).cuda()
    channels = ("length", "force") if cols == 25 else None
    fns, envs = [], []
    for k in (0,) + tuple(ks):
        env = RoboyVecEnv(robot, n, seed=1, integrator=integ, tendon_obs=channels, tendon_obs_scale={"force": 1 / 400} if channels else None,
                          action_obs=k or None)
        env.reset()
        env.sim.set_stream(stream)
        assert env.obs_dim == cols + k * N_T
        outs = [torch.empty(s, dtype=torch.float32, device="cuda") for s in ((n, env.obs_dim), (n,), (n,))]
        fns.append(lambda env=env, outs=outs: env.step_dev(act.data_ptr(), *[o.data_ptr() for o in outs]))
        envs.append(env)
    for f in fns:
        for _ in range(5):
            f()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            times[i].append(_time(f, reps))
    for env in envs:
        env.close()
    plain = float(np.median(times[0]))
    base = 156 - 36 + 4 * cols                            # the nominal env step's 156 bytes hold a row of 36
    out = []
    for i, k in enumerate(ks, 1):
        us = float(np.median(times[i]))
        extra = 4 * k * N_T + 4 * (k - 1) * N_T + 4 * N_T
        out.append({"rows": k, "columns": cols, "obs_dim": cols + k * N_T, "integrator": integ, "n_envs": n, "plain_us": round(plain, 2),
                    "rows_us": round(us, 2), "ratio": round(us / plain, 3), "plain_min_max_us": [round(min(times[0]), 2), round(max(times[0]), 2)],
                    "rows_min_max_us": [round(min(times[i]), 2), round(max(times[i]), 2)], "bytes_per_env_plain": base,
                    "bytes_per_env_rows": base + extra, "byte_ratio": round((base + extra) / base, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    for n in (2097152, 4096):
        for integ in ("euler", "rk4"):
            for cols in (9, 25):
                for row in bench(cols, integ, n, (1, 3, 8), args.reps, args.rounds):
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
