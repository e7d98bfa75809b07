#!/usr/bin/env python3
"""Time the per-env-parameter kernels (rb_params_*) against the nominal kernels of the same configuration, in one
process, alternating, with HIP events on torch's stream.

    python tools/env_params_bench.py [--reps 50] [--rounds 5]

Configurations (MsjRobot): the Euler step at 2 097 152 envs, the RK4 step at 262 144, the fused env step (Euler) at 2 097 152, and
the Euler step at 4 096.  Two handles per configuration - one nominal (RB_KERNEL_AUTO's choice), one with parameters enabled and
drawn from ranges - stepped in turn, --rounds times --reps launches each; per configuration one JSON line with the median
microseconds per launch of each and their ratio, and the algorithmic bytes per env of each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _time(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def bench(kind, integ, n, reps, rounds):
    import torch
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = MsjRobot()
    desc = robot.get_description()
    rng = np.random.default_rng(0)
    ranges = ParamRanges(force_scale=(0.8, 1.2), setpoint_offset=(-0.01, 0.01), mass_scale=(0.8, 1.25), damping_scale=(0.5, 2.0))
    stream = torch.cuda.current_stream().cuda_stream
    act = torch.from_numpy(rng.uniform(-1, 1, (n, desc.n_t)).astype(np.float32)).cuda()
    fns, owners = [], []
    for params in (False, True):
        if kind == "env":
            env = RoboyVecEnv(robot, n, seed=1, integrator=integ, randomization=ranges if params else None)
            env.reset()
            env.sim.set_stream(stream)
            outs = [torch.empty(s, dtype=torch.float32, device="cuda") for s in ((n, 9), (n,), (n,))]
            fns.append(lambda env=env, outs=outs: env.step_dev(act.data_ptr(), *[o.data_ptr() for o in outs]))
            owners.append(env)
        else:
            sim = HipBatchSimulation(robot, n, integrator=integ)
            sim.set_state(rng.uniform(0.9 * desc.q_lo, 0.9 * desc.q_hi, (n, 3)).astype(np.float32),
                          rng.uniform(-desc.qd_max, desc.qd_max, (n, 3)).astype(np.float32))
            if params:
                sim.enable_params()
                sim.set_param_ranges(ranges)
                sim.sample_params()
            sim.set_stream(stream)
            fns.append(lambda sim=sim: sim.step_dev(act.data_ptr(), 0.3))
            owners.append(sim)
    for f in fns:
        for _ in range(5):
            f()
    times = [[], []]
    for _ in range(rounds):
        for k in (0, 1):
            times[k].append(_time(fns[k], reps))
    for o in owners:
        o.close()
    nominal, param = float(np.median(times[0])), float(np.median(times[1]))
    base = 84 if kind == "step" else 156
    P = 2 * desc.n_t + 4
    return {"entry": kind, "integrator": integ, "n_envs": n, "nominal_us": round(nominal, 2), "params_us": round(param, 2),
            "ratio": round(param / nominal, 3), "bytes_per_env_nominal": base, "bytes_per_env_params": base + 4 * P}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    for kind, integ, n in (("step", "euler", 2097152), ("step", "rk4", 262144), ("env", "euler", 2097152), ("step", "euler", 4096)):
        print(json.dumps(bench(kind, integ, n, args.reps, args.rounds)), flush=True)


if __name__ == "__main__":
    main()
