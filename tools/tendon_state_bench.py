#!/usr/bin/env python3
"""Time the tendon-state readout (rb_tendon_state_dev) with HIP events next to the Euler step of the same handle.

    python tools/tendon_state_bench.py [--reps 50]

Configurations: MsjRobot at 262 144 and 2 097 152 envs, the upper body at 8 192 and 65 536 envs.  Per configuration one JSON line:
microseconds per readout (mean over --reps back-to-back launches, all four outputs, set-points given), the algorithmic bytes it
moves - q, qd and the action row read, four [n_t] rows written: 4 (2 n_q + n_t + 4 n_t) per env, 184 B for MsjRobot - the
fraction of the 8 TB/s HBM peak that is, and the Euler step's microseconds on the same handle and batch for comparison."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12


def _time(fn, reps, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def bench(robot, n, reps):
    import torch
    from gym_roboy_amd import _native as nat
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    desc = robot.get_description()
    rng = np.random.default_rng(0)
    sim = HipBatchSimulation(robot, n, integrator="euler")
    sim.set_state(rng.uniform(0.9 * desc.q_lo, 0.9 * desc.q_hi, (n, desc.n_q)).astype(np.float32),
                  rng.uniform(-desc.qd_max, desc.qd_max, (n, desc.n_q)).astype(np.float32))
    sim.set_stream(torch.cuda.current_stream().cuda_stream)
    sp = torch.from_numpy(rng.uniform(-0.3, 0.3, (n, desc.n_t)).astype(np.float32)).cuda()
    outs = [torch.empty((n, desc.n_t), dtype=torch.float32, device="cuda") for _ in range(4)]
    ptrs = [o.data_ptr() for o in outs]
    us = _time(lambda: sim.tendon_state_dev(sp.data_ptr(), nat.RB_SP_SCALED, 1.0, *ptrs), reps)
    step_us = _time(lambda: sim.step_dev(sp.data_ptr(), 1.0), reps)
    sim.close()
    nbytes = 4 * (2 * desc.n_q + desc.n_t + 4 * desc.n_t) * n
    return {"robot": desc.name, "n_envs": n, "n_t": desc.n_t, "readout_us": round(us, 2), "bytes": nbytes,
            "bytes_per_env": nbytes // n, "frac_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3),
            "euler_step_us": round(step_us, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    for robot, n in ((MsjRobot(), 262144), (MsjRobot(), 2097152), (UpperBodyRobot(), 8192), (UpperBodyRobot(), 65536)):
        print(json.dumps(bench(robot, n, args.reps)), flush=True)


if __name__ == "__main__":
    main()
