#!/usr/bin/env python3
"""Time the fused env step with tendon channels in its observation (rb_env_obs_*) against the PARENT commit's
library, in one process, alternating, with HIP events on torch's stream.

    python tools/tendon_obs_bench.py --parent-lib /path/to/parent/libroboy_sim.so [--reps 50] [--rounds 5]

The yardstick is a build of the parent commit (`git worktree add <dir> HEAD~1 && make -C <dir>/gym_roboy_amd/csrc`), loaded next to
this tree's library.  Per configuration three callables are stepped in turn, --rounds times --reps launches each:
    A    the parent's fused env step (RB_KERNEL_AUTO; with randomization: its parameter env step)
    B    A followed by rb_tendon_state_dev for the same channels on the same stream - the only way to get these numbers from the
         parent (not with randomization: the parent refuses the readout on a parameter handle)
    new  this tree's fused env step with the channels in the row
Configurations (MsjRobot): length + force - Euler at 2 097 152 envs, RK4 at 262 144, Euler at 4 096; the first two again with
randomization (no B there); all four channels, Euler at 2 097 152; and an 8-tendon robot on kernarg constants, length + force, Euler
at 2 097 152 and RK4 at 262 144.  One JSON line each: median microseconds per launch, new / A beside the
byte ratio (156 + 32 C) / 156, new / B, and the algorithmic bytes per env (new: 156 + 32 C; B: 156 + 4 (6 + 8 + 8 C)).
Without --parent-lib the baselines run on this tree's library (whose pre-existing kernels are the parent's, instruction for
instruction), and the line says so."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CHANNELS = ("length", "rate", "activation", "force")


def _time(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / reps


def _load_parent(path):
    """The parent's library bound with this tree's signatures, as far as it exports them (it has no rb_env_obs_*)."""
    from gym_roboy_amd import _native as nat
    nat.load()                                   # this tree's library first: it shares its HIP runtime with torch
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in nat.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


class _Library:
    """Objects built inside this block call into `lib`: HipBatchSimulation keeps the library it was built with."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        from gym_roboy_amd import _native as nat
        self.saved = nat.load()                  # (loaded now, so that leaving the block never puts "not loaded" back)
        nat._LIB = self.lib or self.saved

    def __exit__(self, *exc):
        from gym_roboy_amd import _native as nat
        nat._LIB = self.saved


def _kernarg_robot():
    """MsjRobot with every muscle 2 % stronger: an 8-tendon robot whose constants are not the ahead-of-time table's.  The extended
    step takes its kernarg instance (rolled tendon loop); the parent's A is what RB_KERNEL_AUTO gives such a robot (hiprtc-built
    where the headers lie beside the parent's library, its kernarg instance otherwise)."""
    from gym_roboy_amd.envs.robots import MsjRobot, RobotDescription, msj_platform_spec
    spec = msj_platform_spec()
    for t in spec["tendons"]:
        t["f_max"] = 1.02 * t["f_max"]
    desc = RobotDescription(spec)

    class StrongerMsj(MsjRobot):
        @classmethod
        def get_description(cls):
            return desc
    return StrongerMsj()


def bench(parent, integ, n, channels, randomized, reps, rounds, kernarg=False):
    import torch
    from gym_roboy_amd import _native as nat
    from gym_roboy_amd.envs.params import ParamRanges
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = _kernarg_robot() if kernarg else MsjRobot()
    nt = robot.get_description().n_t
    rng = np.random.default_rng(0)
    ranges = ParamRanges(force_scale=(0.8, 1.2), setpoint_offset=(-0.01, 0.01), mass_scale=(0.8, 1.25), damping_scale=(0.5, 2.0))
    stream = torch.cuda.current_stream().cuda_stream
    act = torch.from_numpy(rng.uniform(-1, 1, (n, nt)).astype(np.float32)).cuda()
    C = len(channels)
    new_rows = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")

    def make(tendon_obs):
        env = RoboyVecEnv(robot, n, seed=1, integrator=integ, randomization=ranges if randomized else None, tendon_obs=tendon_obs)
        env.reset()
        env.sim.set_stream(stream)
        outs = [new_rows(n, env.obs_dim), new_rows(n), new_rows(n)]
        return env, outs, (lambda: env.step_dev(act.data_ptr(), *[o.data_ptr() for o in outs]))

    with _Library(parent):
        base, base_outs, step_a = make(None)
        ts = {c: new_rows(n, nt) for c in channels}
        ptrs = [ctypes.c_void_p(ts[c].data_ptr()) if c in ts else None for c in CHANNELS]

        def step_b():
            step_a()
            nat.check(base.sim._lib.rb_tendon_state_dev(base.sim.handle, ctypes.c_void_p(act.data_ptr()), nat.RB_SP_ENV, 1.0, *ptrs))
    ext, ext_outs, step_new = make(channels)
    fns = {"A": step_a, "new": step_new}
    if not randomized:
        fns["B"] = step_b
    for f in fns.values():
        for _ in range(5):
            f()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(_time(f, reps))
    base.close(); ext.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    par_bytes = 4 * (2 * nt + 4) if randomized else 0
    out = {"robot": "8 tendons, kernarg constants" if kernarg else "MsjRobot", "integrator": integ, "n_envs": n, "channels": list(channels), "randomized": randomized,
           "baseline_library": "parent" if parent is not None else "this tree (no --parent-lib)",
           "A_us": round(med["A"], 2), "new_us": round(med["new"], 2), "new_over_A": round(med["new"] / med["A"], 3),
           "byte_ratio": round((156 + par_bytes + 32 * C) / (156 + par_bytes), 3),
           "bytes_per_env_new": 156 + par_bytes + 32 * C}
    if "B" in med:
        out.update({"B_us": round(med["B"], 2), "new_over_B": round(med["new"] / med["B"], 3),
                    "bytes_per_env_B": 156 + 4 * (6 + 8 + 8 * C)})
    else:
        out["B_us"] = "none: the parent refuses rb_tendon_state_dev on a parameter handle"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.environ.get("ROBOY_SIM_PARENT_LIB"),
                    help="libroboy_sim.so of the parent commit (default: $ROBOY_SIM_PARENT_LIB)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    parent = _load_parent(args.parent_lib) if args.parent_lib else None
    lf = ("length", "force")
    for integ, n, ch, rnd in (("euler", 2097152, lf, False), ("rk4", 262144, lf, False), ("euler", 4096, lf, False),
                              ("euler", 2097152, lf, True), ("rk4", 262144, lf, True), ("euler", 2097152, CHANNELS, False)):
        print(json.dumps(bench(parent, integ, n, ch, rnd, args.reps, args.rounds)), flush=True)
    # the instances every other robot takes (constants through the kernarg, rolled tendon loop)
    for integ, n, ch in (("euler", 2097152, lf), ("rk4", 262144, lf)):
        print(json.dumps(bench(parent, integ, n, ch, False, args.reps, args.rounds, kernarg=True)), flush=True)


if __name__ == "__main__":
    main()
