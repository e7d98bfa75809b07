#!/usr/bin/env python3
"""Time the normalising instances of the policy kernels (rp_act_norm_dev, rp_ppo_grad_norm_dev) against the plain ones
of the same build, in one process, alternating, with HIP events on torch's stream after warm-up - and the moments kernel against the
time its bytes take at the Euler kernels' measured HBM rate.

    python tools/obs_norm_bench.py [--reps 20] [--rounds 5] [--lib PATH] [--plain-only]

Configurations: the policy step at 262 144 x (9 -> 8) and 65 536 x (60 -> 38); one gradient call of 65 536 x 128 / 4 samples, gathered
through an index out of the rollout's 8 388 608 rows as PPO calls it, at 9 -> 8 and 25 -> 8; rp_obs_moments_dev over [128 x 262 144, 9].
One JSON line each: the median microseconds per launch of both variants and their ratio.  --lib PATH --plain-only times the plain
entry points of another build of libroboy_policy.so (the parent commit's: identical code, so that run is the box-to-box noise)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# 2 097 152 envs x 84 bytes in 31.4 us (README.md: "2 097 152 envs Euler"), bytes per second
EULER_HBM_RATE = 2097152 * 84 / 31.4e-6


def load_lib(path):
    """libroboy_policy.so by path, without the binding's version check: a parent build lacks the new entry points"""
    from gym_roboy_amd import _policy_native as pn
    lib = ctypes.CDLL(path)
    for name, (res, args) in pn.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def packed_blob(lib, obs_dim, act_dim, rng):
    import torch
    from gym_roboy_amd import _policy_native as pn
    shapes = pn.param_shapes(obs_dim, act_dim)
    keep = [(0.3 * rng.standard_normal(shapes[k])).astype(np.float32) for k in pn.PARAM_ORDER]
    st = pn.MlpParams(*[a.ctypes.data_as(ctypes.c_void_p) for a in keep])
    out = np.zeros(int(lib.rp_train_packed_floats(obs_dim, act_dim)), np.float32)
    assert lib.rp_pack_train(ctypes.byref(st), obs_dim, act_dim, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return torch.from_numpy(out).cuda()


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
    return [float(np.median(t)) for t in times]


def report(what, shape, us, extra=None):
    out = {"what": what, "shape": shape, "plain_us": round(us[0], 2)}
    if len(us) > 1:
        out.update({"norm_us": round(us[1], 2), "ratio": round(us[1] / us[0], 4)})
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libroboy_policy.so")
    ap.add_argument("--plain-only", action="store_true", help="time only the entry points without normalisation")
    args = ap.parse_args()
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = load_lib(args.lib or pn.library_path())
    rng = np.random.default_rng(0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def stats(obs_dim):
        return torch.stack([torch.zeros(obs_dim), torch.full((obs_dim,), 0.5)]).cuda().contiguous()

    for n, od, ad in ((262144, 9, 8), (65536, 60, 38)):
        blob, norm = packed_blob(lib, od, ad, rng), stats(od)
        obs = torch.randn(n, od, device="cuda")
        act, logp, val = torch.empty(n, ad, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        head = (ptr(blob), ptr(obs), ptr(act), ptr(logp), ptr(val), None, n, od, ad, 5, 0, 0, None, 0)
        fns = [lambda head=head: lib.rp_act_dev(*head, stream)]
        if not args.plain_only:
            fns.append(lambda head=head, norm=norm: lib.rp_act_norm_dev(*head, ptr(norm), 10.0, stream))
        assert all(f() == 0 for f in fns)
        report("policy step", "%d x (%d -> %d)" % (n, od, ad), alternate(fns, args.reps, args.rounds))
        del obs, act, logp, val

    B, rows = 65536 * 128 // 4, 65536 * 128
    for od, ad in ((9, 8), (25, 8)):
        blob, norm = packed_blob(lib, od, ad, rng), stats(od)
        obs, act = torch.randn(rows, od, device="cuda"), torch.randn(rows, ad, device="cuda")
        adv, logp, val, ret = (torch.randn(rows, device="cuda") for _ in range(4))
        logp -= 10.0
        index = torch.randperm(rows, device="cuda")[:B].contiguous()
        adv_stats = torch.tensor([0.0, 1.0], device="cuda")
        grad = torch.empty(int(lib.rp_grad_floats(od, ad)), device="cuda")
        ws = torch.empty(int(lib.rp_ppo_workspace_floats(od, ad, B)), device="cuda")
        head = (ptr(blob), ptr(obs), ptr(act), ptr(adv), ptr(adv_stats), ptr(logp), ptr(val), ptr(ret), ptr(index), B, od, ad, 0.2, 0.5)
        fns = [lambda head=head, grad=grad, ws=ws: lib.rp_ppo_grad_dev(*head, ptr(grad), ptr(ws), stream)]
        if not args.plain_only:
            fns.append(lambda head=head, grad=grad, ws=ws, norm=norm: lib.rp_ppo_grad_norm_dev(*head, ptr(norm), 10.0, ptr(grad), ptr(ws), stream))
        assert all(f() == 0 for f in fns)
        report("gradient", "%d of %d x (%d -> %d), form %d" % (B, rows, od, ad, lib.rp_grad_form(od, ad)), alternate(fns, max(args.reps // 4, 2), args.rounds))
        del obs, act, adv, logp, val, ret, index, ws

    if not args.plain_only:
        rows, od = 128 * 262144, 9
        obs = torch.randn(rows, od, device="cuda")
        sums = torch.zeros(1 + 2 * od, dtype=torch.float64, device="cuda")
        shift = torch.zeros(od, dtype=torch.float64, device="cuda")
        scratch = torch.zeros(int(lib.rp_obs_moments_scratch_doubles()), dtype=torch.float64, device="cuda")
        fn = lambda: lib.rp_obs_moments_dev(ptr(obs), rows, od, ptr(shift), ptr(sums), ptr(scratch), stream)
        assert fn() == 0
        us = alternate([fn], max(args.reps // 4, 2), args.rounds)
        floor = 1e6 * rows * od * 4 / EULER_HBM_RATE
        report("moments", "[%d, %d]" % (rows, od), us, {"us_at_the_euler_kernels_hbm_rate": round(floor, 1), "of_that_rate": round(floor / us[0], 3)})


if __name__ == "__main__":
    main()
