#!/usr/bin/env python3
"""What the update diagnostics and the KL-adaptive learning rate cost: the minibatch gradient with the action net's
diagnostics instance (rp_ppo_grad_diag_dev) against the same call without it (rp_ppo_grad_norm_dev; the value net's launch and the two
reductions are the same kernels in both, so the difference is the action net's instance), and rp_clip_adam_kl_dev against
rp_clip_adam_dev - alternating in one process, timed with HIP events on torch's stream after warm-up.

    python tools/ppo_diag_bench.py [--reps 10] [--rounds 7]
    ROBOY_POLICY_PREFETCH=0 python tools/ppo_diag_bench.py --small-only      # the plain small form of (9, 8)
    python tools/ppo_diag_bench.py --iteration                               # a whole PPO iteration, schedule off and on

Shapes, as PPO runs them at 262 144 envs x 128 steps / 4 minibatches: (9, 8) at B = 8 388 608 and (60, 38) at B = 2 097 152, rows
gathered through an index, advantage normalised in the kernel, without and with observation statistics.  The sibling is timed TWICE
(what separates its two series is the run-to-run spread the diagnostics instance is judged against).  One JSON line per case: per
variant the median, the smallest and the largest of the rounds' microseconds per call."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rollout_tail_bench import alternate  # noqa: E402


def summary(names, times):
    out = {}
    for name, t in zip(names, times):
        out[name] = {"median_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}
    return out


def grad_cases(args):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad, MlpPolicy, ObsNorm
    lib = pn.load()
    shapes = [(9, 8, 8_388_608)] + ([] if args.small_only else [(60, 38, 2_097_152)])
    for obs_dim, act_dim, B in shapes:
        torch.manual_seed(obs_dim)
        policy = MlpPolicy(obs_dim, act_dim).cuda()
        g = torch.Generator(device="cuda").manual_seed(B)
        rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
        obs, act, adv, val_old, ret = rnd(B, obs_dim), rnd(B, act_dim), rnd(B) * 3.0 + 1.5, rnd(B), rnd(B)
        with torch.no_grad():
            logp_old = torch.cat([policy.dist(obs[lo:lo + 262144]).log_prob(act[lo:lo + 262144]).sum(-1) for lo in range(0, B, 262144)])
        logp_old += (torch.rand(B, device="cuda", generator=g) - 0.5)
        idx = torch.randperm(B, device="cuda", generator=g)
        for with_norm in (False, True):
            norm = None
            if with_norm:
                norm = ObsNorm(obs_dim, "cuda")
                norm.update(obs)
            fgs = [FusedPolicyGrad(policy) for _ in range(3)]
            stats = fgs[0].minibatch_adv_stats(adv, idx).clone()

            def call(fg, diag):
                return lambda: fg.run(obs, act, adv, logp_old, val_old, ret, 0.2, 0.5, 0.1, index=idx, adv_stats=stats, entropy_grad=False,
                                      norm=norm, diagnostics=diag)
            names = ["sibling_a", "sibling_b", "diagnostics"]
            times = alternate([call(fgs[0], False), call(fgs[1], False), call(fgs[2], True)], args.reps, args.rounds)
            out = {"what": "minibatch gradient (four launches)", "shape": "(%d, %d) B = %d" % (obs_dim, act_dim, B),
                   "form": int(lib.rp_grad_form(obs_dim, act_dim)), "normalize_obs": with_norm}
            out.update(summary(names, times))
            sib = 0.5 * (out["sibling_a"]["median_us"] + out["sibling_b"]["median_us"])
            out["sibling_spread_us"] = round(max(max(times[0]), max(times[1])) - min(min(times[0]), min(times[1])), 2)
            out["diagnostics_minus_sibling_us"] = round(out["diagnostics"]["median_us"] - sib, 2)
            out["diagnostics_over_sibling"] = round(out["diagnostics"]["median_us"] / sib, 4)
            kl, cf = fgs[2].diag()
            out["approx_kl"], out["clip_frac"] = round(kl.item(), 6), round(cf.item(), 6)
            print(json.dumps(out), flush=True)
            del fgs
        del obs, act, adv, val_old, ret, logp_old, idx
        torch.cuda.empty_cache()


def adam_cases(args):
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for obs_dim, act_dim in ((9, 8), (60, 38)):
        layout, n = pn.grad_layout(obs_dim, act_dim)
        g = torch.Generator(device="cuda").manual_seed(n)
        sets = []
        for _ in range(3):
            p, m, v = torch.randn(n, device="cuda", generator=g), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
            grad = torch.randn(n, device="cuda", generator=g) * 0.01
            grad[layout["approx_kl"][0]] = 0.01                 # between the thresholds: the rate stays where it is
            sets.append((p, grad, m, v))
        lr_dev = torch.full((1,), 2.5e-4, device="cuda")
        stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def plain(k):
            p, grad, m, v = sets[k]
            return lambda: pn.check(lib.rp_clip_adam_dev(ptr(p), ptr(grad), ptr(m), ptr(v), obs_dim, act_dim, 2.5e-4, 0.9, 0.999, 1e-5, 7, 0.5, 1.0,
                                                         0.1, stream()))

        def with_kl():
            p, grad, m, v = sets[2]
            return lambda: pn.check(lib.rp_clip_adam_kl_dev(ptr(p), ptr(grad), ptr(m), ptr(v), obs_dim, act_dim, ptr(lr_dev), 0.01, 1.5, 1e-5, 1e-2,
                                                            0.9, 0.999, 1e-5, 7, 0.5, 1.0, 0.1, stream()))
        names = ["clip_adam_a", "clip_adam_b", "clip_adam_kl"]
        times = alternate([plain(0), plain(1), with_kl()], 10 * args.reps, args.rounds)
        out = {"what": "clip + Adam (one launch)", "shape": "(%d, %d): %d floats" % (obs_dim, act_dim, n)}
        out.update(summary(names, times))
        out["sibling_spread_us"] = round(max(max(times[0]), max(times[1])) - min(min(times[0]), min(times[1])), 2)
        out["kl_minus_sibling_us"] = round(out["clip_adam_kl"]["median_us"] - 0.5 * (out["clip_adam_a"]["median_us"] + out["clip_adam_b"]["median_us"]), 2)
        print(json.dumps(out), flush=True)


def iteration(args):
    """A whole PPO iteration (graph rollout + update) at 262 144 MsjRobot envs with the schedule off and on, twice each in turn, timed
    as tools/rollout_tail_bench.py times it: host clock around work that ends in a device synchronise."""
    import time
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    n = 262144
    for on in (False, True, False, True):
        env = RoboyVecEnv(MsjRobot(), n)
        agent = PPO(env, ent_coef=0.1, device="cuda", reward_scale=0.01, use_graphs=True, fused_policy=True, fused_update=True,
                    lr_schedule="adaptive" if on else None)
        roll = agent.collect(); agent.update(roll); torch.cuda.synchronize()
        tc, tu, last = [], [], {}
        for _ in range(3):
            t0 = time.perf_counter(); roll = agent.collect(); torch.cuda.synchronize(); t1 = time.perf_counter()
            last = agent.update(roll); torch.cuda.synchronize(); t2 = time.perf_counter()
            tc.append(t1 - t0); tu.append(t2 - t1)
        out = {"what": "PPO iteration", "envs": n, "lr_schedule": "adaptive" if on else None, "rollout_ms": [round(1e3 * t, 2) for t in tc],
               "update_ms": [round(1e3 * t, 2) for t in tu]}
        out.update({k: last[k] for k in ("approx_kl", "clip_frac", "lr") if k in last})
        print(json.dumps(out), flush=True)
        env.close()
        del agent, env, roll
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small-only", action="store_true", help="(9, 8) only: for a second run under ROBOY_POLICY_PREFETCH=0")
    ap.add_argument("--iteration", action="store_true", help="only: a whole PPO iteration at 262 144 envs, schedule off and on")
    args = ap.parse_args()
    if args.iteration:
        return iteration(args)
    grad_cases(args)
    if not args.small_only:
        adam_cases(args)


if __name__ == "__main__":
    main()
