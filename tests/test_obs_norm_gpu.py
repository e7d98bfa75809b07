"""Running observation normalisation inside the fused policy kernels (csrc/mlp_policy.hip, mlp_train.hip: the *_norm instances;
mlp_update.hip: the statistics), DESIGN.md §15.

The operand is specified to the bit - x' = min(max((x - mean) * rstd, -clip), clip), difference and product each rounded once to float32
- so the main proof needs no tolerance: a kernel given raw observations and the statistics must produce the bits it produces when
given x' computed by numpy in float32, at every site that fetches an observation operand (the policy step; in the gradient the layer-1
forward AND the dW1 accumulation, in the prefetching, the staged and the direct form).  One case per form also runs against float64
with the tolerances tests/test_policy_gpu.py holds for operands in [-2, 2]; the statistics are held to numpy's two-pass moments with
the bound of tests/test_obs_norm_cpu.py; PPO runs end to end on RoboyVecEnv with unscaled tendon channels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from test_obs_norm_cpu import assert_float_form, assert_moments, columns
from test_policy_gpu import _minibatch, _policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7777.0
PAD = 64
CLIPRANGE, VF_COEF, ENT_COEF = 0.2, 0.5, 0.1

# column kinds, cycled over the observation: offset, spread; and the statistics handed to the kernels - NOT the data's own: a mean
# off by MEAN_OFF spreads, an rstd of RSTD_MUL / spread (the constant column: 5), so that some elements clip at 10 and many at 2
MEANS, SPREADS = np.array([0.0, 0.2, 400.0, -3.0]), np.array([1.0, 0.01, 50.0, 0.0])
MEAN_OFF, RSTD_MUL = np.array([0.2, -0.3, 0.5, 0.0]), np.array([1.5, 1.0, 8.0, 1.0])


def wide_case(n, obs_dim, seed, clip):
    """raw [n, obs_dim] float32, norm [2, obs_dim] float32, x' = the spec's formula in numpy float32, and the clipped fractions"""
    rng = np.random.default_rng(seed)
    kind = np.arange(obs_dim) % 4
    raw = (rng.standard_normal((n, obs_dim)) * SPREADS[kind] + MEANS[kind]).astype(np.float32)
    mean = (MEANS[kind] + MEAN_OFF[kind] * SPREADS[kind] - 0.1 * (SPREADS[kind] == 0)).astype(np.float32)
    rstd = np.where(SPREADS[kind] > 0, RSTD_MUL[kind] / np.maximum(SPREADS[kind], 1e-30), 5.0).astype(np.float32)
    norm = np.stack([mean, rstd])
    c = np.float32(clip)
    xn = np.minimum(np.maximum((raw - mean) * rstd, -c), c)
    assert xn.dtype == np.float32
    return raw, norm, xn, float((xn == c).mean()), float((xn == -c).mean())


def obs_norm_of(norm, clip):
    import torch
    from gym_roboy_amd.ppo import ObsNorm
    n = ObsNorm(norm.shape[1], "cuda", clip=clip)
    n.norm.copy_(torch.from_numpy(norm))
    return n


def step_padded(policy, obs, norm=None, seed=5, step=3):
    """one policy step with noise into sentinel-padded outputs: (act, logp, val, mean) device tensors of n + PAD rows"""
    import torch
    from gym_roboy_amd.ppo import FusedPolicyStep
    f = FusedPolicyStep(policy, seed=seed)
    n, ad = obs.shape[0], f.act_dim
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    out = (full(n + PAD, ad), full(n + PAD), full(n + PAD), full(n + PAD, ad))
    f.act_into(obs, out[0], out[1], out[2], mean=out[3], step=step, norm=norm)
    torch.cuda.synchronize()
    return out


# ---- bit identity: the policy step ----
@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("obs_dim,act_dim", [(9, 8), (25, 8), (60, 38), (95, 64)])
def test_policy_step_on_raw_observations_equals_the_step_on_the_normalised_ones(obs_dim, act_dim, n):
    import torch
    clip = 2.0 if (obs_dim, n) in ((9, 4097), (60, 65)) else 10.0
    raw, norm, xn, hi, lo = wide_case(n, obs_dim, n + obs_dim, clip)
    if clip == 2.0:
        assert 0.01 < hi < 0.5 and 0.01 < lo < 0.5 and hi + lo < 0.5, (hi, lo)
    elif n > 1:
        assert hi > 0 and lo > 0
    policy = _policy(obs_dim, act_dim, obs_dim + act_dim).cuda()
    got = step_padded(policy, torch.from_numpy(raw).cuda(), norm=obs_norm_of(norm, clip))
    want = step_padded(policy, torch.from_numpy(xn).cuda())
    for g, w in zip(got, want):
        assert (g[n:] == SENTINEL).all()                       # nothing written past n
        assert torch.equal(g, w)
    assert (got[0][:n] != got[3][:n]).any()                   # with noise


@pytest.mark.parametrize("obs_dim,act_dim,n", [(9, 8, 4097), (95, 64, 65)])
def test_policy_step_without_statistics_is_the_old_entry_point(obs_dim, act_dim, n):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyStep
    raw = wide_case(n, obs_dim, 1, 10.0)[0]
    raw = np.clip(raw, -3.0, 3.0)                              # (operands a tanh layer does not saturate on)
    obs = torch.from_numpy(raw).cuda()
    policy = _policy(obs_dim, act_dim, 3).cuda()
    want = step_padded(policy, obs)
    # identity statistics and no clamp: the same bits
    ident = np.stack([np.zeros(obs_dim, np.float32), np.ones(obs_dim, np.float32)])
    got = step_padded(policy, obs, norm=obs_norm_of(ident, float("inf")))
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # d_norm == NULL through the new entry point launches the old kernel
    f = FusedPolicyStep(policy, seed=5)
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    out = (full(n + PAD, act_dim), full(n + PAD), full(n + PAD), full(n + PAD, act_dim))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    pn.check(pn.load().rp_act_norm_dev(ptr(f.pack()), ptr(obs), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), n, obs_dim, act_dim,
                                       5, 0, 3, None, 0, None, 0.0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for g, w in zip(out, want):
        assert torch.equal(g, w)


# ---- bit identity: the gradient ----
GRAD_CASES = [(9, 8, 1, 2), (9, 8, 37, 2), (9, 8, 1000, 2), (25, 8, 1000, 2), (29, 8, 1000, 2), (9, 8, 70_000, 2), (29, 8, 70_000, 2),
              (30, 8, 129, 1), (40, 12, 777, 0), (60, 38, 777, 0)]


def _want_form(form):
    return 1 if form == 2 and os.environ.get("ROBOY_POLICY_PREFETCH", "1")[0] == "0" else form


@pytest.mark.parametrize("obs_dim,act_dim,B,form", GRAD_CASES)
def test_gradient_on_raw_observations_equals_the_gradient_on_the_normalised_ones(obs_dim, act_dim, B, form):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad
    assert pn.load().rp_grad_form(obs_dim, act_dim) == _want_form(form)
    if form == 2 and B == 70_000:
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert (B + 63) // 64 > 4 * n_cu                       # a second tile per wave: the two prefetch buffers alternate
    clip = 2.0 if (obs_dim, B) in ((9, 1000), (30, 129), (60, 777)) else 10.0          # one case per form
    raw, norm, xn, hi, lo = wide_case(B, obs_dim, B + obs_dim, clip)
    if clip == 2.0:
        assert 0.01 < hi < 0.5 and 0.01 < lo < 0.5 and hi + lo < 0.5, (hi, lo)
    ref = _policy(obs_dim, act_dim, 11 + obs_dim).double()
    rest = [t.float().cuda().contiguous() for t in _minibatch(ref, obs_dim, act_dim, B, B, CLIPRANGE)[1:]]
    fg = FusedPolicyGrad(_policy(obs_dim, act_dim, 11 + obs_dim).cuda())
    stats = obs_norm_of(norm, clip)
    raw_d, xn_d = torch.from_numpy(raw).cuda(), torch.from_numpy(xn).cuda()
    fg.run(xn_d, *rest, CLIPRANGE, VF_COEF, ENT_COEF)
    torch.cuda.synchronize()
    want = fg._g.clone()
    assert torch.isfinite(want).all() and want.abs().max() > 0
    fg._g.zero_()
    fg.run(raw_d, *rest, CLIPRANGE, VF_COEF, ENT_COEF, norm=stats)
    torch.cuda.synchronize()
    assert torch.equal(fg._g, want)
    # the same minibatch addressed through row indices into larger tensors (NaN in the rows outside the index)
    perm = torch.randperm(3 * B, device="cuda")[:B]
    big = [torch.full((3 * B,) + tuple(t.shape[1:]), float("nan"), device="cuda") for t in [raw_d] + rest]
    for t_big, t in zip(big, [raw_d] + rest):
        t_big[perm] = t
    fg._g.zero_()
    fg.run(big[0], big[1], rest[1], big[3], big[4], big[5], CLIPRANGE, VF_COEF, ENT_COEF, index=perm, norm=stats)
    torch.cuda.synchronize()
    assert torch.equal(fg._g, want)


@pytest.mark.parametrize("obs_dim,act_dim,B,form", [(9, 8, 1000, 2), (30, 8, 129, 1), (60, 38, 777, 0)])
def test_gradient_without_statistics_is_the_old_entry_point(obs_dim, act_dim, B, form):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad
    lib = pn.load()
    assert lib.rp_grad_form(obs_dim, act_dim) == _want_form(form)
    ref = _policy(obs_dim, act_dim, 11 + obs_dim).double()
    mb = [t.float().cuda().contiguous() for t in _minibatch(ref, obs_dim, act_dim, B, B, CLIPRANGE)]
    fg = FusedPolicyGrad(_policy(obs_dim, act_dim, 11 + obs_dim).cuda())
    fg.run(*mb, CLIPRANGE, VF_COEF, ENT_COEF, entropy_grad=False)
    torch.cuda.synchronize()
    want = fg._g.clone()
    ident = np.stack([np.zeros(obs_dim, np.float32), np.ones(obs_dim, np.float32)])
    fg._g.zero_()
    fg.run(*mb, CLIPRANGE, VF_COEF, ENT_COEF, entropy_grad=False, norm=obs_norm_of(ident, float("inf")))
    torch.cuda.synchronize()
    assert torch.equal(fg._g, want)
    # d_norm == NULL through the new entry point launches the old kernels
    packed = torch.cat([fg._named[k].detach().reshape(-1) for k in pn.PARAM_ORDER] + [fg._zero])[fg._map]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    fg._g.zero_()
    pn.check(lib.rp_ppo_grad_norm_dev(ptr(packed), ptr(mb[0]), ptr(mb[1]), ptr(mb[2]), None, ptr(mb[3]), ptr(mb[4]), ptr(mb[5]), None, B,
                                      obs_dim, act_dim, CLIPRANGE, VF_COEF, None, 0.0, ptr(fg._g), ptr(fg._ws),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(fg._g, want)


def test_limits_of_the_gradient_kernels_are_what_they_were():
    """The statistics take no LDS: 29 -> 8 is still the last prefetching size, 60 -> 38 still fits, 63 -> 64 still does not."""
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    if os.environ.get("ROBOY_POLICY_PREFETCH", "1")[0] != "0":
        assert [lib.rp_grad_form(o, 8) for o in (9, 29, 30, 31, 32)] == [2, 2, 1, 1, 0]
    assert lib.rp_train_packed_floats(60, 38) > 0 and lib.rp_train_packed_floats(63, 64) < 0 and lib.rp_train_packed_floats(64, 8) < 0


# ---- against float64 ----
def _consistent_minibatch(policy64, x64, act_dim, seed):
    """tests/test_policy_gpu.py's _minibatch on GIVEN (already normalised, float64) observations: every branch of the two clipped
    losses occurs, no sample sits on a clip boundary"""
    import torch
    g = torch.Generator().manual_seed(seed)
    B = x64.shape[0]
    with torch.no_grad():
        d = policy64.dist(x64)
        act = d.mean + d.stddev * torch.randn(B, act_dim, generator=g, dtype=torch.float64)
        logp = d.log_prob(act).sum(-1)
        v = policy64.value(x64)
    logp_old = logp + (torch.rand(B, generator=g, dtype=torch.float64) - 0.5)
    adv = torch.randn(B, generator=g, dtype=torch.float64)
    val_old = v + (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 6 * CLIPRANGE
    ratio = (logp - logp_old).exp()
    near = ((ratio - (1 - CLIPRANGE)).abs() < 1e-4) | ((ratio - (1 + CLIPRANGE)).abs() < 1e-4)
    logp_old = torch.where(near, logp_old + 0.01, logp_old)
    near_v = ((v - val_old).abs() - CLIPRANGE).abs() < 1e-4
    val_old = torch.where(near_v, val_old + 0.01, val_old)
    ret = v + torch.randn(B, generator=g, dtype=torch.float64)
    return act, adv, logp_old, val_old, ret


def _x64(raw, norm, clip):
    """x' in float64 from the float32 statistics"""
    return np.clip((raw.astype(np.float64) - norm[0].astype(np.float64)) * norm[1].astype(np.float64), -clip, clip)


@pytest.mark.parametrize("obs_dim,act_dim,B,form", [(9, 8, 1000, 2), (30, 8, 129, 1), (60, 38, 777, 0)])
def test_normalised_gradient_matches_float64(obs_dim, act_dim, B, form):
    """clip = 2: the operands lie in [-2, 2], the range tests/test_policy_gpu.py's tolerances were set for (5e-4 of each tensor's
    largest gradient, 1e-4 on the loss terms)."""
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad
    from oracle.policy_ref import ppo_grad64
    assert pn.load().rp_grad_form(obs_dim, act_dim) == _want_form(form)
    raw, norm, _, hi, lo = wide_case(B, obs_dim, 7 * B + obs_dim, 2.0)
    assert hi > 0.01 and lo > 0.01
    x64 = torch.from_numpy(_x64(raw, norm, 2.0))
    ref = _policy(obs_dim, act_dim, 11 + obs_dim).double()
    rest = _consistent_minibatch(ref, x64, act_dim, B)
    pg_ref, vf_ref = ppo_grad64(ref, x64, *rest, CLIPRANGE, VF_COEF, ENT_COEF)
    policy = _policy(obs_dim, act_dim, 11 + obs_dim).cuda()
    fg = FusedPolicyGrad(policy)
    pg, vf = fg.run(torch.from_numpy(raw).cuda(), *[t.float().cuda().contiguous() for t in rest], CLIPRANGE, VF_COEF, ENT_COEF,
                    norm=obs_norm_of(norm, 2.0))
    torch.cuda.synchronize()
    worst = 0.0
    for (name, p), (_, q) in zip(policy.named_parameters(), ref.named_parameters()):
        scale = max(q.grad.abs().max().item(), 1e-6)
        worst = max(worst, (p.grad.detach().cpu().double() - q.grad).abs().max().item() / scale)
    print("(%d, %d) B = %d form %d: gradient %.3g  pg %.3g  vf %.3g" % (obs_dim, act_dim, B, form, worst, abs(pg.item() - pg_ref), abs(vf.item() - vf_ref)))
    assert abs(pg.item() - pg_ref) < 1e-4 * max(1.0, abs(pg_ref)) and abs(vf.item() - vf_ref) < 1e-4 * max(1.0, abs(vf_ref))
    assert worst < 5e-4


def test_normalised_policy_step_matches_float64():
    import torch
    obs_dim, act_dim, n = 9, 8, 1000
    raw, norm, _, hi, lo = wide_case(n, obs_dim, 99, 2.0)
    assert hi > 0.01 and lo > 0.01
    x64 = torch.from_numpy(_x64(raw, norm, 2.0))
    ref = _policy(obs_dim, act_dim, 17).double()
    with torch.no_grad():
        d = ref.dist(x64)
        mean_ref, val_ref = d.mean.numpy(), ref.value(x64).numpy()
    act, logp, val, mean = (t[:n].cpu().numpy() for t in step_padded(_policy(obs_dim, act_dim, 17).cuda(), torch.from_numpy(raw).cuda(),
                                                                      norm=obs_norm_of(norm, 2.0)))
    with torch.no_grad():
        logp_ref = d.log_prob(torch.from_numpy(act).double()).sum(-1).numpy()
    e = (np.abs(mean - mean_ref).max(), np.abs(val - val_ref).max(), np.abs(logp - logp_ref).max())
    print("mean %.3g  value %.3g  logp %.3g" % e)
    assert e[0] < 2e-5 * max(1.0, np.abs(mean_ref).max())
    assert e[1] < 2e-5 * max(1.0, np.abs(val_ref).max())
    assert e[2] < 1e-4 * max(1.0, np.abs(logp_ref).max())


# ---- the statistics ----
def _gpu_stats(chunks, obs_dim):
    import torch
    from gym_roboy_amd.ppo import ObsNorm
    n = ObsNorm(obs_dim, "cuda")
    for c in chunks:
        n.update(torch.from_numpy(c).cuda())
    torch.cuda.synchronize()
    return n


@pytest.mark.parametrize("obs_dim", [1, 9, 25, 95])
@pytest.mark.parametrize("rows", [1, 63, 4097, "several_passes"])
def test_moments_and_merge_match_numpy_two_pass(obs_dim, rows):
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    if rows == "several_passes":
        # from the launch geometry: the grid grows with the rows up to a cap, 256 / obs_dim rows per workgroup and pass.  The fewest
        # rows that reach the cap (bisected from the library's own answer), and no fewer than five passes of that grid, so the
        # loop's four-rows-in-flight part and its remainder both run; 37 more for a ragged end
        cap = int(lib.rp_obs_moments_blocks(1 << 40, obs_dim))
        one_pass = cap * (256 // obs_dim)
        lo, hi = 1, 1 << 40
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if int(lib.rp_obs_moments_blocks(mid, obs_dim)) == cap else (mid + 1, hi)
        rows = max(lo, 5 * one_pass) + 37
        assert int(lib.rp_obs_moments_blocks(rows, obs_dim)) == cap and 5 * one_pass < rows < 16 * one_pass
        assert rows % one_pass != 0             # threads take q or q + 1 rows, q >= 5: one of the two is no multiple of four
    data = columns(np.random.default_rng(rows + obs_dim), rows, obs_dim)
    n = _gpu_stats([data], obs_dim)
    mean, var = n.mean.cpu().numpy(), n.var.cpu().numpy()
    assert_moments(mean, var, n.count, data)
    assert_float_form(n.norm.cpu().numpy(), mean, var)
    if obs_dim >= 5 and rows > 1:                              # the constant column
        assert var[4] <= 1e-12 * 9.0 and abs(n.norm[1, 4].item() - 1e4) <= np.spacing(np.float32(1e4))
    again = _gpu_stats([data], obs_dim)                        # the same input twice: the same bits
    assert torch.equal(again.state, n.state) and torch.equal(again.norm, n.norm)


def test_three_merges_equal_the_moments_of_the_concatenation_on_the_gpu():
    import torch
    data = columns(np.random.default_rng(3), 50_000, 25)
    n = _gpu_stats([data[:100], data[100:137], data[137:]], 25)
    mean, var = n.mean.cpu().numpy(), n.var.cpu().numpy()
    assert_moments(mean, var, n.count, data)
    assert_float_form(n.norm.cpu().numpy(), mean, var)
    before = (n.state.clone(), n.norm.clone())
    n.update(torch.zeros(0, 25, device="cuda"))               # no rows: nothing moves
    torch.cuda.synchronize()
    assert torch.equal(n.state, before[0]) and torch.equal(n.norm, before[1])


# ---- PPO end to end ----
def _tendon_agent(**kw):
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env = RoboyVecEnv(MsjRobot(), 512, seed=2, tendon_obs=("length", "force"))          # no tendon_obs_scale: newtons and metres
    return env, PPO(env, n_steps=8, seed=3, reward_scale=0.01, fused_policy=True, fused_update=True, normalize_obs=True, **kw)


def _round(agent):
    """one round; the stored log-probabilities and values are the torch policy's under the statistics the rollout ran with"""
    import torch
    roll = agent.collect()
    with torch.no_grad():
        lp = agent.policy.dist(roll["obs"]).log_prob(roll["act"]).sum(-1)
        v = agent.policy.value(roll["obs"])
    assert torch.isfinite(roll["act"]).all()
    assert (lp - roll["logp"]).abs().max().item() < 1e-4 * max(1.0, lp.abs().max().item())
    assert (v - roll["val"]).abs().max().item() < 1e-4 * max(1.0, v.abs().max().item())
    obs = roll["obs"].reshape(-1, roll["obs"].shape[-1]).cpu().numpy().copy()
    agent.update(roll)
    torch.cuda.synchronize()
    return obs


@pytest.mark.parametrize("mode", ["eager", "graph_one_chain", "graph_two_chains"])
def test_ppo_on_unscaled_tendon_channels(mode):
    import torch
    kw = {"eager": {}, "graph_one_chain": {"use_graphs": True, "rollout_chains": 1},
          "graph_two_chains": {"use_graphs": True, "rollout_chains": 2}}[mode]
    env, agent = _tendon_agent(**kw)
    assert env.observation_space.shape[0] == 25
    _round(agent)                                              # primes first: two rollouts, the second under new statistics
    assert agent.rollout_chains == (2 if mode == "graph_two_chains" else 1)
    n = agent.obs_norm
    assert n.count == 2 * 8 * 512 and agent.num_timesteps == 8 * 512
    assert not torch.equal(n.norm[0], torch.zeros_like(n.norm[0])) and not torch.equal(n.norm[1], torch.ones_like(n.norm[1]))
    obs2 = _round(agent)                                       # a replay reads the statistics merged since through the captured address
    assert n.count == 3 * 8 * 512
    assert np.abs(n.apply(torch.from_numpy(obs2).cuda()).cpu().numpy()).mean() < 3.0
    assert all(torch.isfinite(p).all() for p in agent.policy.parameters())
    if mode != "eager":
        # the same seed without graphs: the same statistics, to the moments bound
        env_e, eager = _tendon_agent()
        _round(eager); _round(eager)
        m, v = eager.obs_norm.mean.cpu().numpy(), eager.obs_norm.var.cpu().numpy()
        assert eager.obs_norm.count == n.count
        assert (np.abs(n.var.cpu().numpy() - v) <= 1e-8 * v + 1e-12 * m ** 2).all()
        assert (np.abs(n.mean.cpu().numpy() - m) <= 1e-8 * np.sqrt(v) + 1e-12 * np.abs(m)).all()
        env_e.close()
    env.close()


def _rank_main(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    env = RoboyVecEnv(MsjRobot(), 256, seed=0, env_id_offset=256 * rank, tendon_obs=("length", "force"))
    agent = PPO(env, n_steps=8, seed=5, dist=dist, reward_scale=0.01, fused_policy=True, fused_update=True, normalize_obs=True)
    for _ in range(2):
        roll = agent.collect()
        agent.update(roll)
    torch.cuda.synchronize()
    torch.save({"params": [p.detach().cpu() for p in agent.policy.parameters()], "act": roll["act"].cpu(),
                "state": agent.obs_norm.state.cpu(), "norm": agent.obs_norm.norm.cpu()}, os.path.join(out_dir, "r%d.pt" % rank))
    env.close()
    dist.destroy_process_group()


def test_two_ranks_hold_identical_statistics_and_parameters(tmp_path):
    """Two ranks (both on the one GPU, collectives over gloo), each a child process under its own time limit: own env shards and
    exploration noise, one all-reduce of the 1 + 2 obs_dim sums per merge - after two rounds parameters AND statistics are equal."""
    import socket
    import torch
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    flags = ["-s"] if sys.flags.no_user_site else []
    procs = [subprocess.Popen([sys.executable] + flags + ["-c", "import test_obs_norm_gpu as t; t._rank_main(%d, 2, %d, %r)"
                                                          % (rank, port, str(tmp_path))],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-4000:]
    a, b = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert (a["act"] - b["act"]).abs().max() > 0.1            # own noise per rank
    for p, q in zip(a["params"], b["params"]):
        assert torch.equal(p, q) and torch.isfinite(p).all()
    assert torch.equal(a["state"], b["state"]) and torch.equal(a["norm"], b["norm"])
    assert a["state"][-1].item() == 3 * 8 * 512              # priming + two rounds, both ranks' rows
