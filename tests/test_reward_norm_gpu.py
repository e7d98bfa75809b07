"""The rollout's tail under running return normalisation of the reward as one kernel (csrc/mlp_update.hip: rollout_tail_kernel,
include/roboy_policy.h: rp_rollout_tail_dev) against tests/reward_norm_ref.py, and PPO(normalize_reward=True) end to end.

Bounds.  rew and done: specified to the bit, compared with ==.  ret_carry: 4 T 2^-53 A, A the recurrence on |r_s| (its a-priori
rounding bound, with either contraction choice).  adv / ret: the rule of tests/test_policy_scale_gpu.py::test_gae_matches_float64 - at
most 4 x the CPU float32 loop's distance from float64, floor 1e-6 max |ref| - both fed the same r~.  The raw sums [n, S, SS]: a sum of n
float64 terms in ANY order is within n 2^-53 sum |term| of the exact one (the terms themselves carry the carry's bound, far below
it).  The merged statistics: 1e-8 relative on var, 1e-8 std on mean against numpy's two-pass moments."""
import ctypes

import numpy as np
import pytest

import reward_norm_ref as ref
from test_reward_norm_cpu import raw_rewards

pytestmark = pytest.mark.gpu

GAMMA, LAM, SCALE = 0.99, 0.95, 0.01
SENTINEL, PAD = -7777.0, 64
SHAPES = [(1, 1), (1, 65), (2, 64), (5, 257), (37, 1000), (128, 4097)]


def _padded(T, N):
    """a [T, N] float32 view of a sentinel-filled device buffer with PAD more elements behind it"""
    import torch
    flat = torch.full((T * N + PAD,), SENTINEL, device="cuda")
    return flat, flat[:T * N].view(T, N)


def _tail(rn, raw, done_i, val, last, scale=SCALE, lam=LAM):
    """RewardNorm.tail into padded outputs -> {rew, done, adv, ret} as numpy, nothing written past the arrays"""
    import torch
    T, N = raw.shape
    bufs = {k: _padded(T, N) for k in ("rew", "done", "adv", "ret")}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rn.tail(dev(raw), dev(done_i), dev(val), dev(last), scale, lam, *[bufs[k][1] for k in ("rew", "done", "adv", "ret")])
    torch.cuda.synchronize()
    for flat, _ in bufs.values():
        assert (flat[T * N:] == SENTINEL).all()
    return {k: v[1].cpu().numpy() for k, v in bufs.items()}


def _assert_gae(out, r_tilde, val, done_i, last, what=""):
    """adv / ret under the rule of test_gae_matches_float64, the float64 statement and the CPU float32 loop fed the same r~"""
    import torch
    from gym_roboy_amd.ppo import gae
    from oracle.policy_ref import gae64
    done = done_i.astype(np.float32)
    adv_ref, ret_ref = gae64(r_tilde, val, done, last, GAMMA, LAM)
    a32, r32 = gae(torch.from_numpy(r_tilde), torch.from_numpy(val), torch.from_numpy(done), torch.from_numpy(last), GAMMA, LAM)
    for name, got, f32, want in (("adv", out["adv"], a32, adv_ref), ("ret", out["ret"], r32, ret_ref)):
        e32 = np.abs(f32.double().numpy() - want).max()
        err = np.abs(got.astype(np.float64) - want).max()
        print("%s %s: fp32 loop %.3g, kernel %.3g, max |ref| %.3g" % (what, name, e32, err, np.abs(want).max()))
        assert err <= max(4.0 * e32, 1e-6 * np.abs(want).max()), (name, err, e32)


def _assert_sums(sums, rets, shift):
    d = rets.reshape(-1) - shift
    n = d.size
    u = 2.0 ** -53
    assert sums[0] == n
    print("sums: S off by %.3g of %.3g, SS by %.3g of %.3g" % (abs(sums[1] - d.sum()), n * u * np.abs(d).sum(),
                                                               abs(sums[2] - (d * d).sum()), (n + 2) * u * (d * d).sum()))
    assert abs(sums[1] - d.sum()) <= 2 * n * u * np.abs(d).sum()            # (numpy's own pairwise sum is within the same bound)
    assert abs(sums[2] - (d * d).sum()) <= 2 * (n + 2) * u * (d * d).sum()


def _case(T, N, dones, seed):
    rng = np.random.default_rng(seed)
    raw, done_i = raw_rewards(rng, T, N), ref.done_pattern(dones, T, N, rng)
    val, last = rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    return raw, done_i, val, last


@pytest.mark.parametrize("dones", ref.DONE_PATTERNS)
@pytest.mark.parametrize("T,N", SHAPES)
def test_kernel_matches_the_reference_over_two_rollouts(T, N, dones):
    """Two successive launches on one RewardNorm: the first under the identity from a non-zero carry, the second under the statistics
    merged from the first (a shift and an rstd) with the carry crossing the boundary; the clamp sits at 0.02 rstd - two spreads of
    the scaled penalty - so that it cuts both sides and leaves an interior."""
    _two_rollouts(T, N, dones, 256)


def _two_rollouts(T, N, dones, per_block):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import RewardNorm
    if N > per_block:
        assert pn.load().rp_rollout_tail_blocks(T, N) == (N + per_block - 1) // per_block > 1          # more than one workgroup: the ticket
    rn = RewardNorm(N, GAMMA, "cuda", clip=0.5)
    rng = np.random.default_rng(T + N)
    carry = rng.normal(0.0, 3.0, N)
    rn.ret_carry.copy_(torch.from_numpy(carry))
    all_rets = []
    for k in range(2):
        raw, done_i, val, last = _case(T, N, dones, 1000 * T + N + k)
        shift, rstd = float(rn.state[0].item()), rn.norm[1, 0].item()
        assert (k == 0) == (shift == 0.0 and rstd == 1.0)
        rn.clip = clip = float(np.float32(0.02) * np.float32(rstd))
        out = _tail(rn, raw, done_i, val, last)
        r_s = ref.scaled(raw, SCALE)
        r_tilde = ref.normalised(r_s, rstd, clip)
        if T * N >= 1000:
            assert (r_tilde == np.float32(clip)).any() and (r_tilde == -np.float32(clip)).any() and (np.abs(r_tilde) < clip).any()
        assert np.array_equal(out["rew"], r_tilde) and np.array_equal(out["done"], done_i.astype(np.float32))
        rets, carry, A = ref.scan(r_s, done_i, GAMMA, carry)
        assert (np.abs(rn.ret_carry.cpu().numpy() - carry) <= ref.carry_bound(T, A)).all()
        _assert_gae(out, r_tilde, val, done_i, last, "(%d, %d) %s #%d" % (T, N, dones, k))
        _assert_sums(rn.sums.cpu().numpy(), rets, shift)
        all_rets.append(rets)
        rn.update()
        torch.cuda.synchronize()
    state = rn.state.cpu().numpy()
    ref.assert_return_moments(state[0], state[1], state[2], all_rets)
    want = np.array([[np.float32(state[0])], [ref.rstd_of(state[1])]])
    assert (np.abs(rn.norm.cpu().numpy() - want) <= np.spacing(np.abs(want))).all()


def _raw_call(lib, raw, done_i, val, last, carry, scratch, norm2=None, shift=None, clip=10.0, gamma=GAMMA, n_steps=None, outs=None):
    """rp_rollout_tail_dev itself (device tensors; None = a null pointer) -> (return code, rew, done, adv, ret, sums)"""
    import torch
    T, N = val.shape
    outs = outs or [torch.empty(T, N, device="cuda") for _ in range(4)]
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = lib.rp_rollout_tail_dev(ptr(raw), ptr(done_i), ptr(val), ptr(last), SCALE, ptr(norm2), clip, ptr(shift), gamma, LAM, ptr(carry),
                                 *[ptr(o) for o in outs], ptr(sums), ptr(scratch), T if n_steps is None else n_steps, N,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (rc, *outs, sums)


def _scratch(lib):
    import torch
    return torch.zeros(int(lib.rp_rollout_tail_scratch_doubles()), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("T,N", [(1, 65), (37, 1000), (128, 4097)])
def test_identity_statistics_give_the_parents_tail(T, N):
    """No statistics (null pointers) and no clamp: rew is rew_raw * scale to the bit, adv / ret are what rp_gae_dev makes of it."""
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import gae_fused
    lib = pn.load()
    raw, done_i, val, last = [torch.from_numpy(a).cuda() for a in _case(T, N, "random", T * N)]
    carry = torch.zeros(N, dtype=torch.float64, device="cuda")
    rc, rew, done, adv, ret, sums = _raw_call(lib, raw, done_i, val, last, carry, _scratch(lib), clip=float("inf"))
    assert rc == 0
    assert torch.equal(rew, raw * SCALE) and torch.equal(done, done_i.to(torch.float32))
    a, r = gae_fused(rew, val, done, last, GAMMA, LAM)
    torch.cuda.synchronize()
    out = {"adv": adv.cpu().numpy(), "ret": ret.cpu().numpy()}
    _assert_gae(out, rew.cpu().numpy(), val.cpu().numpy(), done_i.cpu().numpy(), last.cpu().numpy(), "identity (%d, %d)" % (T, N))
    _assert_gae({"adv": a.cpu().numpy(), "ret": r.cpu().numpy()}, rew.cpu().numpy(), val.cpu().numpy(), done_i.cpu().numpy(),
                last.cpu().numpy(), "rp_gae_dev (%d, %d)" % (T, N))
    # identity statistics given explicitly are the same launch
    norm2 = torch.tensor([[0.0], [1.0]], device="cuda")
    rc, rew2, done2, adv2, ret2, sums2 = _raw_call(lib, raw, done_i, val, last, torch.zeros_like(carry), _scratch(lib), norm2=norm2,
                                                   shift=torch.zeros(1, dtype=torch.float64, device="cuda"), clip=float("inf"))
    assert rc == 0 and all(torch.equal(x, y) for x, y in ((rew, rew2), (done, done2), (adv, adv2), (ret, ret2), (sums, sums2)))


def test_sums_are_reproducible_and_the_scratch_is_reusable():
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    T, N = 37, 4097
    scratch = _scratch(lib)
    case = [torch.from_numpy(a).cuda() for a in _case(T, N, "random", 5)]
    carry_in = torch.from_numpy(np.random.default_rng(5).normal(0.0, 3.0, N)).cuda()
    runs = [_raw_call(lib, *case, carry_in.clone(), scratch) for _ in range(3)]          # three launches on ONE scratch
    assert all(r[0] == 0 for r in runs)
    for r in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(r[1:], runs[0][1:]))                # every output, the sums included, to the bit
    # other inputs, another grid, the same scratch: right, so the ticket was reset
    T2, N2 = 5, 1000
    raw, done_i, val, last = _case(T2, N2, "random", 6)
    carry = torch.zeros(N2, dtype=torch.float64, device="cuda")
    rc, rew, done, adv, ret, sums = _raw_call(lib, *[torch.from_numpy(a).cuda() for a in (raw, done_i, val, last)], carry, scratch)
    rets, carry_ref, A = ref.scan(ref.scaled(raw, SCALE), done_i, GAMMA, np.zeros(N2))
    assert rc == 0
    _assert_sums(sums.cpu().numpy(), rets, 0.0)
    assert (np.abs(carry.cpu().numpy() - carry_ref) <= ref.carry_bound(T2, A)).all()


def test_sums_around_a_shift_far_from_zero():
    """Returns near 1e3 +- 1 with the shift at 1e3: the moments of the batch come out of the shifted sums to the statistics' bound
    (unshifted, SS would cancel seven digits)."""
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    T, N = 16, 4097
    rng = np.random.default_rng(8)
    raw = (rng.normal(0.0, 10.0, (T, N)) + 1000.0).astype(np.float32)                    # r_s near 10: what gamma = 0.99 takes from 1e3
    done_i = np.zeros((T, N), np.int32)
    val, last = np.zeros((T, N), np.float32), np.zeros(N, np.float32)
    carry_in = rng.normal(1000.0, 1.0, N)
    carry = torch.from_numpy(carry_in).cuda()
    shift = torch.tensor([1000.0], dtype=torch.float64, device="cuda")
    rc, _, _, _, _, sums = _raw_call(lib, *[torch.from_numpy(a).cuda() for a in (raw, done_i, val, last)], carry, _scratch(lib), shift=shift)
    assert rc == 0
    rets, carry_ref, A = ref.scan(ref.scaled(raw, SCALE), done_i, GAMMA, carry_in)
    assert abs(rets.mean() - 1000.0) < 1.0 and 0.3 < rets.std() < 3.0
    s = sums.cpu().numpy()
    _assert_sums(s, rets, 1000.0)
    mean, var = 1000.0 + s[1] / s[0], s[2] / s[0] - (s[1] / s[0]) ** 2
    assert abs(var - rets.var()) <= 1e-8 * rets.var() and abs(mean - rets.mean()) <= 1e-8 * rets.std()
    assert (np.abs(carry.cpu().numpy() - carry_ref) <= ref.carry_bound(T, A)).all()


def test_argument_errors_are_codes():
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    T, N = 5, 65
    raw, done_i, val, last = [torch.from_numpy(a).cuda() for a in _case(T, N, "random", 9)]
    carry, scratch = torch.zeros(N, dtype=torch.float64, device="cuda"), _scratch(lib)
    marks = [torch.full((T, N), SENTINEL, device="cuda") for _ in range(4)]
    for kw, word in (({"clip": 0.0}, b"clip"), ({"clip": float("nan")}, b"clip"), ({"n_steps": 0}, b"n_steps"), ({"gamma": 1.5}, b"gamma"),
                     ({"gamma": -0.1}, b"gamma")):
        assert _raw_call(lib, raw, done_i, val, last, carry, scratch, outs=marks, **kw)[0] == -1
        assert word in lib.rp_last_error()
    assert _raw_call(lib, None, done_i, val, last, carry, scratch, outs=marks)[0] == -1 and b"null" in lib.rp_last_error()
    assert _raw_call(lib, raw, done_i, val, last, carry, None, outs=marks)[0] == -1
    assert _raw_call(lib, raw, done_i, val, last, None, scratch, outs=marks)[0] == -1
    assert lib.rp_rollout_tail_blocks(0, 5) == -1 and lib.rp_rollout_tail_blocks(5, 0) == -1 and lib.rp_rollout_tail_blocks(5, 1 << 26) < 0
    assert lib.rp_rollout_tail_blocks(128, 262144) == 1024
    assert lib.rp_rollout_tail_blocks(128, 1 << 21) == 4096 and lib.rp_rollout_tail_scratch_doubles() >= 2 * 4096 + 1
    assert all((m == SENTINEL).all() for m in marks) and (carry == 0).all()              # nothing was launched
    assert _raw_call(lib, raw, done_i, val, last, carry, scratch)[0] == 0                 # and the next call runs


# ---- PPO end to end ----
def _record_rollouts(agent):
    """Every rollout collect() runs - the priming one too - leaves what the reference needs: the statistics it ran under, the agent's
    own raw buffers, its outputs, the carried returns behind it."""
    import torch
    log, inner = [], agent._collect_rollout

    def wrapped():
        frozen = agent.reward_norm.norm.clone()
        roll = inner()
        torch.cuda.synchronize()
        b, T = agent._rb, agent.n_steps
        with torch.no_grad():
            last = agent.policy.value(b["obs"][T])
        log.append({"rstd": frozen[1, 0].item(), "last": last.cpu().numpy(), "carry": agent.reward_norm.ret_carry.cpu().numpy().copy(),
                    **{k: b[k].cpu().numpy().copy() for k in ("rew_raw", "done_i", "val", "rew", "done", "adv", "ret")}})
        return roll

    agent._collect_rollout = wrapped
    return log


@pytest.mark.parametrize("mode", ["one_chain", "two_chains", "with_obs_norm", "torch_policy"])
def test_ppo_with_reward_normalisation(mode):
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    kw = {"one_chain": {"rollout_chains": 1}, "two_chains": {"rollout_chains": 2}, "with_obs_norm": {"normalize_obs": True},
          "torch_policy": {}}[mode]
    fused = mode != "torch_policy"
    env = RoboyVecEnv(MsjRobot(), 512, max_episode_length=5)
    agent = PPO(env, n_steps=8, use_graphs=True, fused_policy=fused, fused_update=fused, normalize_reward=True, reward_scale=SCALE, **kw)
    log = _record_rollouts(agent)
    T, N = 8, 512
    carry, rets, seen = np.zeros(N), [], 0
    for rnd in range(3):
        roll = agent.collect()
        assert len(log) == rnd + 2                             # ONE priming rollout, whichever statistics asked for it
        assert agent.rollout_chains == (2 if mode == "two_chains" else 1)
        for rec in log[seen:]:
            assert rec["done_i"].any() and not rec["done_i"].all()                       # episodes end inside every rollout
            r_s = ref.scaled(rec["rew_raw"], SCALE)
            r_tilde = ref.normalised(r_s, rec["rstd"], 10.0)
            assert np.array_equal(rec["rew"], r_tilde) and np.array_equal(rec["done"], rec["done_i"].astype(np.float32))
            r, carry, A = ref.scan(r_s, rec["done_i"], agent.gamma, carry)
            assert (np.abs(rec["carry"] - carry) <= ref.carry_bound(T, A)).all()
            _assert_gae(rec, r_tilde, rec["val"], rec["done_i"], rec["last"], "%s round %d" % (mode, rnd))
            rets.append(r)
        seen = len(log)
        assert log[0]["rstd"] == 1.0 and log[1]["rstd"] != 1.0                           # primed under the identity, then normalised
        assert np.array_equal(roll["rew"].cpu().numpy(), log[-1]["rew"])
        state = agent.reward_norm.state.cpu().numpy()
        ref.assert_return_moments(state[0], state[1], state[2], rets)
        assert agent.num_timesteps == (rnd + 1) * T * N and state[2] == (rnd + 2) * T * N      # the priming rollout is not counted
        if mode == "with_obs_norm":
            assert agent.obs_norm.count == (rnd + 1) * T * N                             # the same priming rollout, then one merge per update
        agent.update(roll)
        torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in agent.policy.parameters())
    env.close()
