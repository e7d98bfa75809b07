"""Running return normalisation of the reward on the torch path (gym_roboy_amd/ppo.py: RewardNorm, PPO(normalize_reward=True)),
DESIGN.md §16, against tests/reward_norm_ref.py - a numpy per-step loop written from the definition.

Bounds: r~ is specified to the bit (two float32 products, the clamp last) and compared with ==.  The carried return: 4 T 2^-53 A, A the
same recurrence on |r_s| (the recurrence's a-priori rounding bound).  The statistics: the bound of tests/test_obs_norm_cpu.py (§15), 1e-8
relative on var and 1e-8 std on mean against numpy's two-pass float64 moments; the inputs keep the first batch's |mean| / std far below
30 (its sums are taken around the shift 0)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import reward_norm_ref as ref
from gym_roboy_amd._gymcompat import spaces
from gym_roboy_amd.ppo import PPO, RewardNorm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, SCALE = 0.99, 0.01


def raw_rewards(rng, T, N):
    """the env's reward: a few units of penalty, a goal bonus of 1000 on 1 % of the steps"""
    r = rng.normal(-1.0, 2.0, (T, N))
    return np.where(rng.random((T, N)) < 0.01, 1000.0, r).astype(np.float32)


def check_scan(rn, r_s, done, carry_in):
    """one scan() of the torch statement against the loop: the carry to its bound, the sums [n, S, SS] to 1e-12; -> the returns"""
    T = r_s.shape[0]
    mean = float(rn.state[0])
    rets, carry, A = ref.scan(r_s, done, rn.gamma, carry_in)
    sums = rn.scan(torch.from_numpy(r_s), torch.from_numpy(done)).numpy().copy()
    assert (np.abs(rn.ret_carry.numpy() - carry) <= ref.carry_bound(T, A)).all()
    d = rets - mean
    assert sums[0] == r_s.size
    assert abs(sums[1] - d.sum()) <= 1e-12 * np.abs(d).sum() and abs(sums[2] - (d * d).sum()) <= 1e-12 * (d * d).sum()
    return rets


@pytest.mark.parametrize("dones", ref.DONE_PATTERNS)
@pytest.mark.parametrize("T,N", [(1, 1), (5, 7), (37, 33)])
def test_scan_matches_the_numpy_loop(T, N, dones):
    rng = np.random.default_rng(T * 1000 + N)
    r_s, done = ref.scaled(raw_rewards(rng, T, N), SCALE), ref.done_pattern(dones, T, N, rng)
    carry_in = rng.normal(0.0, 3.0, N)                         # a non-zero incoming carry
    rn = RewardNorm(N, GAMMA)
    rn.ret_carry.copy_(torch.from_numpy(carry_in))
    rets = check_scan(rn, r_s, done, carry_in)
    if dones == "all":
        assert (rn.ret_carry == 0).all()
    elif dones == "first_step" and T > 1:
        assert (rn.ret_carry != 0).all()                       # update, THEN zero: the first step's return went into the sums
    rn.update()
    ref.assert_return_moments(float(rn.mean), float(rn.var), rn.count, [rets])
    assert rn.norm[1, 0].item() == ref.rstd_of(float(rn.var)) and rn.norm[0, 0].item() == np.float32(float(rn.mean))


def test_two_rollouts_carry_the_return_across_the_boundary():
    T, N = 16, 33
    rng = np.random.default_rng(2)
    r_s, done = ref.scaled(raw_rewards(rng, 2 * T, N), SCALE), ref.done_pattern("random", 2 * T, N, rng)
    rn = RewardNorm(N, GAMMA)
    first = check_scan(rn, r_s[:T], done[:T], np.zeros(N))
    rn.update()
    assert float(rn.mean) != 0.0                               # the second rollout's sums are taken around a shift
    mid = rn.ret_carry.numpy().copy()
    assert (mid != 0).any()
    second = check_scan(rn, r_s[T:], done[T:], mid)
    rn.update()
    whole, carry, A = ref.scan(r_s, done, GAMMA, np.zeros(N))  # the two halves are ONE run of the recurrence
    assert (np.abs(np.concatenate([first, second]) - whole) <= ref.carry_bound(2 * T, np.abs(whole) + 1.0)).all()
    assert (np.abs(rn.ret_carry.numpy() - carry) <= ref.carry_bound(2 * T, A)).all()
    ref.assert_return_moments(float(rn.mean), float(rn.var), rn.count, [whole])
    rn.reset_returns()
    assert (rn.ret_carry == 0).all()


@pytest.mark.parametrize("clip", [10.0, 0.5, float("inf")])
def test_normalised_reward_is_the_two_float32_products_then_the_clamp(clip):
    rng = np.random.default_rng(4)
    raw = raw_rewards(rng, 64, 65)
    rn = RewardNorm(65, GAMMA, clip=clip)
    rn.norm[1] = 17.0
    r_s = ref.scaled(raw, SCALE)
    want = ref.normalised(r_s, np.float32(17.0), clip)
    got = rn.apply(torch.from_numpy(raw) * SCALE)              # (the agent's own product: a float32 tensor times a Python number)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    if clip == float("inf"):
        assert np.array_equal(want, r_s * np.float32(17.0)) and want.max() > 10.0
    else:
        assert (want == np.float32(clip)).any() and ((want == -np.float32(clip)).any() or clip == 10.0)
    if clip == 0.5:
        assert (want == -np.float32(0.5)).any() and (np.abs(want) < 0.5).any()      # the clamp active on both sides


def test_empty_statistics_are_the_identity_and_no_returns_change_nothing():
    rn = RewardNorm(3, GAMMA)
    assert rn.count == 0 and rn.norm[0, 0].item() == 0.0 and rn.norm[1, 0].item() == 1.0
    r = torch.tensor([[0.3, -2.0, 9.9]])
    assert torch.equal(rn.apply(r), r)
    rn.update()                                                # sums of no returns (n == 0)
    assert rn.count == 0 and torch.equal(rn.norm, torch.tensor([[0.0], [1.0]]))
    rn.scan(r, torch.zeros(1, 3))
    rn.update()
    before = (rn.state.clone(), rn.norm.clone())
    rn.sums.zero_()
    rn.update()
    assert torch.equal(rn.state, before[0]) and torch.equal(rn.norm, before[1]) and rn.count == 3
    with pytest.raises(ValueError):
        RewardNorm(3, GAMMA, clip=0.0)
    with pytest.raises(ValueError):
        RewardNorm(3, 1.5)


def test_state_dict_round_trip():
    rng = np.random.default_rng(5)
    rn = RewardNorm(9, GAMMA, clip=3.0)
    rn.scan(torch.from_numpy(ref.scaled(raw_rewards(rng, 20, 9), SCALE)), torch.zeros(20, 9))
    rn.update()
    sd = rn.state_dict()
    assert set(sd) == {"mean", "var", "count", "clip", "eps", "gamma"}
    other = RewardNorm(4, GAMMA)                               # (the statistics do not depend on the batch's size)
    other.load_state_dict(sd)
    assert torch.equal(other.state, rn.state) and torch.equal(other.norm, rn.norm) and other.clip == 3.0 and other.eps == rn.eps
    assert (other.ret_carry == 0).all()                        # the running returns are not stored
    with pytest.raises(ValueError, match="gamma"):
        RewardNorm(4, 0.9).load_state_dict(sd)


# ---- PPO end to end on a stand-in env ----
class EpisodicVecEnv:
    """Random rewards of the env's spread, episodes that end at random (10 % of the steps)."""

    def __init__(self, n, seed=0):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.observation_space = spaces.Box(low=-10, high=10, shape=(3,), dtype="float32")
        self.action_space = spaces.Box(low=-1, high=1, shape=(2,), dtype="float32")

    def reset(self):
        return self.rng.standard_normal((self.n, 3)).astype(np.float32)

    def step(self, a):
        return self.reset(), raw_rewards(self.rng, 1, self.n)[0], self.rng.random(self.n) < 0.1, [{}] * self.n


def _agent(normalize=True, prime=False, seed=1, **kw):
    return PPO(EpisodicVecEnv(16, seed), n_steps=8, device="cpu", seed=seed, reward_scale=SCALE, normalize_reward=normalize,
               reward_norm_prime=prime, **kw)


def _check_round(agent, carry_in):
    """one collect(): roll["rew"] to the bit under the statistics frozen through it, the carry to its bound; -> (returns, carry)"""
    frozen = agent.reward_norm.norm.clone()
    roll = agent.collect()
    raw, done = agent._rew_raw.numpy(), roll["done"].numpy()
    r_s = ref.scaled(raw, SCALE)
    assert np.array_equal(roll["rew"].numpy(), ref.normalised(r_s, frozen[1, 0].item(), agent.reward_norm.clip))
    rets, carry, A = ref.scan(r_s, done, agent.gamma, carry_in)
    assert (np.abs(agent.reward_norm.ret_carry.numpy() - carry) <= ref.carry_bound(8, A)).all()
    assert not torch.equal(agent.reward_norm.norm, frozen)     # merged at the end of collect()
    return roll, rets, carry


def test_statistics_after_two_rounds_are_the_moments_of_the_returns():
    agent = _agent()
    assert torch.equal(agent.reward_norm.norm, torch.tensor([[0.0], [1.0]]))
    roll, r1, carry = _check_round(agent, np.zeros(16))
    agent.update(roll)
    roll, r2, carry = _check_round(agent, carry)
    n = agent.reward_norm
    ref.assert_return_moments(float(n.mean), float(n.var), n.count, [r1, r2])
    assert agent.num_timesteps == 2 * 8 * 16
    # GAE ran on the normalised reward
    from gym_roboy_amd.ppo import gae
    with torch.no_grad():
        adv, ret = gae(roll["rew"], roll["val"], roll["done"], agent.policy.value(agent._obs), agent.gamma, agent.lam)
    assert torch.equal(adv, roll["adv"]) and torch.equal(ret, roll["ret"])


def test_priming_runs_one_uncounted_rollout_for_both_sets_of_statistics():
    agent = _agent(prime=True, normalize_obs=True)
    agent.collect()
    # primed: the priming rollout is not counted; its returns and the returned rollout's are merged, its observations too
    assert agent.num_timesteps == 8 * 16 and agent.reward_norm.count == 2 * 8 * 16 and agent.obs_norm.count == 8 * 16
    agent.collect()
    assert agent.num_timesteps == 2 * 8 * 16 and agent.reward_norm.count == 3 * 8 * 16          # primes once
    only = _agent(prime=True)                                  # without observation statistics the rule is the same
    only.collect()
    assert only.num_timesteps == 8 * 16 and only.reward_norm.count == 2 * 8 * 16
    off = _agent(prime=False)
    off.collect()
    assert off.num_timesteps == 8 * 16 and off.reward_norm.count == 8 * 16


def test_without_the_option_nothing_is_there():
    agent = _agent(normalize=False)
    roll = agent.collect()
    assert agent.reward_norm is None and agent._rew_raw is None and set(roll) == {"obs", "act", "logp", "val", "rew", "done", "adv", "ret"}


def test_checkpoints_carry_the_statistics_and_refuse_a_mismatch(tmp_path):
    agent = _agent(clip_reward=5.0)
    agent.update(agent.collect())
    path = str(tmp_path / "model.pkl")
    agent.save(path)
    ck = torch.load(path)
    assert set(ck["reward_norm"]) == {"mean", "var", "count", "clip", "eps", "gamma"} and ck["reward_norm"]["clip"] == 5.0
    other = _agent(seed=2, prime=True)
    other.collect()
    assert (other.reward_norm.ret_carry != 0).any()
    other.load(path)
    assert torch.equal(other.reward_norm.state, agent.reward_norm.state) and torch.equal(other.reward_norm.norm, agent.reward_norm.norm)
    assert other.reward_norm.clip == 5.0 and (other.reward_norm.ret_carry == 0).all()
    fresh = _agent(seed=3, prime=True).load(path)
    fresh.collect()
    assert fresh.reward_norm.count == agent.reward_norm.count + 8 * 16          # loaded statistics: no priming
    with pytest.raises(ValueError, match="with reward normalisation, this agent runs without"):
        _agent(normalize=False).load(path)
    plain = _agent(normalize=False)
    plain_path = str(tmp_path / "plain.pkl")
    plain.save(plain_path)
    assert torch.load(plain_path)["reward_norm"] is None
    with pytest.raises(ValueError, match="without reward normalisation, this agent runs with"):
        _agent().load(plain_path)
    old = torch.load(plain_path)                               # a checkpoint written before the key existed
    del old["reward_norm"]
    torch.save(old, plain_path)
    _agent(normalize=False).load(plain_path)
    with pytest.raises(ValueError, match="reward normalisation"):
        _agent().load(plain_path)


def test_learn_reports_the_raw_mean_reward():
    agent = _agent()
    logs = []
    agent.learn(2 * 8 * 16, log=logs.append)
    assert len(logs) == 2
    raw_mean = agent._rew_raw.mean().item()
    assert logs[-1]["mean_reward"] == raw_mean and 0.1 < abs(raw_mean) < 30.0   # the env's scale (-1, and a rare bonus of 1000)
    assert abs(logs[0]["mean_reward"]) > 0.1 and logs[0]["timesteps"] == 8 * 16


def test_cli_parses_and_forwards_the_options(tmp_path, monkeypatch):
    import gym_roboy_amd.envs.vec_env as vec_env
    import gym_roboy_amd.ppo as ppo
    import gym_roboy_amd.train_parallel as tp
    seen = {}

    class Stop(Exception):
        pass

    def fake_ppo(env, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(vec_env, "RoboyVecEnv", lambda *a, **kw: object())
    monkeypatch.setattr(ppo, "PPO", fake_ppo)
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path), "--normalize-reward", "--clip-reward", "7.5"])
    assert seen["normalize_reward"] is True and seen["clip_reward"] == 7.5 and seen["reward_scale"] == 0.01
    seen.clear()
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path)])
    assert seen["normalize_reward"] is False and seen["clip_reward"] == 10.0 and seen["reward_scale"] == 0.01


# ---- two ranks over gloo ----
R_T, R_N, R_SEED = 16, 66, 9


def _rank_data():
    rng = np.random.default_rng(R_SEED)
    return [(ref.scaled(raw_rewards(rng, R_T, R_N), SCALE), ref.done_pattern("random", R_T, R_N, rng)) for _ in range(2)]


def _worker(rank, world, port, out_dir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = rank * R_N // world, (rank + 1) * R_N // world
    rn = RewardNorm(hi - lo, GAMMA)
    for r_s, done in _rank_data():                             # two rollouts of this rank's envs
        rn.scan(torch.from_numpy(r_s[:, lo:hi].copy()), torch.from_numpy(done[:, lo:hi].copy()))
        rn.update(dist)
    torch.save({"state": rn.state, "norm": rn.norm}, os.path.join(out_dir, "r%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_hold_identical_statistics_of_all_returns(tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert torch.equal(a["state"], b["state"]) and torch.equal(a["norm"], b["norm"])          # bit-identical on every rank
    carry, rets = np.zeros(R_N), []
    for r_s, done in _rank_data():
        r, carry, _ = ref.scan(r_s, done, GAMMA, carry)
        rets.append(r)
    state = a["state"].numpy()
    ref.assert_return_moments(state[0], state[1], state[2], rets)
    assert a["norm"][1, 0].item() == ref.rstd_of(state[1])
