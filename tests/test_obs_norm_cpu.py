"""Running observation normalisation on the torch path (gym_roboy_amd/ppo.py: ObsNorm, MlpPolicy.set_obs_norm, PPO(normalize_obs=True)):
the float64 restatement of the shifted sums against numpy's two-pass moments, and PPO end to end on a stand-in env.

The bound on the statistics: sums taken around a shift that is delta away from the batch mean lose a factor
(1 + delta^2 / sigma^2) in the variance; in fp64 over at most 1e7 rows that is a relative error near 1e-9.  Asserted: 1e-8 relative on
var with an absolute floor of 1e-12 (delta^2 + sigma^2) for the constant column, 1e-8 std on mean with that column's floor 1e-12 delta,
1 ulp of float32 on the emitted float form."""
import numpy as np
import pytest
import torch

from gym_roboy_amd._gymcompat import spaces
from gym_roboy_amd.ppo import PPO, MlpPolicy, ObsNorm


def columns(rng, rows, obs_dim):
    """float32 [rows, obs_dim]: offsets and spreads that differ by orders of magnitude; column 0 (when there is more than one column
    it moves to 1) |mean| = 1e3 std - far from the initial shift 0; a constant column."""
    means = np.resize(np.array([3000.0, 0.0, 0.2, 400.0, -3.0]), obs_dim)
    stds = np.resize(np.array([3.0, 1.0, 0.01, 50.0, 0.0]), obs_dim)
    return (rng.standard_normal((rows, obs_dim)) * stds + means).astype(np.float32)


def assert_moments(mean, var, count, data):
    """mean / var / count (float64 arrays) against numpy's two-pass float64 moments of the float32 data, to the bound above.  The
    absolute floor is the constant columns' alone (their two-pass variance is exactly 0; delta = their distance from the shift 0):
    every other column is held to the relative bound."""
    x = data.astype(np.float64)
    m, v = x.mean(0), x.var(0)
    const = (v == 0.0).astype(np.float64)
    assert count == data.shape[0]
    err_v, err_m = np.abs(var - v), np.abs(mean - m)
    assert (err_v <= 1e-8 * v + const * 1e-12 * m ** 2).all(), (err_v, v)
    assert (err_m <= 1e-8 * np.sqrt(v) + const * 1e-12 * np.abs(m)).all(), (err_m, np.sqrt(v))


def assert_float_form(norm, mean, var, eps=1e-8):
    """the emitted float32 [2, obs_dim] against the float64 state, to 1 ulp"""
    want = np.stack([mean, 1.0 / np.sqrt(var + eps)]).astype(np.float32)
    assert (np.abs(norm - want) <= np.spacing(np.abs(want))).all(), (norm, want)


@pytest.mark.parametrize("obs_dim", [1, 9, 25, 95])
@pytest.mark.parametrize("rows", [1, 63, 4097])
def test_torch_statement_matches_numpy_two_pass(obs_dim, rows):
    data = columns(np.random.default_rng(rows + obs_dim), rows, obs_dim)
    n = ObsNorm(obs_dim)
    assert n.count == 0 and torch.equal(n.norm[0], torch.zeros(obs_dim)) and torch.equal(n.norm[1], torch.ones(obs_dim))
    n.update(torch.from_numpy(data))
    assert_moments(n.mean.numpy(), n.var.numpy(), n.count, data)
    assert_float_form(n.norm.numpy(), n.mean.numpy(), n.var.numpy())
    if obs_dim >= 5 and rows > 1:
        assert n.var[4] <= 1e-12 * 9.0 and abs(n.norm[1, 4].item() - 1e4) <= np.spacing(np.float32(1e4))     # the constant column


def test_three_merges_equal_the_moments_of_the_concatenation():
    data = columns(np.random.default_rng(3), 5000, 9)
    n = ObsNorm(9)
    for lo, hi in ((0, 100), (100, 137), (137, 5000)):
        n.update(torch.from_numpy(data[lo:hi]))
    assert_moments(n.mean.numpy(), n.var.numpy(), n.count, data)
    assert_float_form(n.norm.numpy(), n.mean.numpy(), n.var.numpy())
    before = (n.state.clone(), n.norm.clone())
    n.update(torch.zeros(0, 9))                                   # no rows: nothing moves
    assert torch.equal(n.state, before[0]) and torch.equal(n.norm, before[1])


def test_state_dict_round_trip_and_apply():
    data = columns(np.random.default_rng(5), 300, 9)
    n = ObsNorm(9, clip=2.0)
    n.update(torch.from_numpy(data))
    m = ObsNorm(9)
    m.load_state_dict(n.state_dict())
    assert torch.equal(m.state, n.state) and torch.equal(m.norm, n.norm) and m.clip == 2.0 and m.eps == n.eps
    # apply() is the spec's formula in float32: difference and product each rounded once, the clamp last
    x = data[:50]
    want = np.clip((x - n.norm[0].numpy()) * n.norm[1].numpy(), np.float32(-2.0), np.float32(2.0))
    assert np.array_equal(n.apply(torch.from_numpy(x)).numpy(), want)
    with pytest.raises(ValueError):
        ObsNorm(8).load_state_dict(n.state_dict())


def test_policy_without_statistics_is_the_parents_formula_and_keeps_its_keys():
    torch.manual_seed(0)
    p = MlpPolicy(9, 8)
    obs = torch.randn(33, 9) * 5
    assert p.obs_norm is None
    assert torch.equal(p.dist(obs).mean, p.pi(obs)) and torch.equal(p.value(obs), p.vf(obs).squeeze(-1))
    keys = set(p.state_dict())
    n = ObsNorm(9, clip=1.5)
    n.update(obs)
    p.set_obs_norm(n)
    assert set(p.state_dict()) == keys and len(list(p.buffers())) == 0
    x = ((obs - n.norm[0]) * n.norm[1]).clamp(-1.5, 1.5)
    assert torch.equal(p.dist(obs).mean, p.pi(x)) and torch.equal(p.value(obs), p.vf(x).squeeze(-1))
    assert (x.abs() == 1.5).any()
    # no gradient into the statistics
    p.dist(obs).mean.sum().backward()
    assert n.norm.grad is None and not n.norm.requires_grad
    p.set_obs_norm(None)
    assert torch.equal(p.dist(obs).mean, p.pi(obs))


class WideVecEnv:
    """A stand-in env whose observation columns differ by orders of magnitude (a drifting random walk per column)."""
    SCALE = np.array([1.0, 0.01, 400.0], np.float32)
    OFFSET = np.array([0.0, 0.2, 300.0], np.float32)

    def __init__(self, n, seed=0):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.observation_space = spaces.Box(low=-1e4, high=1e4, shape=(3,), dtype="float32")
        self.action_space = spaces.Box(low=-1, high=1, shape=(2,), dtype="float32")

    def _obs(self):
        return (self.z * self.SCALE + self.OFFSET).astype(np.float32)

    def reset(self):
        self.z = self.rng.standard_normal((self.n, 3)).astype(np.float32)
        return self._obs()

    def step(self, a):
        self.z = (0.9 * self.z + 0.3 * self.rng.standard_normal((self.n, 3))).astype(np.float32)
        r = -np.sum(np.asarray(a) ** 2, axis=1).astype(np.float32)
        return self._obs(), r, np.zeros(self.n, bool), [{}] * self.n


def _agent(normalize=True, prime=False, seed=1, **kw):
    return PPO(WideVecEnv(16, seed), n_steps=8, device="cpu", seed=seed, normalize_obs=normalize, obs_norm_prime=prime, **kw)


def test_statistics_after_two_rounds_are_the_moments_of_the_rollouts():
    agent = _agent()
    rolls = []
    for _ in range(2):
        frozen = agent.obs_norm.norm.clone()
        roll = agent.collect()
        # rollout and update see the same statistics: the stored log-probabilities are the policy's, recomputed
        lp = agent.policy.dist(roll["obs"]).log_prob(roll["act"]).sum(-1)
        assert (lp - roll["logp"]).abs().max().item() < 1e-5
        assert torch.equal(agent.obs_norm.norm, frozen)          # frozen through the rollout ...
        rolls.append(roll["obs"].reshape(-1, 3).numpy().copy())
        agent.update(roll)                                        # ... merged after the update
        assert not torch.equal(agent.obs_norm.norm, frozen)
    data = np.concatenate(rolls)
    n = agent.obs_norm
    assert_moments(n.mean.numpy(), n.var.numpy(), n.count, data)
    assert agent.num_timesteps == 2 * 8 * 16


def test_priming_runs_one_uncounted_rollout():
    agent = _agent(prime=True)
    roll = agent.collect()
    assert agent.obs_norm.count == 8 * 16 and agent.num_timesteps == 8 * 16      # primed, the priming rollout not counted
    lp = agent.policy.dist(roll["obs"]).log_prob(roll["act"]).sum(-1)
    assert (lp - roll["logp"]).abs().max().item() < 1e-5
    # the returned rollout ran under the primed statistics: its operands are of order one in every column
    assert agent.obs_norm.apply(roll["obs"]).abs().max() < 10.0 and agent.obs_norm.norm[0, 2] > 100.0
    agent.update(roll)
    assert agent.obs_norm.count == 2 * 8 * 16
    agent.collect()
    assert agent.obs_norm.count == 2 * 8 * 16                                      # primes once


def test_checkpoints_carry_the_statistics_and_refuse_a_mismatch(tmp_path):
    agent = _agent()
    agent.update(agent.collect())
    path = str(tmp_path / "model.pkl")
    agent.save(path)
    ck = torch.load(path)
    assert set(ck["obs_norm"]) == {"mean", "var", "count", "clip", "eps"}
    other = _agent(seed=2, prime=True).load(path)
    assert torch.equal(other.obs_norm.state, agent.obs_norm.state) and torch.equal(other.obs_norm.norm, agent.obs_norm.norm)
    obs = torch.from_numpy(WideVecEnv(5).reset())
    assert torch.equal(other.policy.dist(obs).mean, agent.policy.dist(obs).mean)
    other.collect()
    assert other.obs_norm.count == agent.obs_norm.count          # loaded statistics: no priming
    with pytest.raises(ValueError, match="normalisation"):
        _agent(normalize=False).load(path)
    plain = _agent(normalize=False)
    plain_path = str(tmp_path / "plain.pkl")
    plain.save(plain_path)
    with pytest.raises(ValueError, match="normalisation"):
        _agent().load(plain_path)
    # a checkpoint written before the key existed loads into an agent without normalisation
    old = torch.load(plain_path)
    del old["obs_norm"]
    torch.save(old, plain_path)
    _agent(normalize=False).load(plain_path)
    with pytest.raises(ValueError, match="normalisation"):
        _agent().load(plain_path)


def test_playback_reads_the_statistics(tmp_path):
    """visualize_agent's policy applies the checkpoint's statistics (the hook it uses, on a checkpoint dict)."""
    agent = _agent()
    agent.update(agent.collect())
    path = str(tmp_path / "model.pkl")
    agent.save(path)
    ck = torch.load(path, map_location="cpu")
    policy = MlpPolicy(3, 2)
    policy.load_state_dict(ck["policy"])
    stats = ObsNorm(3)
    stats.load_state_dict(ck["obs_norm"])
    policy.set_obs_norm(stats)
    obs = torch.from_numpy(WideVecEnv(5).reset())
    assert torch.equal(policy.act(obs, deterministic=True)[0], agent.policy.act(obs, deterministic=True)[0])


def test_cli_has_the_flags():
    import gym_roboy_amd.train_parallel as tp
    with pytest.raises(SystemExit):
        tp.main(["--help"])
    import inspect
    src = inspect.getsource(tp.main)
    assert "--normalize-obs" in src and "--clip-obs" in src
