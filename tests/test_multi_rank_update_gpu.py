"""The multi-rank PPO update on the GPU - the fused kernels' path (FusedAdam.step's all-reduce of the flat gradient vector through the
host under gloo, the grad_scale argument, the loss and diagnostics slots scaled afterwards, the two sets of observation sums as one
tensor) and the torch path on device tensors - held to a single process, bit for bit, and to a float64 statement of W ranks
(tests/multi_rank_util.py); and the collect side on real envs with every statistic PPO keeps.

Three launches for the whole module, each started once by a module-scoped fixture: two ranks (the bit-for-bit scenarios and the
float64 ones), three ranks (the float64 ones), two ranks on real envs.  All ranks share the one GPU; collectives go over gloo."""
import numpy as np
import pytest

import multi_rank_util as u

pytestmark = pytest.mark.gpu

# (name, obs_dim, critic_obs_dim, envs per rank, lr_schedule, normalize_obs, fused, the approx_kl of each update's rollout); a minibatch is
# a quarter of 4 * envs samples: one tile and half a tile (96), or a tile and one sample (65)
SAME = [("fixed", 9, None, 96, None, False, True, (0.002, 0.012)),
        ("adaptive", 9, None, 96, "adaptive", False, True, (0.002, 0.012)),
        ("normalised", 25, None, 96, None, True, True, (0.002, 0.012)),
        ("general_form_adaptive", 33, None, 65, "adaptive", False, True, (0.002, 0.012)),
        ("asymmetric_adaptive_normalised", 9, 38, 96, "adaptive", True, True, (0.002, 0.012)),
        ("torch_path_adaptive", 9, None, 96, "adaptive", False, False, (0.002, 0.012))]
# (name, obs_dim, critic_obs_dim, fused)
OWN = [("fused_9", 9, None, True), ("fused_33", 33, None, True), ("asymmetric", 9, 38, True), ("torch", 9, None, False)]
N_ENVS, REWARD_SCALE = 256, 0.01


def _same_specs():
    return [u.scenario("same_" + name, "same", da, dc, n_envs=n, lr_schedule=sched, normalize_obs=norm, kls=[[k] for k in kls], seed=i,
                       fused=fused) for i, (name, da, dc, n, sched, norm, fused, kls) in enumerate(SAME)]


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    return u.run_single_then_ranks(_same_specs(), u.own_shard_scenarios(2, OWN), 2, tmp_path_factory.mktemp("two_ranks"), "cuda")


@pytest.fixture(scope="module")
def three_ranks(tmp_path_factory):
    return u.run_single_then_ranks([], u.own_shard_scenarios(3, OWN), 3, tmp_path_factory.mktemp("three_ranks"), "cuda")


@pytest.fixture(scope="module")
def real_envs(tmp_path_factory):
    spec = {"name": "envs", "kind": "envs", "n_envs": N_ENVS, "reward_scale": REWARD_SCALE}
    return u.launch(2, [spec], tmp_path_factory.mktemp("real_envs"), "cuda")["envs"]


# ---- A. two ranks fed one shard: the single process, bit for bit ----
@pytest.mark.parametrize("name", [s[0] for s in SAME])
def test_two_ranks_fed_one_shard_reproduce_the_single_process_bit_for_bit(two_ranks, name):
    """Parameters, both Adam moments, the step count, the rate sequence, every value update() returns and the observation statistics
    (twice the count) after each of two updates of eight optimiser steps with ent_coef = 0.1: rank 0 against the single process,
    rank 1 against rank 0.  With the schedule on, the single process's rate sequence must hold a rise, a cut and a kept rate.
    Observed on the MI355X: all six scenarios bit-equal; gloo all-reduces the torch path's device tensors (the flat gradient, the
    reported terms) on this build without a host copy."""
    fused = dict((s[0], s[6]) for s in SAME)[name]
    name = "same_" + name
    single, (r0, r1) = two_ranks["single"][name], two_ranks["ranks"][name]
    assert single["fused"] == fused and single["updates"][-1]["post"]["t"] == 16
    if two_ranks["specs"][name]["lr_schedule"] is not None:
        print(name, u.assert_rate_sequence_is_a_test_of_the_rule(single))
    u.assert_same_bits(single, r0, (name, "single / rank 0"), count_factor=2)
    u.assert_same_bits(r0, r1, (name, "rank 0 / rank 1"))


# ---- B. W ranks with their own shards: the float64 statement ----
@pytest.mark.parametrize("side", ["never", "always"])
@pytest.mark.parametrize("shape", [s[0] for s in OWN])
def test_two_ranks_with_their_own_shards_match_the_float64_statement(two_ranks, shape, side):
    """Three updates of one optimiser step, each restated in float64 from the state the device held in front of it; max_grad_norm at
    four times (never clipped) and a quarter of (always clipped) the reference's gradient norm.  Bounds: loss terms and approx_kl
    1e-4, the moments' increments 5.1e-4 and 1.02e-3 of a parameter's largest entry, parameters 2e-6, the rate exactly.
    Observed on the MI355X, worst of the three fused shapes, both sides and the three steps: loss terms 1.6e-7, approx_kl 7.3e-8,
    clip_frac 9.9e-9, first moment 4.5e-6, second moment 2.3e-5, parameters 2.9e-7; the torch path on the device: first moment 3.3e-6,
    second 4.5e-6, parameters 2.0e-7.  (A sum that is not divided by W, or rank 0's gradient alone, is 1 to 2.4 away.)"""
    name = "own_w2_%s_%s" % (shape, side)
    print(u.assert_own_shards_match_float64(two_ranks["specs"][name], two_ranks["ranks"][name]))


@pytest.mark.parametrize("side", ["never", "always"])
@pytest.mark.parametrize("shape", [s[0] for s in OWN])
def test_three_ranks_with_their_own_shards_match_the_float64_statement(three_ranks, shape, side):
    """As the two-rank test, with grad_scale = 1 / 3.  Observed on the MI355X, fused shapes: loss terms 2.9e-7, approx_kl 6.6e-8,
    clip_frac 1.7e-8, first moment 6.4e-6, second moment 1.8e-5, parameters 6.6e-7; the torch path on the device: first moment
    3.3e-6, second 5.5e-6, parameters 1.8e-7."""
    name = "own_w3_%s_%s" % (shape, side)
    print(u.assert_own_shards_match_float64(three_ranks["specs"][name], three_ranks["ranks"][name]))


# ---- C. the collect side on real envs ----
def test_two_ranks_on_real_envs_hold_the_statistics_of_both_shards(real_envs):
    """Two ranks, each on its own 256 MsjRobot envs (tendon channels, critic rows, time limits of 3 steps), PPO with the asymmetric
    critic, observation and return normalisation, bootstrapped time limits and the captured rollout: after the priming rollout and two
    rounds the return statistics are the moments of both ranks' returns (the fused tail's sums, all-reduced), the two observation
    statistics those of both ranks' rows, and parameters and statistics are the same bits on both ranks."""
    import torch
    import reward_norm_ref as ref
    r0, r1 = real_envs
    rets, rows = [], {"obs": [], "cobs": []}
    for r in (r0, r1):
        assert r["graph"] and len(r["rollouts"]) == 3 and r["num_timesteps"] == 2 * u.T * N_ENVS      # the priming rollout and two rounds
        carry = np.zeros(N_ENVS)
        for rec in r["rollouts"]:
            assert rec["trunc"].sum() > 0 and (rec["trunc"] <= rec["done"]).all() and not rec["done"].all()
            x, carry, _ = ref.scan(ref.scaled(rec["rew_raw"].numpy(), REWARD_SCALE), rec["done"].numpy(), r["gamma"], carry)
            rets.append(x)
            for key in rows:
                rows[key].append(rec[key].numpy())
    assert not torch.equal(r0["rollouts"][0]["obs"], r1["rollouts"][0]["obs"])                        # own shards
    state = r0["reward_norm"]["state"].numpy()
    ref.assert_return_moments(state[0], state[1], state[2], rets)
    assert state[2] == 2 * 3 * u.T * N_ENVS
    u.assert_union_moments(r0["obs_norm"]["state"].numpy(), rows["obs"])
    u.assert_union_moments(r0["cobs_norm"]["state"].numpy(), rows["cobs"])
    assert r0["obs_norm"]["state"][-1].item() == r0["cobs_norm"]["state"][-1].item() == 2 * 3 * u.T * N_ENVS
    for key in ("obs_norm", "cobs_norm", "reward_norm"):
        assert torch.equal(r0[key]["state"], r1[key]["state"]) and torch.equal(r0[key]["norm"], r1[key]["norm"]), key
    for p, q in zip(r0["params"], r1["params"]):
        assert torch.equal(p, q) and torch.isfinite(p).all()
