"""The multi-rank PPO update on the torch path (device="cpu", collectives over gloo) held to a single process, bit for bit, and to a
float64 statement of W ranks (tests/multi_rank_util.py).  Identical parameters on every rank follow from any all-reduce
at all; these tests see the gradient's scale (Adam's moments), whose gradient it is, which KL moves the rate, and whether what
update() reports is the ranks' mean.

Two launches for the whole module - two ranks (the bit-for-bit scenarios and the float64 ones) and three ranks - started once each."""
import pytest

import multi_rank_util as u

# (name, obs_dim, critic_obs_dim, lr_schedule, normalize_obs, the approx_kl of each update's rollout)
SAME = [("fixed", 9, None, None, False, (0.002, 0.012)),
        ("adaptive", 9, None, "adaptive", False, (0.002, 0.012)),
        ("normalised", 25, None, None, True, (0.002, 0.012)),
        ("asymmetric_adaptive_normalised", 9, 38, "adaptive", True, (0.002, 0.012))]
OWN = [("torch", 9, None, False)]


def _same_specs():
    return [u.scenario("same_" + name, "same", da, dc, lr_schedule=sched, normalize_obs=norm, kls=[[k] for k in kls], seed=i, fused=False)
            for i, (name, da, dc, sched, norm, kls) in enumerate(SAME)]


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    return u.run_single_then_ranks(_same_specs(), u.own_shard_scenarios(2, OWN), 2, tmp_path_factory.mktemp("two_ranks"), "cpu")


@pytest.fixture(scope="module")
def three_ranks(tmp_path_factory):
    return u.run_single_then_ranks([], u.own_shard_scenarios(3, OWN), 3, tmp_path_factory.mktemp("three_ranks"), "cpu")


@pytest.mark.parametrize("name", [s[0] for s in SAME])
def test_two_ranks_fed_one_shard_reproduce_the_single_process_bit_for_bit(two_ranks, name):
    """Parameters, both Adam moments, the step count, the rate sequence, every value update() returns and the observation statistics
    (twice the count) after each of two updates of eight optimiser steps: rank 0 against the single process, rank 1 against rank 0."""
    name = "same_" + name
    single, (r0, r1) = two_ranks["single"][name], two_ranks["ranks"][name]
    assert not single["fused"] and single["updates"][-1]["post"]["t"] == 16
    u.assert_same_bits(single, r0, (name, "single / rank 0"), count_factor=2)
    u.assert_same_bits(r0, r1, (name, "rank 0 / rank 1"))
    if two_ranks["specs"][name]["lr_schedule"] is not None:
        print(name, u.assert_rate_sequence_is_a_test_of_the_rule(single))


@pytest.mark.parametrize("side", ["never", "always"])
def test_two_ranks_with_their_own_shards_match_the_float64_statement(two_ranks, side):
    """Three updates of one optimiser step, each restated in float64 from the state the ranks held in front of it (tests/multi_rank_util.py:
    assert_own_shards_match_float64 for the bounds).  Observed on the CPU: loss terms 1.0e-7, first moment 2.5e-6, second 5.0e-6 of a
    parameter's largest entry, parameters 4.2e-7."""
    name = "own_w2_torch_" + side
    print(u.assert_own_shards_match_float64(two_ranks["specs"][name], two_ranks["ranks"][name]))


@pytest.mark.parametrize("side", ["never", "always"])
def test_three_ranks_with_their_own_shards_match_the_float64_statement(three_ranks, side):
    """As the two-rank test, the mean of three.  Observed on the CPU: loss terms 1.3e-7, first moment 3.6e-6, second 6.3e-6, parameters
    1.1e-7."""
    name = "own_w3_torch_" + side
    print(u.assert_own_shards_match_float64(three_ranks["specs"][name], three_ranks["ranks"][name]))
