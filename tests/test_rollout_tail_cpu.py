"""``rollout_tail_form`` (gym_roboy_amd/ppo.py; DESIGN.md §16's table): the one place that says which statement computes a rollout's
tail, against the table written out - all 32 inputs - and the two invariants the rollout code relies on.  No GPU."""
import itertools

from gym_roboy_amd.ppo import rollout_tail_form

T, F = True, False
# (fused, eager, reward_norm, boot, asym) -> form
TABLE = {
    # the torch policy step: the torch statements, in every mode
    (F, F, F, F, F): "torch", (F, F, F, F, T): "torch", (F, F, F, T, F): "torch", (F, F, F, T, T): "torch",
    (F, F, T, F, F): "torch", (F, F, T, F, T): "torch", (F, F, T, T, F): "torch", (F, F, T, T, T): "torch",
    (F, T, F, F, F): "torch", (F, T, F, F, T): "torch", (F, T, F, T, F): "torch", (F, T, F, T, T): "torch",
    (F, T, T, F, F): "torch", (F, T, T, F, T): "torch", (F, T, T, T, F): "torch", (F, T, T, T, T): "torch",
    # fused, captured: rp_gae_dev, or one launch of the tail kernel under either option
    (T, F, F, F, F): "gae_kernel", (T, F, F, F, T): "gae_kernel",
    (T, F, F, T, F): "tail_kernel", (T, F, F, T, T): "tail_kernel",
    (T, F, T, F, F): "tail_kernel", (T, F, T, F, T): "tail_kernel",
    (T, F, T, T, F): "tail_kernel", (T, F, T, T, T): "tail_kernel",
    # fused, eager: the captured form under bootstrap_timeouts, and with an asymmetric critic without normalize_reward ...
    (T, T, F, F, T): "gae_kernel",
    (T, T, F, T, F): "tail_kernel", (T, T, F, T, T): "tail_kernel",
    (T, T, T, T, F): "tail_kernel", (T, T, T, T, T): "tail_kernel",
    # ... and the torch statements everywhere else (the historical exception)
    (T, T, F, F, F): "torch", (T, T, T, F, F): "torch", (T, T, T, F, T): "torch",
}


def test_rollout_tail_form_is_the_table():
    inputs = list(itertools.product((F, T), repeat=5))
    assert len(TABLE) == 32 and set(TABLE) == set(inputs)
    for key in inputs:
        assert rollout_tail_form(*key) == TABLE[key], key


def test_the_invariants_the_rollout_relies_on():
    for fused, eager, reward_norm, boot, asym in itertools.product((F, T), repeat=5):
        form = rollout_tail_form(fused, eager, reward_norm, boot, asym)
        assert form in ("torch", "gae_kernel", "tail_kernel")
        if not fused:                      # no kernel without the fused policy step (the CPU path among them)
            assert form == "torch"
        if fused and not eager:            # a captured fused rollout never runs the torch loop
            assert form != "torch"
        if form == "tail_kernel":          # the tail kernel has statistics to run on: the agent's own, or _boot_tail's identity
            assert reward_norm or boot
