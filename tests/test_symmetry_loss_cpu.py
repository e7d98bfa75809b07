"""CPU tests of the mirror-symmetry loss: PPO(symmetry="loss") on the torch path - the statement the kernel
rp_sym_grad_dev is tested against (tests/test_symmetry_loss_gpu.py) - on the stub env of the augmentation's tests."""
import copy

import numpy as np
import pytest
import torch

from symmetry_loss_ref import sym_loss64
from test_symmetry_cpu import MirrorToyEnv


def _agent(symmetry, n=16, seed=3, env=None, **kw):
    from gym_roboy_amd.ppo import PPO
    env = env or MirrorToyEnv(n, seed=5)
    kw.setdefault("nminibatches", 2)
    kw.setdefault("noptepochs", 2)
    return PPO(env, n_steps=8, device="cpu", seed=seed, symmetry=symmetry, **kw)


def _orders(n, epochs, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n, generator=g) for _ in range(epochs)]


def test_the_mode_constructs_and_refuses_what_it_must():
    from gym_roboy_amd.ppo import SYMMETRY_MODES
    assert SYMMETRY_MODES == ("augment", "loss")
    agent = _agent("loss")                                  # (raised "unknown symmetry" before the mode existed)
    assert agent.symmetry == "loss" and agent.symmetry_coef == 1.0
    assert _agent("loss", symmetry_coef=0.25).symmetry_coef == 0.25
    for bad in (-1.0, -1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="symmetry_coef"):
            _agent("loss", symmetry_coef=bad)
    with pytest.raises(ValueError, match="unknown symmetry"):
        _agent("mirror")
    with pytest.raises(ValueError, match="mirror_map"):
        _agent("loss", env=MirrorToyEnv(16, with_map=False))


def test_the_loss_combines_with_an_asymmetric_critic_and_the_augmentation_still_does_not():
    env = MirrorToyEnv(16)
    env.critic_obs_dim = 12                                 # critic rows, and no mirror map for them
    agent = _agent("loss", env=env, asymmetric_critic=True)
    assert agent.asymmetric_critic and agent.cobs_dim == 12 and agent._mirror is not None
    with pytest.raises(ValueError, match="asymmetric_critic"):
        _agent("augment", env=env, asymmetric_critic=True)


def test_coefficient_zero_is_the_agent_without_the_option_bit_for_bit():
    a, b = _agent("loss", symmetry_coef=0.0), _agent(None)
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    roll = a.collect()
    orders = _orders(16 * 8, 2)
    before = [p.detach().clone() for p in a.policy.parameters()]
    sa = a.update({k: v.clone() for k, v in roll.items()}, sample_orders=orders)
    sb = b.update({k: v.clone() for k, v in roll.items()}, sample_orders=orders)
    assert sa.pop("symmetry_loss") == 0.0 and sa == sb
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    assert any(not torch.equal(p, p0) for p, p0 in zip(a.policy.parameters(), before))


def _perm_matrix(src, sign=None):
    """(X v)[c] = sign[c] * v[src[c]]"""
    n = len(src)
    X = torch.zeros(n, n, dtype=torch.float64)
    X[torch.arange(n), torch.as_tensor(np.asarray(src), dtype=torch.int64)] = torch.ones(n, dtype=torch.float64) if sign is None else torch.as_tensor(np.asarray(sign), dtype=torch.float64)
    return X


def _symmetrised(p, M, P, Q):
    with torch.no_grad():
        pi = p.pi
        pi[0].weight.copy_((pi[0].weight + Q @ pi[0].weight @ M) / 2); pi[0].bias.copy_((pi[0].bias + Q @ pi[0].bias) / 2)
        pi[2].weight.copy_((pi[2].weight + Q @ pi[2].weight @ Q) / 2); pi[2].bias.copy_((pi[2].bias + Q @ pi[2].bias) / 2)
        pi[4].weight.copy_((pi[4].weight + P @ pi[4].weight @ Q) / 2); pi[4].bias.copy_((pi[4].bias + P @ pi[4].bias) / 2)
    return p


def test_an_equivariant_net_has_zero_loss_and_zero_gradient():
    """A random net symmetrised in float64: with M the observation map, P the action map and Q a pairing of the hidden units (all
    involutions), W1 = (W1 + Q W1 M) / 2, W2 = (W2 + Q W2 Q) / 2, W3 = (W3 + P W3 Q) / 2 and the biases likewise give
    mu(M s) = P mu(s) up to the rounding of sums taken in another order: e ~ 1e-16 per entry.  The term of PPO._minibatch_loss on an
    agent that holds this net in float64 is below 1e-24 (measured 2.7e-31), and its gradient - linear in e: every entry at most
    2 coef mean|e| max|d mu / d theta|, a few hundred ulp of float64 - below 1e-14 (measured 4.6e-17).  The reference statement
    (symmetry_loss_ref) gives the same numbers on the same rows."""
    from symmetry_loss_ref import random_policy
    obs_src, obs_sign, act_src = MirrorToyEnv(4).mirror_map()
    M, P, Q = _perm_matrix(obs_src, obs_sign), _perm_matrix(act_src), _perm_matrix(np.arange(64)[::-1].copy())
    g = torch.Generator().manual_seed(0)
    n = 200
    obs = torch.rand(n, 9, generator=g, dtype=torch.float64) * 4 - 2
    flat = {"obs": obs, "obs_image": obs @ M.T, "act": torch.randn(n, 8, generator=g, dtype=torch.float64)}
    flat.update({k: torch.randn(n, generator=g, dtype=torch.float64) for k in ("adv", "logp", "val", "ret")})
    idx = torch.randperm(n, generator=g)[:150]
    seen = {}
    for kind in ("symmetrised", "raw"):
        p = random_policy(9, 8, 2).double()
        if kind == "symmetrised":
            _symmetrised(p, M, P, Q)
        agent = _agent("loss", policy=p)
        assert agent.policy is p and p.pi[0].weight.dtype == torch.float64
        loss, _, _, _, _, _, sym = agent._minibatch_loss(flat, idx)
        grads = torch.autograd.grad(sym, list(p.parameters()), allow_unused=True, retain_graph=True)
        named = {name: (gr if gr is not None else torch.zeros_like(q)) for (name, q), gr in zip(p.named_parameters(), grads)}
        worst = max(gr.abs().max().item() for gr in named.values())
        want, want_grads = sym_loss64(p, obs[idx], flat["obs_image"][idx], act_src, 1.0)
        print("%s net: L_sym = %.3g (reference %.3g), max |gradient| = %.3g" % (kind, sym.item(), want, worst))
        assert named["log_std"].abs().max().item() == 0.0 and all(gr.abs().max().item() == 0.0 for k, gr in named.items() if k.startswith("vf."))
        assert torch.isfinite(loss)
        seen[kind] = (sym.item(), worst, want, max(gr.abs().max().item() for gr in want_grads.values()))
    sym, worst, want, want_worst = seen["symmetrised"]
    assert 0.0 <= sym < 1e-24 and worst < 1e-14 and 0.0 <= want < 1e-24 and want_worst < 1e-14
    # the same rows on the net before it was symmetrised: the test can tell the difference, and the product is its statement
    sym, worst, want, want_worst = seen["raw"]
    assert sym > 1e-3 and worst > 1e-4 and abs(sym - want) <= 1e-12 * want and abs(worst - want_worst) <= 1e-12 * want_worst


@pytest.mark.parametrize("coef", [1.0, 0.3])
def test_the_reported_term_is_the_coefficient_times_the_symmetry_gap_of_the_minibatch(coef):
    """one minibatch of all rows, one epoch: the term update() reports was computed on the parameters symmetry_gap sees before it"""
    agent = _agent("loss", symmetry_coef=coef, nminibatches=1, noptepochs=1)
    roll = agent.collect()
    obs = roll["obs"].reshape(-1, 9)
    obs_src, obs_sign, act_src = agent.env.mirror_map()
    from gym_roboy_amd.envs.symmetry import mirror_rows
    want64, _ = sym_loss64(agent.policy, obs, mirror_rows(obs, obs_src, obs_sign), act_src, coef)
    gap32 = agent.symmetry_gap(roll)["action"]
    stats = agent.update(roll)
    print("symmetry_loss %.9g, coef * gap (float32) %.9g, float64 %.9g" % (stats["symmetry_loss"], coef * gap32, want64))
    assert want64 > 0
    assert abs(stats["symmetry_loss"] - want64) <= 1e-5 * want64
    assert abs(coef * gap32 - want64) <= 1e-5 * want64
    assert stats["loss"] == pytest.approx(stats["pg_loss"] - agent.ent_coef * stats["entropy"] + agent.vf_coef * stats["vf_loss"]
                                          + stats["symmetry_loss"], rel=1e-5, abs=1e-6)


def test_training_with_the_loss_ends_closer_to_the_symmetry():
    """Same seed, same sample orders, UPDATES updates on the stub env (whose reward is NOT symmetric: PPO alone drifts away from the
    symmetry).  Measured: symmetry_gap action 1.44e-04 with the loss (coefficient 10, 6 updates) against 7.77e-04 without, ratio 0.185."""
    UPDATES, COEF = 6, 10.0
    gaps = {}
    for mode in ("loss", None):
        agent = _agent(mode, n=64, **({"symmetry_coef": COEF} if mode else {}))
        for u in range(UPDATES):
            roll = agent.collect()
            agent.update(roll, sample_orders=_orders(64 * 8, 2, seed=100 + u))
        probe = _agent("loss", n=64)                         # (the maps to measure the plain agent with)
        probe.policy.load_state_dict(agent.policy.state_dict())
        gaps[mode] = probe.symmetry_gap(roll)["action"]
    print("symmetry_gap action: with the loss %.3g, without %.3g, ratio %.3g" % (gaps["loss"], gaps[None], gaps["loss"] / gaps[None]))
    assert gaps["loss"] < gaps[None]


def test_checkpoint_round_trip_and_mode_mismatch(tmp_path):
    a = _agent("loss", symmetry_coef=0.5)
    a.update(a.collect())
    path = str(tmp_path / "a.pt")
    a.save(path)
    ck = torch.load(path)
    assert ck["symmetry"] == "loss" and ck["symmetry_coef"] == 0.5
    b = _agent("loss", symmetry_coef=0.5).load(path)
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    for other in (None, "augment"):
        with pytest.raises(ValueError, match="symmetry"):
            _agent(other).load(path)
    # the coefficient is a weight, not a layout: the constructor's holds on resume, and the difference is said
    with pytest.warns(UserWarning, match="symmetry_coef"):
        c = _agent("loss", symmetry_coef=2.0).load(path)
    assert c.symmetry_coef == 2.0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _agent("loss", symmetry_coef=0.5).load(path)
    plain = str(tmp_path / "b.pt")
    _agent(None).save(plain)
    assert "symmetry_coef" not in torch.load(plain)
    with pytest.raises(ValueError, match="symmetry"):
        _agent("loss").load(plain)


def test_new_symbols_are_declared_and_exported():
    import os
    import re
    from conftest import ROOT
    from gym_roboy_amd import _policy_native as pn
    header = open(os.path.join(ROOT, "include", "roboy_policy.h")).read()
    lib = pn.load()
    for name in ("rp_sym_grad_dev", "rp_sym_grad_norm_dev", "rp_sym_workspace_floats", "rp_sym_grad_form"):
        assert re.search(r"\b%s\(" % name, header) and name in pn.SIGNATURES and hasattr(lib, name), name
    assert lib.rp_abi_version() == 5
    # the documented forms: every small policy prefetches (its input buffers are obs_dim + 2 rows), everything else is general
    for (o, a), form in {(9, 8): 2, (25, 8): 2, (29, 8): 2, (30, 8): 2, (31, 8): 2, (3, 1): 2, (32, 8): 0, (33, 8): 0, (10, 33): 0,
                         (60, 38): 0, (63, 40): 0}.items():
        if os.environ.get("ROBOY_POLICY_PREFETCH", "1")[0] != "0":
            assert lib.rp_sym_grad_form(o, a) == form, (o, a)
    assert lib.rp_sym_grad_form(64, 8) < 0 and lib.rp_sym_workspace_floats(9, 8, 0) < 0
    assert pn.grad_layout(9, 8)[0]["symmetry_loss"][0] == pn.grad_layout(9, 8)[0]["pi_loss"][0] + 3
