"""GPU tests of the mirror-symmetry loss: the pair-tile gradient kernel rp_sym_grad_dev / rp_sym_grad_norm_dev
against float64 autograd (tests/symmetry_loss_ref.py), its index, accumulate and argument rules, and PPO(symmetry="loss") - fused
against torch path, captured against eager, train_parallel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from symmetry_loss_ref import random_case, sym_loss64

pytestmark = pytest.mark.gpu

# (obs_dim, act_dim, B, P = reversal): one pair and 31 dead ones; the tile edge; more than one tile per wave on 256 CUs x 4 waves (both
# prefetch buffers); the widths of MsjRobot's rows; 29 / 30, where the PPO kernel's small form changes variant (this kernel's does not);
# KX = 2 with a small P; images across the 32-output boundary (OT = 2); the general form's widest; P = [0]
SHAPES = [(9, 8, 1, False), (9, 8, 31, False), (9, 8, 32, False), (9, 8, 33, False), (9, 8, 70000, False), (25, 8, 100, False),
          (29, 8, 140, False), (30, 8, 140, False), (33, 8, 100, False), (60, 38, 77, True), (10, 33, 100, False), (63, 40, 70, False),
          (3, 1, 200, False)]
SMALL_FORM = 2                       # every small policy runs the prefetching variant (rp_sym_grad_form)


def _want_form(obs_dim, act_dim):
    return SMALL_FORM if obs_dim <= 31 and act_dim <= 8 else 0


def _check_against_float64(fg, policy, want_loss, want, loss_slot, fixed_points_only=False):
    """the project's tolerances for rp_ppo_grad_dev (tests/test_policy_gpu.py): per parameter block max |got - want| / max(max |want|,
    1e-6) < 5e-4, the loss to 1e-4 max(1, |want|); log_std exactly 0; the reference's blocks stand well above the 1e-6 floor"""
    got_loss = loss_slot.item()
    print("L_sym %.9g, float64 %.9g" % (got_loss, want_loss))
    assert abs(got_loss - want_loss) < 1e-4 * max(1.0, abs(want_loss))
    for name, p in policy.named_parameters():
        w = want[name]
        got = fg._views[_flat_name(name)].detach().cpu().double().reshape(w.shape)
        if name == "log_std" or name.startswith("vf."):
            assert w.abs().max().item() == 0.0
            if name == "log_std":
                assert got.abs().max().item() == 0.0
            continue
        scale = w.abs().max().item()
        # well above the floor: the relative bound below is a real one.  The one block that is zero by the mathematics: the last bias
        # where EVERY action is a fixed point of P (d L / d b3[k] = c' sum_i (e_i[k] - e_i[P k])) - P = [0] - held to the floor itself
        if not (name == "pi.4.bias" and fixed_points_only):
            assert scale > 1e-4, (name, scale)
        else:
            assert scale == 0.0
        err = (got - w).abs().max().item() / max(scale, 1e-6)
        print("  %-12s max |want| %.3g, relative error %.3g" % (name, scale, err))
        assert err < 5e-4, (name, err, scale)


def _flat_name(name):
    net, layer, kind = name.split(".") if "." in name else (None, None, None)
    if net is None:
        return "log_std"
    return "%s_%s%d" % (net, "w" if kind == "weight" else "b", int(layer) // 2 + 1)


@pytest.mark.parametrize("obs_dim,act_dim,B,reversal", SHAPES)
def test_gradient_matches_float64_autograd(obs_dim, act_dim, B, reversal):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad
    if os.environ.get("ROBOY_POLICY_PREFETCH", "1")[0] != "0":
        assert pn.load().rp_sym_grad_form(obs_dim, act_dim) == _want_form(obs_dim, act_dim)
    coef = 0.7
    policy, obs, image, act_src = random_case(obs_dim, act_dim, B, 5 + obs_dim + B % 97, reversal)
    assert np.array_equal(act_src[act_src], np.arange(act_dim))
    want_loss, want = sym_loss64(policy, obs, image, act_src, coef)
    policy = policy.cuda()
    fg = FusedPolicyGrad(policy)
    fg._g.fill_(float("nan"))                               # accumulate = 0 overwrites whatever is there
    slot = fg.sym_run(obs.cuda(), image.cuda(), act_src, coef, accumulate=False)
    torch.cuda.synchronize()
    L = fg._layout["pi_loss"][0]
    assert torch.isnan(fg._g[L:L + 3]).all() and torch.isnan(fg._g[fg._layout["vf_w1"][0]:]).all()      # not its slots, not the value block
    _check_against_float64(fg, policy, want_loss, want, slot, fixed_points_only=bool(np.array_equal(act_src, np.arange(act_dim))))
    # the same minibatch addressed through row indices into tensors three times as long: bit-identical
    g_direct = fg._g.clone()
    perm = torch.randperm(3 * B, device="cuda")[:B]
    big_obs, big_image = torch.zeros(3 * B, obs_dim, device="cuda"), torch.zeros(3 * B, obs_dim, device="cuda")
    big_obs[perm], big_image[perm] = obs.cuda(), image.cuda()
    fg.sym_run(big_obs, big_image, act_src, coef, index=perm, accumulate=False)
    torch.cuda.synchronize()
    keep = ~torch.isnan(g_direct)
    assert torch.equal(fg._g[keep], g_direct[keep]) and torch.equal(torch.isnan(fg._g), torch.isnan(g_direct))


@pytest.mark.parametrize("obs_dim,act_dim,B", [(9, 8, 100), (33, 8, 100)])
def test_normalising_instance_matches_float64_with_obsnorm_apply(obs_dim, act_dim, B):
    import torch
    from gym_roboy_amd.ppo import FusedPolicyGrad, ObsNorm
    coef = 1.3
    policy, obs, image, act_src = random_case(obs_dim, act_dim, B, 77 + obs_dim)
    rng = np.random.default_rng(obs_dim)
    norm = ObsNorm(obs_dim, "cpu", clip=10.0)
    norm.norm[0] = torch.from_numpy(rng.uniform(-0.5, 0.5, obs_dim).astype(np.float32))
    norm.norm[1] = torch.from_numpy(rng.uniform(0.5, 8.0, obs_dim).astype(np.float32))       # (x 8 on [-2, 2]: some entries clamp at 10)
    policy.set_obs_norm(norm)
    want_loss, want = sym_loss64(policy, obs, image, act_src, coef)
    policy.set_obs_norm(None)
    policy = policy.cuda()
    fg = FusedPolicyGrad(policy)
    dev_norm = ObsNorm(obs_dim, "cuda", clip=10.0)
    dev_norm.norm.copy_(norm.norm)
    slot = fg.sym_run(obs.cuda(), image.cuda(), act_src, coef, norm=dev_norm, accumulate=False)
    torch.cuda.synchronize()
    _check_against_float64(fg, policy, want_loss, want, slot)


def _check_staged_variant(obs_dim, act_dim, B, normalise):
    """the small form's STAGED variant (rp_sym_grad_form 1: the process runs under ROBOY_POLICY_PREFETCH=0) against float64, the
    minibatch addressed directly and through row indices into tensors three times as long whose other rows are NaN"""
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad, ObsNorm
    assert pn.load().rp_sym_grad_form(obs_dim, act_dim) == 1
    coef = 0.7
    policy, obs, image, act_src = random_case(obs_dim, act_dim, B, 31 + obs_dim + B % 97)
    dev_norm = None
    if normalise:
        rng = np.random.default_rng(obs_dim)
        norm = ObsNorm(obs_dim, "cpu", clip=10.0)
        norm.norm[0] = torch.from_numpy(rng.uniform(-0.5, 0.5, obs_dim).astype(np.float32))
        norm.norm[1] = torch.from_numpy(rng.uniform(0.5, 8.0, obs_dim).astype(np.float32))
        policy.set_obs_norm(norm)
        dev_norm = ObsNorm(obs_dim, "cuda", clip=10.0)
        dev_norm.norm.copy_(norm.norm)
    want_loss, want = sym_loss64(policy, obs, image, act_src, coef)
    policy.set_obs_norm(None)
    policy = policy.cuda()
    fg = FusedPolicyGrad(policy)
    fg._g.zero_()
    slot = fg.sym_run(obs.cuda(), image.cuda(), act_src, coef, norm=dev_norm)
    torch.cuda.synchronize()
    _check_against_float64(fg, policy, want_loss, want, slot)
    g_direct = fg._g.clone()
    perm = torch.randperm(3 * B, device="cuda")[:B]
    big_obs, big_image = (torch.full((3 * B, obs_dim), float("nan"), device="cuda") for _ in range(2))
    big_obs[perm], big_image[perm] = obs.cuda(), image.cuda()
    fg.sym_run(big_obs, big_image, act_src, coef, index=perm, norm=dev_norm)
    torch.cuda.synchronize()
    assert torch.equal(fg._g, g_direct)                       # (a row outside the index, or of the wrong array, would bring its NaN)
    print("staged variant (%d, %d) B = %d normalise %d: ok" % (obs_dim, act_dim, B, normalise))


@pytest.mark.parametrize("normalise", [False, True])
def test_staged_small_variant_matches_float64_in_a_child_process(normalise):
    """ROBOY_POLICY_PREFETCH=0 is read once per process: a child runs mlp_sym_kernel<0, 1, 8, false> (and, normalise, its
    mlp_sym_norm_kernel sibling, whose rows are normalised as they are staged) at one pair, across the tile edge, at the width
    where the PPO kernel changes variant and at more than one tile per wave, direct and indexed."""
    env = dict(os.environ, ROBOY_POLICY_PREFETCH="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    cases = [(9, 8, 1), (9, 8, 33), (30, 8, 140), (9, 8, 70000)]
    code = "import test_symmetry_loss_gpu as t\nfor o, a, B in %r: t._check_staged_variant(o, a, B, %r)" % (cases, normalise)
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + ["-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.count("staged variant") == len(cases)


@pytest.mark.parametrize("obs_dim,act_dim,B", [(9, 8, 333), (33, 8, 100)])
def test_accumulate_adds_last_and_leaves_the_other_slots_alone(obs_dim, act_dim, B):
    """the reduction forms the sum over the partials and adds it to what is there LAST: accumulate = 1 onto g0 is exactly
    g0 + (the accumulate = 0 result), element by element - not merely to 1 ulp"""
    import torch
    from gym_roboy_amd.ppo import FusedPolicyGrad
    policy, obs, image, act_src = random_case(obs_dim, act_dim, B, 3)
    fg = FusedPolicyGrad(policy.cuda())
    obs, image = obs.cuda(), image.cuda()
    fg._g.zero_()
    fg.sym_run(obs, image, act_src, 0.9, accumulate=False)
    fresh = fg._g.clone()
    g0 = torch.randn(fg._g.shape, generator=torch.Generator().manual_seed(1)).cuda()
    fg._g.copy_(g0)
    fg.sym_run(obs, image, act_src, 0.9, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(fg._g, g0 + fresh)
    L, S = fg._layout["pi_loss"][0], fg._layout["symmetry_loss"][0]
    assert S == L + 3 and fresh[S].item() > 0 and torch.equal(fresh[L:L + 3], torch.zeros(3, device="cuda"))
    assert torch.equal(fg._g[L:L + 3], g0[L:L + 3]) and torch.equal(fg._g[S + 1:], g0[S + 1:])      # pg, approx_kl, clip_frac; the value block
    # behind the PPO gradient: its loss and diagnostics slots stay what rp_ppo_grad_diag_dev wrote, bit for bit
    g = torch.Generator().manual_seed(2)
    act, adv, logp, val, ret = (torch.randn(B, act_dim, generator=g).cuda(), torch.randn(B, generator=g).cuda(),
                                -8 + torch.randn(B, generator=g).cuda(), torch.randn(B, generator=g).cuda(), torch.randn(B, generator=g).cuda())
    fg.run(obs, act, adv, logp, val, ret, 0.2, 0.5, 0.0, diagnostics=True)
    ppo = fg._g.clone()
    assert ppo[S].item() == 0.0
    fg.sym_run(obs, image, act_src, 0.9, accumulate=True, repack=False)
    torch.cuda.synchronize()
    assert torch.equal(fg._g, ppo + fresh) and torch.equal(fg._g[L:L + 3], ppo[L:L + 3]) and fg._g[S] == fresh[S]
    assert torch.equal(fg._g[fg._layout["vf_w1"][0]:], ppo[fg._layout["vf_w1"][0]:])


def test_coefficient_zero_gives_an_all_zero_block():
    import torch
    from gym_roboy_amd.ppo import FusedPolicyGrad
    policy, obs, image, act_src = random_case(9, 8, 100, 4)
    fg = FusedPolicyGrad(policy.cuda())
    fg._g.fill_(1.0)
    fg.sym_run(obs.cuda(), image.cuda(), act_src, 0.0, accumulate=False)
    torch.cuda.synchronize()
    L = fg._layout["pi_loss"][0]
    assert torch.equal(fg._g[:L], torch.zeros(L, device="cuda")) and fg._g[L + 3].item() == 0.0


def test_arguments_are_checked():
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad
    policy, obs, image, act_src = random_case(9, 8, 10, 4)
    fg = FusedPolicyGrad(policy.cuda())
    obs, image = obs.cuda(), image.cuda()
    for bad in ([1, 2, 0, 3, 4, 5, 6, 7], [0, 0, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 8], [-1, 1, 2, 3, 4, 5, 6, 7]):
        with pytest.raises(RuntimeError, match="involution"):        # a 3-cycle, no permutation, out of range twice
            fg.sym_run(obs, image, bad, 1.0)
    with pytest.raises(RuntimeError, match="coef"):
        fg.sym_run(obs, image, act_src, -1.0)
    lib = pn.load()
    src = (ctypes.c_int32 * 8)(*range(8))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty(int(lib.rp_sym_workspace_floats(9, 8, 10)), device="cuda")
    assert lib.rp_sym_grad_dev(ptr(fg._packed_pi), ptr(obs), None, None, 10, 9, 8, src, 1.0, ptr(fg._g), 0, ptr(ws), None) == -1
    assert b"null" in lib.rp_last_error()
    torch.cuda.synchronize()


# ---- PPO ----
N_ENVS, N_STEPS = 256, 8


def _orders(n, epochs, seed=11):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n, generator=g).cuda() for _ in range(epochs)]


@pytest.mark.parametrize("config", ["tendon", "asymmetric", "normalize"])
def test_fused_update_is_the_torch_update(msj_robot, config):
    """one update() with symmetry="loss", the same rollout and sample orders for both paths: the parameters agree within the bound the
    fused-against-torch update test holds for plain PPO, 2e-6 per optimiser step (tests/test_policy_scale_gpu.py: _assert_adam_close)"""
    import torch
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env_kw = {"tendon": {"tendon_obs": ("length", "force")}, "asymmetric": {"critic_obs": ("state", "age")},
              "normalize": {"tendon_obs": ("length", "force")}}[config]
    kw = {"asymmetric_critic": True} if config == "asymmetric" else ({"normalize_obs": True} if config == "normalize" else {})
    env = RoboyVecEnv(msj_robot, N_ENVS, seed=3, **env_kw)
    try:
        mk = lambda fused: PPO(env, n_steps=N_STEPS, nminibatches=2, noptepochs=2, device="cuda", seed=4, fused_policy=fused,
                               fused_update=fused, symmetry="loss", symmetry_coef=1.0, **kw)
        a, b = mk(True), mk(False)
        assert a._fgrad is not None and b._fgrad is None
        with torch.no_grad():                                # (a fresh policy's last layer is near zero: so would the loss be)
            for p in a.policy.parameters():
                p.add_(0.3 * torch.randn_like(p))
        b.policy.load_state_dict(a.policy.state_dict())
        roll = a.collect()
        if config == "normalize":                            # both agents under the statistics the rollout primed
            b.obs_norm.load_state_dict(a.obs_norm.state_dict())
            b._obs_norm_prime = False
        before = [p.detach().clone() for p in a.policy.parameters()]
        orders = _orders(N_ENVS * N_STEPS, 2)
        sa = a.update({k: v.clone() for k, v in roll.items()}, sample_orders=orders)
        sb = b.update({k: v.clone() for k, v in roll.items()}, sample_orders=orders)
        print(sa, sb)
        assert sa["symmetry_loss"] > 1e-4 and abs(sa["symmetry_loss"] - sb["symmetry_loss"]) < 1e-4 * max(1.0, sb["symmetry_loss"])
        steps = 4
        assert a._fadam.t == steps
        for (name, p), (_, q) in zip(a.policy.named_parameters(), b.policy.named_parameters()):
            err = (p - q).abs().max().item()
            assert err < 2e-6 * steps, (name, err)
        assert any(not torch.equal(p, p0) for p, p0 in zip(a.policy.parameters(), before))
        if config == "normalize":
            assert a.obs_norm.count == b.obs_norm.count == 2 * 2 * N_ENVS * N_STEPS      # rows and images, the priming merge and the update's
        gap = a.symmetry_gap(roll)
        assert gap["action"] > 0 and (np.isnan(gap["value"]) if config == "asymmetric" else gap["value"] >= 0)
    finally:
        env.close()


def test_graph_and_eager_mode_give_the_same_parameters(msj_robot):
    """with the asymmetric critic, where the eager and the captured rollout run the same tail (ppo.py: rollout_tail_form - a plain eager
    agent takes torch's GAE, whose advantages differ from the kernel's in the last bit with or without this option): the same rollout,
    so the same update, bit for bit"""
    import torch
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    out = []
    for graphs in (False, True):
        env = RoboyVecEnv(msj_robot, N_ENVS, seed=3, critic_obs=("state", "age"))
        try:
            agent = PPO(env, n_steps=N_STEPS, nminibatches=2, noptepochs=2, device="cuda", seed=4, use_graphs=graphs, symmetry="loss",
                        asymmetric_critic=True)
            roll = agent.collect()
            assert (agent._rollout_graph is not None) == graphs
            stats = agent.update(roll)
            assert np.isfinite(stats["symmetry_loss"]) and stats["symmetry_loss"] > 0
            out.append([p.detach().clone() for p in agent.policy.parameters()])
        finally:
            env.close()
    for p, q in zip(*out):
        assert torch.equal(p, q)


def test_train_parallel_prints_the_term(tmp_path, capsys):
    import torch
    from gym_roboy_amd import train_parallel
    out = str(tmp_path / "results")
    agent = train_parallel.main(["256", out, "--rounds", "2", "--steps-per-round", str(256 * 8), "--n-steps", "8", "--symmetry", "loss",
                                 "--symmetry-coef", "1", "--critic-obs", "state,age"])
    text = capsys.readouterr().out
    assert "symmetry_loss" in text and "symmetry_gap_action" in text
    assert agent.symmetry == "loss" and agent.asymmetric_critic and agent._mirror.kernel_applies()
    ck = torch.load(os.path.join(out, "model.pkl"))
    assert ck["symmetry"] == "loss" and ck["symmetry_coef"] == 1.0
    agent.env.close()
