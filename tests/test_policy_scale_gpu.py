"""The PPO kernels (csrc/mlp_policy.hip, mlp_train.hip, mlp_update.hip) against the float64 statements of
oracle/policy_ref.py at the batch sizes they run at: the policy step with more work items than waves, the exploration
noise bit for bit in its layout, the gradient in the form PPO calls it (rows gathered through an index, advantage
normalised in the kernel) and many tiles deep, the advantage statistics with all their blocks, clip + Adam and GAE.

Sizes that depend on the CU count are computed from the device and every test asserts the regime it is meant for.
No tolerance here comes from the kernels' own output: each is one tests/test_policy_gpu.py already holds for the same
input distribution, or a stated multiple of what the plain fp32 statement of the operation is away from float64."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_policy_gpu import _minibatch, _policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7777.0
PAD = 64
# the two ends of u1 (seed 5, step 0, block 0, word 0); tests/test_policy_ref_cpu.py finds them again by search
ID_U1_SMALLEST, ID_U1_ONE = 9_271_651, 31_776_762


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _step_padded(policy, obs, with_mean=True, seed=5, **kw):
    """One policy step into outputs that carry PAD sentinel rows past n; returns the device tensors."""
    import torch
    from gym_roboy_amd.ppo import FusedPolicyStep
    f = FusedPolicyStep(policy, seed=seed)
    n, ad = obs.shape[0], f.act_dim
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    act, logp, val = full(n + PAD, ad), full(n + PAD), full(n + PAD)
    mean = full(n + PAD, ad) if with_mean else None
    f.act_into(obs, act, logp, val, mean=mean, **kw)
    torch.cuda.synchronize()
    return act, logp, val, mean


# ---- 1. the policy step where a wave takes a second and later work items ----
@pytest.mark.parametrize("which", ["one_live_sample_in_the_second_item", "three_rounds_ragged", "headline_env_count_ragged"])
@pytest.mark.parametrize("obs_dim,act_dim", [(9, 8), (60, 38), (95, 64)])
def test_policy_step_in_its_persistent_regime(obs_dim, act_dim, which):
    import torch
    n_cu = _n_cu()
    n = {"one_live_sample_in_the_second_item": 256 * n_cu + 1, "three_rounds_ragged": 768 * n_cu + 77,
         "headline_env_count_ragged": 1024 * n_cu + 323}[which]
    n_tiles = (n + 63) // 64
    assert 2 * n_tiles > 8 * n_cu                       # more (tile, net) items than the 2 n_cu workgroups have waves
    assert n % 64 != 0                                  # ragged last tile, met on a later round
    if which == "one_live_sample_in_the_second_item":
        assert n % 64 == 1 and 2 * n_tiles == 8 * n_cu + 2
    policy = _policy(obs_dim, act_dim, obs_dim + act_dim).cuda()
    ref = _policy(obs_dim, act_dim, obs_dim + act_dim).double()
    obs = np.random.default_rng(n).uniform(-2.0, 2.0, (n, obs_dim)).astype(np.float32)
    o64 = torch.from_numpy(obs).double()
    with torch.no_grad():
        d = ref.dist(o64)
        mean_ref, val_ref = d.mean.numpy(), ref.value(o64).numpy()
    o = torch.from_numpy(obs).cuda()
    act, logp, val, mean = _step_padded(policy, o)
    for t in (act, logp, val, mean):
        assert (t[n:] == SENTINEL).all()                # nothing written past n
    act_h, logp_h, val_h, mean_h = (t[:n].cpu().numpy() for t in (act, logp, val, mean))
    e_mean, e_val = np.abs(mean_h - mean_ref).max(), np.abs(val_h - val_ref).max()
    with torch.no_grad():
        logp_ref = d.log_prob(torch.from_numpy(act_h).double()).sum(-1).numpy()
    e_logp = np.abs(logp_h - logp_ref).max()
    print("n = %d: mean %.3g  value %.3g  logp %.3g" % (n, e_mean, e_val, e_logp))
    assert e_mean < 2e-5 * max(1.0, np.abs(mean_ref).max())
    assert e_val < 2e-5 * max(1.0, np.abs(val_ref).max())
    assert e_logp < 1e-4 * max(1.0, np.abs(logp_ref).max())
    # without the mean output: the same bits, and still nothing past n
    act2, logp2, val2, _ = _step_padded(policy, o, with_mean=False)
    assert torch.equal(act2, act) and torch.equal(logp2, logp) and torch.equal(val2, val)
    # deterministic: the action IS the mean
    a_det, _, v_det, m_det = _step_padded(policy, o, deterministic=True)
    assert torch.equal(a_det, m_det) and torch.equal(m_det, mean) and torch.equal(v_det, val)


# ---- 2. the exploration noise against its restatement ----
NOISE_TOL = 2e-3


def _noise_error(obs_dim, act_dim, n, offset=0, step=3, step_base=None, seed=5):
    """max |eps_kernel - eps_restated| with eps_kernel = (act - mean) / std of ONE launch; also returns act (device)."""
    import torch
    from oracle.policy_ref import policy_noise
    policy = _policy(obs_dim, act_dim, 1).cuda()
    obs = torch.from_numpy(np.random.default_rng(act_dim).uniform(-1, 1, (n, obs_dim)).astype(np.float32)).cuda()
    base = None if step_base is None else torch.tensor([step_base], dtype=torch.int32, device="cuda")
    act, _, _, mean = _step_padded(policy, obs, seed=seed, step=step, step_base=base, sample_offset=offset)
    std = np.exp(policy.log_std.detach().cpu().double().numpy())
    eps = (act[:n].cpu().double().numpy() - mean[:n].cpu().double().numpy()) / std
    ids = np.arange(n, dtype=np.uint64) + np.uint64(offset)
    want = policy_noise(seed, ids, step + (step_base or 0), act_dim)
    return np.abs(eps - want).max(), act


@pytest.mark.parametrize("act_dim", [1, 3, 8, 33, 38, 64])
def test_noise_equals_the_restated_draw_for_every_block_and_component(act_dim):
    """Observed on the MI355X: 1.07e-6, 1.50e-6, 1.46e-6, 1.51e-6, 1.48e-6, 1.59e-6 for 1, 3, 8, 33, 38, 64 actions (the fp32
    restatement itself is 1.65e-6 from float64): __logf / __sincosf cost nothing visible on these inputs."""
    err, _ = _noise_error(10, act_dim, 4097)
    print("act_dim %d: max |eps - restated| = %.3g" % (act_dim, err))
    assert err < NOISE_TOL


def test_noise_equals_the_restated_draw_in_the_persistent_regime():
    """Observed on the MI355X (256 CUs, n = 65 537): 1.85e-6."""
    n_cu = _n_cu()
    n = 256 * n_cu + 1
    assert 2 * ((n + 63) // 64) > 8 * n_cu
    err, _ = _noise_error(9, 8, n)
    print("n = %d: max |eps - restated| = %.3g" % (n, err))
    assert err < NOISE_TOL


@pytest.mark.parametrize("offset", [0, 77_777, 2 ** 32 - 5, 2 ** 40 + 3])
def test_noise_is_keyed_by_both_words_of_the_sample_id(offset):
    """Observed on the MI355X: 1.67e-6, 1.31e-6, 1.30e-6, 1.45e-6 for the four offsets."""
    err, _ = _noise_error(9, 8, 4097, offset=offset)
    print("offset %d: max |eps - restated| = %.3g" % (offset, err))
    assert err < NOISE_TOL


def test_noise_step_is_the_sum_of_step_and_step_base():
    import torch
    e0, a0 = _noise_error(9, 8, 4097, step=3)
    e1, a1 = _noise_error(9, 8, 4097, step=0, step_base=3)
    e2, a2 = _noise_error(9, 8, 4097, step=1, step_base=2)
    assert max(e0, e1, e2) < NOISE_TOL
    assert torch.equal(a0, a1) and torch.equal(a0, a2)


def test_noise_at_the_two_ends_of_u1():
    """u1 = 2^-24 (the largest radius, sqrt(48 ln 2) = 5.768) stays finite and as restated; u1 = 1 gives eps = 0, so
    the first two actions equal their means exactly.  Observed on the MI355X at u1 = 2^-24: 1.71e-6."""
    import torch
    from oracle.policy_ref import policy_noise
    policy = _policy(9, 8, 1).cuda()
    std = np.exp(policy.log_std.detach().cpu().double().numpy())
    obs = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (1, 9)).astype(np.float32)).cuda()
    act, logp, _, mean = _step_padded(policy, obs, seed=5, step=0, sample_offset=ID_U1_SMALLEST)
    eps = (act[:1].cpu().double().numpy() - mean[:1].cpu().double().numpy()) / std
    want = policy_noise(5, [ID_U1_SMALLEST], 0, 8)
    assert abs(math.hypot(want[0, 0], want[0, 1]) - math.sqrt(48.0 * math.log(2.0))) < 1e-12
    assert np.isfinite(eps).all() and torch.isfinite(logp[:1]).all()
    print("u1 = 2^-24: max |eps - restated| = %.3g" % np.abs(eps - want).max())
    assert np.abs(eps - want).max() < NOISE_TOL
    act, logp, _, mean = _step_padded(policy, obs, seed=5, step=0, sample_offset=ID_U1_ONE)
    assert torch.equal(act[0, 0:2], mean[0, 0:2]) and torch.isfinite(logp[:1]).all()
    eps = (act[:1].cpu().double().numpy() - mean[:1].cpu().double().numpy()) / std
    assert np.abs(eps - policy_noise(5, [ID_U1_ONE], 0, 8)).max() < NOISE_TOL


# ---- 3. / 4. the gradient in the form PPO._minibatch_step_fused calls it ----
CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.1


def _rollout_form_errors(obs_dim, act_dim, B, rows, want_form, with_fp32_statement=False):
    """FusedPolicyGrad.run(index=, adv_stats=) over rollout tensors of `rows` rows (NaN outside the index, raw advantage
    3 randn + 1.5 everywhere) against ppo_grad64 on the gathered rows with the advantage normalised in float64.
    Returns (worst per-tensor relative error, pg error, vf error, scales, fp32 statement's worst error or None)."""
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad
    from oracle.policy_ref import adv_stats64, ppo_grad64
    assert pn.load().rp_grad_form(obs_dim, act_dim) == want_form
    policy = _policy(obs_dim, act_dim, 11 + obs_dim).cuda()
    ref = _policy(obs_dim, act_dim, 11 + obs_dim).double()
    obs, act, _, logp_old, val_old, ret = [t.float() for t in _minibatch(ref, obs_dim, act_dim, B, B, CLIP)]
    g = torch.Generator().manual_seed(B + 1)
    idx = torch.randperm(rows, generator=g)[:B]
    adv_full = torch.randn(rows, generator=g) * 3.0 + 1.5
    mean, inv = adv_stats64(adv_full.numpy(), idx.numpy())
    adv64 = (adv_full[idx].double() - mean) * inv
    pg_ref, vf_ref = ppo_grad64(ref, obs.double(), act.double(), adv64, logp_old.double(), val_old.double(), ret.double(),
                                CLIP, VF_COEF, ENT_COEF)
    e32 = None
    if with_fp32_statement:
        p32 = _policy(obs_dim, act_dim, 11 + obs_dim)
        ppo_grad64(p32, obs, act, adv64.float(), logp_old, val_old, ret, CLIP, VF_COEF, ENT_COEF)
        e32 = max((p.grad.double() - q.grad).abs().max().item() / max(q.grad.abs().max().item(), 1e-6)
                  for p, q in zip(p32.parameters(), ref.parameters()))
    idx_d = idx.cuda()
    big = []
    for t in (obs, act, logp_old, val_old, ret):
        b = torch.full((rows,) + tuple(t.shape[1:]), float("nan"), device="cuda")
        b[idx_d] = t.cuda()
        big.append(b)
    adv_d = adv_full.cuda()
    fg = FusedPolicyGrad(policy)
    bits = []
    for _ in range(2):
        stats = fg.minibatch_adv_stats(adv_d, idx_d)
        pg, vf = fg.run(big[0], big[1], adv_d, big[2], big[3], big[4], CLIP, VF_COEF, ENT_COEF, index=idx_d, adv_stats=stats)
        torch.cuda.synchronize()
        bits.append(fg._g.clone())
    assert torch.equal(bits[0], bits[1])                       # the same call twice: the same bits
    assert torch.isfinite(fg._g).all()                         # a row outside the index would have brought its NaN
    worst = 0.0
    for (name, p), (_, q) in zip(policy.named_parameters(), ref.named_parameters()):
        scale = max(q.grad.abs().max().item(), 1e-6)
        worst = max(worst, (p.grad.detach().cpu().double() - q.grad).abs().max().item() / scale)
    return worst, abs(pg.item() - pg_ref), abs(vf.item() - vf_ref), (abs(pg_ref), abs(vf_ref)), e32


def _check_rollout_form(obs_dim, act_dim, B, want_form):
    worst, e_pg, e_vf, (s_pg, s_vf), _ = _rollout_form_errors(obs_dim, act_dim, B, 3 * B, want_form)
    print("(%d, %d) B = %d form %d: gradient %.3g  pg %.3g  vf %.3g" % (obs_dim, act_dim, B, want_form, worst, e_pg, e_vf))
    assert e_pg < 1e-4 * max(1.0, s_pg) and e_vf < 1e-4 * max(1.0, s_vf)
    assert worst < 5e-4


@pytest.mark.parametrize("B", [2, 37, 64, 65, 1000, 70001, 200000])
@pytest.mark.parametrize("obs_dim,act_dim,form", [(9, 8, 2), (29, 8, 2), (30, 8, 1), (60, 38, 0)])
def test_gradient_through_index_and_in_kernel_normalisation_matches_float64(obs_dim, act_dim, form, B):
    if os.environ.get("ROBOY_POLICY_PREFETCH", "1")[0] == "0" and form == 2:
        form = 1                                               # the variable turns the prefetching form into the plain small one
    _check_rollout_form(obs_dim, act_dim, B, form)


@pytest.mark.parametrize("B", [65, 70001])
def test_gradient_without_prefetch_matches_float64_too(B):
    """ROBOY_POLICY_PREFETCH=0 is read once per process: a child runs (9, 8) in form 1 against the same float64."""
    env = dict(os.environ, ROBOY_POLICY_PREFETCH="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = "import test_policy_scale_gpu as t; t._check_rollout_form(9, 8, %d, 1)" % B
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + ["-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "form 1" in out.stdout


@pytest.mark.parametrize("B,rows", [(2_097_152, 8_388_608), (8_388_608, 33_554_432)])
def test_gradient_many_tiles_deep(B, rows):
    """(9, 8); 2 097 152 samples out of a rollout of 8 388 608 rows (32 tiles per wave at 256 CUs) and 8 388 608 out of
    33 554 432 (128 tiles per wave: the minibatch of 262 144 envs x 128 steps).  The bound is set by the plain fp32 statement
    (ppo_grad64 on float32 copies, same chunks): the kernel may be 4 times as far from float64 as that, never more than
    5e-3, and passes outright below 5e-4.
    Measured on the MI355X (256 CUs), 32 tiles: fp32 statement 3.19e-5, kernel 3.22e-5 (loss terms 7.5e-9 / 3.2e-8);
    128 tiles: fp32 statement 6.37e-5, kernel 5.97e-5 (loss terms 1.4e-8 / 4.6e-8)."""
    assert ((B + 63) // 64) // (4 * _n_cu()) >= 16            # tiles per wave (4 n_cu waves): deep, whatever the CU count
    worst, e_pg, e_vf, (s_pg, s_vf), e32 = _rollout_form_errors(9, 8, B, rows, 2, with_fp32_statement=True)
    print("depth %d: fp32 statement %.3g, kernel %.3g, pg %.3g, vf %.3g" % (B, e32, worst, e_pg, e_vf))
    assert e_pg < 1e-4 * max(1.0, s_pg) and e_vf < 1e-4 * max(1.0, s_vf)
    assert worst < 5e-3
    assert worst < 5e-4 or worst <= 4.0 * e32


# ---- 5. advantage statistics ----
def _stats_fg():
    from gym_roboy_amd.ppo import FusedPolicyGrad
    return FusedPolicyGrad(_policy(9, 8, 1).cuda())


@pytest.mark.parametrize("B", [522_241, 2_097_152])
def test_advantage_statistics_with_all_256_blocks(B):
    import torch
    from oracle.policy_ref import adv_stats64
    assert (B + 2047) // 2048 >= 256                           # the last block sums 256 partials
    fg = _stats_fg()
    g = torch.Generator().manual_seed(B)
    adv = torch.randn(4 * B, generator=g) * 3.0 + 1.5
    idx = torch.randperm(4 * B, generator=g)[:B]
    mean, inv = adv_stats64(adv.numpy(), idx.numpy())
    adv_d, idx_d = adv.cuda(), idx.cuda()
    for _ in range(3):                                         # the ticket is left ready for the next call
        st = fg.minibatch_adv_stats(adv_d, idx_d).cpu()
        assert abs(st[0].item() - mean) < 1e-5 * max(1.0, abs(mean))
        assert abs(st[1].item() - inv) < 1e-4 * inv


def test_advantage_statistics_of_a_narrow_distribution_far_from_zero():
    import torch
    from oracle.policy_ref import adv_stats64
    fg = _stats_fg()
    g = torch.Generator().manual_seed(7)
    adv = 100.0 + 0.01 * torch.randn(4000, generator=g)
    idx = torch.randperm(4000, generator=g)[:1000]
    mean, inv = adv_stats64(adv.numpy(), idx.numpy())
    for _ in range(3):
        st = fg.minibatch_adv_stats(adv.cuda(), idx.cuda()).cpu()
        assert abs(st[0].item() - mean) < 1e-5 * max(1.0, abs(mean))
        assert abs(st[1].item() - inv) < 1e-4 * inv


def test_advantage_statistics_of_constant_advantages():
    import torch
    fg = _stats_fg()
    for _ in range(3):
        half = torch.full((1000,), 0.5, device="cuda")         # sums exact in fp64: variance exactly 0
        st = fg.minibatch_adv_stats(half, None).cpu()
        assert st[0].item() == 0.5 and abs(st[1].item() - 1e8) < 1e-4 * 1e8
        tenth = torch.full((1000,), 0.1, device="cuda")        # 0.1f: the one-pass variance may keep a rounding residue
        st = fg.minibatch_adv_stats(tenth, None)
        assert st[0].item() == tenth[0].item() and math.isfinite(st[1].item())
        assert ((tenth - st[0]) * st[1] == 0).all()


# ---- 6. clip + Adam ----
LR, BETAS, ADAM_EPS, MAX_NORM = 2.5e-4, (0.9, 0.999), 1e-5, 0.5
# Bounds for the moments, which the parameters' tolerance (2e-6 per step, as tests/test_policy_gpu.py) cannot see because
# Adam's step is insensitive to the gradient's scale: the squared norm is summed in fp32 by 1 024 threads (each ~10 to 20
# terms, 6 shuffle steps, 16 partials: some 40 roundings of 2^-24 = 2.4e-6 relative at worst, half of it after the square
# root), and m, v take three more roundings each; v carries the coefficient squared.
M_TOL, V_TOL = 1e-5, 2e-5


def _adam_setup(obs_dim, act_dim):
    import torch
    from gym_roboy_amd import _policy_native as pn
    layout, n = pn.grad_layout(obs_dim, act_dim)
    shapes = pn.param_shapes(obs_dim, act_dim)
    slots = [(layout[k][0], layout[k][0] + int(np.prod(shapes[k]))) for k in pn.PARAM_ORDER]
    is_param = np.zeros(n, dtype=bool)
    for lo, hi in slots:
        is_param[lo:hi] = True
    ls = (layout["log_std"][0], layout["log_std"][0] + act_dim)
    assert not is_param[layout["pi_loss"][0]] and not is_param[layout["vf_loss"][0]] and (~is_param).sum() >= 4
    return n, slots, torch.from_numpy(is_param).cuda(), ls


def _clip_adam(params, grad, m, v, obs_dim, act_dim, step, scale, ent_coef):
    import torch
    from gym_roboy_amd import _policy_native as pn
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pn.check(pn.load().rp_clip_adam_dev(p(params), p(grad), p(m), p(v), obs_dim, act_dim, LR, BETAS[0], BETAS[1], ADAM_EPS, step,
                                        MAX_NORM, scale, ent_coef, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _assert_adam_close(got, want, is_param, steps_taken=1):
    mask = is_param.cpu().numpy()
    for name, g, w, tol in (("params", got[0], want[0], None), ("m", got[1], want[1], M_TOL), ("v", got[2], want[2], V_TOL)):
        g, w = g.cpu().double().numpy()[mask], w[mask]
        assert np.isfinite(g).all()
        err = np.abs(g - w).max()
        assert err < (2e-6 * steps_taken if tol is None else tol * np.abs(w).max()), (name, err)


def _state(n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    params = torch.randn(n, device="cuda", generator=g)
    m = 0.01 * torch.randn(n, device="cuda", generator=g)
    v = (0.01 * torch.randn(n, device="cuda", generator=g)) ** 2 + 1e-6
    return params, m, v, g


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.125])
@pytest.mark.parametrize("obs_dim,act_dim", [(9, 8), (60, 38)])
def test_clip_adam_takes_the_mean_over_ranks_of_gradients_that_each_carry_the_entropy_term(obs_dim, act_dim, scale):
    """The kernel is fed the SUM of the ranks' raw gradients and grad_scale = 1 / world; the float64 statement is fed
    the mean of the ranks' gradients after each subtracted ent_coef on its log-std.  Step numbers 1, 2, 1 000, 100 000."""
    import torch
    from oracle.policy_ref import clip_adam64
    n, slots, is_param, ls = _adam_setup(obs_dim, act_dim)
    world = int(round(1.0 / scale))
    for step, mag in ((1, 5.0), (2, 1e-3), (1000, 0.02), (100_000, 2.0)):        # norms on both sides of the bound
        params, m, v, g = _state(n, step)
        per_rank = [torch.randn(n, device="cuda", generator=g) * mag / math.sqrt(n) for _ in range(world)]
        summed = torch.stack(per_rank).sum(0)
        mean64 = np.zeros(n)
        for r in per_rank:
            r64 = r.cpu().double().numpy()
            r64[ls[0]:ls[1]] -= ENT_COEF
            mean64 += r64 / world
        want = clip_adam64(params.cpu().numpy(), mean64, m.cpu().numpy(), v.cpu().numpy(), slots, LR, BETAS, ADAM_EPS, step,
                           MAX_NORM, 1.0, 0.0, ls)
        _clip_adam(params, summed, m, v, obs_dim, act_dim, step, scale, ENT_COEF)
        _assert_adam_close((params, m, v), want, is_param)


@pytest.mark.parametrize("obs_dim,act_dim", [(9, 8), (60, 38)])
def test_clip_adam_just_below_and_just_above_the_norm_bound(obs_dim, act_dim):
    import torch
    from oracle.policy_ref import clip_adam64
    n, slots, is_param, ls = _adam_setup(obs_dim, act_dim)
    ent = 0.01                                                 # sqrt(act_dim) * ent is the norm's floor: well under the bound
    for k, factor in enumerate((0.999, 1.001)):
        params, m, v, g = _state(n, 10 + k)
        m.zero_(); v.zero_()
        grad = torch.randn(n, device="cuda", generator=g)
        grad[~is_param] = 1e3                                  # were these counted, both cases would be clipped hard
        g64 = grad.cpu().double().numpy()
        g64[ls[0]:ls[1]] -= ent
        norm = math.sqrt((g64[is_param.cpu().numpy()] ** 2).sum())
        # scale the raw gradient so that the norm WITH the entropy term lands at factor * MAX_NORM (two passes: the term is fixed)
        for _ in range(30):
            grad[is_param] *= factor * MAX_NORM / norm
            g64 = grad.cpu().double().numpy()
            g64[ls[0]:ls[1]] -= ent
            norm = math.sqrt((g64[is_param.cpu().numpy()] ** 2).sum())
        assert abs(norm / MAX_NORM - factor) < 1e-5
        want = clip_adam64(params.cpu().numpy(), grad.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), slots, LR, BETAS, ADAM_EPS, 1,
                           MAX_NORM, 1.0, ent, ls)
        _clip_adam(params, grad, m, v, obs_dim, act_dim, 1, 1.0, ent)
        _assert_adam_close((params, m, v), want, is_param)
        # the first moment of step 1 is 0.1 g coef: below the bound coef = 1, above it max_norm / (norm + 1e-6)
        coef = 1.0 if factor < 1 else MAX_NORM / (norm + 1e-6)
        mask = is_param.cpu().numpy()
        assert np.abs(m.cpu().double().numpy()[mask] - 0.1 * coef * g64[mask]).max() < M_TOL * 0.1 * np.abs(g64[mask]).max()


@pytest.mark.parametrize("obs_dim,act_dim", [(9, 8), (60, 38)])
def test_clip_adam_with_a_zero_gradient_changes_nothing(obs_dim, act_dim):
    import torch
    from gym_roboy_amd.ppo import FusedAdam, FusedPolicyGrad
    fg = FusedPolicyGrad(_policy(obs_dim, act_dim, 3).cuda())
    fa = FusedAdam(fg, LR, eps=ADAM_EPS, max_grad_norm=MAX_NORM)
    before = fa.params.clone()
    fg._g.zero_()
    for _ in range(3):
        fa.step(0.0)
    torch.cuda.synchronize()
    assert torch.equal(fa.params, before) and (fa.m == 0).all() and (fa.v == 0).all()
    assert torch.isfinite(fa.params).all()


@pytest.mark.parametrize("obs_dim,act_dim", [(9, 8), (60, 38)])
def test_clip_adam_neither_reads_nor_writes_the_slots_that_hold_no_parameter(obs_dim, act_dim):
    """The two loss blocks, the value net's log-std slot and the padding of d_grad hold NaN: the update is finite, equals the
    float64 statement, and those slots of params / m / v keep their bits."""
    import torch
    from oracle.policy_ref import clip_adam64
    n, slots, is_param, ls = _adam_setup(obs_dim, act_dim)
    params, m, v, g = _state(n, 21)
    marks = (torch.arange(n, device="cuda", dtype=torch.float32) + 0.25)
    for t in (params, m, v):
        t[~is_param] = marks[~is_param]
    grad = torch.randn(n, device="cuda", generator=g) * 0.01
    grad[~is_param] = float("nan")
    want = clip_adam64(params.cpu().numpy(), grad.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), slots, LR, BETAS, ADAM_EPS, 7,
                       MAX_NORM, 1.0, ENT_COEF, ls)
    _clip_adam(params, grad, m, v, obs_dim, act_dim, 7, 1.0, ENT_COEF)
    _assert_adam_close((params, m, v), want, is_param)
    for t in (params, m, v):
        assert torch.equal(t[~is_param], marks[~is_param])


# ---- 7. GAE ----
@pytest.mark.parametrize("dones", ["none", "all", "last_step", "random"])
@pytest.mark.parametrize("T,N", [(1, 1), (1, 65), (37, 1000), (128, 4097), (16, 262144)])
def test_gae_matches_float64(T, N, dones):
    """The kernel may be 4 times as far from gae64 as ppo.gae in float32 on the CPU is (floor 1e-6 max |ref|).
    Measured on the MI355X: in all 20 cases the kernel is no farther from gae64 than the fp32 loop (equal where T = 1 or
    every step is done, up to 25 % nearer elsewhere: fma contraction).  Largest: ret at (128, 4 097), done on the last step,
    kernel 5.0e-6 against 5.2e-6 for the loop, max |ref| 13.7."""
    import torch
    from gym_roboy_amd.ppo import gae, gae_fused
    from oracle.policy_ref import gae64
    g = torch.Generator().manual_seed(T * 1000003 + N)
    rew, val = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g)
    last = torch.randn(N, generator=g)
    done = torch.zeros(T, N)
    if dones == "all":
        done[:] = 1.0
    elif dones == "last_step":
        done[-1] = 1.0
    elif dones == "random":
        done = (torch.rand(T, N, generator=g) < 0.05).float()
    adv_ref, ret_ref = gae64(rew.numpy(), val.numpy(), done.numpy(), last.numpy(), 0.99, 0.95)
    a32, r32 = gae(rew, val, done, last, 0.99, 0.95)           # the plain fp32 statement, on the CPU
    a, r = gae_fused(rew.cuda(), val.cuda(), done.cuda(), last.cuda(), 0.99, 0.95)
    torch.cuda.synchronize()
    for name, got, f32, ref in (("adv", a, a32, adv_ref), ("ret", r, r32, ret_ref)):
        e32 = np.abs(f32.double().numpy() - ref).max()
        err = np.abs(got.cpu().double().numpy() - ref).max()
        print("%s (%d, %d) %s: fp32 loop %.3g, kernel %.3g, max |ref| %.3g" % (name, T, N, dones, e32, err, np.abs(ref).max()))
        assert err <= max(4.0 * e32, 1e-6 * np.abs(ref).max())
