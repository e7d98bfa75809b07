"""Update diagnostics and the KL-adaptive learning rate on the GPU: the two slots rp_ppo_grad_diag_dev leaves in the
gradient vector against float64 in every kernel form, rp_clip_adam_kl_dev against the float32 restatement of the rule (bits) and
float64 Adam at that rate, the fused and the torch path taking the same decisions on the same rollout, and PPO under HIP graphs.

Bounds.  approx_kl: the project's loss-slot bound, 1e-4 max(1, |ref|).  clip_frac: the count may differ from float64's only by samples
within 1e-4 of the clip range ("borderline"), i.e. by borderline / B - plus what a float32 sum of float32 terms can be away from the
rational count / B at all: 2^-24 per rounding, one per addition along the longest chain of the sum (a lane's tiles, six shuffle steps,
three folds of the workgroup's waves, a quarter of the workgroups in the reduction, its three last additions) and one for 1 / B, each
on a value of at most `ref`.  At B = 70 001 that is 3e-6 against 1 / B = 1.4e-5: a sample counted wrongly still fails.  (For B = 2 and
B = 64 every term is exact and the allowance is not needed.)  Gradient and loss terms: _check_rollout_form's 5e-4 and 1e-4.
Adam: _assert_adam_close's bounds."""
import ctypes
import math

import numpy as np
import pytest

import ppo_diag_ref as dref
from test_policy_gpu import _minibatch, _policy
from test_policy_scale_gpu import ADAM_EPS, BETAS, CLIP, ENT_COEF, MAX_NORM, VF_COEF, _adam_setup, _assert_adam_close, _state

pytestmark = pytest.mark.gpu
F32 = np.float32

_CACHE = {}


def _case(obs_dim, act_dim, B, seed):
    """The minibatch of _rollout_form_errors (tests/test_policy_scale_gpu.py) for `seed`, with its float64 statements - computed once per
    (shape, B) and shared by the plain and the normalised test."""
    import torch
    from oracle.policy_ref import adv_stats64, ppo_grad64
    key = (obs_dim, act_dim, B, seed)
    if key not in _CACHE:
        ref = _policy(obs_dim, act_dim, 11 + obs_dim).double()
        obs, act, _, logp_old, val_old, ret = [t.float() for t in _minibatch(ref, obs_dim, act_dim, B, seed, CLIP)]
        g = torch.Generator().manual_seed(B + 1)
        rows = 3 * B
        idx = torch.randperm(rows, generator=g)[:B]
        adv_full = torch.randn(rows, generator=g) * 3.0 + 1.5
        _CACHE[key] = dict(ref=ref, obs=obs, act=act, logp_old=logp_old, val_old=val_old, ret=ret, idx=idx, adv_full=adv_full, rows=rows)
    return _CACHE[key]


def _clip_frac_rounding(B, ref, n_cu):
    tiles = (B + 63) // 64
    blocks = min((tiles + 3) // 4, n_cu)
    depth = -(-tiles // (4 * blocks)) + 6 + 3 + -(-blocks // 4) + 3 + 1
    return 2.0 ** -24 * depth * ref


# seeds of the minibatch per batch size (tests/test_policy_gpu.py: _minibatch draws logp_old = logp + U(-0.5, 0.5): approx_kl about 1 / 24,
# some 60 % of the ratios outside 1 -+ 0.2): the seed is B, as in _rollout_form_errors, but for B = 2, which needs a seed per shape
# with one sample inside the range and one outside (found on the CPU in float64; asserted again below)
SEEDS_B2 = {9: 0, 30: 1, 60: 1}


def _diag_slots(obs_dim, act_dim, form, B, with_norm):
    import torch
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import FusedPolicyGrad, ObsNorm
    from oracle.policy_ref import adv_stats64, ppo_grad64
    assert pn.load().rp_grad_form(obs_dim, act_dim) == form
    c = _case(obs_dim, act_dim, B, SEEDS_B2[obs_dim] if B == 2 else B)
    ref, idx, rows = c["ref"], c["idx"], c["rows"]
    norm = None
    obs_net = c["obs"]                                           # what the reference policy sees
    obs_raw = c["obs"]                                           # what the kernel reads
    if with_norm:
        # statistics under which the raw observation is obs * s + m: the normalised operand is obs again, up to its two float32 roundings
        g = torch.Generator().manual_seed(7)
        m, s = torch.randn(obs_dim, generator=g), torch.rand(obs_dim, generator=g) + 0.5
        obs_raw = (c["obs"] * s + m).contiguous()
        norm = ObsNorm(obs_dim, "cuda", clip=10.0)
        norm.norm[0] = m.cuda(); norm.norm[1] = (1.0 / s).cuda()
        obs_net = norm.apply(obs_raw.cuda()).cpu()               # the float32 statement of the operand (bit for bit the kernels')
    # the float64 statements, qualified before the GPU is asked
    d = dref.diag64(ref, obs_net, c["act"], c["logp_old"], CLIP)
    print("(%d, %d) B = %d form %d norm %d: float64 approx_kl %.6g clip_frac %.6g (%d low, %d high, %d borderline)"
          % (obs_dim, act_dim, B, form, with_norm, d["approx_kl"], d["clip_frac"], d["n_low"], d["n_high"], d["borderline"]))
    assert 0.005 <= d["approx_kl"] <= 0.5
    assert 0.05 <= d["clip_frac"] <= 0.95
    if B == 2:
        assert d["n_clipped"] == 1                               # not both samples on the same side
    assert d["borderline"] <= 0.01 * B
    mean, inv = adv_stats64(c["adv_full"].numpy(), idx.numpy())
    adv64 = (c["adv_full"][idx].double() - mean) * inv
    pg_ref, vf_ref = ppo_grad64(ref, obs_net.double(), c["act"].double(), adv64, c["logp_old"].double(), c["val_old"].double(),
                                c["ret"].double(), CLIP, VF_COEF, ENT_COEF)
    policy = _policy(obs_dim, act_dim, 11 + obs_dim).cuda()
    idx_d = idx.cuda()
    big = []
    for t in (obs_raw, c["act"], c["logp_old"], c["val_old"], c["ret"]):
        b = torch.full((rows,) + tuple(t.shape[1:]), float("nan"), device="cuda")
        b[idx_d] = t.cuda()
        big.append(b)
    adv_d = c["adv_full"].cuda()
    fg = FusedPolicyGrad(policy)
    fg._g.fill_(float("nan"))                                    # the slots are written, not added to
    bits = []
    for _ in range(2):
        stats = fg.minibatch_adv_stats(adv_d, idx_d)
        pg, vf = fg.run(big[0], big[1], adv_d, big[2], big[3], big[4], CLIP, VF_COEF, ENT_COEF, index=idx_d, adv_stats=stats, norm=norm,
                        diagnostics=True)
        torch.cuda.synchronize()
        bits.append(fg._g.clone())
    assert torch.equal(bits[0], bits[1])                         # the same call twice: the same bits
    assert torch.isfinite(fg._g).all()                           # a dead lane or a row outside the index would have brought its NaN
    kl, cf = (t.item() for t in fg.diag())
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tol_cf = d["borderline"] / B + _clip_frac_rounding(B, d["clip_frac"], n_cu)
    print("   kernel approx_kl %.9g (error %.3g)  clip_frac %.9g (error %.3g, allowed %.3g)"
          % (kl, abs(kl - d["approx_kl"]), cf, abs(cf - d["clip_frac"]), tol_cf))
    worst = 0.0
    for (name, p), (_, q) in zip(policy.named_parameters(), ref.named_parameters()):
        worst = max(worst, (p.grad.detach().cpu().double() - q.grad).abs().max().item() / max(q.grad.abs().max().item(), 1e-6))
    # the same call through the entry point without diagnostics: is everything but the two slots the same bits?
    fg.run(big[0], big[1], adv_d, big[2], big[3], big[4], CLIP, VF_COEF, ENT_COEF, index=idx_d, adv_stats=stats, norm=norm)
    torch.cuda.synchronize()
    lay = fg._layout
    keep = torch.ones_like(fg._g, dtype=torch.bool)
    keep[lay["pi_loss"][0] + 1:lay["pi_loss"][0] + 4] = False
    same = torch.equal(fg._g[keep], bits[0][keep])
    print("   gradient %.3g  pg %.3g  vf %.3g; gradient and loss terms bit-equal to the entry point without diagnostics: %s"
          % (worst, abs(pg.item() - pg_ref), abs(vf.item() - vf_ref), same))
    assert abs(kl - d["approx_kl"]) <= 1e-4 * max(1.0, abs(d["approx_kl"]))
    assert abs(cf - d["clip_frac"]) <= tol_cf
    assert abs(bits[0][lay["pi_loss"][0]].item() - pg_ref) < 1e-4 * max(1.0, abs(pg_ref))
    assert abs(bits[0][lay["vf_loss"][0]].item() - vf_ref) < 1e-4 * max(1.0, abs(vf_ref))
    assert worst < 5e-4


# ---- 6. the slots against float64 ----
@pytest.mark.parametrize("B", [2, 37, 64, 65, 1000, 70001])
@pytest.mark.parametrize("obs_dim,act_dim,form", [(9, 8, 2), (30, 8, 1), (60, 38, 0)])
def test_diagnostics_slots_match_float64(obs_dim, act_dim, form, B):
    _diag_slots(obs_dim, act_dim, form, B, False)


@pytest.mark.parametrize("B", [65, 1000])
@pytest.mark.parametrize("obs_dim,act_dim,form", [(9, 8, 2), (30, 8, 1), (60, 38, 0)])
def test_diagnostics_slots_match_float64_under_observation_normalisation(obs_dim, act_dim, form, B):
    _diag_slots(obs_dim, act_dim, form, B, True)


# ---- 7. clip + Adam with the rule ----
D, F, LO, HI = 0.01, 1.5, 1e-5, 1e-2


def _clip_adam_kl(params, grad, m, v, lr_dev, obs_dim, act_dim, step, scale, ent_coef, d=D, f=F, lo=LO, hi=HI):
    import torch
    from gym_roboy_amd import _policy_native as pn
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = pn.load().rp_clip_adam_kl_dev(p(params), p(grad), p(m), p(v), obs_dim, act_dim, p(lr_dev), d, f, lo, hi, BETAS[0], BETAS[1], ADAM_EPS,
                                       step, MAX_NORM, scale, ent_coef, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("obs_dim,act_dim", [(9, 8), (60, 38)])
def test_clip_adam_kl_moves_the_rate_by_the_rule_and_steps_at_it(obs_dim, act_dim):
    import torch
    from gym_roboy_amd import _policy_native as pn
    n, slots, is_param, ls = _adam_setup(obs_dim, act_dim)
    layout, _ = pn.grad_layout(obs_dim, act_dim)
    kl_slot = layout["approx_kl"][0]
    assert not is_param[kl_slot]
    nan = float("nan")
    #        lr before, KL slot, grad_scale
    calls = [(2.5e-4, 0.05, 1.0),             # above 2 d: cut
             (2.5e-4, 0.001, 1.0),            # below d / 2: raised
             (2.5e-4, 0.01, 1.0),             # between: unchanged
             (2.5e-4, 0.0, 1.0),              # 0: unchanged
             (2.5e-4, nan, 1.0),              # NaN: unchanged
             (HI, 0.001, 1.0),                # at lr_max, low KL: stays
             (LO, 0.05, 1.0),                 # at lr_min, high KL: stays
             (2.5e-4, 0.03 + 0.004, 0.5)]     # two ranks: 0.03 (above 2 d) + 0.004 (below d / 2); their mean 0.017 lies between: unchanged
    moved = []
    for step, (lr0, slot, scale) in enumerate(calls, start=1):
        params, m, v, g = _state(n, 40 + step)
        marks = torch.arange(n, device="cuda", dtype=torch.float32) + 0.25
        for t in (params, m, v):
            t[~is_param] = marks[~is_param]
        grad = torch.randn(n, device="cuda", generator=g) * 0.02
        grad[~is_param] = nan                                    # every other non-parameter slot must not be read
        grad[kl_slot] = slot
        lr_dev = torch.full((1,), float(F32(lr0)), device="cuda")
        want_lr, want = dref.clip_adam_kl64(params.cpu().numpy(), grad.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), slots, lr0, kl_slot,
                                            D, F, LO, HI, BETAS, ADAM_EPS, step, MAX_NORM, scale, ENT_COEF, ls)
        assert _clip_adam_kl(params, grad, m, v, lr_dev, obs_dim, act_dim, step, scale, ENT_COEF) == 0
        got_lr = lr_dev.cpu().numpy()[0]
        print("call %d: lr %.9g -> %.9g (restated %.9g), slot %r x %g" % (step, F32(lr0), got_lr, want_lr, slot, scale))
        assert got_lr.tobytes() == want_lr.tobytes()
        _assert_adam_close((params, m, v), want, is_param)
        for t in (params, m, v):
            assert torch.equal(t[~is_param], marks[~is_param])
        moved.append(float(want_lr) / float(F32(lr0)))
    assert moved[0] < 1 < moved[1] and moved[2:] == [1.0] * 6    # the cases are what they say
    # the step really is taken at the new rate: at the old one the parameters would be off by (1 - 1 / f) of a step of about lr
    assert abs(1.0 / F - moved[0]) < 1e-6


def test_clip_adam_kl_argument_errors():
    import torch
    from gym_roboy_amd import _policy_native as pn
    n = pn.grad_layout(9, 8)[1]
    params, m, v, _ = _state(n, 3)
    grad = torch.zeros(n, device="cuda")
    lr_dev = torch.full((1,), 2.5e-4, device="cuda")
    before = params.clone()
    for kw in (dict(d=0.0), dict(d=-1.0), dict(f=1.0), dict(f=0.5), dict(lo=0.0), dict(lo=1e-2, hi=1e-3)):
        assert _clip_adam_kl(params, grad, m, v, lr_dev, 9, 8, 1, 1.0, 0.0, **kw) == -1, kw
    assert _clip_adam_kl(params, grad, m, v, None, 9, 8, 1, 1.0, 0.0) == -1
    assert _clip_adam_kl(None, grad, m, v, lr_dev, 9, 8, 1, 1.0, 0.0) == -1
    assert _clip_adam_kl(params, grad, m, v, lr_dev, 9, 8, 0, 1.0, 0.0) == -1
    assert torch.equal(params, before) and lr_dev.item() == float(F32(2.5e-4))


# ---- 8. fused and torch paths take the same decisions ----
DESIRED_KL_8, SEED_8 = 1e-3, 4


def test_fused_and_torch_paths_take_the_same_decisions():
    """Both optimiser paths on the SAME rollout and sample orders, lr_schedule="adaptive": the per-minibatch learning rates are equal
    bit for bit, provided no minibatch's KL lies within 5 % of a threshold (asserted on the torch path).  MsjRobot, 256 envs x 8 steps,
    desired_kl = 1e-3 and lr_max = 1e-3, seed 4: on the MI355X the KL climbs from 2.3e-4 to 4e-3, the rate is raised four times (to
    lr_max) and cut seven times, the closest KL is 13.7 % from a threshold and the parameters end 1.2e-7 apart."""
    import copy
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env = RoboyVecEnv(MsjRobot(), 256, seed=1)
    kw = dict(n_steps=8, seed=SEED_8, reward_scale=0.01, lr_schedule="adaptive", desired_kl=DESIRED_KL_8, lr_max=1e-3)
    a = PPO(env, fused_update=True, **kw)
    b = PPO(env, fused_policy=False, fused_update=False, **kw)
    assert a._fgrad is not None and b._fgrad is None
    roll = a.collect()
    # the update starts from a policy slightly off the one that collected the rollout, as every epoch but the first does: with the very
    # same policy the first minibatch's KL is the rounding noise between two evaluations of one log-probability (1e-13, or exactly 0),
    # and whether the rule's `kl > 0` holds is then an accident of either path's arithmetic
    gp = torch.Generator(device="cuda").manual_seed(SEED_8 + 100)
    with torch.no_grad():
        for p in a.policy.parameters():
            p.add_(0.003 * torch.randn(p.shape, device="cuda", generator=gp))
    b.policy.load_state_dict(copy.deepcopy(a.policy.state_dict()))
    n = roll["obs"].shape[0] * roll["obs"].shape[1]
    g = torch.Generator(device="cuda").manual_seed(SEED_8)
    orders = [torch.randperm(n, device="cuda", generator=g) for _ in range(a.noptepochs)]
    a.lr_history, b.lr_history = [], []
    sa = a.update({k: v.clone() for k, v in roll.items()}, sample_orders=orders)
    sb = b.update({k: v.clone() for k, v in roll.items()}, sample_orders=orders)
    kl_a, lr_a = [float(k.item()) for k, _ in a.lr_history], [float(l.item()) for _, l in a.lr_history]
    kl_b, lr_b = [k for k, _ in b.lr_history], [l for _, l in b.lr_history]
    print("torch kl", ["%.3g" % k for k in kl_b]); print("fused kl", ["%.3g" % k for k in kl_a])
    print("torch lr", ["%.4g" % l for l in lr_b]); print("fused lr", ["%.4g" % l for l in lr_a])
    assert len(lr_a) == len(lr_b) == a.noptepochs * a.nminibatches
    d = DESIRED_KL_8
    for k in kl_b:                                               # qualification: no decision hangs on rounding
        assert k > 1e-8 and abs(k - 0.5 * d) >= 0.05 * 0.5 * d and abs(k - 2 * d) >= 0.05 * 2 * d, k
    steps = [y / x for x, y in zip([float(F32(2.5e-4))] + lr_b[:-1], lr_b)]
    assert any(s < 1 for s in steps) and any(s > 1 for s in steps)       # at least one cut and one raise
    assert lr_a == lr_b
    assert sa["lr"] == sb["lr"] == lr_b[-1] == a.learning_rate == b.learning_rate
    print("last minibatch: fused", sa["approx_kl"], sa["clip_frac"], "torch", sb["approx_kl"], sb["clip_frac"])
    for (name, p), (_, q) in zip(a.policy.named_parameters(), b.policy.named_parameters()):
        assert (p - q).abs().max().item() < 2e-4, name          # tests/test_policy_gpu.py: 16 clip + Adam steps apart by rounding only
    env.close()


# ---- 9. under HIP graphs, and across a checkpoint ----
def test_ppo_under_graphs_with_the_schedule_and_its_checkpoint(tmp_path):
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env = RoboyVecEnv(MsjRobot(), 4096, seed=2)
    kw = dict(n_steps=16, seed=2, reward_scale=0.01, use_graphs=True, lr_schedule="adaptive")
    agent = PPO(env, **kw)
    assert agent._fgrad is not None and agent.use_graphs
    for _ in range(2):
        stats = agent.update(agent.collect())
        print(stats)
        assert math.isfinite(stats["approx_kl"]) and stats["approx_kl"] >= 0.0 and 0.0 <= stats["clip_frac"] <= 1.0
        assert agent.lr_min <= stats["lr"] <= agent.lr_max and stats["lr"] == agent.learning_rate
        assert all(math.isfinite(x) for x in stats.values())
    assert stats["lr"] != float(F32(2.5e-4))                     # two rounds of 16 minibatches moved it
    path = str(tmp_path / "model.pkl")
    agent.save(path)
    assert torch.load(path)["lr_schedule"]["lr"] == agent.learning_rate
    env2 = RoboyVecEnv(MsjRobot(), 4096, seed=3)
    other = PPO(env2, **kw).load(path)
    assert other.learning_rate == agent.learning_rate
    for p, q in zip(agent.policy.parameters(), other.policy.parameters()):
        assert torch.equal(p, q)
    stats = other.update(other.collect())
    assert math.isfinite(stats["approx_kl"]) and other.lr_min <= stats["lr"] <= other.lr_max
    env.close(); env2.close()
