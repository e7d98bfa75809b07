"""The float64 statements of the PPO operations (oracle/policy_ref.py) against what they restate: torch's own
optimiser, autograd and the GAE loop of gym_roboy_amd/ppo.py in float64, and the noise's distribution.  No GPU."""
import math

import numpy as np

from oracle import philox_np
from oracle import policy_ref as pr

# the two ends of u1 = ((w >> 8) + 1) / 2^24 (seed 5, step 0, block 0, word 0), by sample id
ID_U1_SMALLEST, ID_U1_ONE = 9_271_651, 31_776_762


def _policy64(obs_dim, act_dim, seed):
    import torch
    from gym_roboy_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    p = MlpPolicy(obs_dim, act_dim)
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.3 * torch.randn_like(q))
    return p.double()


def test_noise_is_standard_normal_and_its_fp32_evaluation_is_close():
    ids = np.arange(300_000, dtype=np.uint64) + np.uint64(12345)
    eps = pr.policy_noise(5, ids, 3, 8)                                   # 2.4e6 draws
    assert eps.shape == (300_000, 8) and eps.dtype == np.float64
    assert abs(eps.mean()) < 0.005 and abs(eps.var() - 1.0) < 0.005 and abs((eps ** 4).mean() - 3.0) < 0.05
    assert np.abs(np.corrcoef(eps.T) - np.eye(8)).max() < 0.01
    assert abs(np.corrcoef(eps[:-1, 0], eps[1:, 0])[0, 1]) < 0.01
    eps32 = pr.policy_noise(5, ids, 3, 8, dtype=np.float32)
    assert eps32.dtype == np.float32
    err = np.abs(eps32.astype(np.float64) - eps).max()
    print("fp32 evaluation against fp64: %.3g, max |eps| %.3f" % (err, np.abs(eps).max()))
    assert err < 1e-5
    # the layout: action j = component j & 3 of block j >> 2; a narrower policy sees a prefix of a wider one's noise
    wide = pr.policy_noise(5, ids[:1000], 3, 38)
    assert np.array_equal(wide[:, :8], eps[:1000])
    assert np.array_equal(pr.policy_noise(5, ids[:1000], 3, 3), eps[:1000, :3])
    w = philox_np.draw(5, ids[:1000], 3, pr.STREAM_POLICY, 9)
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) / 2.0 ** 24
    u2 = (w[:, 1] >> np.uint32(8)).astype(np.float64) / 2.0 ** 24
    assert np.allclose(wide[:, 36], np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2), rtol=0, atol=1e-14)
    assert np.allclose(wide[:, 37], np.sqrt(-2.0 * np.log(u1)) * np.sin(2.0 * np.pi * u2), rtol=0, atol=1e-14)
    # another step, another seed, the high word of the id: other draws
    for other in (pr.policy_noise(5, ids[:1000], 4, 8), pr.policy_noise(6, ids[:1000], 3, 8),
                  pr.policy_noise(5, ids[:1000] + (np.uint64(1) << np.uint64(32)), 3, 8)):
        assert np.abs(other - eps[:1000]).max() > 1.0


def test_the_two_edge_draws_of_u1_are_where_the_gpu_test_says():
    """Searches the ids below 2^25 for word 0 of (seed 5, step 0, block 0) with w >> 8 == 0 and == 0xFFFFFF."""
    found = {0: [], 0xFFFFFF: []}
    for lo in range(0, 1 << 25, 1 << 22):
        ids = np.arange(lo, lo + (1 << 22), dtype=np.uint64)
        top = philox_np.draw(5, ids, 0, pr.STREAM_POLICY, 0)[:, 0] >> np.uint32(8)
        for k in found:
            found[k] += [int(i) for i in ids[top == k]]
    assert ID_U1_SMALLEST in found[0] and ID_U1_ONE in found[0xFFFFFF]
    lo = pr.policy_noise(5, [ID_U1_SMALLEST], 0, 8)
    rad = math.sqrt(48.0 * math.log(2.0))                                # u1 = 2^-24
    assert abs(math.hypot(lo[0, 0], lo[0, 1]) - rad) < 1e-12 and abs(rad - 5.768) < 1e-3 and np.isfinite(lo).all()
    lo32 = pr.policy_noise(5, [ID_U1_SMALLEST], 0, 8, dtype=np.float32)
    assert np.isfinite(lo32).all() and np.abs(lo32 - lo).max() < 1e-5
    one = pr.policy_noise(5, [ID_U1_ONE], 0, 8)
    assert one[0, 0] == 0.0 and one[0, 1] == 0.0 and np.abs(one[0, 2:]).min() > 0.0


def test_gae64_equals_the_torch_loop_in_float64():
    import torch
    from gym_roboy_amd.ppo import gae
    g = torch.Generator().manual_seed(0)
    for T, N in ((1, 1), (1, 65), (37, 100)):
        rew, val = torch.randn(T, N, generator=g).double(), torch.randn(T, N, generator=g).double()
        done = (torch.rand(T, N, generator=g) < 0.1).double()
        done[-1, ::2] = 1.0
        last = torch.randn(N, generator=g).double()
        a0, r0 = gae(rew, val, done, last, 0.99, 0.95)
        a1, r1 = pr.gae64(rew.numpy(), val.numpy(), done.numpy(), last.numpy(), 0.99, 0.95)
        assert np.abs(a0.numpy() - a1).max() < 1e-13 and np.abs(r0.numpy() - r1).max() < 1e-13


def test_adv_stats64_equals_torch_mean_and_std():
    import torch
    g = torch.Generator().manual_seed(1)
    adv = torch.randn(5000, generator=g).double() * 3 + 1.5
    idx = torch.randperm(5000, generator=g)[:777]
    mean, inv = pr.adv_stats64(adv.numpy(), idx.numpy())
    assert abs(mean - adv[idx].mean().item()) < 1e-13 and abs(inv - 1.0 / (adv[idx].std().item() + 1e-8)) < 1e-12
    assert pr.adv_stats64(np.array([2.5]))[0] == 2.5 and pr.adv_stats64(np.array([2.5]))[1] == 1e8
    assert pr.adv_stats64(np.full(1000, 0.5)) == (0.5, 1e8)


def _flatten(policy, what):
    import torch
    return torch.cat([what(p).reshape(-1) for p in policy.parameters()]).numpy().copy()


def test_clip_adam64_equals_torch_clip_and_adam_in_float64():
    import torch
    policy = _policy64(9, 8, 3)
    opt = torch.optim.Adam(policy.parameters(), lr=2.5e-4, eps=1e-5)
    n = sum(p.numel() for p in policy.parameters())
    off, ls = 0, None
    for name, p in policy.named_parameters():
        if name == "log_std":
            ls = (off + 3, off + 3 + p.numel())                          # +3: the flat vector below starts with a non-parameter gap
        off += p.numel()
    # a flat vector with slots that hold no parameter in front and behind: they must come back untouched
    slots = [(3, 3 + n)]
    pad = lambda x: np.concatenate([np.full(3, 7.0), x, np.full(2, -7.0)])
    p64, m64, v64 = pad(_flatten(policy, lambda p: p.detach())), pad(np.zeros(n)), pad(np.zeros(n))
    gen = torch.Generator().manual_seed(1)
    ent_coef, scale = 0.1, 0.5
    for step, mag in enumerate((5.0, 1e-3, 0.3, 2.0, 1e-2, 0.0), start=1):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * mag       # "the sum over two ranks"
        off = 0
        for name, p in policy.named_parameters():
            p.grad = (g[off:off + p.numel()] * scale).view_as(p).clone()
            if name == "log_std":
                p.grad -= ent_coef
            off += p.numel()
        torch.nn.utils.clip_grad_norm_(policy.parameters(), 0.5)
        opt.step()
        gp = pad(g.numpy()); gp[:3] = np.nan; gp[-2:] = np.nan              # never read
        p64, m64, v64 = pr.clip_adam64(p64, gp, m64, v64, slots, 2.5e-4, (0.9, 0.999), 1e-5, step, 0.5, scale, ent_coef, ls)
        assert np.abs(p64[3:-2] - _flatten(policy, lambda p: p.detach())).max() < 1e-12, step
        assert np.array_equal(p64[:3], np.full(3, 7.0)) and np.array_equal(p64[-2:], np.full(2, -7.0))
        assert np.array_equal(m64[:3], np.full(3, 7.0)) and np.array_equal(v64[-2:], np.full(2, -7.0))
    st = opt.state_dict()["state"]
    m_t = np.concatenate([st[i]["exp_avg"].reshape(-1).numpy() for i in range(len(st))])
    v_t = np.concatenate([st[i]["exp_avg_sq"].reshape(-1).numpy() for i in range(len(st))])
    assert np.abs(m64[3:-2] - m_t).max() < 1e-12 and np.abs(v64[3:-2] - v_t).max() < 1e-12


def test_chunked_ppo_grad64_equals_one_autograd_pass():
    import torch
    from test_policy_gpu import _minibatch, _torch_loss
    cliprange, vf_coef, ent_coef = 0.2, 0.5, 0.1
    policy = _policy64(9, 8, 20)
    mb = _minibatch(policy, 9, 8, 5000, 5000, cliprange)
    loss, pg_ref, vf_ref = _torch_loss(policy, *mb, cliprange, vf_coef, ent_coef)
    loss.backward()
    want = [p.grad.clone() for p in policy.parameters()]
    for chunk in (5000, 1024, 333):
        pg, vf = pr.ppo_grad64(policy, *mb, cliprange, vf_coef, ent_coef, chunk=chunk)
        assert abs(pg - pg_ref.item()) < 1e-12 and abs(vf - vf_ref.item()) < 1e-12
        for p, w in zip(policy.parameters(), want):
            assert (p.grad - w).abs().max().item() < 1e-12 * max(1.0, w.abs().max().item())
    # the plain fp32 statement: the same function on float32 copies, close to float64 and not equal to it
    p32 = _policy64(9, 8, 20).float()
    pr.ppo_grad64(p32, *[t.float() for t in mb], cliprange, vf_coef, ent_coef, chunk=1024)
    for p, w in zip(p32.parameters(), want):
        assert p.grad.dtype == torch.float32
        assert (p.grad.double() - w).abs().max().item() < 1e-4 * max(1.0, w.abs().max().item())
