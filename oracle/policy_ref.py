"""TEST INFRASTRUCTURE - float64 statements of the PPO consumer's operations (include/roboy_policy.h), written for
obviousness: the exploration noise of the policy step, GAE, the minibatch's advantage statistics, clip + Adam and the
minibatch gradient.  numpy / torch on the CPU only; nothing here is loaded by the product.

The noise (csrc/mlp_policy.hip): Philox4x32-10 keyed (seed; sample id, step), stream 2; action j takes component j & 3 of
block j >> 2; a block's four words make two Box-Muller pairs, (0, 1) and (2, 3):
    u1 = ((w_a >> 8) + 1) / 2^24 in (0, 1],  u2 = (w_b >> 8) / 2^24 in [0, 1),  rad = sqrt(-2 ln u1)
    eps_a = rad cos(2 pi u2),  eps_b = rad sin(2 pi u2)
"""
import numpy as np

from . import philox_np

STREAM_POLICY = 2


def policy_noise(seed, sample_ids, step, act_dim, dtype=np.float64):
    """eps [n, act_dim] of the samples with ids sample_ids (uint64: sample index + offset) at `step`; every operation
    in `dtype` (float32: the plain fp32 evaluation of the same draw)."""
    ids = np.asarray(sample_ids, dtype=np.uint64).reshape(-1)
    f = np.dtype(dtype).type
    out = np.empty((ids.shape[0], act_dim), dtype=dtype)
    for block in range((act_dim + 3) // 4):
        w = philox_np.draw(int(seed), ids, np.uint32(int(step) & 0xFFFFFFFF), STREAM_POLICY, block)
        for pair in range(2):
            u1 = ((w[:, 2 * pair] >> np.uint32(8)).astype(dtype) + f(1.0)) * f(1.0 / 16777216.0)
            u2 = (w[:, 2 * pair + 1] >> np.uint32(8)).astype(dtype) * f(1.0 / 16777216.0)
            rad = np.sqrt(f(-2.0) * np.log(u1))
            ang = f(2.0 * np.pi) * u2
            for k, e in ((0, rad * np.cos(ang)), (1, rad * np.sin(ang))):
                j = 4 * block + 2 * pair + k
                if j < act_dim:
                    out[:, j] = e
    return out


def gae64(rew, val, done, last_val, gamma, lam):
    """adv, ret [T, N] in float64: delta_t = rew_t + gamma V_{t+1} (1 - done_t) - V_t,
    adv_t = delta_t + gamma lam (1 - done_t) adv_{t+1}, ret = adv + V."""
    rew, val, done = (np.asarray(x, dtype=np.float64) for x in (rew, val, done))
    next_value = np.asarray(last_val, dtype=np.float64)
    T = rew.shape[0]
    adv = np.zeros_like(rew)
    last = np.zeros_like(next_value)
    for t in range(T - 1, -1, -1):
        nonterminal = 1.0 - done[t]
        delta = rew[t] + gamma * next_value * nonterminal - val[t]
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
        next_value = val[t]
    return adv, adv + val


def adv_stats64(adv, index=None):
    """(mean, 1 / (unbiased std + 1e-8)) of adv[index] in float64; one sample has std 0."""
    a = np.asarray(adv, dtype=np.float64).reshape(-1)
    if index is not None:
        a = a[np.asarray(index, dtype=np.int64)]
    mean = a.sum() / a.shape[0]
    std = np.sqrt(((a - mean) ** 2).sum() / (a.shape[0] - 1)) if a.shape[0] > 1 else 0.0
    return float(mean), float(1.0 / (std + 1e-8))


def clip_adam64(params, grad, m, v, slots, lr, betas, eps, step, max_norm, grad_scale, ent_coef, log_std_slice):
    """One clip_grad_norm_ + Adam.step over flat float64 vectors; returns the new (params, m, v).  slots: the
    [(begin, end)] ranges that hold parameters - everything else of the vectors is neither read nor changed.
    log_std_slice: (begin, end) of the log-std, whose entropy bonus -ent_coef joins the scaled gradient."""
    p, m, v = (np.array(x, dtype=np.float64) for x in (params, m, v))
    grad = np.asarray(grad, dtype=np.float64)
    is_param = np.zeros(p.shape[0], dtype=bool)
    for lo, hi in slots:
        is_param[lo:hi] = True
    g = np.zeros_like(p)
    g[is_param] = grad[is_param] * grad_scale
    g[log_std_slice[0]:log_std_slice[1]] -= ent_coef
    norm = np.sqrt((g[is_param] ** 2).sum())
    g = g * min(max_norm / (norm + 1e-6), 1.0)
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m[is_param] = b1 * m[is_param] + (1.0 - b1) * g[is_param]
    v[is_param] = b2 * v[is_param] + (1.0 - b2) * g[is_param] ** 2
    p[is_param] -= (lr / bc1) * m[is_param] / (np.sqrt(v[is_param]) / np.sqrt(bc2) + eps)       # torch's denominator
    return p, m, v


def ppo_grad64(policy, obs, act, adv, logp_old, val_old, ret, cliprange, vf_coef, ent_coef, chunk=262144):
    """The gradient of PPO's minibatch loss (gym_roboy_amd/ppo.py: _minibatch_loss with the advantage already
    normalised), left in p.grad of the policy's parameters, and the two loss terms (floats): sum-over-chunk / B and one
    backward() per chunk, so that millions of samples fit in host memory.  Runs in the dtype of `policy` and its
    inputs: float64 is the referee, a float32 policy with float32 inputs the plain fp32 statement."""
    import torch
    B = obs.shape[0]
    for p in policy.parameters():
        p.grad = None
    pg_total, vf_total = 0.0, 0.0
    for lo in range(0, B, chunk):
        o, a, ad, lpo, vo, r = (t[lo:lo + chunk] for t in (obs, act, adv, logp_old, val_old, ret))
        d = policy.dist(o)
        ratio = (d.log_prob(a).sum(-1) - lpo).exp()
        pg = torch.max(-ad * ratio, -ad * ratio.clamp(1 - cliprange, 1 + cliprange)).sum() / B
        val = policy.value(o)
        v_clip = vo + (val - vo).clamp(-cliprange, cliprange)
        vf = 0.5 * torch.max((val - r) ** 2, (v_clip - r) ** 2).sum() / B
        ent = d.entropy().sum(-1).sum() / B
        (pg - ent_coef * ent + vf_coef * vf).backward()
        pg_total += pg.item(); vf_total += vf.item()
    return pg_total, vf_total
