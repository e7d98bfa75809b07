"""TEST INFRASTRUCTURE - the statements the update diagnostics and the KL-adaptive learning rate are tested against:
the rule restated in numpy float32 (what rp_clip_adam_kl_dev's d_lr is compared with bit for bit), approx_kl and clip_frac of a minibatch
in float64, and clip + Adam at the adapted rate (oracle/policy_ref.py: clip_adam64).  numpy / torch on the CPU only."""
import numpy as np

from oracle.policy_ref import clip_adam64

F32 = np.float32
BORDER = 1e-4          # a sample is "borderline" when its float64 |ratio - 1| lies within this of the cliprange


def adapt_lr(lr, kl, desired_kl, lr_factor, lr_min, lr_max):
    """The new learning rate (numpy float32) from the old one and the minibatch's KL, every operand rounded to float32 first:
        kl > 2 d              ->  max(lr_min, lr / f)      one IEEE division
        kl < d / 2 and kl > 0 ->  min(lr_max, lr * f)
        otherwise (a NaN fails every comparison)  ->  lr"""
    lr, kl, d, f, lo, hi = (F32(x) for x in (lr, kl, desired_kl, lr_factor, lr_min, lr_max))
    if kl > F32(2.0) * d:
        new = lr / f
        return new if new > lo else lo
    if kl < F32(0.5) * d and kl > F32(0.0):
        new = lr * f
        return new if new < hi else hi
    return lr


def kl_of_slot(slot, grad_scale):
    """What the kernel compares: the approx_kl slot of the (summed) gradient vector times grad_scale, one float32 product."""
    return F32(slot) * F32(grad_scale)


def diag64(policy64, obs, act, logp_old, cliprange):
    """approx_kl = mean 0.5 x^2 and clip_frac = mean [ratio outside 1 -+ c] of a minibatch in float64 (x = logp - logp_old, ratio =
    exp x), with what a test needs to qualify its input: how many samples are borderline, how many lie below / above the range."""
    import torch
    with torch.no_grad():
        x = policy64.dist(obs.double()).log_prob(act.double()).sum(-1) - logp_old.double()
    x = x.numpy()
    ratio = np.exp(x)
    low, high = ratio < 1.0 - cliprange, ratio > 1.0 + cliprange
    return {"approx_kl": float((0.5 * x * x).mean()), "clip_frac": float((low | high).mean()), "n_clipped": int((low | high).sum()),
            "borderline": int((np.abs(np.abs(ratio - 1.0) - cliprange) < BORDER).sum()), "n_low": int(low.sum()), "n_high": int(high.sum())}


def clip_adam_kl64(params, grad, m, v, slots, lr, kl_slot, desired_kl, lr_factor, lr_min, lr_max, betas, eps, step, max_norm,
                   grad_scale, ent_coef, log_std_slice):
    """rp_clip_adam_kl_dev: the float32 rule on grad[kl_slot] * grad_scale, then float64 clip + Adam at the new rate.
    Returns (new lr as numpy float32, (params, m, v))."""
    new_lr = adapt_lr(lr, kl_of_slot(grad[kl_slot], grad_scale), desired_kl, lr_factor, lr_min, lr_max)
    return new_lr, clip_adam64(params, grad, m, v, slots, float(new_lr), betas, eps, step, max_norm, grad_scale, ent_coef, log_std_slice)
