"""PPO (clipped surrogate) with an MLP policy, on torch-ROCm.

Consumer of the env: the reference trains with
stable_baselines' TF1 ``PPO2("MlpPolicy", env, ent_coef=0.1)`` over a
``SubprocVecEnv`` (``/root/reference/gym_roboy/train_parallel.py:28-35``).  Here
the rollout never leaves the GPU: ``RoboyVecEnv.step`` takes the policy's action
tensor and returns observation / reward / done tensors on the same HIP stream.
Hyper-parameters default to stable_baselines PPO2's (n_steps 128, 4 minibatches,
4 epochs, gamma 0.99, lambda 0.95, lr 2.5e-4, clip 0.2, vf 0.5, max grad norm
0.5) with the reference's ``ent_coef = 0.1``.  With several ranks (one per GPU)
gradients are averaged with ``torch.distributed.all_reduce`` (RCCL over xGMI).

``use_graphs=True`` (device env) captures a whole rollout - policy forward, sampling, the fused
env kernel launched through the C ABI, GAE - in one HIP graph and replays it, on every rank of a
multi-rank run (the rollout is rank-local), instead of launching ~30 small kernels per env step
from Python: at 4 096 envs 375 -> 102 us per vectorised step (``tools/ppo_profile.py``).

On a GPU the policy's work runs in the kernels of ``include/roboy_policy.h`` by default (exact f32
on the matrix cores): the policy step and GAE of the rollout (``FusedPolicyStep``, ``gae_fused``),
the minibatch gradient (``FusedPolicyGrad``) and the rest of the update - the epoch's sample order
as a keyed bijection evaluated on the device, the minibatch's advantage statistics applied inside
the gradient kernel, ``clip_grad_norm_`` + ``Adam.step`` as one launch over a flat parameter buffer
the module's parameters are views of (``FusedAdam``); with several ranks that flat gradient vector
is all-reduced once per minibatch.  At 262 144 envs a PPO iteration goes from 49 ms + 1.06 s
(rollout + update, torch: ~40 memory-bound passes over [8.4 M x 64] activations per minibatch) to
11 ms + 0.11 s.  ``fused_policy=False, fused_update=False`` select the torch path, which is what
the kernels are tested against.

``diagnostics=True`` adds stable-baselines PPO2's ``approxkl`` and ``clipfrac`` of the last minibatch to what ``update()`` returns;
``lr_schedule="adaptive"`` moves the learning rate by them, minibatch by minibatch (rsl_rl's schedule: cut above twice the desired KL,
raised below half of it).  On the fused path the two sums come out of the action net's gradient kernel and the learning rate lives
on the device, read and moved by the optimiser's own launch: no read-back between minibatches.

``normalize_obs=True`` keeps a running mean / variance of every observation column (``ObsNorm``: what stable-baselines calls
``VecNormalize``, for the observation) and feeds the networks ``clip((obs - mean) / sqrt(var + eps))``.  The fused kernels
normalise as they fetch their operands (``rp_act_norm_dev``, ``rp_ppo_grad_norm_dev``): the rollout buffers keep the raw
observation and no normalised copy is ever written.  The statistics are frozen through a rollout and the update on it and merged
with that rollout's moments after the update's last minibatch.

``symmetry="augment"`` (an env with ``mirror_map()``: a robot with a mirror plane) runs every update on the rollout's samples and
their mirror images: one streaming kernel (``rp_mirror_rows_dev``) writes the mirrored half of the [2 n, ...] sample set, and the
gradient, statistics, sample-order and optimiser kernels run unchanged on twice the rows.
``symmetry="loss"`` keeps the samples and adds ``symmetry_coef`` x the mean squared distance of the action mean from the symmetry to
every minibatch's loss, the gradient through both branches: one more gradient kernel per minibatch (``rp_sym_grad_dev``) whose wave
tile is 32 (sample, image) pairs, added into the PPO gradient in front of clip + Adam.  It reads the action net and the actor's rows
only and combines with ``asymmetric_critic``.
"""
import math

import numpy as np
import torch
from torch import nn

from .envs.options import check_env_checkpoint, env_checkpoint_record, env_io_record as _env_io_of  # noqa: F401 (the last: old name)
from .sharding import dist_ranks

LR_SCHEDULES = ("adaptive",)
SYMMETRY_MODES = ("augment", "loss")


def adapt_lr(lr, kl, desired_kl, lr_factor, lr_min, lr_max):
    """The KL-adaptive learning-rate rule in numpy float32, rounding as rp_clip_adam_kl_dev does: cut by ``lr_factor``
    (one IEEE division) above twice the desired KL, raised by it below half of it - unless the KL is 0 or NaN - and kept inside
    [lr_min, lr_max]."""
    f32 = np.float32
    lr, kl, d, f = f32(lr), f32(kl), f32(desired_kl), f32(lr_factor)
    if kl > f32(2.0) * d:
        return max(f32(lr_min), lr / f)
    if kl < f32(0.5) * d and kl > f32(0.0):
        return min(f32(lr_max), lr * f)
    return lr


class ObsNorm:
    """Running per-column mean / variance of the observation and the form the networks apply.

    State (float64): ``state`` = [mean (obs_dim), var (obs_dim, population), count].  The form the kernels read (float32):
    ``norm`` [2, obs_dim] = mean, rstd = 1 / sqrt(var + eps) - the identity (0, 1) while count == 0.  A column value enters the
    network as ``min(max((x - mean) * rstd, -clip), clip)``, difference and product each rounded once to float32 (``apply``; the
    kernels compute the same bits).  ``update(rows)`` merges the moments of a [rows, obs_dim] float32 batch (Chan's parallel
    formula over sums taken around the current mean); the tensors are updated in place, so a captured launch that holds
    ``norm``'s address sees the new statistics on its next replay.  Not an ``nn.Module``: nothing here is a parameter or a
    buffer of the policy."""

    def __init__(self, obs_dim, device="cpu", clip=10.0, eps=1e-8):
        self.obs_dim, self.device, self.clip, self.eps = int(obs_dim), torch.device(device), float(clip), float(eps)
        if not self.clip > 0.0:
            raise ValueError("clip must be > 0")
        self.state = torch.zeros(2 * self.obs_dim + 1, dtype=torch.float64, device=self.device)
        self.norm = torch.zeros(2, self.obs_dim, dtype=torch.float32, device=self.device)
        self._reset()
        self._native = None

    def _reset(self):
        self.state.zero_(); self.state[self.obs_dim:2 * self.obs_dim] = 1.0
        self.norm[0] = 0.0; self.norm[1] = 1.0

    mean = property(lambda self: self.state[:self.obs_dim])
    var = property(lambda self: self.state[self.obs_dim:2 * self.obs_dim])
    count = property(lambda self: float(self.state[-1].item()))

    def apply(self, obs):
        """The normalised observation in ``obs``'s dtype (the torch statement of the kernels' operand fetch)."""
        norm = self.norm.to(obs.dtype)
        return ((obs - norm[0]) * norm[1]).clamp(-self.clip, self.clip)

    def _lib(self):
        if self._native is None:
            import ctypes
            from . import _policy_native as pn
            lib = pn.load()
            self._native = (pn, ctypes, lib)
            self._scratch = torch.zeros(int(lib.rp_obs_moments_scratch_doubles()), dtype=torch.float64, device=self.device)
            self._sums = torch.zeros(1 + 2 * self.obs_dim, dtype=torch.float64, device=self.device)
        return self._native

    @torch.no_grad()
    def moments(self, rows):
        """[rows, sum (x - mean), sum (x - mean)^2] (float64, 1 + 2 obs_dim) of a [rows, obs_dim] float32 batch around the running
        mean: one HIP launch on a GPU, the torch float64 statement of the same sums on the CPU."""
        if rows.dim() != 2 or rows.shape[1] != self.obs_dim or rows.dtype != torch.float32:
            raise ValueError("expected float32 rows of %d columns, got %s %r" % (self.obs_dim, rows.dtype, tuple(rows.shape)))
        if rows.device.type != "cuda":
            d = rows.to(torch.float64) - self.mean.to(rows.device)
            n = torch.tensor([float(rows.shape[0])], dtype=torch.float64, device=rows.device)
            return torch.cat([n, d.sum(0), (d * d).sum(0)])
        pn, c, lib = self._lib()
        if rows.shape[0] == 0:
            return self._sums.zero_()
        rows = rows.contiguous()
        pn.check(lib.rp_obs_moments_dev(c.c_void_p(rows.data_ptr()), int(rows.shape[0]), self.obs_dim, c.c_void_p(self.state.data_ptr()),
                                        c.c_void_p(self._sums.data_ptr()), c.c_void_p(self._scratch.data_ptr()),
                                        c.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)))
        return self._sums

    @torch.no_grad()
    def merge(self, sums):
        """Chan's merge of ``moments()`` sums (taken around the CURRENT mean) into the state, and the float form."""
        if self.device.type == "cuda":
            pn, c, lib = self._lib()
            pn.check(lib.rp_obs_norm_merge_dev(c.c_void_p(self.state.data_ptr()), c.c_void_p(sums.data_ptr()), self.obs_dim, self.eps,
                                               c.c_void_p(self.norm.data_ptr()), c.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            return
        od = self.obs_dim
        n, count = float(sums[0]), float(self.state[-1])
        if not n > 0.0:
            return
        S, SS = sums[1:1 + od], sums[1 + od:]
        tot = count + n
        delta = S / n                                         # batch mean - running mean
        m2b = (SS - S * delta).clamp_min(0.0)                 # the batch's sum of squares around its own mean
        mean = self.mean + delta * (n / tot)
        var = (self.var * count + m2b + delta * delta * (count * n / tot)) / tot
        self.state[:od] = mean; self.state[od:2 * od] = var; self.state[-1] = tot
        self.norm[0] = mean.to(torch.float32)
        self.norm[1] = (1.0 / torch.sqrt(var + self.eps)).to(torch.float32)

    @torch.no_grad()
    def update(self, obs_rows, dist=None):
        """Merge the moments of ``obs_rows`` [rows, obs_dim].  With several ranks the 1 + 2 obs_dim sums - taken around the same
        mean on every rank, so they add - are all-reduced once (the device tensor under nccl, through the host under gloo, as
        ``FusedAdam.step``): every rank then merges the same numbers and holds bit-identical statistics."""
        sums = self.moments(obs_rows.to(self.device))
        _all_reduce_sums(sums, dist)
        self.merge(sums)

    def state_dict(self):
        od = self.obs_dim
        return {"mean": self.state[:od].clone(), "var": self.state[od:2 * od].clone(), "count": self.count,
                "clip": self.clip, "eps": self.eps}

    @torch.no_grad()
    def load_state_dict(self, sd):
        od = self.obs_dim
        if tuple(sd["mean"].shape) != (od,) or tuple(sd["var"].shape) != (od,):
            raise ValueError("observation statistics of %d columns, this policy's observation has %d" % (sd["mean"].numel(), od))
        self.clip, self.eps = float(sd["clip"]), float(sd["eps"])
        self._reset()
        if float(sd["count"]) > 0.0:
            self.state[:od] = sd["mean"].to(self.device, torch.float64); self.state[od:2 * od] = sd["var"].to(self.device, torch.float64)
            self.state[-1] = float(sd["count"])
            self.norm[0] = self.mean.to(torch.float32)
            self.norm[1] = (1.0 / torch.sqrt(self.var + self.eps)).to(torch.float32)


def _all_reduce_sums(sums, dist):
    """Sum a small float64 tensor over the ranks: the device tensor under nccl, through the host under gloo."""
    if dist_ranks(dist) > 1:
        if sums.device.type != "cuda" or dist.get_backend() == "nccl":
            dist.all_reduce(sums)
        else:
            host = sums.cpu()
            dist.all_reduce(host)
            sums.copy_(host)


class RewardNorm:
    """Running mean / variance of the discounted return and the reward scaling that follows from it: what
    stable-baselines calls ``VecNormalize(norm_reward=True)``, the counterpart of ``ObsNorm``.

    State (float64): ``state`` = [mean, var (population), count] of the discounted return; ``norm`` (float32 [2, 1]) = mean, rstd = 1 /
    sqrt(var + eps) - the identity (0, 1) while count == 0; ``ret_carry`` (float64 [n_envs]) every env's running discounted return,
    carried from one rollout into the next.  Per env and step: r_s = the scaled reward (float32), R = gamma R + r_s in float64,
    d = R - mean joins the rollout's sums [n, S, SS], then R = 0 where the step ended an episode (``scan``).  The reward the agent
    learns from is ``min(max(r_s * rstd, -clip), clip)``, the product rounded once to float32, the mean not subtracted (``apply``).
    The statistics are frozen through a rollout; ``update(dist)`` merges its sums (Chan's formula, shift = the state's mean) after
    an all-reduce over the ranks.  On a GPU ``tail()`` is the whole tail of a rollout - scan, scaling, done conversion, GAE - as one
    launch (include/roboy_policy.h: rp_rollout_tail_dev)."""

    def __init__(self, n_envs, gamma, device="cpu", clip=10.0, eps=1e-8):
        self.n_envs, self.gamma, self.device = int(n_envs), float(gamma), torch.device(device)
        self.clip, self.eps = float(clip), float(eps)
        if not self.clip > 0.0:
            raise ValueError("clip must be > 0")
        if not 0.0 <= self.gamma <= 1.0:
            raise ValueError("gamma must lie in [0, 1]")
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=self.device)
        self.state, self.norm, self.ret_carry, self.sums = z(3), z(2, 1, dtype=torch.float32), z(self.n_envs), z(3)
        self._reset()
        self._native = None

    def _reset(self):
        self.state.zero_(); self.state[1] = 1.0
        self.norm[0] = 0.0; self.norm[1] = 1.0

    mean = property(lambda self: self.state[0])
    var = property(lambda self: self.state[1])
    count = property(lambda self: float(self.state[2].item()))

    def reset_returns(self, n_envs=None):
        """The envs were reset: no return runs across that.  n_envs: the batch's size, where it was not known before."""
        if n_envs is not None and int(n_envs) != self.n_envs:
            self.n_envs = int(n_envs)
            self.ret_carry = torch.zeros(self.n_envs, dtype=torch.float64, device=self.device)
        self.ret_carry.zero_()

    def apply(self, r_s):
        """The reward GAE sees, from the scaled reward ``r_s`` (float32): the torch statement of the kernel's."""
        return (r_s * self.norm[1, 0]).clamp(-self.clip, self.clip)

    @torch.no_grad()
    def scan(self, r_s, done):
        """The forward scan of a [T, n_envs] rollout in float64: moves ``ret_carry`` on and leaves [n, S, SS] - the sums of the
        T * n_envs returns around the running mean - in ``sums``.  No host synchronisation: it can be captured."""
        if r_s.dim() != 2 or r_s.shape[1] != self.n_envs or r_s.dtype != torch.float32:
            raise ValueError("expected float32 rewards of %d envs, got %s %r" % (self.n_envs, r_s.dtype, tuple(r_s.shape)))
        R, mean = self.ret_carry, self.state[0]
        S, SS = torch.zeros_like(mean), torch.zeros_like(mean)
        for t in range(r_s.shape[0]):
            R.mul_(self.gamma).add_(r_s[t].to(torch.float64))
            d = R - mean
            S = S + d.sum(); SS = SS + (d * d).sum()
            R.masked_fill_(done[t] != 0, 0.0)
        # (fill_ / copy_ between device tensors: assigning a Python number to an element is a host-to-device copy, which a capture refuses)
        self.sums[0:1].fill_(float(r_s.numel())); self.sums[1:2].copy_(S.reshape(1)); self.sums[2:3].copy_(SS.reshape(1))
        return self.sums

    def _lib(self):
        if self._native is None:
            import ctypes
            from . import _policy_native as pn
            lib = pn.load()
            self._native = (pn, ctypes, lib)
            self._scratch = torch.zeros(int(lib.rp_rollout_tail_scratch_doubles()), dtype=torch.float64, device=self.device)
        return self._native

    @torch.no_grad()
    def tail(self, rew_raw, done_i, val, last_val, reward_scale, lam, rew, done, adv, ret, ret_carry=None, boot=False, identity=False):
        """One launch for the tail of a [T, n_envs] rollout (contiguous tensors on the GPU; done_i int32): ``scan`` on
        fl32(rew_raw * reward_scale), then rew = ``apply`` of it, done = done_i as floats, adv / ret = GAE over rew.
        boot: done_i holds episode-end codes (0 / 1 terminated / 2 truncated) and GAE bootstraps the truncated steps
        (rp_rollout_tail_boot_dev, ``gae_boot``).  identity: the kernel runs without statistics (rstd 1, shift 0), whatever the state."""
        pn, c, lib = self._lib()
        T, N = rew_raw.shape
        if N != self.n_envs:
            raise ValueError("a rollout of %d envs, these statistics carry the returns of %d" % (N, self.n_envs))
        carry = self.ret_carry if ret_carry is None else ret_carry
        ptr = lambda t: c.c_void_p(t.data_ptr())
        fn = lib.rp_rollout_tail_boot_dev if boot else lib.rp_rollout_tail_dev
        pn.check(fn(ptr(rew_raw), ptr(done_i), ptr(val), ptr(last_val), float(reward_scale), None if identity else ptr(self.norm),
                    self.clip, None if identity else ptr(self.state), self.gamma, float(lam), ptr(carry), ptr(rew), ptr(done), ptr(adv),
                    ptr(ret), ptr(self.sums), ptr(self._scratch), int(T), int(N),
                    c.c_void_p(torch.cuda.current_stream(rew_raw.device).cuda_stream)))

    @torch.no_grad()
    def merge(self, sums):
        """Chan's merge of [n, S, SS] (taken around the CURRENT mean) into the state, and the float form."""
        if self.device.type == "cuda":
            pn, c, lib = self._lib()
            pn.check(lib.rp_obs_norm_merge_dev(c.c_void_p(self.state.data_ptr()), c.c_void_p(sums.data_ptr()), 1, self.eps,
                                               c.c_void_p(self.norm.data_ptr()), c.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            return
        n, S, SS = float(sums[0]), float(sums[1]), float(sums[2])
        count = float(self.state[2])
        if not n > 0.0:
            return
        tot = count + n
        delta = S / n                                         # batch mean - running mean
        m2b = max(SS - S * delta, 0.0)                        # the batch's sum of squares around its own mean
        mean = float(self.state[0]) + delta * (n / tot)
        var = (float(self.state[1]) * count + m2b + delta * delta * (count * n / tot)) / tot
        self.state[0] = mean; self.state[1] = var; self.state[2] = tot
        self.norm[0] = torch.tensor(mean, dtype=torch.float64).to(torch.float32)
        self.norm[1] = torch.tensor(1.0 / math.sqrt(var + self.eps), dtype=torch.float64).to(torch.float32)

    @torch.no_grad()
    def update(self, dist=None):
        """Merge the last rollout's sums.  With several ranks the three doubles - taken around the same mean on every rank, so they
        add - are all-reduced first, as ``ObsNorm.update``: every rank then holds bit-identical statistics."""
        _all_reduce_sums(self.sums, dist)
        self.merge(self.sums)

    def state_dict(self):
        return {"mean": float(self.state[0].item()), "var": float(self.state[1].item()), "count": self.count,
                "clip": self.clip, "eps": self.eps, "gamma": self.gamma}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if float(sd["gamma"]) != self.gamma:
            raise ValueError("return statistics under gamma = %r, this agent discounts with %r" % (float(sd["gamma"]), self.gamma))
        self.clip, self.eps = float(sd["clip"]), float(sd["eps"])
        self._reset()
        if float(sd["count"]) > 0.0:
            self.state[0] = float(sd["mean"]); self.state[1] = float(sd["var"]); self.state[2] = float(sd["count"])
            self.norm[0] = self.state[0].to(torch.float32)
            self.norm[1] = (1.0 / torch.sqrt(self.state[1] + self.eps)).to(torch.float32)


class MlpPolicy(nn.Module):
    """Two tanh layers of 64 units for the policy and for the value function,
    diagonal Gaussian with a state-independent log-std (stable_baselines' MlpPolicy)."""

    obs_norm = None        # an ObsNorm once set_obs_norm() was called: a plain attribute, not a parameter or buffer
    critic_obs_norm = None  # ... and the critic rows' own, where the critic is asymmetric

    def __init__(self, obs_dim: int, act_dim: int, hidden: int = 64, critic_obs_dim=None):
        """critic_obs_dim: an asymmetric critic - the value net's first layer takes that many columns and ``value()``
        reads the env's privileged critic rows, not the observation; only the action net is ever deployed.  None: both nets read the
        observation.  The ``state_dict`` keys are the same either way."""
        super().__init__()
        self.critic_obs_dim = None if critic_obs_dim is None else int(critic_obs_dim)
        def mlp(out, width=obs_dim):
            return nn.Sequential(nn.Linear(width, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                                 nn.Linear(hidden, out))
        self.pi, self.vf = mlp(act_dim), mlp(1, obs_dim if critic_obs_dim is None else self.critic_obs_dim)
        self.log_std = nn.Parameter(torch.zeros(act_dim))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.orthogonal_(m.weight, math.sqrt(2))
                nn.init.zeros_(m.bias)
        nn.init.orthogonal_(self.pi[-1].weight, 0.01)
        nn.init.orthogonal_(self.vf[-1].weight, 1.0)

    def set_obs_norm(self, obs_norm, critic_obs_norm=None):
        """An ``ObsNorm`` (or None): ``dist()`` and ``value()`` then see the normalised observation.  The statistics are neither
        parameters nor buffers of the module (``state_dict()`` keeps its keys) and carry no gradient.  critic_obs_norm: a second
        ``ObsNorm`` over the critic rows, which is what ``value()`` of an asymmetric critic applies."""
        self.obs_norm = obs_norm
        self.critic_obs_norm = critic_obs_norm
        return self

    def dist(self, obs):
        if self.obs_norm is not None:
            obs = self.obs_norm.apply(obs)
        # validate_args=False: the check reads a device flag back (a host sync per call)
        return torch.distributions.Normal(self.pi(obs), self.log_std.exp(), validate_args=False)

    def value(self, obs):
        """The value of observation rows - of CRITIC rows [.., critic_obs_dim] where the critic is asymmetric."""
        norm = self.obs_norm if self.critic_obs_dim is None else self.critic_obs_norm
        if norm is not None:
            obs = norm.apply(obs)
        return self.vf(obs).squeeze(-1)

    @torch.no_grad()
    def act(self, obs, deterministic=False, cobs=None):
        """cobs: the critic rows that belong to ``obs`` (an asymmetric critic needs them for the value; None there: no value)"""
        d = self.dist(obs)
        # mean + std * eps rather than d.sample(): torch.normal(mean, std) checks std >= 0 on the host
        a = d.mean if deterministic else d.mean + d.stddev * torch.randn_like(d.mean)
        if self.critic_obs_dim is not None:
            return a, d.log_prob(a).sum(-1), (self.value(cobs) if cobs is not None else None)
        return a, d.log_prob(a).sum(-1), self.value(obs)


def gae(rewards, values, dones, last_value, gamma, lam):
    """Generalised advantage estimation over a [T, N] rollout (dones[t] = the
    step t ended an episode)."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(last_value)
    next_value = last_value
    for t in range(T - 1, -1, -1):
        nonterminal = 1.0 - dones[t]
        delta = rewards[t] + gamma * next_value * nonterminal - values[t]
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
        next_value = values[t]
    return adv, adv + values


def gae_boot(rew, val, done_code, last_value, gamma, lam):
    """``gae`` over episode-end codes (``done_code`` [T, N]: 0 not done, 1 terminated, 2 truncated - RoboyVecEnv's
    ``report_truncation``): any non-zero code ends the episode as ``dones`` does in ``gae``, and a truncated step takes
    ``rew + gamma * val`` for its reward - the value of the state the episode was cut at, so that the return the critic learns does not
    collapse at a time limit the observation does not show.  The torch statement of rp_rollout_tail_boot_dev's recurrence."""
    T = rew.shape[0]
    adv = torch.zeros_like(rew)
    last = torch.zeros_like(last_value)
    next_value = last_value
    for t in range(T - 1, -1, -1):
        nonterminal = 1.0 - (done_code[t] != 0).to(rew.dtype)
        r = torch.where(done_code[t] == 2, rew[t] + gamma * val[t], rew[t])
        delta = r + gamma * next_value * nonterminal - val[t]
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
        next_value = val[t]
    return adv, adv + val


def gae_fused(rewards, values, dones, last_value, gamma, lam, adv_out=None, ret_out=None):
    """gae() as one kernel (include/roboy_policy.h: rp_gae_dev): the [T, N] tensors must be contiguous fp32 on the GPU."""
    import ctypes as c
    from . import _policy_native as pn
    T, N = rewards.shape
    adv = torch.empty_like(rewards) if adv_out is None else adv_out
    ret = torch.empty_like(rewards) if ret_out is None else ret_out
    ptr = lambda t: c.c_void_p(t.data_ptr())
    pn.check(pn.load().rp_gae_dev(ptr(rewards), ptr(values), ptr(dones), ptr(last_value), float(gamma), float(lam), ptr(adv), ptr(ret),
                                  int(T), int(N), c.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream)))
    return adv, ret


def rollout_tail_form(fused, eager, reward_norm, boot, asym):
    """Which statement turns a rollout's (rew_raw, done codes, val, last value) into (rew, done, adv, ret) - DESIGN.md §16's table:
    "torch" (the scale, ``RewardNorm.scan`` / ``apply``, ``gae`` / ``gae_boot``), "gae_kernel" (the torch scale and ``gae_fused``) or
    "tail_kernel" (one launch of ``RewardNorm.tail``: the agent's own statistics under ``reward_norm``, identity statistics on a
    private carry under ``boot`` alone).  fused: the fused policy step; eager: through ``env.step``, not a captured graph; reward_norm,
    boot, asym: PPO's ``normalize_reward``, ``bootstrap_timeouts``, ``asymmetric_critic``.  A captured fused rollout always runs a
    kernel; an eager fused one runs the same kernel only under ``boot``, or under ``asym`` without ``reward_norm`` - the historical
    exception (NEXT.md), which is why eager and captured advantages differ in the last bits everywhere else."""
    if not fused:
        return "torch"
    if boot or (reward_norm and not eager):
        return "tail_kernel"
    if not eager or (asym and not reward_norm):
        return "gae_kernel"
    return "torch"


def _check_norm(norm, obs_dim, device):
    if norm.obs_dim != obs_dim or norm.norm.device != device or norm.norm.dtype != torch.float32 or not norm.norm.is_contiguous():
        raise ValueError("observation statistics of %d columns on %s, the kernel reads %d on %s"
                         % (norm.obs_dim, norm.norm.device, obs_dim, device))


class FusedPolicyStep:
    """``MlpPolicy.act`` as one kernel on the matrix cores (include/roboy_policy.h, csrc/mlp_policy.hip): observation
    -> action sample, log-probability, value, written straight into the rollout buffers.  The parameters stay torch
    tensors (the optimiser - torch's or ``FusedAdam`` - updates them in place); ``pack()`` is one device-side gather into the operand order the
    kernel reads (the gather map depends on the dimensions only and is built once on the host).  Exploration noise is
    the library's Philox stream keyed (seed; sample, step), not torch's generator."""

    def __init__(self, policy, seed=0):
        import ctypes
        from . import _policy_native as pn
        self._pn, self._ct, self._lib = pn, ctypes, pn.load()
        self.policy = policy
        self.obs_dim, self.act_dim = policy.pi[0].in_features, policy.pi[-1].out_features
        if policy.pi[0].out_features != 64 or len(policy.pi) != 5:
            raise ValueError("the fused policy step is built for MlpPolicy's two hidden layers of 64 units")
        dev = policy.log_std.device
        # an asymmetric critic: the value net reads rows of its own width through a blob of its own
        self.cobs_dim = getattr(policy, "critic_obs_dim", None)
        if self.cobs_dim is None:
            m, total = pn.gather_map(self.obs_dim, self.act_dim)
            self._map = torch.from_numpy(m).to(dev)
        else:
            m_pi, m_vf, total = pn.gather_map_asym(self.obs_dim, self.cobs_dim, self.act_dim)
            self._map = torch.from_numpy(np.concatenate((m_pi, m_vf))).to(dev)
            self._split = int(m_pi.shape[0])
        self._zero = torch.zeros(1, device=dev)
        self.seed = int(seed)

    def _params(self):
        pi, vf = self.policy.pi, self.policy.vf
        return [pi[0].weight, pi[0].bias, pi[2].weight, pi[2].bias, pi[4].weight, pi[4].bias,
                vf[0].weight, vf[0].bias, vf[2].weight, vf[2].bias, vf[4].weight, vf[4].bias, self.policy.log_std]

    @torch.no_grad()
    def pack(self):
        """The operand blob - with an asymmetric critic both blobs, one behind the other (one gather)"""
        flat = torch.cat([p.detach().reshape(-1) for p in self._params()] + [self._zero])
        return flat[self._map]

    @torch.no_grad()
    def act_into(self, obs, act, logp, val, step=0, packed=None, mean=None, sample_offset=0, deterministic=False,
                 step_base=None, norm=None, cobs=None, cnorm=None):
        """obs [n, obs_dim] (contiguous, fp32, cuda) -> act [n, act_dim], logp [n], val [n] (preallocated).
        norm (an ``ObsNorm``, optional): the observation is normalised as the kernel fetches it (rp_act_norm_dev).
        cobs [n, critic_obs_dim] and cnorm: the critic rows and their statistics, for a policy with an asymmetric critic
        (rp_act_asym_dev / rp_act_asym_norm_dev)."""
        c = self._ct
        packed = self.pack() if packed is None else packed
        ptr = lambda t: c.c_void_p(t.data_ptr()) if t is not None else None
        stream = c.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        if self.cobs_dim is not None:
            if cobs is None or tuple(cobs.shape) != (obs.shape[0], self.cobs_dim) or not cobs.is_contiguous() or cobs.dtype != torch.float32:
                raise ValueError("an asymmetric critic needs contiguous float32 critic rows [%d, %d]" % (obs.shape[0], self.cobs_dim))
            if (norm is None) != (cnorm is None):
                raise ValueError("statistics for both nets, or for neither")
            blobs = (ptr(packed[:self._split]), ptr(packed[self._split:]))
            head = blobs + (ptr(obs), ptr(cobs), ptr(act), ptr(logp), ptr(val), ptr(mean), int(obs.shape[0]), self.obs_dim, self.cobs_dim,
                            self.act_dim, self.seed, int(sample_offset), int(step), ptr(step_base), int(bool(deterministic)))
            if norm is None:
                self._pn.check(self._lib.rp_act_asym_dev(*head, stream))
            else:
                _check_norm(norm, self.obs_dim, obs.device)
                _check_norm(cnorm, self.cobs_dim, obs.device)
                self._pn.check(self._lib.rp_act_asym_norm_dev(*head, ptr(norm.norm), ptr(cnorm.norm), float(norm.clip), float(cnorm.clip), stream))
            return packed
        if norm is None:
            self._pn.check(self._lib.rp_act_dev(
                ptr(packed), ptr(obs), ptr(act), ptr(logp), ptr(val), ptr(mean), int(obs.shape[0]), self.obs_dim, self.act_dim,
                self.seed, int(sample_offset), int(step), ptr(step_base), int(bool(deterministic)), stream))
        else:
            _check_norm(norm, self.obs_dim, obs.device)
            self._pn.check(self._lib.rp_act_norm_dev(
                ptr(packed), ptr(obs), ptr(act), ptr(logp), ptr(val), ptr(mean), int(obs.shape[0]), self.obs_dim, self.act_dim,
                self.seed, int(sample_offset), int(step), ptr(step_base), int(bool(deterministic)), ptr(norm.norm), float(norm.clip),
                stream))
        return packed


class FusedPolicyGrad:
    """The PPO minibatch gradient of an ``MlpPolicy`` as MFMA kernels (include/roboy_policy.h: rp_ppo_grad_dev,
    csrc/mlp_train.hip): forward, clipped-surrogate / clipped-value loss derivative, back-propagation and the weight
    gradients of both networks without materialising an activation in memory.  ``run()`` fills ``p.grad`` of every
    parameter (views of one flat buffer) and returns the two loss terms.  The advantage's per-minibatch normalisation
    happens inside (``adv_stats`` from ``minibatch_adv_stats()``); clipping and the optimiser step are ``FusedAdam``."""

    def __init__(self, policy):
        import ctypes
        from . import _policy_native as pn
        self._pn, self._ct, self._lib = pn, ctypes, pn.load()
        self.policy = policy
        self.obs_dim, self.act_dim = policy.pi[0].in_features, policy.pi[-1].out_features
        # the gather map and the gradient layout are built for MlpPolicy's shape: anything else would be indexed wrongly
        if (len(policy.pi) != 5 or len(policy.vf) != 5 or policy.pi[0].out_features != 64 or policy.pi[2].out_features != 64
                or policy.vf[0].out_features != 64 or policy.vf[2].out_features != 64):
            raise ValueError("the fused PPO gradient is built for MlpPolicy's two hidden layers of 64 units")
        dev = policy.log_std.device
        self.cobs_dim = getattr(policy, "critic_obs_dim", None)      # an asymmetric critic: the value net's own width, blob and rows
        if self.cobs_dim is None:
            m, _ = pn.gather_map(self.obs_dim, self.act_dim, train=True)
            self._map = torch.from_numpy(m).to(dev)
        else:
            m_pi, m_vf, _ = pn.gather_map_asym(self.obs_dim, self.cobs_dim, self.act_dim, train=True)
            self._map = torch.from_numpy(np.concatenate((m_pi, m_vf))).to(dev)
            self._split = int(m_pi.shape[0])
        self._zero = torch.zeros(1, device=dev)
        layout, n = pn.grad_layout(self.obs_dim, self.act_dim, self.cobs_dim)
        self._g = torch.zeros(n, device=dev)
        self._layout = layout
        pi, vf = policy.pi, policy.vf
        self._named = {"pi_w1": pi[0].weight, "pi_b1": pi[0].bias, "pi_w2": pi[2].weight, "pi_b2": pi[2].bias,
                       "pi_w3": pi[4].weight, "pi_b3": pi[4].bias, "vf_w1": vf[0].weight, "vf_b1": vf[0].bias,
                       "vf_w2": vf[2].weight, "vf_b2": vf[2].bias, "vf_w3": vf[4].weight, "vf_b3": vf[4].bias,
                       "log_std": policy.log_std}
        self._views = {}
        for name, p in self._named.items():
            off, shape = layout[name]
            self._views[name] = self._g[off:off + p.numel()].view(shape)
        self._ws = None
        self._stats = torch.zeros(2, device=dev)
        self._stat_scratch = torch.zeros(int(self._lib.rp_adv_stats_scratch_doubles()), dtype=torch.float64, device=dev)

    @torch.no_grad()
    def minibatch_adv_stats(self, adv_full, index):
        """{mean, 1 / (std + 1e-8)} of adv_full[index] (device tensor of 2 floats, overwritten by the next call)."""
        c = self._ct
        self._pn.check(self._lib.rp_adv_stats_dev(
            c.c_void_p(adv_full.data_ptr()), c.c_void_p(index.data_ptr()) if index is not None else None,
            int(index.shape[0] if index is not None else adv_full.shape[0]), c.c_void_p(self._stats.data_ptr()),
            c.c_void_p(self._stat_scratch.data_ptr()), c.c_void_p(torch.cuda.current_stream(adv_full.device).cuda_stream)))
        return self._stats

    @torch.no_grad()
    def run(self, obs, act, adv, logp_old, val_old, ret, cliprange, vf_coef, ent_coef, index=None, adv_stats=None,
            entropy_grad=True, norm=None, diagnostics=False, cobs=None, cnorm=None):
        """index (int64 [B], optional): minibatch sample i is row index[i] of obs / act / logp_old / val_old / ret
        (the whole rollout's tensors, no gathered copies).  adv: in minibatch order and normalised by the caller, or
        - with adv_stats (minibatch_adv_stats()) - the rollout's raw advantage, indexed like the rest and normalised
        in the kernel.  entropy_grad=False leaves the entropy bonus of the log-std to FusedAdam.step().  norm (an ``ObsNorm``,
        optional): obs holds raw observations, normalised where the kernels fetch them (rp_ppo_grad_norm_dev).  diagnostics: the
        action net's launch is its diagnostics instance (rp_ppo_grad_diag_dev), which also leaves the minibatch's approx_kl and
        clip_frac in the vector (``diag()``).  cobs, cnorm: the critic rows (indexed like obs) and their statistics, for a policy
        with an asymmetric critic (rp_ppo_grad_asym_dev: the same kernels, the value net's launch on its own arguments)."""
        c = self._ct
        B = int(index.shape[0]) if (index is not None and adv_stats is not None) else int(adv.shape[0])
        flat = torch.cat([self._named[k].detach().reshape(-1) for k in self._pn.PARAM_ORDER] + [self._zero])
        packed = flat[self._map]
        self._packed_pi = packed if self.cobs_dim is None else packed[:self._split]      # (kept for sym_run() on the same parameters)
        if self.cobs_dim is None:
            need = int(self._lib.rp_ppo_workspace_floats(self.obs_dim, self.act_dim, B))
        else:
            need = int(self._lib.rp_ppo_asym_workspace_floats(self.obs_dim, self.cobs_dim, self.act_dim, B))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=obs.device)
        ptr = lambda t: c.c_void_p(t.data_ptr()) if t is not None else None
        stream = c.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        if self.cobs_dim is not None:
            if cobs is None or cobs.shape[-1] != self.cobs_dim or not cobs.is_contiguous() or cobs.dtype != torch.float32:
                raise ValueError("an asymmetric critic needs contiguous float32 critic rows of %d columns" % self.cobs_dim)
            if (norm is None) != (cnorm is None):
                raise ValueError("statistics for both nets, or for neither")
            if norm is not None:
                _check_norm(norm, self.obs_dim, obs.device)
                _check_norm(cnorm, self.cobs_dim, obs.device)
            self._pn.check(self._lib.rp_ppo_grad_asym_dev(
                ptr(packed[:self._split]), ptr(packed[self._split:]), ptr(obs), ptr(cobs), ptr(act), ptr(adv), ptr(adv_stats), ptr(logp_old),
                ptr(val_old), ptr(ret), ptr(index), B, self.obs_dim, self.cobs_dim, self.act_dim, float(cliprange), float(vf_coef),
                ptr(norm.norm) if norm is not None else None, ptr(cnorm.norm) if cnorm is not None else None,
                float(norm.clip) if norm is not None else 0.0, float(cnorm.clip) if cnorm is not None else 0.0, int(bool(diagnostics)),
                ptr(self._g), ptr(self._ws), stream))
        elif diagnostics:
            if norm is not None:
                _check_norm(norm, self.obs_dim, obs.device)
            self._pn.check(self._lib.rp_ppo_grad_diag_dev(
                ptr(packed), ptr(obs), ptr(act), ptr(adv), ptr(adv_stats), ptr(logp_old), ptr(val_old), ptr(ret), ptr(index), B,
                self.obs_dim, self.act_dim, float(cliprange), float(vf_coef), ptr(norm.norm) if norm is not None else None,
                float(norm.clip) if norm is not None else 0.0, ptr(self._g), ptr(self._ws), stream))
        elif norm is None:
            self._pn.check(self._lib.rp_ppo_grad_dev(
                ptr(packed), ptr(obs), ptr(act), ptr(adv), ptr(adv_stats), ptr(logp_old), ptr(val_old), ptr(ret), ptr(index), B,
                self.obs_dim, self.act_dim,
                float(cliprange), float(vf_coef), ptr(self._g), ptr(self._ws), stream))
        else:
            _check_norm(norm, self.obs_dim, obs.device)
            self._pn.check(self._lib.rp_ppo_grad_norm_dev(
                ptr(packed), ptr(obs), ptr(act), ptr(adv), ptr(adv_stats), ptr(logp_old), ptr(val_old), ptr(ret), ptr(index), B,
                self.obs_dim, self.act_dim, float(cliprange), float(vf_coef), ptr(norm.norm), float(norm.clip), ptr(self._g),
                ptr(self._ws), stream))
        if entropy_grad:
            self._views["log_std"] -= ent_coef        # entropy bonus of a state-independent log-std
        for name, p in self._named.items():
            p.grad = self._views[name]
        pg = self._g[self._layout["pi_loss"][0]]
        vf = self._g[self._layout["vf_loss"][0]]
        return pg, vf

    @torch.no_grad()
    def sym_run(self, obs, obs_image, act_src, coef, index=None, norm=None, accumulate=False, repack=True):
        """The mirror-symmetry loss of the action mean (rp_sym_grad_dev) on the minibatch ``index`` of obs and of
        obs_image (the rows M obs).  accumulate=False (the C ABI's 0) overwrites the action block's parameter entries and L_sym's
        slot; accumulate=True, behind ``run()`` on the same parameters, adds its gradient into the vector ``run()`` left, in front of
        ``FusedAdam.step``.  act_src: the action map P, a sequence of act_dim ints.  Returns the
        view of L_sym's slot.  repack=False: the operand blob ``run()`` packed is read again (the parameters have not moved since)."""
        c = self._ct
        if repack or getattr(self, "_packed_pi", None) is None:
            flat = torch.cat([self._named[k].detach().reshape(-1) for k in self._pn.PARAM_ORDER] + [self._zero])
            packed = flat[self._map]
            self._packed_pi = packed if self.cobs_dim is None else packed[:self._split]
        B = int(index.shape[0]) if index is not None else int(obs.shape[0])
        need = int(self._lib.rp_sym_workspace_floats(self.obs_dim, self.act_dim, B))
        if getattr(self, "_sym_ws", None) is None or self._sym_ws.numel() < need:
            self._sym_ws = torch.empty(need, device=obs.device)
        for name, t in (("obs", obs), ("obs_image", obs_image)):
            if t.dim() != 2 or t.shape[1] != self.obs_dim or not t.is_contiguous() or t.dtype != torch.float32 or t.device != self._g.device:
                raise ValueError("%s must be contiguous float32 rows of %d columns on %s" % (name, self.obs_dim, self._g.device))
        if tuple(obs_image.shape) != tuple(obs.shape):
            raise ValueError("the image rows must have the observation rows' shape")
        if index is not None and (index.dim() != 1 or index.dtype != torch.int64 or not index.is_contiguous() or index.device != self._g.device):
            raise ValueError("index must be a contiguous int64 vector on %s" % (self._g.device,))
        src = (c.c_int32 * self.act_dim)(*[int(j) for j in act_src])
        ptr = lambda t: c.c_void_p(t.data_ptr()) if t is not None else None
        stream = c.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        head = (ptr(self._packed_pi), ptr(obs), ptr(obs_image), ptr(index), B, self.obs_dim, self.act_dim, src, float(coef))
        tail = (ptr(self._g), int(bool(accumulate)), ptr(self._sym_ws), stream)
        if norm is None:
            self._pn.check(self._lib.rp_sym_grad_dev(*head, *tail))
        else:
            _check_norm(norm, self.obs_dim, obs.device)
            self._pn.check(self._lib.rp_sym_grad_norm_dev(*head, ptr(norm.norm), float(norm.clip), *tail))
        return self._g[self._layout["symmetry_loss"][0]]

    def diag(self):
        """(approx_kl, clip_frac) of the last ``run(diagnostics=True)``: views of the gradient vector's two slots."""
        return self._g[self._layout["approx_kl"][0]], self._g[self._layout["clip_frac"][0]]


class FusedAdam:
    """``clip_grad_norm_`` + ``torch.optim.Adam.step`` as ONE launch (include/roboy_policy.h: rp_clip_adam_dev) over the
    flat gradient vector of a ``FusedPolicyGrad``.  The policy's parameters become views of one flat buffer laid out
    like that vector, so the kernel updates them in place and the cross-rank average is one all-reduce of one
    contiguous tensor.  State (first / second moments, step count) is checkpointed by ``state_dict()``.
    schedule ({"desired_kl", "lr_factor", "lr_min", "lr_max"}, optional): the learning rate is a one-float device tensor
    (``lr_dev``) that rp_clip_adam_kl_dev moves by the KL-adaptive rule in front of every step, from the approx_kl slot a
    ``FusedPolicyGrad.run(diagnostics=True)`` left in the gradient vector - summed over the ranks with the rest of it."""

    def __init__(self, fgrad, lr, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, schedule=None):
        self._f = fgrad
        self.schedule = dict(schedule) if schedule is not None else None
        self.lr_dev = torch.full((1,), float(np.float32(lr)), device=fgrad._g.device) if schedule is not None else None
        self.lr, self.betas, self.eps, self.max_grad_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_grad_norm)
        g = fgrad._g
        self.params = torch.zeros_like(g)
        with torch.no_grad():
            for name, p in fgrad._named.items():
                off, shape = fgrad._layout[name]
                view = self.params[off:off + p.numel()].view(shape)
                view.copy_(p.data)
                p.data = view                              # the module's parameter IS the slice of the flat buffer
        self.m, self.v = torch.zeros_like(g), torch.zeros_like(g)
        self.t = 0

    @torch.no_grad()
    def step(self, ent_coef, dist=None):
        f, c = self._f, self._f._ct
        scale = 1.0
        if dist_ranks(dist) > 1:
            if dist.get_backend() == "nccl":
                dist.all_reduce(f._g)                      # one bucket: the whole gradient vector, contiguous
            else:                                          # rehearsal over gloo: through the host
                host = f._g.cpu()
                dist.all_reduce(host)
                f._g.copy_(host)
            scale = 1.0 / dist.get_world_size()
        self.t += 1
        ptr = lambda t: c.c_void_p(t.data_ptr())
        stream = c.c_void_p(torch.cuda.current_stream(f._g.device).cuda_stream)
        if f.cobs_dim is not None:              # an asymmetric critic: the same kernels over its longer vector
            if self.schedule is not None:
                k = self.schedule
                f._pn.check(f._lib.rp_clip_adam_kl_asym_dev(ptr(self.params), ptr(f._g), ptr(self.m), ptr(self.v), f.obs_dim, f.cobs_dim,
                                                            f.act_dim, ptr(self.lr_dev), k["desired_kl"], k["lr_factor"], k["lr_min"],
                                                            k["lr_max"], self.betas[0], self.betas[1], self.eps, self.t,
                                                            self.max_grad_norm, scale, float(ent_coef), stream))
            else:
                f._pn.check(f._lib.rp_clip_adam_asym_dev(ptr(self.params), ptr(f._g), ptr(self.m), ptr(self.v), f.obs_dim, f.cobs_dim,
                                                         f.act_dim, self.lr, self.betas[0], self.betas[1], self.eps, self.t,
                                                         self.max_grad_norm, scale, float(ent_coef), stream))
            return scale
        if self.schedule is not None:
            k = self.schedule
            f._pn.check(f._lib.rp_clip_adam_kl_dev(ptr(self.params), ptr(f._g), ptr(self.m), ptr(self.v), f.obs_dim, f.act_dim,
                                                   ptr(self.lr_dev), k["desired_kl"], k["lr_factor"], k["lr_min"], k["lr_max"],
                                                   self.betas[0], self.betas[1], self.eps, self.t, self.max_grad_norm, scale,
                                                   float(ent_coef), stream))
            return scale
        f._pn.check(f._lib.rp_clip_adam_dev(ptr(self.params), ptr(f._g), ptr(self.m), ptr(self.v), f.obs_dim, f.act_dim, self.lr,
                                            self.betas[0], self.betas[1], self.eps, self.t, self.max_grad_norm, scale, float(ent_coef),
                                            stream))
        return scale

    def state_dict(self):
        return {"fused_adam": True, "m": self.m.clone(), "v": self.v.clone(), "t": self.t}

    def load_state_dict(self, sd):
        if tuple(sd["m"].shape) != tuple(self.m.shape) or tuple(sd["v"].shape) != tuple(self.v.shape):
            raise ValueError("optimiser state of another policy layout: moments of %d values, this policy's flat vector has %d "
                             "(obs_dim %d, act_dim %d)" % (sd["m"].numel(), self.m.numel(), self._f.obs_dim, self._f.act_dim))
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"]); self.t = int(sd["t"])

    def rebind(self, state_dict):
        """load_state_dict() of the module copies INTO the views (in place), so nothing to re-point; kept for clarity."""
        return state_dict


def _flat_names(policy):
    """layout name (include/roboy_policy.h: the flat gradient / parameter vector) -> parameter of an MlpPolicy"""
    pi, vf = policy.pi, policy.vf
    return {"pi_w1": pi[0].weight, "pi_b1": pi[0].bias, "pi_w2": pi[2].weight, "pi_b2": pi[2].bias, "pi_w3": pi[4].weight,
            "pi_b3": pi[4].bias, "vf_w1": vf[0].weight, "vf_b1": vf[0].bias, "vf_w2": vf[2].weight, "vf_b2": vf[2].bias,
            "vf_w3": vf[4].weight, "vf_b3": vf[4].bias, "log_std": policy.log_std}


def _param_slices(policy, layout):
    """[(offset, shape)] in the flat vector for policy.parameters(), in that order"""
    by_id = {id(p): name for name, p in _flat_names(policy).items()}
    return [layout[by_id[id(p)]] for p in policy.parameters()]


def adam_state_torch_to_flat(sd, policy, layout, m, v):
    """Moments and step count of a ``torch.optim.Adam`` state_dict over ``policy.parameters()`` into the flat vectors m, v of
    the fused optimiser; returns the step count, or None if the state holds no moments yet (an optimiser that never stepped)."""
    state = sd.get("state", {})
    if not state:
        return None
    order = [i for g in sd["param_groups"] for i in g["params"]]
    slices = _param_slices(policy, layout)
    if len(order) != len(slices):
        raise ValueError("optimiser state of another module: %d parameters, this policy has %d" % (len(order), len(slices)))
    # every parameter or none: moments of some parameters under ONE step count would resume the others with zero moments and a
    # bias correction that assumes they have been stepping all along
    # (a parameter with requires_grad = False is never stepped by torch.optim.Adam and has no state: zero moments are exact for it)
    frozen = {idx for idx, p in zip(order, policy.parameters()) if not p.requires_grad}
    missing = [idx for idx in order if state.get(idx) is None and idx not in frozen]
    if missing:
        raise ValueError("partial optimiser state: %d of %d parameters carry no moments (a torch.optim.Adam that stepped only some of "
                         "its parameters cannot be converted to the flat form)" % (len(missing), len(order)))
    t = 0
    for idx, (off, shape) in zip(order, slices):
        st = state.get(idx)
        if st is None:                                       # frozen: leave its (zero) moments alone
            continue
        if tuple(st["exp_avg"].shape) != tuple(shape):
            raise ValueError("optimiser state of another policy layout: %r against %r" % (tuple(st["exp_avg"].shape), tuple(shape)))
        n = int(st["exp_avg"].numel())
        m[off:off + n].copy_(st["exp_avg"].reshape(-1)); v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
        t = max(t, int(st["step"]))
    return t


def adam_state_flat_to_torch(fsd, policy, layout, template_sd):
    """A ``FusedAdam`` state (flat moments m, v and step count t) as the state_dict of a ``torch.optim.Adam`` over
    ``policy.parameters()`` with the parameter groups of ``template_sd``."""
    order = [i for g in template_sd["param_groups"] for i in g["params"]]
    state = {}
    for idx, (off, shape) in zip(order, _param_slices(policy, layout)):
        n = 1
        for d in shape:
            n *= int(d)
        state[idx] = {"step": torch.tensor(float(fsd["t"])), "exp_avg": fsd["m"][off:off + n].view(shape).clone(),
                      "exp_avg_sq": fsd["v"][off:off + n].view(shape).clone()}
    return {"state": state, "param_groups": template_sd["param_groups"]}


def average_gradients(module, dist=None):
    world = dist_ranks(dist)
    if world <= 1:
        return
    flat = torch.cat([p.grad.reshape(-1) for p in module.parameters() if p.grad is not None])
    dist.all_reduce(flat)          # one bucket: the policy is ~10^4 parameters
    flat /= world
    off = 0
    for p in module.parameters():
        if p.grad is not None:
            n = p.grad.numel()
            p.grad.copy_(flat[off:off + n].view_as(p.grad))
            off += n


def _fused_kernels_apply(policy, obs_dim, act_dim):
    """MlpPolicy's shape (two hidden layers of 64 units per net) in dimensions the kernels of include/roboy_policy.h
    support, and the library is there."""
    try:
        from . import _policy_native as pn
        ok_shape = (isinstance(policy, MlpPolicy) and len(policy.pi) == 5 and len(policy.vf) == 5
                    and all(l.out_features == 64 for l in (policy.pi[0], policy.pi[2], policy.vf[0], policy.vf[2])))
        cd = getattr(policy, "critic_obs_dim", None)
        return bool(ok_shape and pn.load().rp_train_packed_floats(obs_dim, act_dim) > 0
                    and (cd is None or pn.load().rp_train_packed_floats(cd, act_dim) > 0))
    except Exception:
        return False


class _MirrorMaps:
    """An env's ``mirror_map()`` on the agent's device: the column sources as int64 (torch indexing) and int32 (the
    kernel's), the signs as float32 - and for the per-sample scalars the identity map of width 1.  ``rows(x, kind)`` is the torch
    statement; ``rows_into(src, out, kind)`` fills a [2 n, width] buffer, first half = ``src``, second half = its image, with one
    launch of rp_mirror_rows_dev."""

    def __init__(self, maps, obs_dim, act_dim, device):
        obs_src, obs_sign, act_src = (np.asarray(m) for m in maps)
        for name, src, width in (("obs_src", obs_src, obs_dim), ("act_src", act_src, act_dim)):
            if src.shape != (width,) or sorted(int(i) for i in src) != list(range(width)):
                raise ValueError("mirror_map(): %s must be a permutation of the row's %d columns" % (name, width))
        if obs_sign.shape != (obs_dim,) or not np.all(np.abs(obs_sign) == 1.0):
            raise ValueError("mirror_map(): obs_sign must hold %d entries of +-1" % obs_dim)
        dev = torch.device(device)
        t = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)
        self.device = dev
        self.src = {"obs": t(obs_src, torch.int64), "act": t(act_src, torch.int64)}
        self.sign = {"obs": t(obs_sign, torch.float32), "act": None}
        self._src32 = {"obs": t(obs_src, torch.int32), "act": t(act_src, torch.int32), "one": torch.zeros(1, dtype=torch.int32, device=dev)}
        self._sign32 = {"obs": self.sign["obs"], "act": torch.ones(act_dim, device=dev), "one": torch.ones(1, device=dev)}
        self._native = None

    def rows(self, x, kind):
        """the image of rows of kind "obs" or "act" (``envs.symmetry.mirror_rows``: ``x[..., src] * sign``)"""
        out = x[..., self.src[kind]]
        return out if self.sign[kind] is None else out * self.sign[kind]

    def kernel_applies(self):
        """on a GPU the second halves come from rp_mirror_rows_dev (a missing library is an error there, as it is for the statistics'
        kernels: no quiet torch path); on the CPU from ``rows``"""
        if self.device.type != "cuda":
            return False
        if self._native is None:
            import ctypes
            from . import _policy_native as pn
            self._native = (pn, ctypes, pn.load())           # (raises without the library, at every call)
        return True

    @torch.no_grad()
    def rows_into(self, src, out, kind, plain=True):
        """out [2 n, width] (or [2 n]) <- [src; image of src], src [n, width] (or [n]) contiguous float32 on the GPU; kind: "obs",
        "act", or "one" - the per-sample scalars, which are copied.  plain=False: out [n, width] <- the image alone"""
        pn, c, lib = self._native
        n = int(src.shape[0])
        width = int(src.shape[1]) if src.dim() == 2 else 1
        ptr = lambda t: c.c_void_p(t.data_ptr())
        pn.check(lib.rp_mirror_rows_dev(ptr(src), ptr(out) if plain else None, ptr(out[n:]) if plain else ptr(out), n, width,
                                        ptr(self._src32[kind]), ptr(self._sign32[kind]),
                                        c.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)))


@torch.no_grad()
def evaluate_policy(policy, env, episodes_per_env=1, poll_every=32, fused=None, obs_norm=None, cobs_norm=None, device="cuda"):
    """Run ``policy``'s DETERMINISTIC action (the mean) on every env of ``env`` - a ``RoboyVecEnv`` with ``episode_log >=
    episodes_per_env`` - until each env has finished ``episodes_per_env`` episodes, and return ``env.episode_log_summary(first_k=
    episodes_per_env)`` plus ``"steps"``.  Every env contributes exactly its first ``episodes_per_env`` episodes (envs that finish early
    go on stepping, unrecorded), so the figures are not biased towards short episodes.  The loop: reset, clear the log, then policy
    step and ``env.step`` on device tensors; every ``poll_every`` steps one 4-byte read tells whether every env is done.  An episode
    has at most ``env.max_episode_length`` steps, so ``episodes_per_env * max_episode_length`` steps always suffice: a log that is not
    complete then is an error.  fused: a ``FusedPolicyStep`` over ``policy`` (its kernel then takes the step, with ``obs_norm`` /
    ``cobs_norm`` as ``act_into`` takes them); None: ``policy.act`` (which applies the statistics the policy holds).  No statistics are
    updated, no noise is drawn.  An asymmetric critic's value is not needed: the env's critic rows are handed where it writes them
    at the policy's width, else zeros, and the value is discarded."""
    E, poll = int(episodes_per_env), int(poll_every)
    if E < 1 or poll < 1:
        raise ValueError("episodes_per_env and poll_every must be >= 1, got %r and %r" % (episodes_per_env, poll_every))
    obs_dim, act_dim = policy.pi[0].in_features, policy.pi[-1].out_features
    if env.observation_space.shape[0] != obs_dim:
        raise ValueError("the policy reads %d observation columns, this env gives %d: the row's layout (tendon_obs, action_obs) must be "
                         "the one the policy was trained on" % (obs_dim, env.observation_space.shape[0]))
    if int(getattr(env, "episode_log_capacity", 0) or 0) < E:
        raise ValueError("evaluation of %d episodes per env needs an env built with episode_log >= %d, this one has episode_log=%r"
                         % (E, E, getattr(env, "episode_log_capacity", 0) or None))
    device = torch.device(device)
    n = env.num_envs
    obs = torch.as_tensor(env.reset(), dtype=torch.float32, device=device)
    env.clear_episode_log()
    cobs_dim = getattr(policy, "critic_obs_dim", None)
    own_rows = cobs_dim is not None and getattr(env, "critic_obs_dim", 0) == cobs_dim
    cobs = None
    if cobs_dim is not None and fused is not None:
        cobs = torch.as_tensor(env.critic_obs(), dtype=torch.float32, device=device) if own_rows else torch.zeros((n, cobs_dim), device=device)
    if fused is not None:
        packed = fused.pack()
        act, logp, val = torch.empty((n, act_dim), device=device), torch.empty(n, device=device), torch.empty(n, device=device)
    bound = E * int(env.max_episode_length)
    steps = 0
    while steps < bound:
        if fused is not None:
            fused.act_into(obs, act, logp, val, packed=packed, deterministic=True, norm=obs_norm, cobs=cobs, cnorm=cobs_norm)
            action = act
        else:
            action = policy.act(obs, deterministic=True)[0].clamp(-1.0, 1.0).contiguous()
        obs = env.step(action)[0]
        if own_rows and fused is not None:
            cobs = env.critic_obs()
        steps += 1
        if (steps % poll == 0 or steps == bound) and env.episode_log_full() == n:
            break
    summary = env.episode_log_summary(first_k=E)
    if not summary["complete"]:
        raise RuntimeError("evaluation: after %d steps (%d episodes of at most %d steps) only %d of %d envs have their %d records"
                           % (steps, E, env.max_episode_length, summary["n_complete"], n, E))
    summary["steps"] = steps
    return summary


def pack_arrays(x):
    """a nest of dicts, lists and tuples with its numpy arrays as ``{"__ndarray__": bytes as a uint8 tensor, "dtype", "shape"}``: what
    ``torch.load`` takes under ``weights_only=True``, whatever the arrays' types (a resume record holds the env's state blob)"""
    if isinstance(x, dict):
        return {k: pack_arrays(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(pack_arrays(v) for v in x)
    if isinstance(x, np.ndarray):
        flat = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        return {"__ndarray__": torch.from_numpy(flat.copy()), "dtype": str(x.dtype), "shape": [int(d) for d in x.shape]}
    if isinstance(x, np.generic):
        return x.item()
    return x


def _tensors_to(x, device):
    """a checkpoint's nest with its tensors on ``device`` (what ``torch.load(map_location=device)`` gives)"""
    if isinstance(x, dict):
        return type(x)((k, _tensors_to(v, device)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return type(x)(_tensors_to(v, device) for v in x)
    return x.to(device) if torch.is_tensor(x) else x


def unpack_arrays(x):
    if isinstance(x, dict):
        if "__ndarray__" in x:
            return x["__ndarray__"].cpu().numpy().view(np.dtype(x["dtype"])).reshape(x["shape"]).copy()
        return {k: unpack_arrays(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(unpack_arrays(v) for v in x)
    return x


class PPO:
    def __init__(self, env, policy=None, n_steps=128, nminibatches=4, noptepochs=4, gamma=0.99, lam=0.95,
                 learning_rate=2.5e-4, cliprange=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5,
                 device="cuda", dist=None, reward_scale=1.0, seed=0, use_graphs=False, fused_policy=None,
                 fused_update=None, rollout_chains=None, normalize_obs=False, clip_obs=10.0, obs_norm_prime=True,
                 normalize_reward=False, clip_reward=10.0, reward_norm_prime=True, bootstrap_timeouts=False,
                 lr_schedule=None, desired_kl=0.01, lr_factor=1.5, lr_min=1e-5, lr_max=1e-2, diagnostics=False,
                 asymmetric_critic=False, symmetry=None, symmetry_coef=1.0):
        """fused_policy / fused_update: None = the fused MFMA kernels whenever they apply (a GPU, MlpPolicy's shape,
        dimensions the kernels support), True = insist, False = the torch path (the statement the kernels are
        tested against).  The gradient kernel takes up to 63 observation columns: an env with ``action_obs=K`` stays fused while
        ``obs_dim`` fits (MsjRobot with length and force: 25 + 8 K columns, K <= 4) and falls back to the torch path above that
        unless the fused kernels are insisted on.
        rollout_chains: graph mode with the fused policy step - 2 = the rollout as two independent chains of (policy step, env
        step) launches over the two halves of the batch on two streams, joined in front of GAE (the sub-range entry points of
        include/roboy_sim.h: one half's launch gaps and load / store phases lie under the other half's kernels; the results do
        not depend on the split); 1 = one chain over the whole batch; None = two from ``CHAIN_BATCH`` envs on where the env's
        kernel form steps sub-ranges and the policy is of MsjRobot's size.
        normalize_obs: running mean / variance normalisation of the observation (``ObsNorm``), clamped to +-clip_obs; the
        statistics are frozen through a rollout and the update on it, then merged with that rollout's moments.  obs_norm_prime:
        while no statistics exist, the first ``collect()`` runs one rollout under the identity for its moments alone (not
        returned, not counted in ``num_timesteps``) and collects again.
        normalize_reward: the scaled reward is divided by the running standard deviation of the discounted return and clamped to
        +-clip_reward (``RewardNorm``); the statistics are frozen through a rollout and merged with its returns at the end of
        ``collect()``.  reward_norm_prime: the same priming rollout, run while either set of statistics is empty.
        bootstrap_timeouts: an episode that ended at the env's time limit is not treated as if its return stopped there - GAE adds
        gamma * V(last observation before the limit) to that step's reward (``gae_boot``).  Needs an env built with
        ``report_truncation=True``.  With the fused policy step the rollout's tail is one launch (rp_rollout_tail_boot_dev), under
        ``normalize_reward`` or not; the rollout dict gains ``"trunc"`` ([T, N] floats, 1 where the step was truncated).
        diagnostics: ``update()`` also returns ``"approx_kl"`` = mean 0.5 (logp - logp_old)^2 and ``"clip_frac"`` = the share of samples
        whose ratio left [1 - cliprange, 1 + cliprange], of the last minibatch (stable-baselines PPO2's approxkl / clipfrac).  With several
        ranks the loss terms and these two are the ranks' means, on both optimiser paths.
        lr_schedule: None = ``learning_rate`` for the whole run; "adaptive" (implies diagnostics) = rsl_rl's schedule, applied in front
        of every minibatch's optimiser step in float32 (``adapt_lr``): approx_kl above 2 desired_kl divides the learning rate by
        lr_factor, approx_kl below desired_kl / 2 (and above 0) multiplies it, within [lr_min, lr_max]; with several ranks the KL is
        their mean, so every rank takes the same decision.  ``update()`` then returns ``"lr"`` too and ``agent.learning_rate`` reads
        the current value.  ``lr_history``: assign a list and every minibatch appends its (approx_kl, lr after the rule) - device
        tensors on the fused path, which adds no synchronisation by it.  DESIGN.md §19.
        asymmetric_critic: the value net is trained on the env's privileged critic rows (``RoboyVecEnv(critic_obs=...)``: the exact
        state, the env's own parameters and delay) instead of the noisy, late observation the actor gets - in simulation they are
        free, and only the actor is deployed.  The rollout keeps ``cobs`` beside ``obs`` and every value - the rollout's, the last
        one, the minibatch loss - reads it; ``normalize_obs`` keeps a second set of statistics for it.  Eager and graph modes, torch
        and fused paths.  DESIGN.md §20.
        symmetry: None, or "augment" - every update runs on the rollout's samples AND their mirror images (``augment``): for a robot
        with a mirror plane the twin ``(M s, P a, r, M s')`` of a transition is as valid as the original and costs no simulation.
        The same number of optimiser steps on minibatches twice the size; ``sample_orders`` index ``[0, 2 T N)``; the observation
        statistics of ``normalize_obs`` are merged over the rows and their images.  Needs an env with ``mirror_map()`` (RoboyVecEnv on
        a robot with a mirror plane); not with ``asymmetric_critic``, whose critic rows have no map yet.  ``symmetry_gap(roll)``
        measures how far the policy is from the symmetry.  Eager and graph modes, torch and fused paths; the augmentation is
        rank-local and sits in front of the collectives.  DESIGN.md §25.
        "loss" - the samples stay the rollout's; every minibatch's loss gains
        ``symmetry_coef * mean_i,j (mu(M s_i)[j] - mu(s_i)[P j])^2`` (mu: the action mean, M / P: the env's observation / action maps),
        with the gradient through both branches: ``symmetry_coef * symmetry_gap(...)["action"]`` on the minibatch's rows.  It touches the
        action net and the actor's rows only, so it combines with ``asymmetric_critic``; log_std and the value net get no gradient from
        it.  On the fused path one more gradient kernel per minibatch (rp_sym_grad_dev) adds into the PPO gradient in front of
        clip + Adam; the image rows are written once per update.  ``normalize_obs`` merges the rows and their images, as "augment" does.
        ``update()`` also returns ``"symmetry_loss"``, the last minibatch's term.  symmetry_coef (>= 0) is used by "loss" only; the
        checkpoint records it, and ``load`` keeps the constructor's value, warning where the checkpoint's differs.
        DESIGN.md §26."""
        if symmetry not in (None,) + SYMMETRY_MODES:
            raise ValueError("unknown symmetry %r: None or one of %r" % (symmetry, SYMMETRY_MODES))
        if not float(symmetry_coef) >= 0.0 or math.isinf(float(symmetry_coef)):
            raise ValueError("symmetry_coef must be finite and >= 0")
        if symmetry == "augment" and asymmetric_critic:
            raise ValueError("symmetry=%r does not combine with asymmetric_critic: the critic rows (parameters, delay, age) have no "
                             "mirror map yet" % (symmetry,))
        if symmetry is not None and not callable(getattr(env, "mirror_map", None)):
            raise ValueError("symmetry=%r needs an env that knows its mirror image: env.mirror_map() (RoboyVecEnv on a robot with a "
                             "mirror plane)" % (symmetry,))
        if lr_schedule is not None and lr_schedule not in LR_SCHEDULES:
            raise ValueError("unknown lr_schedule %r: None or one of %r" % (lr_schedule, LR_SCHEDULES))
        if not desired_kl > 0.0:
            raise ValueError("desired_kl must be > 0")
        if not lr_factor > 1.0:
            raise ValueError("lr_factor must be > 1")
        if not (lr_min > 0.0 and lr_min <= lr_max):
            raise ValueError("need 0 < lr_min <= lr_max")
        if lr_schedule is not None and not lr_min <= learning_rate <= lr_max:
            raise ValueError("learning_rate %r outside [lr_min, lr_max] = [%r, %r]" % (learning_rate, lr_min, lr_max))
        self.lr_schedule = lr_schedule
        self.diagnostics = bool(diagnostics) or lr_schedule is not None
        self.desired_kl, self.lr_factor, self.lr_min, self.lr_max = float(desired_kl), float(lr_factor), float(lr_min), float(lr_max)
        self._lr0 = learning_rate
        self._lr32 = np.float32(learning_rate)       # the scheduled learning rate of the torch path, float32 as the kernel's
        self.lr_history = None
        self.env, self.dist, self.device = env, dist, torch.device(device)
        self._chains_arg = rollout_chains
        torch.manual_seed(seed)
        obs_dim = env.observation_space.shape[0]
        act_dim = env.action_space.shape[0]
        self.asymmetric_critic = bool(asymmetric_critic)
        self.cobs_dim = None
        if self.asymmetric_critic:
            self.cobs_dim = int(getattr(env, "critic_obs_dim", 0) or 0)
            if self.cobs_dim < 1:
                raise ValueError("asymmetric_critic needs an env that writes critic rows: RoboyVecEnv(critic_obs=(\"state\", ...))")
            if policy is not None and getattr(policy, "critic_obs_dim", None) != self.cobs_dim:
                raise ValueError("asymmetric_critic: the env's critic rows have %d columns, the policy's value net reads %r"
                                 % (self.cobs_dim, getattr(policy, "critic_obs_dim", None)))
        elif policy is not None and getattr(policy, "critic_obs_dim", None) is not None:
            raise ValueError("a policy with an asymmetric critic needs PPO(asymmetric_critic=True)")
        self.policy = (policy or MlpPolicy(obs_dim, act_dim, critic_obs_dim=self.cobs_dim)).to(self.device)
        self.obs_norm = ObsNorm(obs_dim, self.device, clip=clip_obs) if normalize_obs else None
        self.cobs_norm = ObsNorm(self.cobs_dim, self.device, clip=clip_obs) if normalize_obs and self.asymmetric_critic else None
        self._obs_norm_prime = bool(obs_norm_prime)
        if self.obs_norm is not None or getattr(self.policy, "obs_norm", None) is not None:
            if self.asymmetric_critic:
                self.policy.set_obs_norm(self.obs_norm, self.cobs_norm)
            else:
                self.policy.set_obs_norm(self.obs_norm)
        if dist_ranks(dist) > 0:                        # an initialised group, be it of one rank
            for p in self.policy.parameters():          # same initial weights on every rank
                dist.broadcast(p.data, 0)
            # ... but each rank's own exploration noise and minibatch order: the reference seeds worker
            # `rank` with seed + rank (/root/reference/gym_roboy/train_parallel.py:24)
            torch.manual_seed(seed + dist.get_rank())
        multi_rank = dist_ranks(dist) > 1
        # the rollout (policy step, env step, GAE) is rank-local, so it is captured on every rank; the collectives
        # (gradient average, statistics) stay outside the graph
        self.use_graphs = bool(use_graphs) and self.device.type == "cuda" and hasattr(env, "step_dev")
        if fused_policy is None or fused_update is None:
            auto = self.device.type == "cuda" and _fused_kernels_apply(self.policy, obs_dim, act_dim)
            fused_policy = auto if fused_policy is None else fused_policy
            fused_update = auto if fused_update is None else fused_update
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=float(self._lr32) if lr_schedule is not None else learning_rate, eps=1e-5)
        self._epoch = 0                       # update epochs so far: keys the fused path's sample order
        self._seed = int(seed) + (7919 * dist.get_rank() if multi_rank else 0)
        self._rollout_graph = None
        self.rollout_chains = 1
        # fused_policy: the rollout's policy step runs as one MFMA kernel (FusedPolicyStep) instead of ~30 torch kernels
        self._fused = None
        if fused_policy:
            if self.device.type != "cuda":
                raise ValueError("fused_policy needs a GPU")
            rank = dist.get_rank() if multi_rank else 0
            self._fused = FusedPolicyStep(self.policy, seed=seed + 7919 * rank)
            self._step_base = torch.zeros(1, dtype=torch.int32, device=self.device)    # rollout steps taken so far
        # fused_update: the minibatch gradient comes from the MFMA kernels (FusedPolicyGrad) instead of torch autograd
        self._fgrad = None
        if fused_update:
            if self.device.type != "cuda":
                raise ValueError("fused_update needs a GPU")
            self._fgrad = FusedPolicyGrad(self.policy)
            schedule = None
            if lr_schedule is not None:
                schedule = {"desired_kl": self.desired_kl, "lr_factor": self.lr_factor, "lr_min": self.lr_min, "lr_max": self.lr_max}
            self._fadam = FusedAdam(self._fgrad, learning_rate, eps=1e-5, max_grad_norm=max_grad_norm, schedule=schedule)
        self.n_steps, self.nminibatches, self.noptepochs = n_steps, nminibatches, noptepochs
        self.gamma, self.lam, self.cliprange = gamma, lam, cliprange
        self.ent_coef, self.vf_coef, self.max_grad_norm = ent_coef, vf_coef, max_grad_norm
        self.reward_scale = reward_scale
        self.reward_norm = None
        if normalize_reward:
            self.reward_norm = RewardNorm(getattr(env, "num_envs", 0), gamma, self.device, clip=clip_reward)
        self._reward_norm_prime = bool(reward_norm_prime)
        self.bootstrap_timeouts = bool(bootstrap_timeouts)
        self._boot_tail = None                # the fused boot tail without normalize_reward: identity statistics, a private return carry
        if self.bootstrap_timeouts:
            if not getattr(env, "report_truncation", False):
                raise ValueError("bootstrap_timeouts needs an env that tells truncated episodes from terminated ones: "
                                 "RoboyVecEnv(report_truncation=True)")
            if self._fused is not None and self.reward_norm is None:
                self._boot_tail = RewardNorm(getattr(env, "num_envs", 0), gamma, self.device, clip=math.inf)
        elif self.use_graphs and getattr(env, "report_truncation", False):
            raise ValueError("an env built with report_truncation=True leaves episode-end codes (0 / 1 / 2) in the done words of "
                             "step_dev, which the captured rollout reads as 0 / 1: pass bootstrap_timeouts=True or build the env without it")
        self._rew_raw = None                  # the last rollout's raw reward (kept with normalize_reward: learn() reports it)
        self.symmetry = symmetry
        self.symmetry_coef = float(symmetry_coef)
        self._mirror = None                   # symmetry: the env's row maps on the agent's device (_MirrorMaps)
        if symmetry is not None:
            self._mirror = _MirrorMaps(env.mirror_map(), obs_dim, act_dim, self.device)
            self._act_src_host = [int(j) for j in np.asarray(env.mirror_map()[2])]      # P for rp_sym_grad_dev (a host array)
        self.last_rollout = None              # learn(): the rollout of its last update (graph mode: views of the graph's buffers)
        self.num_timesteps = 0
        self._obs = None
        self._cobs = None                     # the critic rows that belong to _obs (asymmetric_critic)

    def _critic_rows(self):
        """the env's critic rows of the observation last returned, on the agent's device"""
        return self._to_tensor(self.env.critic_obs())

    def _update_obs_norms(self, obs_rows, cobs_rows, image_rows=None):
        """Merge a rollout's moments into the observation statistics - and the critic rows' into theirs, the two sets of sums
        all-reduced over the ranks as ONE tensor.  image_rows (``symmetry="loss"``): the rows' mirror images join the observation's
        moments - both sets of sums are taken around the same mean, so they add, and no [2 n, obs_dim] copy is made."""
        a, c = self.obs_norm, self.cobs_norm
        if image_rows is not None:
            sa = a.moments(obs_rows.to(a.device)).clone()            # (moments() hands out one buffer)
            sa += a.moments(image_rows.to(a.device))
            if c is None:
                _all_reduce_sums(sa, self.dist)
                return a.merge(sa)
        elif c is None:
            return a.update(obs_rows, self.dist)
        else:
            sa = a.moments(obs_rows.to(a.device))
        sc = c.moments(cobs_rows.to(c.device))
        if dist_ranks(self.dist) > 1:
            both = torch.cat([sa, sc])
            _all_reduce_sums(both, self.dist)
            sa.copy_(both[:sa.numel()]); sc.copy_(both[sa.numel():])
        a.merge(sa); c.merge(sc)

    @property
    def learning_rate(self):
        """The learning rate the next optimiser step starts from (with a schedule on the fused path: read back from the device)."""
        if self._fgrad is not None:
            return float(self._fadam.lr_dev.item()) if self.lr_schedule is not None else self._fadam.lr
        return float(self.opt.param_groups[0]["lr"])

    def _set_lr(self, lr):
        self._lr32 = np.float32(lr)
        self.opt.param_groups[0]["lr"] = float(self._lr32)
        if self._fgrad is not None and self._fadam.lr_dev is not None:
            self._fadam.lr_dev.fill_(float(self._lr32))

    def _to_tensor(self, x, dtype=torch.float32):
        return x.to(self.device, dtype) if torch.is_tensor(x) else torch.as_tensor(x, dtype=dtype, device=self.device)

    # -- HIP-graph mode ------------------------------------------------------------
    # two chains from this many envs on, for policies of MsjRobot's size (measured, us per vectorised rollout step, one -> two chains,
    # profiles/r4_a/ppo_chains.log: MsjRobot 32 768 envs 21.7 -> 25.8, 65 536 envs 31.5 -> 28.4, 262 144 envs 87.6 -> 76.9, 1 M envs
    # 349 -> 296; the upper body's 60 -> 38 policy step does not share the chip with a second launch: 65 536 envs 92.8 -> 91.5,
    # 32 768 envs 55.6 -> 101.8)
    CHAIN_BATCH = 65536
    CHAIN_MAX_OBS = 29

    def _rollout_steps(self, b, lo, hi, stream_ptr=None):
        """The T (policy step, env step) pairs of envs [lo, hi): the whole batch on the env's stream (stream_ptr None), or one
        chain's half on its own stream."""
        env, T = self.env, self.n_steps
        asym = self.asymmetric_critic
        b["obs"][0][lo:hi].copy_(b["carry"][lo:hi])
        if asym:
            b["cobs"][0][lo:hi].copy_(b["ccarry"][lo:hi])
        packed = self._fused.pack() if self._fused is not None else None     # (inside the graph: re-gathered on every replay)
        for t in range(T):
            self._policy_step(b["obs"][t][lo:hi], b["cobs"][t][lo:hi] if asym else None, b["act"][t][lo:hi], b["logp"][t][lo:hi],
                              b["val"][t][lo:hi], t, packed, lo)
            # the fused step's action goes to the env kernel as it is: the kernel clamps it to its box itself
            act = b["act"][t] if self._fused is not None else b["act"][t].clamp(-1.0, 1.0).contiguous()
            # (asymmetric critic: the env step writes the critic rows of its range straight into the rollout's next slice)
            ptrs = (act.data_ptr(), b["obs"][t + 1].data_ptr(), b["rew_raw"][t].data_ptr(), b["done_i"][t].data_ptr(),
                    b["cobs"][t + 1].data_ptr() if asym else None)
            if stream_ptr is None:
                env.step_dev(*ptrs)
            else:
                env.step_range_dev(lo, hi - lo, stream_ptr, *ptrs)

    def _policy_step(self, obs_t, cobs_t, act_t, logp_t, val_t, t, packed, sample_offset=0):
        """Step t's policy step on rows of the rollout's tensors (cobs_t: their critic rows, None with a symmetric critic): one launch
        of the fused kernel straight into ``act_t``, ``logp_t``, ``val_t``, or ``policy.act`` and three copies.  The kernel's noise is
        keyed by the GLOBAL sample index (``sample_offset`` + row): the same draw however the batch is cut."""
        if self._fused is not None:
            self._fused.act_into(obs_t, act_t, logp_t, val_t, step=t, packed=packed, step_base=self._step_base,
                                 sample_offset=sample_offset, norm=self.obs_norm, cobs=cobs_t, cnorm=self.cobs_norm)
            return
        # (a caller's own policy whose act() takes no ``cobs`` keyword keeps working where the critic is symmetric)
        a, logp, v = self.policy.act(obs_t) if cobs_t is None else self.policy.act(obs_t, cobs=cobs_t)
        act_t.copy_(a); logp_t.copy_(logp); val_t.copy_(v)

    def _tail_kernel(self, b, last_value, ret_carry=None):
        """The tail as one launch (rp_rollout_tail_dev / rp_rollout_tail_boot_dev): on the agent's own return statistics under
        ``normalize_reward``, under identity statistics on ``_boot_tail``'s private carry (its sums are discarded) otherwise."""
        rn = self.reward_norm if self.reward_norm is not None else self._boot_tail
        rn.tail(b["rew_raw"], b["done_i"], b["val"], last_value, self.reward_scale, self.lam, b["rew"], b["done"], b["adv"], b["ret"],
                ret_carry=ret_carry, boot=self.bootstrap_timeouts, identity=self.reward_norm is None)

    def _rollout_tail(self, b, value_rows=None, eager=False):
        """Everything behind a rollout's last env step, for the captured graph (one chain and two) and the eager rollout alike: the
        [T, N] tensors ``rew_raw``, ``done_i`` (int32: 0 / 1, episode-end codes under ``bootstrap_timeouts``) and ``val`` of ``b`` and
        the value of ``value_rows`` - the rows the value net reads for the last observation; None: the graph's buffers' own, which are
        then carried over as the next replay's first - become ``rew``, ``done``, ``adv``, ``ret`` (and ``trunc``), by the form
        ``rollout_tail_form`` names.  The all-reduce and merge of the return statistics are the caller's: they stay outside a graph."""
        T, rn, boot = self.n_steps, self.reward_norm, self.bootstrap_timeouts
        if value_rows is None:
            value_rows = b["cobs"][T] if self.asymmetric_critic else b["obs"][T]
        form = rollout_tail_form(self._fused is not None, eager, rn is not None, boot, self.asymmetric_critic)
        if self._fused is not None:
            self._step_base += T                                             # fresh noise on the next rollout
        with torch.no_grad():
            last_value = self.policy.value(value_rows)
        if form == "tail_kernel":
            self._tail_kernel(b, last_value.contiguous())
        else:
            r_s = b["rew_raw"] * self.reward_scale
            if rn is not None:                   # the returns' scan on the scaled reward, the statistics frozen through it
                rn.scan(r_s, b["done_i"])
                r_s = rn.apply(r_s)
            b["rew"].copy_(r_s)
            b["done"].copy_(((b["done_i"] != 0) if boot else b["done_i"]).to(torch.float32))
            if form == "gae_kernel":
                gae_fused(b["rew"], b["val"], b["done"], last_value.contiguous(), self.gamma, self.lam, b["adv"], b["ret"])
            else:
                adv, ret = (gae_boot(b["rew"], b["val"], b["done_i"], last_value, self.gamma, self.lam) if boot else
                            gae(b["rew"], b["val"], b["done"], last_value, self.gamma, self.lam))
                b["adv"].copy_(adv); b["ret"].copy_(ret)
        if boot:
            b["trunc"].copy_((b["done_i"] == 2).to(torch.float32))
        if not eager:
            b["carry"].copy_(b["obs"][T])
            if self.asymmetric_critic:
                b["ccarry"].copy_(b["cobs"][T])

    def _rollout_body(self, b):
        self._rollout_steps(b, 0, b["carry"].shape[0])
        self._rollout_tail(b)

    def _pick_chains(self, N):
        asked = self._chains_arg is not None and int(self._chains_arg) >= 2
        why = None
        if self._fused is None:
            why = "the fused policy step is off (fused_policy=False)"
        elif not hasattr(self.env, "step_range_dev") or not self.env.range_capable():
            why = "the env's kernel form steps whole batches only"
        elif asked and N < 512:
            why = "fewer than 512 envs"
        if why is not None:
            if asked:      # an explicit request that cannot be honoured is said, not dropped silently
                import warnings
                warnings.warn("rollout_chains=%r not honoured (%s): the rollout runs as one chain" % (self._chains_arg, why), RuntimeWarning, stacklevel=3)
            return 1
        if self._chains_arg is not None:
            return 2 if asked else 1
        return 2 if N >= self.CHAIN_BATCH and self._fused.obs_dim <= self.CHAIN_MAX_OBS else 1

    def _build_rollout_graph(self):
        env, T, dev = self.env, self.n_steps, self.device
        N, od, ad = env.num_envs, env.observation_space.shape[0], env.action_space.shape[0]
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        b = {"obs": z(T + 1, N, od), "act": z(T, N, ad), "logp": z(T, N), "val": z(T, N), "rew_raw": z(T, N),
             "rew": z(T, N), "done_i": z(T, N, dtype=torch.int32), "done": z(T, N), "adv": z(T, N), "ret": z(T, N),
             "carry": z(N, od)}
        if self.bootstrap_timeouts:
            b["trunc"] = z(T, N)
        asym = self.asymmetric_critic
        if asym:
            b["cobs"], b["ccarry"] = z(T + 1, N, self.cobs_dim), z(N, self.cobs_dim)
        fresh = self._obs is None             # (not fresh: load() restored a run - its observation and running returns go on)
        if fresh and self.reward_norm is not None:
            self.reward_norm.reset_returns(N)
        if self._boot_tail is not None and (fresh or self._boot_tail.n_envs != N):
            self._boot_tail.reset_returns(N)
        b["carry"].copy_(self._to_tensor(env.reset()) if fresh else self._obs)
        if asym:
            b["ccarry"].copy_(self._critic_rows() if fresh else self._cobs)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        # the env kernel is launched on the simulation's stream: make that the capture stream
        env.set_stream(side.cuda_stream)
        # kernels the simulation specialises at run time (hiprtc) are built now: a compilation and a module load
        # must not fall into the capture below
        if hasattr(getattr(env, "sim", None), "specialization"):
            env.sim.specialization()
        with torch.cuda.stream(side), torch.no_grad():
            # first use of the GEMM library for these shapes (handle, workspace) must not fall into the capture
            self.policy.act(b["carry"], cobs=b["ccarry"]) if asym else self.policy.act(b["carry"])
            self.policy.value(b["ccarry"] if asym else b["carry"])
            if self._fused is not None:       # its one-time launch configuration must not fall into the capture either
                self._fused.act_into(b["carry"], b["act"][0], b["logp"][0], b["val"][0], deterministic=True, norm=self.obs_norm,
                                     cobs=b["ccarry"] if asym else None, cnorm=self.cobs_norm)
                tail = self.reward_norm if self.reward_norm is not None else self._boot_tail
                if tail is not None:          # nor the tail kernel's (on a copy of the returns: they must not move)
                    self._tail_kernel(b, b["val"][0], ret_carry=tail.ret_carry.clone())
        side.synchronize()
        self.rollout_chains = self._pick_chains(N)
        # thread-local capture mode: another thread of the process (RCCL's watchdog in a multi-rank run) may call into
        # the runtime while this one captures
        if self.rollout_chains == 1:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                self._rollout_body(b)
            self._rollout_graph = graph
        else:
            # two chains: one graph per half of the batch (each on a stream of its own when replayed) and one for what follows
            # the join.  Two LINEAR graphs, not one with two branches: csrc/roboy_sim.hip, rb_rollout_dev.
            mid = ((N // 2 + 255) // 256) * 256
            side2 = torch.cuda.Stream(device=dev)
            self._chain_stream = side2
            graphs = []
            for (lo, hi), st in (((0, mid), side), ((mid, N), side2)):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st, capture_error_mode="thread_local"):
                    self._rollout_steps(b, lo, hi, stream_ptr=st.cuda_stream)
                graphs.append(g)
            tail = torch.cuda.CUDAGraph()
            with torch.cuda.graph(tail, stream=side, capture_error_mode="thread_local"):
                self._rollout_tail(b)
            self._rollout_graph = (graphs[0], graphs[1], tail)
        torch.cuda.current_stream(dev).wait_stream(side)
        # replays (and every later eager env call) run on the caller's current stream
        env.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        if hasattr(env, "note_replayed_steps"):
            env.note_replayed_steps(-T)    # the capture pass went through the counting entry point without running
        self._rb = b

    def _collect_graph(self):
        if self._rollout_graph is None:
            self._build_rollout_graph()
        if self.rollout_chains == 1:
            self._rollout_graph.replay()
        else:
            # fork - the second chain on its own stream, launched first (rb_rollout_dev's order) - replay, join, tail
            ga, gb, tail = self._rollout_graph
            cur = torch.cuda.current_stream(self.device)
            self._chain_stream.wait_stream(cur)
            with torch.cuda.stream(self._chain_stream):
                gb.replay()
            ga.replay()
            cur.wait_stream(self._chain_stream)
            tail.replay()
        b, T = self._rb, self.n_steps
        if hasattr(self.env, "note_replayed_steps"):
            self.env.note_replayed_steps(T)
        self._obs = b["carry"]
        if self.asymmetric_critic:
            self._cobs = b["ccarry"]
        self.num_timesteps += T * b["carry"].shape[0]
        if self.reward_norm is not None:
            # behind the replay and outside the graph: the all-reduce and the merge of the rollout's return moments
            self._rew_raw = b["rew_raw"]
            self.reward_norm.update(self.dist)
        roll = {"obs": b["obs"][:T], "act": b["act"], "logp": b["logp"], "val": b["val"], "rew": b["rew"],
                "done": b["done"], "adv": b["adv"], "ret": b["ret"]}
        if self.bootstrap_timeouts:
            roll["trunc"] = b["trunc"]
        if self.asymmetric_critic:
            roll["cobs"] = b["cobs"][:T]
        return roll

    def collect(self):
        ask_obs = self.obs_norm is not None and self._obs_norm_prime
        ask_rew = self.reward_norm is not None and self._reward_norm_prime
        if ask_obs or ask_rew:
            self._obs_norm_prime = self._reward_norm_prime = False     # (asked once: the counts are read back from the device)
            prime_obs = ask_obs and self.obs_norm.count == 0
            if prime_obs or (ask_rew and self.reward_norm.count == 0):
                # priming: one rollout under the identity, for its moments alone (one rollout serves both sets of statistics; the
                # returns' moments are merged where every rollout's are, at the end of _collect_rollout)
                before = self.num_timesteps
                roll = self._collect_rollout()
                self.num_timesteps = before
                if prime_obs and self.symmetry is not None:      # every merge is over the rows and their images: this one too
                    self._update_obs_norms(self._with_images(roll["obs"].reshape(-1, roll["obs"].shape[-1])),
                                           roll["cobs"].reshape(-1, roll["cobs"].shape[-1]) if self.asymmetric_critic else None)
                elif prime_obs:
                    self._update_obs_norms(roll["obs"].reshape(-1, roll["obs"].shape[-1]),
                                           roll["cobs"].reshape(-1, roll["cobs"].shape[-1]) if self.asymmetric_critic else None)
        return self._collect_rollout()

    def _collect_rollout(self):
        """One rollout: the captured graph's replay, or - eager, on any device, torch or fused policy step - T (policy step,
        ``env.step``) pairs and the tail the captured rollout runs too (``_rollout_tail``)."""
        if self.use_graphs:
            return self._collect_graph()
        env, T = self.env, self.n_steps
        asym = self.asymmetric_critic
        if self._obs is None:
            self._obs = self._to_tensor(env.reset())
            if asym:
                self._cobs = self._critic_rows()
            if self.reward_norm is not None:
                self.reward_norm.reset_returns(self._obs.shape[0])
        N = self._obs.shape[0]
        if self._boot_tail is not None and self._boot_tail.n_envs != N:
            self._boot_tail.reset_returns(N)
        boot = self.bootstrap_timeouts
        # fresh tensors on every call, filled step by step: a caller may keep an eager rollout beyond the next one
        z = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=self.device)
        roll = {"obs": z(T, N, self._obs.shape[1]), "act": z(T, N, env.action_space.shape[0])}
        roll.update({k: z(T, N) for k in ("logp", "val", "rew", "done", "adv", "ret") + (("trunc",) if boot else ())})
        if asym:
            roll["cobs"] = z(T, N, self.cobs_dim)
        rew_raw, codes = z(T, N), z(T, N, dtype=torch.int32)
        packed = self._fused.pack() if self._fused is not None else None
        for t in range(T):
            roll["obs"][t].copy_(self._obs)
            if asym:
                roll["cobs"][t].copy_(self._cobs)
            self._policy_step(roll["obs"][t], roll["cobs"][t] if asym else None, roll["act"][t], roll["logp"][t], roll["val"][t], t, packed)
            clipped = roll["act"][t].clamp(-1.0, 1.0).contiguous()      # the env's action box (roboy_env.py:31)
            obs, rew, done, _ = env.step(clipped if self.device.type == "cuda" else clipped.cpu().numpy())
            rew_raw[t].copy_(torch.as_tensor(rew))           # (copy_ converts dtype and device in its one launch)
            codes[t].copy_(torch.as_tensor(done))
            if boot:                                         # the codes: 0, 1 terminated, 2 truncated
                codes[t] += torch.as_tensor(env.truncated()).to(self.device)
            self._obs = self._to_tensor(obs)
            if asym:
                self._cobs = self._critic_rows()
        self._rollout_tail(dict(roll, rew_raw=rew_raw, done_i=codes), self._cobs if asym else self._obs, eager=True)
        if self.reward_norm is not None:
            self._rew_raw = rew_raw
            self.reward_norm.update(self.dist)
        self.num_timesteps += T * N
        return roll

    def _minibatch_loss(self, flat, idx):
        obs, act = flat["obs"][idx], flat["act"][idx]
        adv = flat["adv"][idx]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        d = self.policy.dist(obs)
        logp = d.log_prob(act).sum(-1)
        ratio = (logp - flat["logp"][idx]).exp()
        pg = torch.max(-adv * ratio, -adv * ratio.clamp(1 - self.cliprange, 1 + self.cliprange)).mean()
        v = self.policy.value(flat["cobs"][idx] if self.asymmetric_critic else obs)
        v_clip = flat["val"][idx] + (v - flat["val"][idx]).clamp(-self.cliprange, self.cliprange)
        vf = 0.5 * torch.max((v - flat["ret"][idx]) ** 2, (v_clip - flat["ret"][idx]) ** 2).mean()
        ent = d.entropy().sum(-1).mean()
        kl = cf = None
        if self.diagnostics:
            with torch.no_grad():
                x = logp - flat["logp"][idx]
                kl = (0.5 * x * x).mean()
                cf = ((ratio < 1 - self.cliprange) | (ratio > 1 + self.cliprange)).to(x.dtype).mean()
        loss = pg - self.ent_coef * ent + self.vf_coef * vf
        sym = None
        if self.symmetry == "loss":
            # the statement rp_sym_grad_dev is tested against: symmetry_coef * symmetry_gap's "action" on these rows, both branches live
            e = self.policy.dist(flat["obs_image"][idx]).mean - d.mean[:, self._mirror.src["act"]]
            sym = self.symmetry_coef * (e ** 2).mean()
            loss = loss + sym
        return loss, pg, vf, ent, kl, cf, sym

    def _minibatch_step_fused(self, flat, idx):
        """Four launches + two small reductions per minibatch: advantage statistics, the two gradient kernels (which
        gather the rollout's rows through idx and normalise the advantage per sample), clip + Adam."""
        stats = self._fgrad.minibatch_adv_stats(flat["adv"], idx)
        pg, vf = self._fgrad.run(flat["obs"], flat["act"], flat["adv"], flat["logp"], flat["val"], flat["ret"], self.cliprange,
                                 self.vf_coef, self.ent_coef, index=idx, adv_stats=stats, entropy_grad=False, norm=self.obs_norm,
                                 diagnostics=self.diagnostics, cobs=flat["cobs"] if self.asymmetric_critic else None,
                                 cnorm=self.cobs_norm)
        sym = None
        if self.symmetry == "loss":
            # one more gradient kernel on the same rows, added into the vector the optimiser (and the all-reduce in front of it) reads
            sym = self._fgrad.sym_run(flat["obs"], flat["obs_image"], self._act_src_host, self.symmetry_coef, index=idx, norm=self.obs_norm,
                                     accumulate=True, repack=False)
        scale = self._fadam.step(self.ent_coef, self.dist)          # all-reduces the gradient vector first when ranks > 1
        ent = (0.5 + 0.5 * math.log(2 * math.pi) + self.policy.log_std.detach()).sum()
        pg, vf = pg * scale, vf * scale                              # (the loss slots were summed over the ranks with the rest)
        kl = cf = None
        if self.diagnostics:
            kl, cf = (t * scale for t in self._fgrad.diag())         # (... and so were the diagnostics' slots)
            if self.lr_history is not None and self.lr_schedule is not None:
                self.lr_history.append((kl, self._fadam.lr_dev[0].clone()))
        loss = pg - self.ent_coef * ent + self.vf_coef * vf
        if sym is not None:
            sym = sym * scale                                        # (L_sym's slot too)
            loss = loss + sym
        return loss, pg, vf, ent, kl, cf, sym

    def _minibatch_step(self, flat, idx):
        if self._fgrad is not None:
            return self._minibatch_step_fused(flat, idx)
        loss, pg, vf, ent, kl, cf, sym = self._minibatch_loss(flat, idx)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        average_gradients(self.policy, self.dist)
        nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
        dist = self.dist
        if dist_ranks(dist) > 1:
            # what update() reports is the mean over the ranks, as the fused path's slots are (one small all-reduce); the KL with it
            terms = torch.stack([pg.detach(), vf.detach()] + ([kl, cf] if self.diagnostics else []) + ([sym.detach()] if sym is not None else []))
            dist.all_reduce(terms)
            terms = terms / dist.get_world_size()
            pg, vf = terms[0], terms[1]
            if self.diagnostics:
                kl, cf = terms[2], terms[3]
            loss = pg - self.ent_coef * ent.detach() + self.vf_coef * vf
            if sym is not None:
                sym = terms[-1]
                loss = loss + sym
        if self.lr_schedule is not None:
            # the rule, in front of the step of the same minibatch; with ranks on their mean KL: the same decision everywhere
            self._lr32 = adapt_lr(self._lr32, kl.item(), self.desired_kl, self.lr_factor, self.lr_min, self.lr_max)
            self.opt.param_groups[0]["lr"] = float(self._lr32)
            if self.lr_history is not None:
                self.lr_history.append((float(kl.item()), float(self._lr32)))
        self.opt.step()
        return loss, pg, vf, ent, kl, cf, sym

    def _sample_order(self, n):
        """The epoch's sample order.  Torch path: torch.randperm (a sort of n random keys).  Fused path: a keyed bijection
        of [0, n) evaluated per element on the device (rp_perm_dev), key = (seed, epochs so far)."""
        self._epoch += 1
        if self._fgrad is None:
            return torch.randperm(n, device=self.device)
        import ctypes as c
        if getattr(self, "_perm_buf", None) is None or self._perm_buf.numel() != n:
            self._perm_buf = torch.empty(n, dtype=torch.int64, device=self.device)
        key = ((self._seed & 0xFFFFFFFF) << 32) | (self._epoch & 0xFFFFFFFF)
        f = self._fgrad
        f._pn.check(f._lib.rp_perm_dev(key, n, 0, n, c.c_void_p(self._perm_buf.data_ptr()),
                                       c.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return self._perm_buf

    AUGMENTED_KEYS = (("obs", "obs"), ("act", "act"), ("adv", "one"), ("logp", "one"), ("val", "one"), ("ret", "one"))

    @torch.no_grad()
    def augment(self, roll):
        """The rollout and its mirror image as the update's sample set (``symmetry="augment"``): with n = T N,
        ``{"obs", "act", "adv", "logp", "val", "ret"}`` as [2 n, ...] tensors - rows [0, n) the rollout's, rows [n, 2 n) ``obs = M obs``,
        ``act = P act`` (the raw samples, as stored) and ``adv, logp, val, ret`` copied.  The old log-probability is the original's on
        purpose: the mirrored sample was generated by the mirrored behaviour policy, whose density at (M s, P a) is pi_old(a | s) - the
        permutation's Jacobian is 1.  On a GPU the halves are written by rp_mirror_rows_dev into buffers kept between updates (the
        next ``augment`` overwrites them); on the CPU by the torch statement, the same numbers bit for bit."""
        mm = self._mirror
        if mm is None:
            raise RuntimeError("this agent was built without symmetry")
        flat = {k: roll[k].reshape(-1, *roll[k].shape[2:]) for k, _ in self.AUGMENTED_KEYS}
        if not mm.kernel_applies():
            return {k: torch.cat([flat[k], flat[k] if kind == "one" else mm.rows(flat[k], kind)]).contiguous()
                    for k, kind in self.AUGMENTED_KEYS}
        n = int(flat["obs"].shape[0])
        bufs = getattr(self, "_aug_bufs", None)
        if bufs is None or bufs["obs"].shape[0] != 2 * n:
            bufs = self._aug_bufs = {k: torch.empty((2 * n,) + tuple(flat[k].shape[1:]), dtype=torch.float32, device=self.device)
                                     for k, _ in self.AUGMENTED_KEYS}
        for k, kind in self.AUGMENTED_KEYS:
            mm.rows_into(flat[k].to(torch.float32).contiguous(), bufs[k], kind)
        return dict(bufs)

    @torch.no_grad()
    def _obs_images(self, obs_rows):
        """the image rows M obs of [n, obs_dim] rows (``symmetry="loss"``): on a GPU one launch of rp_mirror_rows_dev into a buffer
        kept between updates (the next update overwrites it), on the CPU the torch statement - the same numbers bit for bit"""
        mm = self._mirror
        if not mm.kernel_applies():
            return mm.rows(obs_rows, "obs").contiguous()
        src = obs_rows.to(torch.float32).contiguous()
        buf = getattr(self, "_image_buf", None)
        if buf is None or tuple(buf.shape) != tuple(src.shape):
            buf = self._image_buf = torch.empty_like(src)
        mm.rows_into(src, buf, "obs", plain=False)
        return buf

    @torch.no_grad()
    def _with_images(self, obs_rows):
        """observation rows [rows, obs_dim] followed by their mirror images (the priming rollout's moments, as ``augment``'s are)"""
        return torch.cat([obs_rows, self._mirror.rows(obs_rows, "obs")])

    @torch.no_grad()
    def _means_values(self, obs):
        """(action mean [rows, act_dim], value [rows]) of observation rows by the agent's own policy step: the fused one
        (deterministic, with its ``mean`` output) where the agent is fused, torch otherwise"""
        if self._fused is None:
            return self.policy.dist(obs).mean, self.policy.value(obs)
        rows = int(obs.shape[0])
        z = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        act, mean, logp, val = z(rows, self._fused.act_dim), z(rows, self._fused.act_dim), z(rows), z(rows)
        self._fused.act_into(obs.contiguous(), act, logp, val, deterministic=True, mean=mean, norm=self.obs_norm)
        return mean, val

    @torch.no_grad()
    def symmetry_gap(self, roll, max_rows=65536):
        """How far the policy is from the robot's mirror symmetry on the first ``max_rows`` observation rows s of a rollout:
        ``{"action": mean |mu(M s) - P mu(s)|^2 / act_dim, "value": mean |V(M s) - V(s)|}`` (0, 0 for an equivariant actor and an
        invariant critic).  Needs ``symmetry``, either mode, which is where the maps come from.  With an asymmetric critic, whose rows
        have no mirror map, the value gap is not defined: NaN."""
        mm = self._mirror
        if mm is None:
            raise RuntimeError("this agent was built without symmetry")
        obs = roll["obs"].reshape(-1, roll["obs"].shape[-1])[:int(max_rows)].to(self.device, torch.float32).contiguous()
        if self.asymmetric_critic:
            d = self.policy.dist(mm.rows(obs, "obs")).mean - mm.rows(self.policy.dist(obs).mean, "act")
            return {"action": ((d * d).sum(-1).mean() / d.shape[-1]).item(), "value": float("nan")}
        mu, v = self._means_values(obs)
        mu_m, v_m = self._means_values(mm.rows(obs, "obs").contiguous())
        d = mu_m - mm.rows(mu, "act")
        return {"action": ((d * d).sum(-1).mean() / d.shape[-1]).item(), "value": (v_m - v).abs().mean().item()}

    def update(self, roll, sample_orders=None):
        """sample_orders (optional): one int64 index tensor per epoch instead of the generated order (tests feed the
        same orders to both optimiser paths)."""
        if self.symmetry == "augment":
            # everything below is the update it always was, on 2 n samples: the rollout's and their mirror images
            flat = self.augment(roll)
        else:
            flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in roll.items()}
            if self._fgrad is not None:          # the gradient kernels index the rollout tensors directly
                flat = {k: v.contiguous() for k, v in flat.items()}
            if self.symmetry == "loss":          # the image rows M obs of all n rows, once per update
                flat["obs_image"] = self._obs_images(flat["obs"])
        n = flat["obs"].shape[0]
        mb = max(n // self.nminibatches, 1)
        out = None
        for ep in range(self.noptepochs):
            perm = self._sample_order(n) if sample_orders is None else sample_orders[ep].contiguous()
            for s in range(0, n - mb + 1, mb):
                out = self._minibatch_step(flat, perm[s:s + mb])
        if self.obs_norm is not None:
            # the statistics move only now: rollout and update saw the same ones (old and new log-probabilities of the same inputs)
            # (symmetry="loss": over the rows and their images, as "augment"'s 2 n rows are - a policy cannot be equivariant under
            # statistics that are not mirror-consistent)
            self._update_obs_norms(flat["obs"], flat["cobs"] if self.asymmetric_critic else None,
                                   flat["obs_image"] if self.symmetry == "loss" else None)
        if out is None:
            return {}
        loss, pg, vf, ent, kl, cf, sym = out
        stats = {"loss": loss.item(), "pg_loss": pg.item(), "vf_loss": vf.item(), "entropy": ent.item()}
        if sym is not None:
            stats["symmetry_loss"] = sym.item()
        if self.diagnostics:
            stats["approx_kl"], stats["clip_frac"] = kl.item(), cf.item()
        if self.lr_schedule is not None:
            stats["lr"] = self.learning_rate
        return stats

    def evaluate(self, env, episodes_per_env=1, poll_every=32):
        """The agent's deterministic policy on ``env`` - a ``RoboyVecEnv`` of its own with ``episode_log >= episodes_per_env``, under
        whatever conditions it was built with - for exactly ``episodes_per_env`` episodes of every env (``evaluate_policy``): the
        summary of ``env.episode_log_summary`` plus ``"steps"``.  The fused policy step where the agent has one, with the frozen
        ``obs_norm``.  ``ValueError`` for the training env itself (evaluation never touches it, its carried observation, a captured
        rollout or the noise counters), for another observation width and for a log capacity that is too small.
        ``num_timesteps``, the step base and every optimiser and normaliser state are as before the call.  DESIGN.md §29."""
        if env is self.env:
            raise ValueError("evaluate() takes an env of its own: the training env carries the rollout's observation and episodes "
                             "(build a second RoboyVecEnv with episode_log=%d)" % int(episodes_per_env))
        return evaluate_policy(self.policy, env, episodes_per_env, poll_every, fused=self._fused, obs_norm=self.obs_norm,
                               cobs_norm=self.cobs_norm, device=self.device)

    def learn(self, total_timesteps, log=None):
        target = self.num_timesteps + total_timesteps
        while self.num_timesteps < target:
            roll = self.collect()
            if self.symmetry is not None:        # kept for symmetry_gap()
                self.last_rollout = roll
            stats = self.update(roll)
            if self.reward_norm is not None:     # the env's raw reward, not the normalised one the agent learns from
                stats["mean_reward"] = self._rew_raw.mean().item()
            else:
                stats["mean_reward"] = roll["rew"].mean().item() / self.reward_scale
            stats["timesteps"] = self.num_timesteps
            if log:
                log(stats)
        return self

    def resume_record(self):
        """What ``collect()`` and ``update()`` carry from one call to the next beyond the checkpoint's own keys, and the env's state
        (``save(path, resume=True)``'s ``"resume"`` key; a multi-rank trainer writes one per rank): with it a loaded agent continues the
        run - on the fused paths bit for bit.  Only tensors, numbers and strings: ``torch.load`` takes it as it is."""
        cpu = lambda t: None if t is None else t.detach().to("cpu", copy=True)
        norm = lambda n: None if n is None else {"state": cpu(n.state), "norm": cpu(n.norm)}
        rec = {"env": pack_arrays(self.env.state_dict()), "obs": cpu(self._obs), "cobs": cpu(self._cobs), "epoch": self._epoch,
               "step_base": int(self._step_base.item()) if self._fused is not None else None,
               "obs_norm_prime": self._obs_norm_prime, "reward_norm_prime": self._reward_norm_prime,
               "obs_norm": norm(self.obs_norm), "critic_obs_norm": norm(self.cobs_norm), "reward_norm": norm(self.reward_norm),
               "ret_carry": cpu(self.reward_norm.ret_carry) if self.reward_norm is not None else None,
               "boot_ret_carry": cpu(self._boot_tail.ret_carry) if self._boot_tail is not None else None}
        if self._fused is None or self._fgrad is None:       # the torch paths draw from torch's generators (no bit-for-bit claim)
            rec["torch_rng"] = torch.get_rng_state()
            rec["torch_cuda_rng"] = torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None
        return rec

    def load_resume_record(self, rec):
        """Continue from ``resume_record()``'s dict, behind a ``load()`` of the checkpoint written with it: the env's state first
        (``ValueError`` for a record of another env, and nothing has changed then), then the agent's carries."""
        self._load_resume_env(rec)
        self._load_resume_agent(rec)

    def _load_resume_env(self, rec):
        if not callable(getattr(self.env, "load_state_dict", None)):
            raise ValueError("a resume record needs an env with state_dict() / load_state_dict() (RoboyVecEnv)")
        self.env.load_state_dict(unpack_arrays(rec["env"]))      # (compares identity and segment table first)

    def _load_resume_agent(self, rec):
        """the agent's side of a resume record (the env's has been loaded): tensors that a captured rollout reads by address are
        written in place where they exist"""
        def put(name, value):
            cur = getattr(self, name)
            if value is None:
                setattr(self, name, None)
            elif torch.is_tensor(cur) and tuple(cur.shape) == tuple(value.shape):
                cur.copy_(value)                             # (graph mode: _obs IS the rollout's carry buffer)
            else:
                setattr(self, name, value.to(self.device))
        put("_obs", rec["obs"]); put("_cobs", rec["cobs"])
        self._epoch = int(rec["epoch"])
        if self._fused is not None and rec["step_base"] is not None:
            self._step_base.fill_(int(rec["step_base"]))     # the exact value: a priming rollout counts, num_timesteps does not know it
        self._obs_norm_prime, self._reward_norm_prime = bool(rec["obs_norm_prime"]), bool(rec["reward_norm_prime"])
        for n, saved in ((self.obs_norm, rec["obs_norm"]), (self.cobs_norm, rec["critic_obs_norm"]), (self.reward_norm, rec["reward_norm"])):
            if n is not None and saved is not None:          # the float64 state and the float32 form as the device's merge left them
                n.state.copy_(saved["state"]); n.norm.copy_(saved["norm"])
        for rn, carry in ((self.reward_norm, rec["ret_carry"]), (self._boot_tail, rec["boot_ret_carry"])):
            if rn is not None and carry is not None:
                if rn.n_envs != int(carry.numel()):
                    rn.reset_returns(int(carry.numel()))
                rn.ret_carry.copy_(carry)
        if rec.get("torch_rng") is not None and (self._fused is None or self._fgrad is None):
            torch.set_rng_state(rec["torch_rng"].cpu())
            if rec.get("torch_cuda_rng") is not None and self.device.type == "cuda":
                torch.cuda.set_rng_state(rec["torch_cuda_rng"].cpu(), self.device)

    def save(self, path, resume=False):
        """``resume=True`` adds ONE key, ``"resume"``: the env's state (``RoboyVecEnv.state_dict``), the carried observation and
        critic rows, the exact noise step base, the epoch count, the priming flags, the statistics as the device holds them and the
        running returns - ``load`` then continues the run where it stopped instead of restarting the envs (on the fused paths the
        continued run is the uninterrupted one bit for bit; the torch paths also restore torch's generators and claim nothing).
        Without it the checkpoint is the one it always was."""
        opt = self._fadam.state_dict() if self._fgrad is not None else self.opt.state_dict()
        ck = {"policy": self.policy.state_dict(), "optimizer": opt, "num_timesteps": self.num_timesteps,
              "epoch": self._epoch, **env_checkpoint_record(self.env, critic=self.asymmetric_critic),
              "obs_norm": self.obs_norm.state_dict() if self.obs_norm is not None else None,
              "reward_norm": self.reward_norm.state_dict() if self.reward_norm is not None else None,
              "bootstrap_timeouts": self.bootstrap_timeouts}
        if self.asymmetric_critic:                   # (an agent without the option writes the checkpoint it always wrote)
            ck["critic_obs_dim"] = self.cobs_dim
            ck["critic_obs_norm"] = self.cobs_norm.state_dict() if self.cobs_norm is not None else None
        if self.symmetry is not None:                # (an agent without the option writes the checkpoint it always wrote)
            ck["symmetry"] = self.symmetry
            if self.symmetry == "loss":
                ck["symmetry_coef"] = self.symmetry_coef
        if self.lr_schedule is not None:             # (an agent without a schedule writes the checkpoint it always wrote)
            ck["lr_schedule"] = {"kind": self.lr_schedule, "desired_kl": self.desired_kl, "lr_factor": self.lr_factor,
                                 "lr_min": self.lr_min, "lr_max": self.lr_max, "lr": self.learning_rate}
        if resume:
            if not callable(getattr(self.env, "state_dict", None)):
                raise ValueError("save(resume=True) needs an env with state_dict() / load_state_dict() (RoboyVecEnv)")
            ck["resume"] = self.resume_record()
        torch.save(ck, path)

    def _check_layout_options(self, ck):
        if ("critic_obs" in ck) != self.asymmetric_critic:
            raise ValueError("the checkpoint was trained %s an asymmetric critic, this agent runs %s one (PPO's asymmetric_critic)"
                             % (("with", "without") if not self.asymmetric_critic else ("without", "with")))
        if ck.get("symmetry") != self.symmetry:
            raise ValueError("the checkpoint was trained with symmetry=%r, this agent runs symmetry=%r (PPO's symmetry)"
                             % (ck.get("symmetry"), self.symmetry))

    def _check_norm_options(self, ck):
        if (ck.get("obs_norm") is not None) != (self.obs_norm is not None):      # (a checkpoint without the key: written without it)
            raise ValueError("the checkpoint was trained %s observation normalisation, this agent runs %s it (PPO's normalize_obs)"
                             % (("with", "without") if self.obs_norm is None else ("without", "with")))
        if (ck.get("reward_norm") is not None) != (self.reward_norm is not None):
            raise ValueError("the checkpoint was trained %s reward normalisation, this agent runs %s it (PPO's normalize_reward)"
                             % (("with", "without") if self.reward_norm is None else ("without", "with")))

    def load(self, path, resume=None):
        """``resume``: None - continue from the checkpoint's ``"resume"`` record where it has one (``save(path, resume=True)``);
        False - ignore the record: the envs start over as they always did; True - insist (``ValueError`` without a record).  A
        record whose env is not this agent's env - another batch size, seed or option - raises ``RoboyVecEnv.load_state_dict``'s
        ``ValueError`` before anything of the agent or the env has changed, and so do the agent options ``load`` has always refused
        (asymmetric critic, symmetry, the normalisations): with a record they are looked at before the env is written."""
        ck = torch.load(path, map_location="cpu")            # (the record's env blob stays on the host: the env takes numpy)
        record = ck.pop("resume", None)
        ck = _tensors_to(ck, self.device)                   # ... everything else where it always was
        if not (resume is None or resume):
            record = None
        if resume and record is None:
            raise ValueError("load(resume=True): the checkpoint has no resume record (save(path, resume=True))")
        if record is not None:
            self._check_layout_options(ck)
            self._check_norm_options(ck)
            self._load_resume_env(record)
        self._check_layout_options(ck)
        if self.symmetry == "loss" and float(ck.get("symmetry_coef", self.symmetry_coef)) != self.symmetry_coef:
            # the coefficient is a weight, not a layout: the constructor's holds (a run may be resumed under another one), and says so
            import warnings
            warnings.warn("the checkpoint was trained with symmetry_coef=%r, this agent goes on with symmetry_coef=%r"
                          % (float(ck["symmetry_coef"]), self.symmetry_coef))
        # the env's side; what the env does not take over is kept as checkpoint_goals, _goal_row_stats, _goal_curriculum and _env_push
        for key, value in check_env_checkpoint(self.env, ck, self.cobs_dim).items():
            setattr(self, "checkpoint_" + key, value)
        self._check_norm_options(ck)
        if self.obs_norm is not None:
            self.obs_norm.load_state_dict(ck["obs_norm"])
            self._obs_norm_prime = self._obs_norm_prime and float(ck["obs_norm"]["count"]) == 0.0
            if self.cobs_norm is not None:
                self.cobs_norm.load_state_dict(ck["critic_obs_norm"])
        if self.reward_norm is not None:
            self.reward_norm.load_state_dict(ck["reward_norm"])
            self.reward_norm.reset_returns()                 # the running returns are not stored: they start afresh
            self._reward_norm_prime = self._reward_norm_prime and float(ck["reward_norm"]["count"]) == 0.0
        self.policy.load_state_dict(ck["policy"])      # copies in place: the views of the fused optimiser's flat buffer stay valid
        fused_ck = isinstance(ck["optimizer"], dict) and ck["optimizer"].get("fused_adam", False)
        if self._fgrad is not None and fused_ck:
            self._fadam.load_state_dict(ck["optimizer"])
        elif self._fgrad is None and not fused_ck:
            self.opt.load_state_dict(ck["optimizer"])
        elif self._fgrad is not None:
            # a checkpoint of the torch path (fused_update=False, or written before the fused update was the default): its
            # moments and step count move into the flat vectors
            t = adam_state_torch_to_flat(ck["optimizer"], self.policy, self._fgrad._layout, self._fadam.m, self._fadam.v)
            if t is None:
                import warnings
                warnings.warn("the checkpoint's optimiser had not stepped yet: Adam's moments start afresh")
            else:
                self._fadam.t = t
        else:
            # a checkpoint of the fused path resumed on the torch path: torch's per-parameter state from the flat moments
            from . import _policy_native as pn
            layout, n = pn.grad_layout(self.policy.pi[0].in_features, self.policy.pi[-1].out_features, self.cobs_dim)
            if int(ck["optimizer"]["m"].numel()) != int(n):
                raise ValueError("optimiser state of another policy layout: %d values, this policy's flat vector has %d"
                                 % (ck["optimizer"]["m"].numel(), n))
            self.opt.load_state_dict(adam_state_flat_to_torch(ck["optimizer"], self.policy, layout, self.opt.state_dict()))
        # torch's optimiser state brings its learning rate along: a schedule continues from the checkpoint's scheduled rate where
        # both sides have one; otherwise the agent keeps its own (also against a rate some schedule had moved)
        sched = ck.get("lr_schedule")
        if self.lr_schedule is not None:
            self._set_lr(sched["lr"] if sched is not None else self._lr32)
        elif sched is not None:
            self.opt.param_groups[0]["lr"] = self._lr0
        self.num_timesteps = ck["num_timesteps"]
        self._epoch = int(ck.get("epoch", 0))
        if self._fused is not None:
            # the exploration noise is keyed (seed; sample, step): continue the step count where the run stopped, so that a
            # resumed run does not replay the noise of its first rollouts
            n_envs = getattr(self.env, "num_envs", 1)
            self._step_base.fill_(int(self.num_timesteps // max(n_envs, 1)) & 0x7FFFFFFF)
        if record is not None:
            self._load_resume_agent(record)
        return self
