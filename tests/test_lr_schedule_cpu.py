"""Update diagnostics and the KL-adaptive learning rate without a GPU: the rule restated in numpy float32
(tests/ppo_diag_ref.py - what the GPU test compares rp_clip_adam_kl_dev's bits with), PPO(lr_schedule="adaptive") on the torch path over
a stand-in env, the option switched off, checkpoints, the ABI and what the shipped code objects say about the new kernels.

The bound on approx_kl / clip_frac against float64 is the one tests/test_policy_gpu.py holds fp32 loss terms to: 1e-4 max(1, |ref|)."""
import copy
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import ppo_diag_ref as dref
from gym_roboy_amd import _policy_native as pn
from gym_roboy_amd._gymcompat import spaces
from gym_roboy_amd.ppo import PPO, adapt_lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY_HEADER = open(os.path.join(ROOT, "include", "roboy_policy.h")).read()
F32 = np.float32
D, F, LO, HI = 0.01, 1.5, 1e-5, 1e-2


# ---- 1. the rule ----
def _next(x, up):
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


def test_the_rule_in_float32_at_its_thresholds_and_bounds():
    lr = F32(2.5e-4)
    two_d, half_d = F32(2.0) * F32(D), F32(0.5) * F32(D)
    cut, rise = lr / F32(F), lr * F32(F)
    assert cut.dtype == np.float32 and cut < lr < rise
    cases = [(two_d, lr), (_next(two_d, True), cut), (_next(two_d, False), lr),          # strictly above 2 d cuts
             (half_d, lr), (_next(half_d, False), rise), (_next(half_d, True), lr),      # strictly below d / 2 raises
             (F32(0.0), lr), (F32(np.nan), lr), (F32(1.0), cut), (_next(0.0, True), rise), (F32(-1.0), lr), (F32(np.inf), cut)]
    for kl, want in cases:
        for fn in (dref.adapt_lr, adapt_lr):                     # the reference and the statement PPO's torch path applies
            got = fn(lr, kl, D, F, LO, HI)
            assert isinstance(got, np.float32) and got.tobytes() == F32(want).tobytes(), (fn.__module__, kl, got, want)
    # both bounds: at lr_max a low KL changes nothing, just under it the product is clamped; the same at lr_min
    for fn in (dref.adapt_lr, adapt_lr):
        assert fn(HI, 1e-4, D, F, LO, HI) == F32(HI) and fn(LO, 1.0, D, F, LO, HI) == F32(LO)
        assert fn(0.9 * HI, 1e-4, D, F, LO, HI) == F32(HI) and fn(1.1 * LO, 1.0, D, F, LO, HI) == F32(LO)
        assert fn(HI, 1.0, D, F, LO, HI) == F32(HI) / F32(F) and fn(LO, 1e-4, D, F, LO, HI) == F32(LO) * F32(F)
    # one rounding: the float32 quotient, not the float64 one rounded
    odd = F32(3.3333334e-4)
    assert dref.adapt_lr(odd, 1.0, D, 1.7, LO, HI).tobytes() == (odd / F32(1.7)).tobytes()
    assert dref.kl_of_slot(0.03, 0.5).tobytes() == (F32(0.03) * F32(0.5)).tobytes()


# ---- a stand-in env: the reward likes actions near a linear function of the observation ----
class ToyVecEnv:
    def __init__(self, n, seed=0):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.observation_space = spaces.Box(low=-10, high=10, shape=(5,), dtype="float32")
        self.action_space = spaces.Box(low=-1, high=1, shape=(3,), dtype="float32")
        self.W = self.rng.standard_normal((5, 3)).astype(np.float32) * 0.5

    def reset(self):
        self.obs = self.rng.standard_normal((self.n, 5)).astype(np.float32)
        return self.obs

    def step(self, a):
        rew = -np.square(np.asarray(a) - np.tanh(self.obs @ self.W)).sum(1).astype(np.float32)
        done = self.rng.random(self.n) < 0.05
        return self.reset(), rew, done, [{}] * self.n


def _agent(seed=1, n=64, **kw):
    return PPO(ToyVecEnv(n, seed), n_steps=16, device="cpu", seed=seed, nminibatches=2, noptepochs=3, **kw)


# ---- 2. the torch path under the schedule ----
def test_torch_path_follows_the_rule_and_reports_the_last_minibatch():
    kw = dict(lr_schedule="adaptive", desired_kl=2e-3, lr_factor=F, lr_min=LO, lr_max=HI, learning_rate=1e-3)
    agent = _agent(**kw)
    assert agent.diagnostics and agent.learning_rate == float(F32(1e-3))
    agent.lr_history = []
    seen = []                                                  # (policy before the minibatch's step, its index) of every minibatch
    step = agent._minibatch_step
    agent._minibatch_step = lambda flat, idx: (seen.append((copy.deepcopy(agent.policy).double(), idx.clone(), flat)), step(flat, idx))[1]
    lr = F32(1e-3)
    lrs = [lr]
    for _ in range(2):
        roll = agent.collect()
        first = len(agent.lr_history)
        stats = agent.update(roll)
        assert set(stats) == {"loss", "pg_loss", "vf_loss", "entropy", "approx_kl", "clip_frac", "lr"}
        for kl, got in agent.lr_history[first:]:
            lr = dref.adapt_lr(lr, kl, 2e-3, F, LO, HI)
            assert F32(got).tobytes() == lr.tobytes(), (kl, got, lr)
            assert F32(LO) <= lr <= F32(HI)
            lrs.append(lr)
        assert stats["lr"] == float(lr) == agent.learning_rate == agent.opt.param_groups[0]["lr"]
        assert stats["approx_kl"] == agent.lr_history[-1][0]
        # the diagnostics against float64 on the same minibatch, with the policy as it was before that minibatch's step
        policy64, idx, flat = seen[-1]
        ref = dref.diag64(policy64, flat["obs"][idx], flat["act"][idx], flat["logp"][idx], agent.cliprange)
        print("approx_kl %.6g (float64 %.6g)  clip_frac %.6g (float64 %.6g)  borderline %d  lr %.4g"
              % (stats["approx_kl"], ref["approx_kl"], stats["clip_frac"], ref["clip_frac"], ref["borderline"], lr))
        assert ref["borderline"] == 0 and ref["approx_kl"] > 1e-6      # the input qualifies: no sample the two precisions may count apart
        assert abs(stats["approx_kl"] - ref["approx_kl"]) <= 1e-4 * max(1.0, abs(ref["approx_kl"]))
        assert abs(stats["clip_frac"] - ref["clip_frac"]) <= 1e-4 * max(1.0, abs(ref["clip_frac"]))
    assert len(agent.lr_history) == 2 * 3 * 2 and len(set(float(x) for x in lrs)) > 1      # the rate moved
    kls = [kl for kl, _ in agent.lr_history]
    print("kl", ["%.3g" % k for k in kls], "lr", ["%.3g" % x for x in lrs])
    assert any(k > 2 * 2e-3 for k in kls) and any(0 < k < 0.5 * 2e-3 for k in kls)          # both branches were taken


def test_diagnostics_without_a_schedule_leave_the_learning_rate_alone():
    agent = _agent(diagnostics=True)
    stats = agent.update(agent.collect())
    assert set(stats) == {"loss", "pg_loss", "vf_loss", "entropy", "approx_kl", "clip_frac"}
    assert agent.learning_rate == 2.5e-4 and 0.0 <= stats["clip_frac"] <= 1.0 and stats["approx_kl"] >= 0.0


# ---- 3. the option switched off ----
def test_without_the_option_nothing_changes(tmp_path):
    a = _agent(seed=3)                                         # (one after the other: they draw from torch's one generator)
    ra = a.collect(); sa = a.update(ra)
    b = _agent(seed=3, diagnostics=False, lr_schedule=None)
    rb = b.collect(); sb = b.update(rb)
    for k in ra:
        assert torch.equal(ra[k], rb[k])
    assert set(sa) == set(sb) == {"loss", "pg_loss", "vf_loss", "entropy"} and sa == sb
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    path = str(tmp_path / "model.pkl")
    a.save(path)
    ck = torch.load(path)
    assert "lr_schedule" not in ck
    assert set(ck) == {"policy", "optimizer", "num_timesteps", "epoch", "tendon_obs", "env_io", "obs_norm", "reward_norm", "bootstrap_timeouts"}
    assert a.learning_rate == 2.5e-4


# ---- 4. checkpoints and constructor errors ----
def test_checkpoint_round_trips_the_learning_rate(tmp_path):
    kw = dict(lr_schedule="adaptive", desired_kl=2e-3, learning_rate=1e-3)
    a = _agent(seed=5, **kw)
    a.update(a.collect())
    assert a.learning_rate != float(F32(1e-3))
    path = str(tmp_path / "model.pkl")
    a.save(path)
    ck = torch.load(path)
    assert ck["lr_schedule"] == {"kind": "adaptive", "desired_kl": 2e-3, "lr_factor": 1.5, "lr_min": 1e-5, "lr_max": 1e-2, "lr": a.learning_rate}
    b = _agent(seed=6, **kw).load(path)
    assert b.learning_rate == a.learning_rate == b.opt.param_groups[0]["lr"] and b._lr32.tobytes() == a._lr32.tobytes()
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    # a checkpoint without a schedule leaves a scheduled agent its own rate; a scheduled checkpoint loads into a plain agent
    plain = _agent(seed=7)
    plain_path = str(tmp_path / "plain.pkl")
    plain.save(plain_path)
    c = _agent(seed=8, **kw).load(plain_path)
    assert c.learning_rate == float(F32(1e-3))
    d = _agent(seed=9).load(path)
    assert d.learning_rate == 2.5e-4 and "lr" not in d.update(d.collect())


def test_constructor_refuses_bad_schedules():
    env = ToyVecEnv(4)
    for kw, match in ((dict(lr_schedule="linear"), "unknown lr_schedule"), (dict(lr_schedule="adaptive", desired_kl=0.0), "desired_kl"),
                      (dict(lr_schedule="adaptive", lr_factor=1.0), "lr_factor"), (dict(lr_schedule="adaptive", lr_min=0.0), "lr_min"),
                      (dict(lr_schedule="adaptive", lr_min=1e-2, lr_max=1e-3), "lr_min"),
                      (dict(lr_schedule="adaptive", learning_rate=0.1), "outside"), (dict(lr_schedule="adaptive", learning_rate=1e-6), "outside")):
        with pytest.raises(ValueError, match=match):
            PPO(env, n_steps=4, device="cpu", **kw)
    PPO(env, n_steps=4, device="cpu", learning_rate=0.1)        # without a schedule the bounds bind nothing


def test_cli_forwards_the_schedule(tmp_path, monkeypatch):
    import gym_roboy_amd.envs.vec_env as vec_env
    import gym_roboy_amd.ppo as ppo
    import gym_roboy_amd.train_parallel as tp
    seen = {}

    class Stop(Exception):
        pass

    def fake_ppo(env, **kw):
        seen["ppo"] = kw
        raise Stop

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(vec_env, "RoboyVecEnv", lambda *a, **kw: object())
    monkeypatch.setattr(ppo, "PPO", fake_ppo)
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path), "--lr-schedule", "adaptive", "--desired-kl", "0.02", "--lr-min", "1e-4", "--lr-max", "1e-3"])
    assert (seen["ppo"]["lr_schedule"], seen["ppo"]["desired_kl"], seen["ppo"]["lr_min"], seen["ppo"]["lr_max"]) == ("adaptive", 0.02, 1e-4, 1e-3)
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path)])
    assert seen["ppo"]["lr_schedule"] is None
    line = tp.log_line({"loss": 1.234567, "approx_kl": 0.000123456, "lr": 1.2345e-5, "clip_frac": 0.123456})
    assert line == {"loss": 1.2346, "approx_kl": 0.000123, "lr": 1.23e-5, "clip_frac": 0.1235}


# ---- 5. symbols and code objects ----
def test_entry_points_are_declared_exported_and_mirrored():
    lib = pn.load()
    for name in ("rp_ppo_grad_diag_dev", "rp_clip_adam_kl_dev"):
        assert re.search(r"\bint %s\(" % name, POLICY_HEADER), name
        assert name in pn.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    assert pn.SIGNATURES["rp_ppo_grad_diag_dev"] == pn.SIGNATURES["rp_ppo_grad_norm_dev"]
    args = {n: re.sub(r"\s+", " ", re.search(r"int %s\((.*?)\);" % n, POLICY_HEADER, re.S).group(1))
            for n in ("rp_ppo_grad_norm_dev", "rp_ppo_grad_diag_dev")}
    assert args["rp_ppo_grad_norm_dev"] == args["rp_ppo_grad_diag_dev"]
    assert lib.rp_abi_version() == pn.RP_ABI_VERSION == 5 and re.search(r"#define RP_ABI_VERSION 5\b", POLICY_HEADER)
    layout, n = pn.grad_layout(9, 8)
    assert layout["approx_kl"] == (layout["pi_loss"][0] + 1, ()) and layout["clip_frac"] == (layout["pi_loss"][0] + 2, ())
    assert layout["clip_frac"][0] < layout["vf_w1"][0]            # inside the action net's block
    # argument errors need no device
    f, null = ctypes.c_void_p(64), None
    ok = dict(desired_kl=0.01, lr_factor=1.5, lr_min=1e-5, lr_max=1e-2)
    def call(ptrs=(f, f, f, f), lr=f, **kw):
        k = dict(ok, **kw)
        return lib.rp_clip_adam_kl_dev(*ptrs, 9, 8, lr, k["desired_kl"], k["lr_factor"], k["lr_min"], k["lr_max"], 0.9, 0.999, 1e-5, 1, 0.5, 1.0, 0.0, None)
    for bad in (dict(desired_kl=0.0), dict(desired_kl=float("nan")), dict(lr_factor=1.0), dict(lr_factor=float("nan")), dict(lr_min=0.0),
                dict(lr_min=1e-2, lr_max=1e-3), dict(lr_max=float("nan")), dict(lr=null), dict(ptrs=(null, f, f, f)), dict(ptrs=(f, f, f, null))):
        assert call(**bad) == -1 and lib.rp_last_error(), bad


def test_diagnostics_instances_use_no_more_scratch_than_their_siblings():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object_meta as com
    meta = {com.short(k): v for k, v in com.kernel_metadata(os.path.join(ROOT, "gym_roboy_amd", "csrc", "libroboy_policy.so")).items()}
    pairs = 0
    for norm in ("", "_norm"):
        for inst in ("<0, 1, 8, true>", "<0, 1, 8, false>", "<0, 2, 64, false>"):
            sib, diag = meta["mlp_grad%s_kernel%s" % (norm, inst)], meta["mlp_grad%s_diag_kernel%s" % (norm, inst)]
            print("mlp_grad%s_kernel%s: scratch %d, with diagnostics %d (vgpr %d / %d, sgpr spills %d / %d)"
                  % (norm, inst, sib["private_segment_fixed_size"], diag["private_segment_fixed_size"], sib["vgpr_count"], diag["vgpr_count"],
                     sib.get("sgpr_spill_count", 0), diag.get("sgpr_spill_count", 0)))
            assert diag["private_segment_fixed_size"] <= sib["private_segment_fixed_size"]
            pairs += 1
    assert pairs == 6 and not any("diag" in k and "<1," in k for k in meta)        # the value net has no diagnostics instance
    assert len([k for k in meta if "clip_adam" in k]) == 2
    for k in ("clip_adam_kernel", "clip_adam_kl_kernel"):
        assert meta[k]["private_segment_fixed_size"] == 0
