"""The rollout's tail by the form ``rollout_tail_form`` names (gym_roboy_amd/ppo.py; DESIGN.md §16's table), on the GPU: for every
fused combination of (eager / captured) x normalize_reward x bootstrap_timeouts x asymmetric_critic, ``adv`` and ``ret`` recomputed on
the rollout's own ``rew``, ``val``, ``done`` (+ ``trunc``) and last value with the function the table names - ``gae`` / ``gae_boot`` on
the device, ``gae_fused``, the tail kernel through ``RewardNorm.tail`` on copies - are the rollout's, bit for bit: the same statement
on the same inputs on the same device.  1 024 envs x 4 steps, episodes of 3 steps: every env resets (and, where the env reports it,
is truncated) inside the rollout."""
import itertools
import math

import pytest

pytestmark = pytest.mark.gpu

N_ENVS, T, SCALE = 1024, 4, 0.01
CASES = list(itertools.product(("eager", "captured"), (False, True), (False, True), (False, True)))


@pytest.mark.parametrize("mode,reward_norm,boot,asym", CASES)
def test_adv_and_ret_are_the_named_form_on_the_rollouts_own_tensors(mode, reward_norm, boot, asym):
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO, RewardNorm, gae, gae_boot, gae_fused, rollout_tail_form
    eager = mode == "eager"
    form = rollout_tail_form(True, eager, reward_norm, boot, asym)
    env = RoboyVecEnv(MsjRobot(), N_ENVS, seed=5, max_episode_length=3, report_truncation=boot,
                      critic_obs=("state", "age") if asym else None)
    try:
        agent = PPO(env, n_steps=T, seed=3, reward_scale=SCALE, use_graphs=not eager, fused_policy=True, fused_update=True,
                    normalize_reward=reward_norm, bootstrap_timeouts=boot, asymmetric_critic=asym)
        roll = agent.collect()            # (under normalize_reward: behind the priming rollout, on real statistics)
        assert agent._fused is not None and (agent._rollout_graph is None) == eager
        with torch.no_grad():
            last = agent.policy.value(agent._cobs if asym else agent._obs).contiguous()
        rew, val, done, adv, ret = (roll[k].clone() for k in ("rew", "val", "done", "adv", "ret"))
        assert set(roll) == {"obs", "act", "logp", "val", "rew", "done", "adv", "ret"} | ({"trunc"} if boot else set()) | ({"cobs"} if asym else set())
        assert done.sum() >= N_ENVS and set(done.unique().tolist()) == {0.0, 1.0}        # every env ended an episode in the rollout
        codes = done.to(torch.int32)
        if boot:
            assert roll["trunc"].sum() >= N_ENVS // 2 and bool((roll["trunc"] <= done).all())
            codes = (done + roll["trunc"]).to(torch.int32)
        if reward_norm:
            assert agent.reward_norm.count == 2 * T * N_ENVS and not torch.equal(rew, agent._rew_raw * SCALE)
        if form == "torch":
            want = gae_boot(rew, val, codes, last, agent.gamma, agent.lam) if boot else gae(rew, val, done, last, agent.gamma, agent.lam)
        elif form == "gae_kernel":
            want = gae_fused(rew, val, done, last, agent.gamma, agent.lam)
        else:
            # the kernel under identity statistics, fed the rollout's own reward as the raw one at scale 1: its scaling and its
            # normalisation are then exact (r * 1, no clamp), and its recurrence runs on the very floats the rollout's ran on
            assert form == "tail_kernel"
            tail = RewardNorm(N_ENVS, agent.gamma, "cuda", clip=math.inf)
            out = [torch.full_like(rew, float("nan")) for _ in range(4)]
            tail.tail(rew, codes.contiguous(), val, last, 1.0, agent.lam, *out, boot=boot, identity=True)
            assert torch.equal(out[0], rew) and torch.equal(out[1], done)
            want = out[2:]
        torch.cuda.synchronize()
        assert torch.isfinite(adv).all() and adv.abs().max() > 0
        assert torch.equal(want[0], adv), (mode, form, "adv", (want[0] - adv).abs().max().item())
        assert torch.equal(want[1], ret), (mode, form, "ret", (want[1] - ret).abs().max().item())
    finally:
        env.close()
