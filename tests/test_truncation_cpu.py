"""Episode-end codes and value bootstrapping of truncated episodes without a GPU: the float64 reference of the coded
recurrence (tests/truncation_ref.py) against oracle/policy_ref.py and a case worked by hand, ``gae_boot`` in torch float32 against it,
PPO(bootstrap_timeouts=True) on the torch path, the ABI - and the qualification of the scenario the GPU env tests run: on the host
model of the env (tests/host_env_model.py over the C oracle) every code, and the coincidence of goal and time limit, occurs in at
least eight envs, so that no GPU test passes vacuously.

Bound of the float32 statement: 20 T 2^-24 A, A the recurrence on absolute values (truncation_ref.gae_boot32_bound) - the a-priori
rounding bound of the recurrence, counted as tests/test_reward_norm_cpu.py counts its own."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import reward_norm_ref as rref
import truncation_ref as tr
from gym_roboy_amd import _native as nat
from gym_roboy_amd import _policy_native as pn
from gym_roboy_amd._gymcompat import spaces
from gym_roboy_amd.ppo import PPO, RewardNorm, gae, gae_boot
from oracle.policy_ref import gae64
from test_reward_norm_cpu import raw_rewards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()
POLICY_HEADER = open(os.path.join(ROOT, "include", "roboy_policy.h")).read()
GAMMA, LAM, SCALE = 0.99, 0.95, 0.01


def _case(T, N, dones, seed):
    rng = np.random.default_rng(seed)
    rew = rref.scaled(raw_rewards(rng, T, N), SCALE)
    done = rref.done_pattern(dones, T, N, rng)
    val, last = rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    return rew, done, val, last, rng


# ---- the reference ----
@pytest.mark.parametrize("dones", rref.DONE_PATTERNS)
def test_reference_without_truncation_is_gae64(dones):
    rew, done, val, last, _ = _case(37, 130, dones, 3)
    a, r = tr.gae_boot64(rew, val, done, last, GAMMA, LAM)
    a0, r0 = gae64(rew, val, done.astype(np.float32), last, GAMMA, LAM)
    assert np.array_equal(a, a0) and np.array_equal(r, r0)
    # ... and so is the torch statement, to the bit, against gae
    at, rt = gae_boot(*[torch.from_numpy(x) for x in (rew, val, done, last)], GAMMA, LAM)
    ag, rg = gae(*[torch.from_numpy(x) for x in (rew, val, done.astype(np.float32), last)], GAMMA, LAM)
    assert torch.equal(at, ag) and torch.equal(rt, rg)


def test_reference_on_a_case_worked_by_hand():
    """T = 3, one env, V = 2 everywhere, rewards 1, time-out at t = 1, gamma = 0.5, lam = 0.5:
       t = 2: delta = 1 + 0.5 * 2 - 2 = 0,                      adv = 0
       t = 1: truncated: r^ = 1 + 0.5 * 2 = 2, delta = 2 - 2 = 0,  adv = 0      (a done there would give 1 - 2 = -1)
       t = 0: delta = 1 + 0.5 * 2 - 2 = 0,                      adv = 0 + 0.25 * 0 = 0
    A constant value that is right for a reward stream that never ends has no advantage anywhere: the bias is gone.  With code 1
    at t = 1 instead: adv = [0 + 0.25 * -1, -1, 0]."""
    rew, val, last = np.ones((3, 1)), np.full((3, 1), 2.0), np.array([2.0])
    a, r = tr.gae_boot64(rew, val, np.array([[0], [2], [0]]), last, 0.5, 0.5)
    assert np.array_equal(a, np.zeros((3, 1))) and np.array_equal(r, np.full((3, 1), 2.0))
    a, r = tr.gae_boot64(rew, val, np.array([[0], [1], [0]]), last, 0.5, 0.5)
    assert np.array_equal(a, np.array([[-0.25], [-1.0], [0.0]])) and np.array_equal(r, np.array([[1.75], [1.0], [2.0]]))
    at, rt = gae_boot(torch.ones(3, 1), torch.full((3, 1), 2.0), torch.tensor([[0], [2], [0]]), torch.tensor([2.0]), 0.5, 0.5)
    assert torch.equal(at, torch.zeros(3, 1)) and torch.equal(rt, torch.full((3, 1), 2.0))


@pytest.mark.parametrize("kind", tr.CODE_PATTERNS)
@pytest.mark.parametrize("dones", ["random", "all", "none"])
def test_gae_boot_in_float32_matches_the_reference(dones, kind):
    T, N = 37, 257
    rew, done, val, last, rng = _case(T, N, dones, 5)
    code = tr.codes_of(done, kind, rng)
    if dones != "none" or kind.startswith("truncated"):
        assert (code == 2).any()
    a64, r64 = tr.gae_boot64(rew, val, code, last, GAMMA, LAM)
    a32, r32 = gae_boot(*[torch.from_numpy(x) for x in (rew, val, code, last)], GAMMA, LAM)
    assert a32.dtype == torch.float32
    bound = tr.gae_boot32_bound(T, tr.gae_boot_magnitude(rew, val, code, last, GAMMA, LAM))
    ea, er = np.abs(a32.double().numpy() - a64), np.abs(r32.double().numpy() - r64)
    print("gae_boot fp32 vs fp64: adv %.3g, ret %.3g, smallest bound %.3g" % (ea.max(), er.max(), bound.min()))
    assert (ea <= bound).all() and (er <= bound).all()
    # a truncated step differs from a terminated one by exactly the bootstrap
    term = np.where(code == 2, 1, code)
    a_t, _ = tr.gae_boot64(rew, val, term, last, GAMMA, LAM)
    m = code == 2
    assert np.allclose((a64 - a_t)[m], GAMMA * val.astype(np.float64)[m], rtol=0, atol=1e-12)


def test_reward_norm_scan_treats_every_code_as_done():
    rew, done, _, _, rng = _case(16, 33, "random", 7)
    code = tr.codes_of(done, "half", rng)
    assert (code == 2).any() and (code == 1).any()
    a, b = RewardNorm(33, GAMMA), RewardNorm(33, GAMMA)
    sa = a.scan(torch.from_numpy(rew), torch.from_numpy(code)).clone()
    sb = b.scan(torch.from_numpy(rew), torch.from_numpy(done)).clone()
    assert torch.equal(sa, sb) and torch.equal(a.ret_carry, b.ret_carry)


# ---- PPO on the torch path, a stand-in env ----
class TimeLimitVecEnv:
    """Random rewards; episodes end at random (5 % of the steps, 'terminated') or when they are `limit` steps old ('truncated')."""
    report_truncation = True

    def __init__(self, n, seed=0, limit=5):
        self.n, self.rng, self.limit = n, np.random.default_rng(seed), limit
        self.age = np.zeros(n, np.int64)
        self.observation_space = spaces.Box(low=-10, high=10, shape=(3,), dtype="float32")
        self.action_space = spaces.Box(low=-1, high=1, shape=(2,), dtype="float32")
        self.codes = []

    def reset(self):
        return self.rng.standard_normal((self.n, 3)).astype(np.float32)

    def step(self, a):
        self.age += 1
        term = self.rng.random(self.n) < 0.05
        self._trunc = ~term & (self.age >= self.limit)
        done = term | self._trunc
        self.age[done] = 0
        self.codes.append(np.where(term, 1, np.where(self._trunc, 2, 0)))
        return self.reset(), raw_rewards(self.rng, 1, self.n)[0], done, [{}] * self.n

    def truncated(self):
        return self._trunc


@pytest.mark.parametrize("normalize", [False, True])
def test_ppo_bootstraps_on_the_torch_path(normalize):
    env = TimeLimitVecEnv(16, 1)
    agent = PPO(env, n_steps=8, device="cpu", seed=1, reward_scale=SCALE, bootstrap_timeouts=True, normalize_reward=normalize,
                reward_norm_prime=False)
    roll = agent.collect()
    assert set(roll) == {"obs", "act", "logp", "val", "rew", "done", "adv", "ret", "trunc"}
    codes = np.stack(env.codes)
    assert (codes == 2).any() and (codes == 1).any() and (codes == 0).any()
    assert np.array_equal(roll["trunc"].numpy(), (codes == 2).astype(np.float32)) and roll["trunc"].dtype == torch.float32
    assert np.array_equal(roll["done"].numpy(), (codes != 0).astype(np.float32))
    with torch.no_grad():
        last = agent.policy.value(agent._obs).numpy()
    rew, val = roll["rew"].numpy(), roll["val"].numpy()
    a64, r64 = tr.gae_boot64(rew, val, codes, last, agent.gamma, agent.lam)
    bound = tr.gae_boot32_bound(8, tr.gae_boot_magnitude(rew, val, codes, last, agent.gamma, agent.lam))
    assert (np.abs(roll["adv"].double().numpy() - a64) <= bound).all() and (np.abs(roll["ret"].double().numpy() - r64) <= bound).all()
    # the bootstrap is there: without it the truncated steps' advantages are gamma V lower
    a_plain, _ = gae64(rew, val, (codes != 0).astype(np.float64), last, agent.gamma, agent.lam)
    m = codes == 2
    assert np.allclose((a64 - a_plain)[m], agent.gamma * val.astype(np.float64)[m], rtol=0, atol=1e-12) and np.abs(val[m]).min() > 0
    if normalize:                                   # the return statistics saw rewards and dones only
        r_s = rref.scaled(agent._rew_raw.numpy(), SCALE)
        rets, carry, A = rref.scan(r_s, codes, agent.gamma, np.zeros(16))
        assert (np.abs(agent.reward_norm.ret_carry.numpy() - carry) <= rref.carry_bound(8, A)).all()
        assert agent.reward_norm.count == 8 * 16
    stats = agent.update(roll)                      # the extra key does not disturb the update
    assert np.isfinite(stats["loss"])


def test_ppo_refuses_an_env_that_does_not_report_truncation(tmp_path):
    env = TimeLimitVecEnv(4)
    env.report_truncation = False
    with pytest.raises(ValueError, match="report_truncation=True"):
        PPO(env, n_steps=4, device="cpu", bootstrap_timeouts=True)
    env.report_truncation = True
    agent = PPO(env, n_steps=4, device="cpu", bootstrap_timeouts=True)
    path = str(tmp_path / "model.pkl")
    agent.save(path)
    assert torch.load(path)["bootstrap_timeouts"] is True
    off = PPO(TimeLimitVecEnv(4), n_steps=4, device="cpu")
    assert off.bootstrap_timeouts is False and "trunc" not in off.collect()
    off.load(path)                                  # loading does not depend on the flag
    off.save(path)
    assert torch.load(path)["bootstrap_timeouts"] is False
    agent.load(path)


def test_cli_forwards_the_flag_to_env_and_agent(tmp_path, monkeypatch):
    import gym_roboy_amd.envs.vec_env as vec_env
    import gym_roboy_amd.ppo as ppo
    import gym_roboy_amd.train_parallel as tp
    seen = {}

    class Stop(Exception):
        pass

    def fake_env(*a, **kw):
        seen["env"] = kw
        return object()

    def fake_ppo(env, **kw):
        seen["ppo"] = kw
        raise Stop

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(vec_env, "RoboyVecEnv", fake_env)
    monkeypatch.setattr(ppo, "PPO", fake_ppo)
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path), "--bootstrap-timeouts"])
    assert seen["env"]["report_truncation"] is True and seen["ppo"]["bootstrap_timeouts"] is True
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path)])
    assert seen["env"]["report_truncation"] is False and seen["ppo"]["bootstrap_timeouts"] is False


# ---- the ABI ----
def test_entry_points_are_declared_exported_and_mirrored():
    lib = nat.load()
    for name in ("rb_env_done_kind_configure", "rb_env_done_kind_ptr"):
        assert re.search(r"\bint %s\(" % name, SIM_HEADER), name
        assert name in nat.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    for name, value in (("RB_DONE_NONE", 0), ("RB_DONE_TERMINATED", 1), ("RB_DONE_TRUNCATED", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), SIM_HEADER) and getattr(nat, name) == value
    plib = pn.load()
    assert re.search(r"\bint rp_rollout_tail_boot_dev\(", POLICY_HEADER) and hasattr(plib, "rp_rollout_tail_boot_dev")
    assert pn.SIGNATURES["rp_rollout_tail_boot_dev"] == pn.SIGNATURES["rp_rollout_tail_dev"]
    # the two declarations take the same argument list
    args = {n: re.sub(r"\s+", " ", re.search(r"int %s\((.*?)\);" % n, POLICY_HEADER, re.S).group(1))
            for n in ("rp_rollout_tail_dev", "rp_rollout_tail_boot_dev")}
    assert args["rp_rollout_tail_dev"] == args["rp_rollout_tail_boot_dev"]
    assert plib.rp_abi_version() == pn.RP_ABI_VERSION == 5 and re.search(r"#define RP_ABI_VERSION 5\b", POLICY_HEADER)


def test_null_handle_is_an_error_not_an_abort():
    lib = nat.load()
    kind = ctypes.c_void_p()
    assert lib.rb_env_done_kind_configure(None, 1) == nat.RB_EINVAL
    assert lib.rb_env_done_kind_ptr(None, ctypes.byref(kind)) == nat.RB_EINVAL
    assert lib.rb_last_error()


def test_both_new_kernels_are_in_the_shipped_code_objects_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object_meta as com
    for lib, kernel in (("libroboy_sim.so", "done_kind_kernel"), ("libroboy_policy.so", "rollout_tail_boot_kernel")):
        metas = [v for name, v in com.kernel_metadata(os.path.join(ROOT, "gym_roboy_amd", "csrc", lib)).items() if kernel in name]
        assert len(metas) == 1, (kernel, metas)
        k = metas[0]
        print(kernel, {f: k.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert k["private_segment_fixed_size"] == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k


# ---- the scenario of the GPU env tests, qualified on the host model ----
def run_host_scenario(n, upper_body=False):
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    from host_env_model import COracleStepper, HostEnvModel
    robot = UpperBodyRobot() if upper_body else MsjRobot()
    host = HostEnvModel(robot, COracleStepper(robot, n), n, 3, tr.MAX_LEN, False, True, True)
    host.goal = host.draw(np.ones(n, bool))         # (the env's configure drew goal 0, reset() goal 1)
    desc = robot.get_description()
    goal, step_num, actions, groups = tr.scenario(n, desc.n_q, desc.n_t, host.goal)
    host.goal, host.step_num = goal.copy(), step_num.astype(np.int64)
    codes, timed_out = [], []
    for t in range(tr.STEPS):
        clock = host.step_num + 1 > tr.MAX_LEN
        _, rew, done, _ = host.step(actions[t])
        assert ((rew > 0) <= done).all() and (clock <= done).all()
        codes.append(tr.expected_codes(done, rew))
        timed_out.append(clock)
    return np.stack(codes), np.stack(timed_out), groups


def test_the_scenario_shows_every_code_on_the_host_model():
    """MsjRobot, max_episode_length = 5, goal bonus on, 12 steps, on the batch sizes the GPU tests step: a third of the envs at their
    goal, a third at their goal on the last permitted step."""
    for n, upper in ((200, False), (320, False), (576, False), (64, True)):       # (the upper body at 64 envs runs the scenario on the GPU too)
        codes, clock, groups = run_host_scenario(n, upper)
        tr.assert_every_code_occurs(codes, groups)
        coincide = (codes == tr.TERMINATED) & clock
        assert coincide.any(axis=0).sum() >= 8 and coincide[0, groups == 1].all()
        assert ((codes == tr.TRUNCATED) <= clock).all()
        print("n = %d: envs showing 0 / 1 / 2 / coincidence: %s" % (n, [(codes == c).any(axis=0).sum() for c in (0, 1, 2)] + [coincide.any(axis=0).sum()]))
