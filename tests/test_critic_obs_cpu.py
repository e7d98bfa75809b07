"""The asymmetric critic without a GPU: the names and dependencies of the critic row, MlpPolicy(critic_obs_dim), the
two libraries' new symbols and unchanged ABI numbers, the new kernels' resource figures read from the shipped code objects, and
PPO(asymmetric_critic=True) on the torch path over a stand-in env."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gym_roboy_amd import _native as nat
from gym_roboy_amd import _policy_native as pn
from gym_roboy_amd._gymcompat import spaces
from gym_roboy_amd.envs.vec_env import critic_obs_spec
from gym_roboy_amd.ppo import PPO, MlpPolicy, ObsNorm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()
POLICY_HEADER = open(os.path.join(ROOT, "include", "roboy_policy.h")).read()
ALL = ("state", "age", "params", "delay", "actions")


# ---- the row: names, order, width, dependencies ----
def test_names_are_put_in_row_order_and_state_is_always_there():
    full = dict(randomization=True, action_delay=(0, 3), action_obs=2)
    assert critic_obs_spec(None, 3, 8) == ((), 0, 0) and critic_obs_spec((), 3, 8) == ((), 0, 0)
    assert critic_obs_spec("state", 3, 8) == (("state",), 1, 9)
    assert critic_obs_spec(("age",), 3, 8) == (("state", "age"), 3, 10)
    assert critic_obs_spec(("actions", "delay", "params", "age", "state"), 3, 8, **full) == (ALL, 31, 9 + 1 + 20 + 1 + 16)
    assert critic_obs_spec(("params",), 3, 12, randomization=True) == (("state", "params"), 5, 9 + 28)
    assert critic_obs_spec(("delay",), 3, 8, action_delay=2) == (("state", "delay"), 9, 10)
    for mask_bit, name in enumerate(nat.CRITIC_OBS_BLOCKS):
        assert getattr(nat, "RB_CRITIC_" + name.upper()) == 1 << mask_bit
        assert re.search(r"#define RB_CRITIC_%s %du\b" % (name.upper(), 1 << mask_bit), SIM_HEADER)
    assert nat.RB_CRITIC_OBS_MAX_DIM == 63 and re.search(r"#define RB_CRITIC_OBS_MAX_DIM 63\b", SIM_HEADER)
    # the library's own count of the same rows (no GPU needed)
    lib = nat.load()
    assert lib.rb_env_critic_obs_count(3, 8, 31, 20, 2) == 47 and lib.rb_env_critic_obs_count(3, 8, 2, 0, 0) == 10
    assert lib.rb_env_critic_obs_count(3, 8, 0, 0, 0) == 0 and lib.rb_env_critic_obs_count(3, 8, 32, 0, 0) == -1


@pytest.mark.parametrize("names,kw,word", [
    (("state", "speed"), {}, "distinct names"), (("age", "age"), {}, "distinct names"),
    (("params",), {}, "randomization"), (("params",), dict(action_delay=2, action_obs=2), "randomization"),
    (("delay",), {}, "action_delay"), (("delay",), dict(action_delay=0), "action_delay"), (("delay",), dict(randomization=True), "action_delay"),
    (("actions",), {}, "action_obs"), (("actions",), dict(action_obs=0), "action_obs"),
    # Dc > 63, the gradient kernels' input limit: MsjRobot's full row is 31 + 8 K columns
    (ALL, dict(randomization=True, action_delay=(0, 3), action_obs=5), "at most 63"),
    (("params", "actions"), dict(randomization=True, action_obs=5), "at most 63"),
])
def test_refusals(names, kw, word):
    with pytest.raises(ValueError, match=word):
        critic_obs_spec(names, 3, 8, **kw)


def test_the_widest_rows_that_fit():
    assert critic_obs_spec(ALL, 3, 8, randomization=True, action_delay=(0, 3), action_obs=4)[2] == 63
    assert critic_obs_spec(("params", "actions"), 3, 8, randomization=True, action_obs=4)[2] == 61


def test_the_env_refuses_before_anything_is_allocated(monkeypatch):
    import gym_roboy_amd.envs.vec_env as vec_env
    from gym_roboy_amd.envs.robots import MsjRobot

    def no_sim(*a, **kw):
        raise AssertionError("a simulation was created")

    monkeypatch.setattr(vec_env, "HipBatchSimulation", no_sim)
    for kw, word in ((dict(critic_obs=("params",)), "randomization"), (dict(critic_obs=("delay",), sensor_noise={"q": 0.1}), "action_delay"),
                     (dict(critic_obs=("actions",)), "action_obs"), (dict(critic_obs=("goal",)), "distinct names"),
                     (dict(critic_obs=("age", "actions"), action_obs=7), "at most 63")):
        with pytest.raises(ValueError, match=word):
            vec_env.RoboyVecEnv(MsjRobot(), 4, **kw)


# ---- the policy ----
def test_policy_shapes_and_state_dict_keys():
    sym, asym = MlpPolicy(25, 8), MlpPolicy(25, 8, critic_obs_dim=47)
    assert list(sym.state_dict()) == list(asym.state_dict())
    for k, v in sym.state_dict().items():
        assert tuple(asym.state_dict()[k].shape) == ((64, 47) if k == "vf.0.weight" else tuple(v.shape)), k
    assert sym.critic_obs_dim is None and asym.critic_obs_dim == 47
    obs, cobs = torch.randn(5, 25), torch.randn(5, 47)
    assert tuple(asym.value(cobs).shape) == (5,) and tuple(asym.dist(obs).mean.shape) == (5, 8)
    a, logp, v = asym.act(obs, cobs=cobs)
    assert torch.equal(v, asym.value(cobs).detach()) and tuple(a.shape) == (5, 8)
    assert asym.act(obs, deterministic=True)[2] is None              # the actor alone: playback needs no critic row
    with pytest.raises(RuntimeError):
        asym.value(obs)
    # None is today's module
    torch.manual_seed(3); p = MlpPolicy(9, 8)
    torch.manual_seed(3); r = MlpPolicy(9, 8, critic_obs_dim=None)
    assert all(torch.equal(x, y) for x, y in zip(p.parameters(), r.parameters()))


def test_the_critic_has_its_own_statistics():
    p = MlpPolicy(4, 2, critic_obs_dim=6)
    na, nc = ObsNorm(4, clip=2.0), ObsNorm(6, clip=3.0)
    nc.update(torch.randn(100, 6) * 5 + 2)
    na.update(torch.randn(100, 4) * 0.1 - 1)
    p.set_obs_norm(na, nc)
    obs, cobs = torch.randn(7, 4), torch.randn(7, 6)
    assert torch.equal(p.value(cobs), p.vf(nc.apply(cobs)).squeeze(-1))
    assert torch.equal(p.dist(obs).mean, p.pi(na.apply(obs)))
    assert p.set_obs_norm(None).critic_obs_norm is None
    assert list(p.state_dict()) == list(MlpPolicy(4, 2).state_dict())


def test_layout_and_gather_maps_of_the_asymmetric_vector():
    lib = pn.load()
    for da, dc, act in ((9, 38, 8), (33, 10, 8), (25, 47, 8), (9, 9, 8)):
        lay, n = pn.grad_layout(da, act, dc)
        gs_pi, gs_vf = lib.rp_grad_floats(da, act) // 2, lib.rp_grad_floats(dc, act) // 2
        assert n == gs_pi + gs_vf == lib.rp_grad_asym_floats(da, dc, act)
        sym_a, sym_c = pn.grad_layout(da, act)[0], pn.grad_layout(dc, act)[0]
        for k, (off, shape) in lay.items():
            if k.startswith("vf_"):
                assert (off - gs_pi, shape) == (sym_c[k][0] - gs_vf, sym_c[k][1]), k
            else:
                assert (off, shape) == sym_a[k], k
        assert lib.rp_ppo_asym_workspace_floats(da, dc, act, 1000) == (lib.rp_ppo_workspace_floats(da, act, 1000)
                                                                       + lib.rp_ppo_workspace_floats(dc, act, 1000)) // 2
        # each blob of the pair is the symmetric blob of its width wherever its own net is concerned
        shapes = pn.param_shapes(da, act, critic_obs_dim=dc)
        rng = np.random.default_rng(da + dc)
        params = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}
        flat = np.concatenate([params[k].reshape(-1) for k in pn.PARAM_ORDER] + [np.zeros(1, np.float32)])
        for train in (False, True):
            m_pi, m_vf, off = pn.gather_map_asym(da, dc, act, train=train)
            assert off == flat.shape[0] - 1
            want_pi = pn.pack(dict(params, vf_w1=np.zeros((64, da), np.float32)), da, act, train)
            want_vf = pn.pack(dict(params, pi_w1=np.zeros((64, dc), np.float32)), dc, act, train)
            assert np.array_equal(flat[m_pi], want_pi) and np.array_equal(flat[m_vf], want_vf)
    assert lib.rp_grad_asym_floats(9, 64, 8) < 0 and lib.rp_grad_asym_floats(64, 9, 8) < 0


# ---- the ABI ----
SIM_SYMBOLS = ("rb_env_critic_obs_configure", "rb_env_critic_obs_dim", "rb_env_critic_obs_ptr", "rb_env_step_critic_dev",
               "rb_env_step_range_critic_dev")
POLICY_SYMBOLS = ("rp_act_asym_dev", "rp_act_asym_norm_dev", "rp_ppo_grad_asym_dev", "rp_clip_adam_asym_dev", "rp_clip_adam_kl_asym_dev")


def test_entry_points_are_declared_exported_and_mirrored():
    lib, plib = nat.load(), pn.load()
    for name in SIM_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, SIM_HEADER), name
        assert name in nat.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    assert re.search(r"\bint32_t rb_env_critic_obs_count\(", SIM_HEADER) and "rb_env_critic_obs_count" in nat.SIGNATURES
    for name in POLICY_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, POLICY_HEADER), name
        assert name in pn.SIGNATURES and hasattr(plib, name)
    for name in ("rp_grad_asym_floats", "rp_ppo_asym_workspace_floats"):
        assert re.search(r"\bint64_t %s\(" % name, POLICY_HEADER) and name in pn.SIGNATURES and hasattr(plib, name)
    # every argument list of the binding is as long as the header's
    for header, sigs, names in ((SIM_HEADER, nat.SIGNATURES, SIM_SYMBOLS + ("rb_env_critic_obs_count",)),
                                (POLICY_HEADER, pn.SIGNATURES, POLICY_SYMBOLS + ("rp_grad_asym_floats", "rp_ppo_asym_workspace_floats"))):
        for name in names:
            args = re.search(r"\bint(?:32_t|64_t)? %s\((.*?)\);" % name, header, re.S).group(1)
            assert len(args.split(",")) == len(sigs[name][1]), name
    # additive: both ABI numbers are what they were
    assert lib.rb_abi_version() == 6 and re.search(r"#define RB_ABI_VERSION 6\b", SIM_HEADER)
    assert plib.rp_abi_version() == pn.RP_ABI_VERSION == 5 and re.search(r"#define RP_ABI_VERSION 5\b", POLICY_HEADER)


def test_null_arguments_are_errors_not_aborts():
    lib, plib = nat.load(), pn.load()
    out = ctypes.c_void_p()
    dim = ctypes.c_int32()
    assert lib.rb_env_critic_obs_configure(None, 1) == nat.RB_EINVAL
    assert lib.rb_env_critic_obs_dim(None, ctypes.byref(dim)) == nat.RB_EINVAL
    assert lib.rb_env_critic_obs_ptr(None, ctypes.byref(out)) == nat.RB_EINVAL
    assert lib.rb_env_step_critic_dev(None, None, None, None, None, None) == nat.RB_EINVAL
    assert lib.rb_env_step_range_critic_dev(None, 0, 256, None, None, None, None, None, None) == nat.RB_EINVAL
    assert lib.rb_last_error()
    assert plib.rp_act_asym_dev(*([None] * 8), 4, 9, 38, 8, 0, 0, 0, None, 0, None) != 0 and b"null" in plib.rp_last_error()
    assert plib.rp_ppo_grad_asym_dev(*([None] * 11), 4, 9, 38, 8, 0.2, 0.5, None, None, 0.0, 0.0, 0, None, None, None) != 0
    assert plib.rp_clip_adam_asym_dev(None, None, None, None, 9, 38, 8, 1e-3, 0.9, 0.999, 1e-5, 1, 0.5, 1.0, 0.0, None) != 0


def test_the_new_kernels_are_in_the_shipped_code_objects_without_scratch_or_spills():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object_meta as com
    for lib, kernel in (("libroboy_sim.so", "critic_rows_kernel"), ("libroboy_policy.so", "mlp_act_asym_kernel"),
                        ("libroboy_policy.so", "mlp_act_asym_norm_kernel")):
        metas = [v for name, v in com.kernel_metadata(os.path.join(ROOT, "gym_roboy_amd", "csrc", lib)).items() if kernel in name]
        assert len(metas) == 1, (kernel, metas)
        k = metas[0]
        print(kernel, {f: k.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                                             "group_segment_fixed_size", "max_flat_workgroup_size")})
        assert k["private_segment_fixed_size"] == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
        assert k["max_flat_workgroup_size"] == 256


# ---- PPO on the torch path, a stand-in env ----
class CriticRowVecEnv:
    """Random observation rows [n, 3] and critic rows [n, 5]; the reward is the critic row's first column, which the observation
    does not show."""
    critic_obs_names = ("state", "age")

    def __init__(self, n, seed=0, critic_obs_dim=5):
        self.n, self.rng, self.critic_obs_dim = n, np.random.default_rng(seed), critic_obs_dim
        self.observation_space = spaces.Box(low=-10, high=10, shape=(3,), dtype="float32")
        self.action_space = spaces.Box(low=-1, high=1, shape=(2,), dtype="float32")
        self._rows()

    def _rows(self):
        self._cobs = self.rng.standard_normal((self.n, 5)).astype(np.float32)
        return self.rng.standard_normal((self.n, 3)).astype(np.float32)

    def reset(self):
        return self._rows()

    def step(self, a):
        rew = self._cobs[:, 0].copy()
        return self._rows(), rew, self.rng.random(self.n) < 0.1, [{}] * self.n

    def critic_obs(self):
        return self._cobs


@pytest.mark.parametrize("normalize", [False, True])
def test_ppo_collects_and_updates_on_the_torch_path(normalize):
    env = CriticRowVecEnv(16, 1)
    agent = PPO(env, n_steps=8, device="cpu", seed=1, asymmetric_critic=True, normalize_obs=normalize, obs_norm_prime=False)
    assert agent.policy.critic_obs_dim == 5 and agent.policy.vf[0].in_features == 5 and agent.policy.pi[0].in_features == 3
    assert (agent.cobs_norm is not None) == normalize
    roll = agent.collect()
    assert set(roll) == {"obs", "cobs", "act", "logp", "val", "rew", "done", "adv", "ret"}
    assert tuple(roll["cobs"].shape) == (8, 16, 5) and tuple(roll["obs"].shape) == (8, 16, 3)
    # the rows belong together: the reward of step t is the critic row's first column at step t
    assert torch.equal(roll["rew"], roll["cobs"][..., 0])
    with torch.no_grad():
        assert torch.equal(agent.policy.value(roll["cobs"]), roll["val"])
    stats = agent.update(roll)
    assert np.isfinite(stats["loss"])
    if normalize:
        assert agent.cobs_norm.count == 8 * 16 == agent.obs_norm.count and agent.cobs_norm.obs_dim == 5


def test_the_value_nets_gradient_does_not_depend_on_the_observation():
    env = CriticRowVecEnv(16, 2)
    agent = PPO(env, n_steps=8, device="cpu", seed=2, asymmetric_critic=True)
    roll = agent.collect()
    flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in roll.items()}
    idx = torch.arange(flat["obs"].shape[0])

    def grads(f):
        agent.policy.zero_grad(set_to_none=True)
        agent._minibatch_loss(f, idx)[0].backward()
        return ([p.grad.clone() for p in agent.policy.vf.parameters()], [p.grad.clone() for p in agent.policy.pi.parameters()])

    vf0, pi0 = grads(flat)
    vf1, pi1 = grads(dict(flat, obs=flat["obs"] + torch.randn_like(flat["obs"])))
    vf2, pi2 = grads(dict(flat, cobs=flat["cobs"] + torch.randn_like(flat["cobs"])))
    assert all(torch.equal(a, b) for a, b in zip(vf0, vf1)) and not all(torch.equal(a, b) for a, b in zip(pi0, pi1))
    assert all(torch.equal(a, b) for a, b in zip(pi0, pi2)) and not all(torch.equal(a, b) for a, b in zip(vf0, vf2))
    assert all(g.abs().max() > 0 for g in vf0)


def test_ppo_refusals_and_the_checkpoint(tmp_path):
    class Plain(CriticRowVecEnv):
        critic_obs_names = ()

        def __init__(self, n):
            super().__init__(n, critic_obs_dim=0)

    with pytest.raises(ValueError, match="critic_obs"):
        PPO(Plain(4), n_steps=4, device="cpu", asymmetric_critic=True)
    with pytest.raises(ValueError, match="asymmetric_critic=True"):
        PPO(Plain(4), MlpPolicy(3, 2, critic_obs_dim=5), n_steps=4, device="cpu")
    with pytest.raises(ValueError, match="value net reads"):
        PPO(CriticRowVecEnv(4), MlpPolicy(3, 2, critic_obs_dim=6), n_steps=4, device="cpu", asymmetric_critic=True)
    agent = PPO(CriticRowVecEnv(4), n_steps=4, device="cpu", asymmetric_critic=True, normalize_obs=True, obs_norm_prime=False)
    agent.update(agent.collect())
    path = str(tmp_path / "model.pkl")
    agent.save(path)
    ck = torch.load(path)
    assert ck["critic_obs"] == ["state", "age"] and ck["critic_obs_dim"] == 5 and ck["critic_obs_norm"]["count"] == 16
    assert tuple(ck["policy"]["vf.0.weight"].shape) == (64, 5)
    again = PPO(CriticRowVecEnv(4), n_steps=4, device="cpu", asymmetric_critic=True, normalize_obs=True)
    again.load(path)
    assert torch.equal(again.cobs_norm.state, agent.cobs_norm.state)
    assert all(torch.equal(p, q) for p, q in zip(again.policy.parameters(), agent.policy.parameters()))
    # another row, or an agent without the option: refused; a checkpoint without the option still loads where it was written
    other = CriticRowVecEnv(4)
    other.critic_obs_names = ("state", "delay")
    with pytest.raises(ValueError, match="critic was trained on the rows"):
        PPO(other, n_steps=4, device="cpu", asymmetric_critic=True, normalize_obs=True).load(path)
    sym = PPO(CriticRowVecEnv(4), n_steps=4, device="cpu", normalize_obs=True)
    with pytest.raises(ValueError, match="asymmetric critic"):
        sym.load(path)
    plain = str(tmp_path / "plain.pkl")
    sym.save(plain)
    assert "critic_obs" not in torch.load(plain)
    sym.load(plain)
    with pytest.raises(ValueError, match="asymmetric critic"):
        again.load(plain)


def test_cli_forwards_the_names_to_env_and_agent(tmp_path, monkeypatch):
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
        tp.main(["4", str(tmp_path), "--critic-obs", "state,age,delay,actions", "--action-delay", "0:3", "--action-obs", "2"])
    assert seen["env"]["critic_obs"] == ("state", "age", "delay", "actions") and seen["ppo"]["asymmetric_critic"] is True
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path)])
    assert seen["env"]["critic_obs"] is None and seen["ppo"]["asymmetric_critic"] is False
