"""CPU tests of the mirror-symmetry augmentation: the row maps of gym_roboy_amd/envs/symmetry.py, the fp64 oracle's
word that the map IS the plant's symmetry (and that the other sign pattern is not), the env layer's reward and done on mirrored
pairs, PPO(symmetry="augment") on the CPU against an agent without the option that is fed the concatenated rollout, and the two
new symbols with the new kernel's resources."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, random_states
from gym_roboy_amd.envs import reward as rw
from gym_roboy_amd.envs.symmetry import mirror_rows, row_mirror_map
from oracle.physics_np import EULER, RK4, TendonRobotOracle
from symmetry_util import AUGMENTED, JOINT_SIGN, MSJ_IMAGE, MirrorToyEnv, bits, concatenated, is_involution

CHANNELS = ("length", "rate", "activation", "force")


# ---- the row maps ----
@pytest.mark.parametrize("plane", [0, 1])
@pytest.mark.parametrize("tendon_obs, action_obs", [((), 0), (("length", "force"), 0), ((), 3), (CHANNELS, 2)])
def test_row_mirror_map_layouts(plane, tendon_obs, action_obs):
    n_q, n_t = 3, 8
    image = MSJ_IMAGE if plane == 0 else np.array([1, 0, 3, 2, 6, 7, 4, 5])
    src, sign, act_src = row_mirror_map(n_q, n_t, JOINT_SIGN[plane], image, tendon_obs, action_obs)
    obs_dim = 3 * n_q + len(tendon_obs) * n_t + action_obs * n_t          # RoboyVecEnv's documented width
    assert src.shape == sign.shape == (obs_dim,) and src.dtype == np.int32 and sign.dtype == np.float32
    assert act_src.dtype == np.int32 and np.array_equal(act_src, image)
    assert is_involution(src, sign) and is_involution(act_src, np.ones(n_t))
    # [q, qd, goal]: the column itself, the joints' signs
    assert np.array_equal(src[:9], np.arange(9)) and np.array_equal(sign[:9], np.tile(JOINT_SIGN[plane], 3))
    # every block of n_t columns behind: the partner's column of the same block, sign +1
    for b in range(len(tendon_obs) + action_obs):
        lo = 9 + b * n_t
        assert np.array_equal(src[lo:lo + n_t], lo + image) and np.all(sign[lo:lo + n_t] == 1.0)
    # the statement on a row: numpy and torch agree bit for bit, and a flipped 0 is -0
    x = np.random.default_rng(plane).standard_normal((5, obs_dim)).astype(np.float32)
    x[0] = 0.0
    y = mirror_rows(x, src, sign)
    assert np.array_equal(bits(y), bits(mirror_rows(torch.from_numpy(x), src, sign)))
    assert np.array_equal(np.signbit(y[0]), sign < 0)
    assert np.array_equal(bits(mirror_rows(y, src, sign)[1:]), bits(x[1:]))


def test_row_mirror_map_refuses_what_is_no_mirror():
    with pytest.raises(ValueError):
        row_mirror_map(3, 8, (-1, 1, 0), MSJ_IMAGE)
    with pytest.raises(ValueError):
        row_mirror_map(3, 8, (-1, 1, -1), np.arange(8))                  # fixed points
    with pytest.raises(ValueError):
        row_mirror_map(3, 8, (-1, 1, -1), [1, 2, 0, 4, 5, 3, 7, 6])      # a permutation, not an involution
    with pytest.raises(ValueError):
        row_mirror_map(3, 8, (-1, 1, -1), MSJ_IMAGE, ("tension",))


# ---- the map is the physics' symmetry ----
@pytest.fixture(scope="module")
def mirror_cases(hostmath_lib):
    """(description, plane, tendon pairing): MsjRobot's by hand, the rotated robot's as the product's own detection finds it
    (csrc/msj_build.hpp: find_mirror_pairs, built for the host)"""
    from test_mirror_pairs import _pairs, _rotated_msj
    from gym_roboy_amd.envs.robots import MsjRobot
    cases = {"msj": (MsjRobot.get_description(), 0, MSJ_IMAGE)}
    desc = _rotated_msj()
    q, qd, sp = random_states(desc, 4, 0)
    rc, _, _, _, plane, half = _pairs(hostmath_lib, desc, q, qd, sp, 0)
    assert rc == 0 and plane == 1
    image = np.zeros(8, np.int64)
    image[half[:4]], image[half[4:]] = half[4:], half[:4]
    cases["rotated"] = (desc, 1, image)
    return cases


@pytest.mark.parametrize("integ", [EULER, RK4])
@pytest.mark.parametrize("which", ["msj", "rotated"])
def test_the_map_is_the_plants_symmetry(mirror_cases, which, integ):
    desc, plane, image = mirror_cases[which]
    oracle = TendonRobotOracle(desc)
    q, qd, sp = (a.astype(np.float64) for a in random_states(desc, 500, 7))
    S = JOINT_SIGN[plane].astype(np.float64)
    q1, qd1, f1 = oracle.step(q, qd, sp, integrator=integ)
    q2, qd2, f2 = oracle.step(q * S, qd * S, sp[:, image], integrator=integ)
    err = max(np.abs(q2 - q1 * S).max(), np.abs(qd2 - qd1 * S).max())
    print("%s, integrator %d: |step(S q, S qd, P sp) - S step(q, qd, sp)| = %.3g" % (which, integ, err))
    assert err < 1e-12 and np.array_equal(f1, f2)
    # the other plane's sign pattern with the same pairing is NOT a symmetry: the test can tell the planes apart
    W = JOINT_SIGN[1 - plane].astype(np.float64)
    q3, qd3, _ = oracle.step(q * W, qd * W, sp[:, image], integrator=integ)
    miss = max(np.abs(q3 - q1 * W).max(), np.abs(qd3 - qd1 * W).max())
    print("%s, integrator %d: the other sign pattern misses by %.3g" % (which, integ, miss))
    assert miss > 1e-2


@pytest.mark.parametrize("which", ["msj", "rotated"])
def test_tendon_channels_are_permuted_by_the_mirror(mirror_cases, which):
    from env_obs_util import readout64
    desc, plane, image = mirror_cases[which]
    q, qd, sp = (a.astype(np.float64) for a in random_states(desc, 500, 7))
    S = JOINT_SIGN[plane].astype(np.float64)
    a, _ = readout64(desc, q, qd, sp)
    b, _ = readout64(desc, q * S, qd * S, sp[:, image])
    for c in CHANNELS:
        err = np.abs(b[c] - a[c][:, image]).max()
        print("%s %s: |mirrored - permuted| = %.3g" % (which, c, err))
        assert err < 1e-12, c                                                  # absolute, in the channel's own unit (m, m/s, 1, N)
    assert a["force"].max() > 1.0 and np.abs(a["rate"]).max() > 1e-3          # the comparison is not between zeros


@pytest.mark.parametrize("integ", [EULER, RK4])
def test_every_twin_env_is_feasible_and_clear_of_its_limits(msj_robot, integ):
    """The premise of tests/test_symmetry_gpu.py's equivariance test, by the fp64 oracle: under the set-points its three configurations
    apply (the actions; under action_delay=2 the rest command twice, then the first action) every env stays feasible and further than
    10 x the state tolerance 2e-5 from a joint limit - neither twin can see a limit hit (the flag, the boundary penalty, the dropped
    velocity: the discontinuous ones) that the other does not - and nobody comes near a goal.  The velocity saturation needs no
    margin: it is a continuous clamp, so twins on either side of it still agree within the tolerance (some envs do saturate)."""
    from env_obs_util import env_rescale64
    from symmetry_util import twin_case
    desc, q, qd, acts, goal = twin_case(msj_robot)
    o = TendonRobotOracle(desc)

    def clear(q1, qd1, f1):
        margin = np.minimum(q1 - desc.q_lo, desc.q_hi - q1).min()
        assert f1.all() and margin > 10 * 2e-5, margin
        assert np.linalg.norm(q1 - goal, axis=1).min() > 0.1
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)
    clear(*o.step(q64, qd64, env_rescale64(msj_robot, acts[0]), integrator=integ))
    state = (q64, qd64)
    for sp in (np.zeros(acts[0].shape), np.zeros(acts[0].shape), env_rescale64(msj_robot, acts[0])):
        out = o.step(state[0], state[1], sp, integrator=integ)
        clear(*out)
        state = out[:2]


# ---- reward and done ----
@pytest.mark.parametrize("vel_penalty", [False, True])
def test_reward_and_done_are_symmetric(msj_robot, vel_penalty):
    angles, vels = msj_robot.get_joint_angles_space(), msj_robot.get_joint_vels_space()
    S = JOINT_SIGN[0]
    for box in (angles, vels):
        for j in np.nonzero(S < 0)[0]:
            assert box.low[j] == -box.high[j]
    desc = msj_robot.get_description()
    q, qd, _ = random_states(desc, 500, 7)
    rng = np.random.default_rng(8)
    goal = rng.uniform(desc.q_lo, desc.q_hi, q.shape).astype(np.float32)
    goal[:40] = q[:40] + np.float32(1e-4) * rng.standard_normal((40, 3)).astype(np.float32)      # some envs at their goal ...
    qd[:20] *= np.float32(1e-3)                                                                     # ... and slow enough to be done
    feas = rng.random(len(q)) > 0.1
    max_da, max_dv = rw.l2_distance(angles.low, angles.high), rw.l2_distance(vels.low, vels.high)
    out = []
    for s in (np.ones(3), S.astype(np.float64)):
        q64, qd64, g64 = q.astype(np.float64) * s, qd.astype(np.float64) * s, goal.astype(np.float64) * s
        zero = np.zeros_like(qd64)
        r = rw.compute_reward(q64, qd64, feas, g64, zero, (angles.low, angles.high), (vels.low, vels.high), max_da, max_dv,
                              vel_penalty, True)
        out.append((r, rw.did_reach_goal(q64, qd64, g64, zero, max_da, max_dv)))
    assert np.array_equal(out[0][0].view(np.int64), out[1][0].view(np.int64))
    assert np.array_equal(out[0][1], out[1][1]) and 0 < out[0][1].sum() < 40


# ---- PPO on the CPU ----
def _agent(symmetry, n=16, seed=3, env=None, **kw):
    from gym_roboy_amd.ppo import PPO
    env = env or MirrorToyEnv(n, seed=5)
    return PPO(env, n_steps=8, nminibatches=2, noptepochs=2, device="cpu", seed=seed, symmetry=symmetry, **kw)


def _orders(n2, epochs, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n2, generator=g) for _ in range(epochs)]


def test_augment_is_the_concatenation():
    agent = _agent("augment")
    roll = agent.collect()
    flat = agent.augment(roll)
    maps = agent.env.mirror_map()
    want = concatenated({k: v.numpy() for k, v in roll.items()}, maps)
    n = 8 * 16
    assert sorted(flat) == sorted(AUGMENTED)
    for k in AUGMENTED:
        assert tuple(flat[k].shape) == tuple(want[k][0].shape) and flat[k].shape[0] == 2 * n
        assert np.array_equal(bits(flat[k]), bits(want[k][0])), k
    assert np.array_equal(bits(flat["logp"][n:]), bits(flat["logp"][:n]))           # the ORIGINAL's old log-probability
    assert not np.array_equal(bits(flat["obs"][n:]), bits(flat["obs"][:n]))


@pytest.mark.parametrize("diagnostics", [False, True])
def test_update_is_the_update_on_the_concatenated_rollout(diagnostics):
    a, b = _agent("augment", diagnostics=diagnostics), _agent(None, diagnostics=diagnostics)
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    roll = a.collect()
    before = [p.detach().clone() for p in a.policy.parameters()]
    orders = _orders(2 * 8 * 16, 2)
    sa = a.update(roll, sample_orders=orders)
    sb = b.update(concatenated(roll, a.env.mirror_map()), sample_orders=orders)
    assert sa == sb
    moved = 0
    for p, q, p0 in zip(a.policy.parameters(), b.policy.parameters(), before):
        assert np.array_equal(bits(p), bits(q))
        moved += int(not torch.equal(p, p0))
    assert moved > 0
    # the same number of optimiser steps as without the option, on minibatches twice the size
    assert int(a.opt.state_dict()["state"][0]["step"]) == 2 * 2


def test_observation_statistics_commute_with_the_mirror():
    """after ONE merge over rows <= 1e5 the mean of a sign-flipped column is 0 up to the fp64 summation bound rows * 2^-52 * max|x|"""
    agent = _agent("augment", n=64, normalize_obs=True, obs_norm_prime=False)
    src, sign, _ = agent.env.mirror_map()
    roll = agent.collect()
    assert agent.obs_norm.count == 0
    agent.update(roll)                            # the merge: over the rollout's rows and their images
    rows = 2 * 8 * 64
    assert agent.obs_norm.count == rows and rows <= 1e5
    bound = rows * 2.0 ** -52 * float(roll["obs"].abs().max())
    mean = agent.obs_norm.mean.numpy()
    print("|mean| of the flipped columns %.3g, bound %.3g" % (np.abs(mean[sign < 0]).max(), bound))
    assert np.abs(mean[sign < 0]).max() <= bound and np.abs(mean[sign > 0]).max() > 1e-3
    # the priming rollout's merge is over rows and images as well
    # (the priming rollout is not returned: the rows its merge summed are read where the statistics take them)
    primed = _agent("augment", n=64, normalize_obs=True)
    merged, moments = [], primed.obs_norm.moments
    primed.obs_norm.moments = lambda x: (merged.append(x.clone()), moments(x))[1]
    primed.collect()
    assert primed.obs_norm.count == rows and len(merged) == 1 and merged[0].shape[0] == rows
    assert np.array_equal(bits(merged[0][rows // 2:]), bits(mirror_rows(merged[0][:rows // 2], src, sign)))
    assert np.abs(primed.obs_norm.mean.numpy()[sign < 0]).max() <= rows * 2.0 ** -52 * float(merged[0].abs().max())


def test_refusals():
    with pytest.raises(ValueError, match="unknown symmetry"):
        _agent("mirror")
    with pytest.raises(ValueError, match="mirror_map"):
        _agent("augment", env=MirrorToyEnv(16, with_map=False))
    env = MirrorToyEnv(16)
    env.critic_obs_dim = 12
    with pytest.raises(ValueError, match="asymmetric_critic"):
        _agent("augment", env=env, asymmetric_critic=True)
    with pytest.raises(RuntimeError, match="symmetry"):
        plain = _agent(None)
        plain.augment(plain.collect())


def test_on_a_gpu_a_missing_policy_library_is_an_error_not_a_torch_path(monkeypatch, tmp_path):
    """the maps of an agent on a GPU take the kernel; without libroboy_policy.so they raise what every other user of the library
    raises - on the torch path too - and never hand out the torch statement silently.  On the CPU the statement is the path."""
    from gym_roboy_amd import _policy_native as pn
    from gym_roboy_amd.ppo import _MirrorMaps
    maps = MirrorToyEnv(4).mirror_map()
    on_cpu = _MirrorMaps(maps, 9, 8, "cpu")
    assert on_cpu.kernel_applies() is False
    monkeypatch.setattr(pn, "_LIB", None)
    monkeypatch.setenv("ROBOY_POLICY_LIB", str(tmp_path / "no_such_library.so"))
    assert on_cpu.kernel_applies() is False                                    # the CPU never asks for the library
    on_gpu = _MirrorMaps(maps, 9, 8, "cpu")
    on_gpu.device = torch.device("cuda")                                       # (the question is asked of the device's type alone)
    with pytest.raises(RuntimeError, match="not found"):
        on_gpu.kernel_applies()
    with pytest.raises(RuntimeError, match="not found"):                       # ... every time, not only the first
        on_gpu.kernel_applies()


def test_checkpoint_has_the_key_only_when_the_option_is_set(tmp_path):
    a, b = _agent("augment"), _agent(None)
    a.save(str(tmp_path / "a.pt")); b.save(str(tmp_path / "b.pt"))
    ca, cb = torch.load(str(tmp_path / "a.pt")), torch.load(str(tmp_path / "b.pt"))
    assert ca["symmetry"] == "augment" and "symmetry" not in cb
    assert sorted(set(ca) - {"symmetry"}) == sorted(cb)
    _agent("augment").load(str(tmp_path / "a.pt"))
    _agent(None).load(str(tmp_path / "b.pt"))
    with pytest.raises(ValueError, match="symmetry"):
        _agent(None).load(str(tmp_path / "a.pt"))
    with pytest.raises(ValueError, match="symmetry"):
        _agent("augment").load(str(tmp_path / "b.pt"))


def test_symmetry_gap_on_the_cpu_is_the_torch_expression():
    agent = _agent("augment")
    roll = agent.collect()
    src, sign, act_src = agent.env.mirror_map()
    obs = roll["obs"].reshape(-1, 9)[:50]
    with torch.no_grad():
        mu, mu_m = agent.policy.dist(obs).mean, agent.policy.dist(mirror_rows(obs, src, sign)).mean
        v, v_m = agent.policy.value(obs), agent.policy.value(mirror_rows(obs, src, sign))
    d = mu_m - mirror_rows(mu, act_src)
    gap = agent.symmetry_gap(roll, max_rows=50)
    assert gap == {"action": ((d * d).sum(-1).mean() / 8).item(), "value": (v_m - v).abs().mean().item()}
    assert gap["action"] > 0 and gap["value"] > 0


# ---- the ABI ----
def test_new_symbols_are_declared_and_exported():
    from gym_roboy_amd import _native as nat, _policy_native as pn
    for header, name, sigs, lib in (("roboy_sim.h", "rb_mirror_info", nat.SIGNATURES, nat.load()),
                                    ("roboy_policy.h", "rp_mirror_rows_dev", pn.SIGNATURES, pn.load())):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert re.search(r"\bint %s\s*\(" % name, text) and name in sigs and hasattr(lib, name)
    assert nat.load().rb_abi_version() == 6 and pn.load().rp_abi_version() == 5
    # argument errors are reported, not fatal (no GPU is touched in front of them)
    lib = pn.load()
    assert lib.rp_mirror_rows_dev(None, None, None, 4, 9, None, None, None) == -1 and b"null" in lib.rp_last_error()
    one = 16
    assert lib.rp_mirror_rows_dev(one, None, 2 * one, 4, 129, one, one, None) == -1 and b"width" in lib.rp_last_error()
    assert lib.rp_mirror_rows_dev(one, None, 2 * one, 4, 0, one, one, None) == -1
    assert lib.rp_mirror_rows_dev(one, None, 2 * one, -1, 9, one, one, None) == -1 and b"rows" in lib.rp_last_error()
    assert lib.rp_mirror_rows_dev(one, None, one, 4, 9, one, one, None) == -1
    # overlapping arrays of rows x width floats are refused, partial overlaps included; only plain == src is allowed
    src, far, n = 1 << 20, 1 << 24, 4 * 9 * 4
    for plain, mirror, word in ((None, src + 4, b"source"), (None, src + n - 4, b"source"), (None, src - n + 4, b"source"),
                                (src + 8, far, b"plain rows overlap their source"), (far + n - 4, far, b"plain and the mirrored"),
                                (src, src + n - 4, b"source")):
        assert lib.rp_mirror_rows_dev(src, plain, mirror, 4, 9, one, one, None) == -1 and word in lib.rp_last_error(), (plain, mirror)
    assert lib.rp_mirror_rows_dev(one, None, 2 * one, 0, 9, one, one, None) == 0            # no rows: nothing is launched
    assert nat.load().rb_mirror_info(None, None, None, None) == nat.RB_EINVAL


def test_the_mirror_kernel_needs_no_scratch():
    import code_object_meta as com
    metas = [v for name, v in com.kernel_metadata(os.path.join(ROOT, "gym_roboy_amd", "csrc", "libroboy_policy.so")).items()
             if "mirror_rows_kernel" in name]
    assert len(metas) == 1, metas
    k = metas[0]
    print("mirror_rows_kernel", {f: k.get(f) for f in com.FIELDS})
    assert k["private_segment_fixed_size"] == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
    assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] <= 17 * 1024
