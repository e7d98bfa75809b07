"""Mirror-symmetry augmentation on the GPU: the streaming kernel against its numpy statement bit for bit at every
alignment its outputs can have, the library's word on the robot's mirror plane, the env step's equivariance THROUGH the kernels
(two envs, one the mirror image of the other), and PPO(symmetry="augment") - torch and fused paths, eager and captured - against an
agent without the option that is fed the concatenated rollout."""
import ctypes
import os

import numpy as np
import pytest

from gym_roboy_amd.envs.symmetry import mirror_rows
from symmetry_util import AUGMENTED, JOINT_SIGN, MSJ_IMAGE, bits, concatenated, is_involution, random_involution_map, twin_case

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
PAD = 64


# ---- rp_mirror_rows_dev ----
def _mirror_launch(src, plain, mirror, rows, width, col_src, col_sign):
    import torch
    from gym_roboy_amd import _policy_native as pn
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    pn.check(pn.load().rp_mirror_rows_dev(ptr(src), ptr(plain), ptr(mirror), rows, width, ptr(col_src), ptr(col_sign),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("plain_mode", ["null", "src", "separate"])
@pytest.mark.parametrize("width", [1, 9, 25, 95])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 321])
def test_mirror_rows_kernel_is_the_statement_bit_for_bit(rows, width, plain_mode):
    """The outputs are the two halves of ONE [2 rows, width] allocation (the mirrored half of 321 x 9 starts 4-byte aligned and no
    more) between sentinels; with plain == src the source IS the first half."""
    import torch
    rng = np.random.default_rng(1000 * rows + width)
    col_src, col_sign = random_involution_map(width, rng)
    x = rng.standard_normal((rows, width)).astype(np.float32)
    x[rng.random((rows, width)) < 0.1] = 0.0                      # zeros: a flipped 0 must come out as -0
    x[0, 0] = -0.0
    want = mirror_rows(x, col_src, col_sign)
    n = rows * width
    buf = torch.full((PAD + 2 * n + PAD,), SENTINEL, device="cuda")
    first, second = buf[PAD:PAD + n].view(rows, width), buf[PAD + n:PAD + 2 * n].view(rows, width)
    if (rows, width) == (321, 9):
        assert first.data_ptr() % 16 == 0 and second.data_ptr() % 16 == 4     # the misaligned half the kernel must serve
    if plain_mode == "src":
        first.copy_(torch.from_numpy(x))
        src, plain = first, first
    else:
        src = torch.from_numpy(x).cuda()
        plain = first if plain_mode == "separate" else None
    _mirror_launch(src, plain, second, rows, width, torch.from_numpy(col_src).cuda(), torch.from_numpy(col_sign).cuda())
    torch.cuda.synchronize()
    assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + 2 * n:] == SENTINEL).all()
    assert np.array_equal(bits(second), bits(want))
    if plain_mode == "null":
        assert (first == SENTINEL).all()                          # not written
    else:
        assert np.array_equal(bits(first), bits(x))
    assert np.array_equal(bits(src), bits(x))                     # the source is only read


@pytest.mark.parametrize("gap", [1, 3, 64])
@pytest.mark.parametrize("rows, width", [(1, 1), (63, 9), (65, 25), (321, 9), (321, 95), (1100, 9)])
def test_neither_output_runs_into_the_other(rows, width, gap):
    """the adjacent halves above leave the seam between the plain and the mirrored output unguarded (an overrun of the plain write is
    overwritten by the mirror's): here sentinels stand in front of, BETWEEN and behind the two outputs, the gap of 1 or 3 floats
    also moving the second output over every alignment"""
    import torch
    rng = np.random.default_rng(7 * rows + width + gap)
    col_src, col_sign = random_involution_map(width, rng)
    x = rng.standard_normal((rows, width)).astype(np.float32)
    n = rows * width
    buf = torch.full((PAD + n + gap + n + PAD,), SENTINEL, device="cuda")
    first, second = buf[PAD:PAD + n].view(rows, width), buf[PAD + n + gap:PAD + 2 * n + gap].view(rows, width)
    _mirror_launch(torch.from_numpy(x).cuda(), first, second, rows, width, torch.from_numpy(col_src).cuda(), torch.from_numpy(col_sign).cuda())
    torch.cuda.synchronize()
    assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + n:PAD + n + gap] == SENTINEL).all() and (buf[PAD + 2 * n + gap:] == SENTINEL).all()
    assert np.array_equal(bits(first), bits(x)) and np.array_equal(bits(second), bits(mirror_rows(x, col_src, col_sign)))


def test_mirror_rows_kernel_over_many_workgroups_and_the_widest_row():
    """more rows than one workgroup's run at every width class, 128 columns (the limit), and a run that ends inside a tile"""
    import torch
    for rows, width in ((5003, 8), (1031, 128), (9001, 1), (517, 95)):
        rng = np.random.default_rng(rows)
        col_src, col_sign = random_involution_map(width, rng)
        x = rng.standard_normal((rows, width)).astype(np.float32)
        n = rows * width
        buf = torch.full((PAD + 1 + 2 * n + PAD,), SENTINEL, device="cuda")          # (+ 1: both halves off the 16-byte grid)
        first, second = buf[PAD + 1:PAD + 1 + n].view(rows, width), buf[PAD + 1 + n:PAD + 1 + 2 * n].view(rows, width)
        _mirror_launch(torch.from_numpy(x).cuda(), first, second, rows, width, torch.from_numpy(col_src).cuda(), torch.from_numpy(col_sign).cuda())
        torch.cuda.synchronize()
        assert (buf[:PAD + 1] == SENTINEL).all() and (buf[PAD + 1 + 2 * n:] == SENTINEL).all()
        assert np.array_equal(bits(first), bits(x)) and np.array_equal(bits(second), bits(mirror_rows(x, col_src, col_sign)))


# ---- rb_mirror_info ----
def _turned(msj_robot):
    from test_mirror_pairs import _rotated_msj
    desc = _rotated_msj()

    class Turned(type(msj_robot)):
        @classmethod
        def get_description(cls):
            return desc
    return Turned()


def test_mirror_info(msj_robot):
    from gym_roboy_amd import _native as nat
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    from test_physics_gpu import _ball_joint_robot
    sim = HipBatchSimulation(msj_robot, 64)
    info = sim.mirror_info()
    assert info["plane"] == 0 and info["joint_sign"].tolist() == [-1, 1, -1] and info["tendon_image"].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    sim.select_kernel(1)                                           # whatever kernel form is selected
    again = sim.mirror_info()
    assert again["plane"] == 0 and np.array_equal(again["joint_sign"], info["joint_sign"]) and np.array_equal(again["tendon_image"], info["tendon_image"])
    sim.close()
    sim = HipBatchSimulation(_turned(msj_robot), 64)
    info = sim.mirror_info()
    assert info["plane"] == 1 and info["joint_sign"].tolist() == [1, -1, -1]
    assert is_involution(info["tendon_image"], np.ones(8)) and not np.any(info["tendon_image"] == np.arange(8))
    sim.close()
    for robot in (UpperBodyRobot(), _ball_joint_robot(msj_robot, 8, 4), _ball_joint_robot(msj_robot, 6, 5)):
        sim = HipBatchSimulation(robot, 16)
        with pytest.raises(nat.NativeError, match="mirror plane"):
            sim.mirror_info()
        assert b"mirror plane" in nat.load().rb_last_error()
        plane, sign, image = ctypes.c_int32(), (ctypes.c_int32 * 32)(), (ctypes.c_int32 * 64)()
        assert nat.load().rb_mirror_info(sim.handle, ctypes.byref(plane), sign, image) == nat.RB_EUNSUPPORTED
        sim.close()


def test_env_mirror_map_is_the_row_map_of_the_env_as_configured(msj_robot):
    from gym_roboy_amd import _native as nat
    from gym_roboy_amd.envs.robots import UpperBodyRobot
    from gym_roboy_amd.envs.symmetry import row_mirror_map
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    for kw in ({}, {"tendon_obs": ("force", "length")}, {"action_obs": 2, "tendon_obs": ("rate",)}):
        env = RoboyVecEnv(msj_robot, 8, **kw)
        got = env.mirror_map()
        want = row_mirror_map(3, 8, JOINT_SIGN[0], MSJ_IMAGE, env.tendon_obs, env.action_obs)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[0].shape == (env.obs_dim,)
        env.close()
    env = RoboyVecEnv(UpperBodyRobot(), 8)
    with pytest.raises(nat.NativeError, match="mirror plane"):
        env.mirror_map()
    env.close()


# ---- the env step is equivariant through the kernels ----
STATE_TOL = 2 * 2e-5              # both sides lie within tests/test_physics_gpu.py's ball-joint tolerance of one fp64 result


@pytest.mark.parametrize("config", ["bare", "tendon", "delay"])
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_env_step_is_equivariant_through_the_kernels(msj_robot, integ, config):
    from env_obs_util import column_tolerances
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from oracle.physics_np import TendonRobotOracle
    desc, q, qd, acts, goal = twin_case(msj_robot)
    n = len(q)
    kw = {"bare": {}, "tendon": {"tendon_obs": ("length", "force")}, "delay": {"action_delay": 2, "action_obs": 2}}[config]
    steps = 3 if config == "delay" else 1
    S = JOINT_SIGN[0].astype(np.float32)
    envs = [RoboyVecEnv(msj_robot, n, integrator=integ, **kw) for _ in range(2)]
    try:
        src, sign, act_src = envs[0].mirror_map()
        outs = []
        for env, twin in zip(envs, (False, True)):
            env.reset()
            env.sim.set_state(q * S if twin else q, qd * S if twin else qd)
            env.set_goal(goal * S if twin else goal, step_num=np.ones(n, np.uint32))
            outs.append([env.step(np.ascontiguousarray(a[:, act_src]) if twin else a)[:3] for a in acts[:steps]])
        tol = np.full(envs[0].obs_dim, STATE_TOL)
        tol[6:9] = 0.0                                                               # the goal columns: S g exactly
        if config == "tendon":
            tol[9:] = 2 * column_tolerances(TendonRobotOracle(desc), ("length", "force"))
        elif config == "delay":
            tol[9:] = 0.0                                                            # the action blocks: bit-equal
        for t, ((obs_a, rew_a, done_a), (obs_b, rew_b, done_b)) in enumerate(zip(*outs)):
            want = mirror_rows(obs_a, src, sign)
            err = np.abs(obs_b.astype(np.float64) - want)
            print("%s %s step %d: state columns %.3g (tol %.3g), behind them %.3g, reward rel %.3g"
                  % (config, integ, t, err[:, :6].max(), STATE_TOL, err[:, 9:].max() if err.shape[1] > 9 else 0.0,
                     np.abs(rew_b / rew_a - 1).max()))
            assert np.all(err <= tol), (t, (err - tol).max())
            exact = tol == 0.0
            assert np.array_equal(bits(obs_b[:, exact]), bits(want[:, exact]))
            assert np.all(np.abs(rew_b - rew_a) <= 1e-4 * np.abs(rew_a))
            assert np.array_equal(done_a, done_b) and not done_a.any()
        assert np.abs(outs[0][-1][0][:, :6]).max() > 0.05                            # the envs moved: not a comparison of zeros
        if config == "delay":
            assert np.abs(outs[0][-1][0][:, 9:]).max() > 0.5                          # the action blocks hold actions
    finally:
        for env in envs:
            env.close()


# ---- PPO ----
N_ENVS, N_STEPS = 256, 8


def _agents(msj_robot, fused, graphs, env_kw=None, **kw):
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env = RoboyVecEnv(msj_robot, N_ENVS, seed=3, **(env_kw or {}))
    mk = lambda symmetry: PPO(env, n_steps=N_STEPS, nminibatches=2, noptepochs=2, device="cuda", seed=4, use_graphs=graphs,
                              fused_policy=fused, fused_update=fused, symmetry=symmetry, **kw)
    return env, mk("augment"), mk(None)


def _orders(n2, epochs, seed=11):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n2, generator=g).cuda() for _ in range(epochs)]


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_ppo_update_is_the_update_on_the_concatenated_rollout(msj_robot, fused, graphs):
    import torch
    env, a, b = _agents(msj_robot, fused, graphs, diagnostics=True)
    try:
        assert (a._fgrad is not None) == fused and (a._fused is not None) == fused
        for p, q in zip(a.policy.parameters(), b.policy.parameters()):
            assert torch.equal(p, q)
        roll = a.collect()
        assert (a._rollout_graph is not None) == graphs
        maps = env.mirror_map()
        want = concatenated(roll, maps)
        flat = a.augment(roll)
        n = N_ENVS * N_STEPS
        for k in AUGMENTED:
            assert flat[k].shape[0] == 2 * n and np.array_equal(bits(flat[k]), bits(want[k][0])), k
        assert a._mirror.kernel_applies()                                     # the halves came from the kernel
        before = [p.detach().clone() for p in a.policy.parameters()]
        orders = _orders(2 * n, 2)
        sa = a.update(roll, sample_orders=orders)
        sb = b.update({k: v.clone() for k, v in want.items()}, sample_orders=orders)
        assert sa == sb and "approx_kl" in sa and "clip_frac" in sa, (sa, sb)
        for p, q in zip(a.policy.parameters(), b.policy.parameters()):
            assert np.array_equal(bits(p), bits(q))
        assert any(not torch.equal(p, p0) for p, p0 in zip(a.policy.parameters(), before))
        if fused:
            assert a._fadam.t == b._fadam.t == 4
            assert np.array_equal(bits(a._fadam.m), bits(b._fadam.m)) and np.array_equal(bits(a._fadam.v), bits(b._fadam.v))
        # a second rollout and update run (graph mode: a replay; the buffers of augment are reused)
        roll = a.collect()
        stats = a.update(roll)
        assert np.isfinite(stats["loss"]) and a.num_timesteps == 2 * n
    finally:
        env.close()


@pytest.mark.parametrize("fused", [False, True])
def test_observation_statistics_commute_with_the_mirror(msj_robot, fused):
    env, a, _ = _agents(msj_robot, fused, True, env_kw={"tendon_obs": ("length", "force")}, normalize_obs=True)
    try:
        src, sign, _ = env.mirror_map()
        roll = a.collect()                                                    # primed: one merge over rows and images
        rows = 2 * N_ENVS * N_STEPS
        assert a.obs_norm.count == rows
        for merges in (1, 2):
            mean = a.obs_norm.mean.cpu().numpy()
            norm = a.obs_norm.norm.cpu().numpy()
            partner = src != np.arange(len(src))
            assert partner.sum() == 16
            ulp = np.spacing(np.abs(norm).astype(np.float32))
            gap = np.abs(norm[:, src] - norm)
            print("merge %d: |mean| of the flipped columns %.3g, partner columns %.3g ulp" % (merges, np.abs(mean[sign < 0]).max(), (gap / ulp)[:, partner].max()))
            assert np.all(gap[:, partner] <= 2 * ulp[:, partner])
            if merges == 1:
                # the fp64 summation bound of one merge; max|x|: the joint columns stay inside the joint and velocity limits
                desc = msj_robot.get_description()
                assert np.abs(mean[sign < 0]).max() <= rows * 2.0 ** -52 * float(max(np.abs(desc.q_lo).max(), np.abs(desc.q_hi).max(), np.max(desc.qd_max)))
                a.update(roll)
                assert a.obs_norm.count == 2 * rows
    finally:
        env.close()


@pytest.mark.parametrize("fused", [False, True])
def test_symmetry_gap(msj_robot, fused):
    import torch
    env, a, _ = _agents(msj_robot, fused, False)
    try:
        src, sign, act_src = env.mirror_map()
        roll = a.collect()
        rows = 1000
        obs = roll["obs"].reshape(-1, 9)[:rows].contiguous()
        m_obs = mirror_rows(obs, src, sign).contiguous()

        def step(o):
            if not fused:
                with torch.no_grad():
                    return a.policy.dist(o).mean, a.policy.value(o)
            z = lambda *shape: torch.empty(shape, device="cuda")
            act, mean, logp, val = z(rows, 8), z(rows, 8), z(rows), z(rows)
            a._fused.act_into(o, act, logp, val, deterministic=True, mean=mean)
            return mean, val
        (mu, v), (mu_m, v_m) = step(obs), step(m_obs)
        d = mu_m - mirror_rows(mu, act_src)
        want = {"action": ((d * d).sum(-1).mean() / 8).item(), "value": (v_m - v).abs().mean().item()}
        got = a.symmetry_gap(roll, max_rows=rows)
        assert got == want and got["action"] > 0 and got["value"] > 0, (got, want)
        # an equivariant actor and an invariant critic by construction: a zero last action layer, and a value net whose first layer
        # does not read the columns the mirror flips (the bare row has no partner columns) - the gap is exactly 0
        with torch.no_grad():
            a.policy.pi[4].weight.zero_(); a.policy.pi[4].bias.zero_()
            a.policy.vf[0].weight[:, torch.from_numpy(sign < 0).cuda()] = 0.0
        assert a.symmetry_gap(roll) == {"action": 0.0, "value": 0.0}
    finally:
        env.close()


def test_train_parallel_round_trip(tmp_path, capsys):
    import torch
    from gym_roboy_amd import train_parallel
    out = str(tmp_path / "results")
    argv = ["256", out, "--rounds", "1", "--steps-per-round", str(256 * 8 * 2), "--n-steps", "8", "--symmetry", "augment"]
    agent = train_parallel.main(argv)
    text = capsys.readouterr().out
    assert "symmetry_gap_action" in text
    assert agent.symmetry == "augment" and agent._rollout_graph is not None and agent._mirror.kernel_applies()
    ck = torch.load(os.path.join(out, "model.pkl"))
    assert ck["symmetry"] == "augment"
    steps = agent.num_timesteps
    agent.env.close()
    again = train_parallel.main(argv)                                # resumes from the checkpoint
    assert again.num_timesteps == 2 * steps
    again.env.close()
    with pytest.raises(ValueError, match="symmetry"):                # an agent without the option refuses it
        train_parallel.main(argv[:-2])
