"""Episode-end codes of the fused env step (csrc/roboy_sim.hip: done_kind_kernel; include/roboy_sim.h: rb_env_done_kind_*) and the
rollout tail that bootstraps truncated episodes (csrc/rollout_tail_kernel.inc: rollout_tail_boot_kernel; include/roboy_policy.h:
rp_rollout_tail_boot_dev), DESIGN.md §17, on the GPU.

Env layer: a twin env without the option runs the same seed and actions.  With the goal bonus on the reward is positive exactly when
the goal was reached (every other term is <= -1), so the twin's (done, reward) say what every code must be; obs, reward and
`done != 0` are compared to the bit.  The scenario (tests/truncation_ref.py) is qualified on the host model by
tests/test_truncation_cpu.py and its non-vacuity is asserted again here.

Tail kernel.  rew, done, the sums and the carry: bit-equal to rp_rollout_tail_dev's on the same inputs.  adv / ret: the rule of
tests/test_reward_norm_gpu.py - at most 4 x the CPU float32 loop's distance from float64, floor 1e-6 max |ref|, both fed the same
r~; the loop and the reference are here the coded recurrence (ppo.gae_boot, truncation_ref.gae_boot64) - plus the two extra roundings
of a truncated step, fl32(gamma32 v) and fl32(r~ + that): each within 2^-24 of its result, entering delta_t of a step behind which
nothing feeds it (nonterminal = 0) and reaching the advantages before it with weights (gamma lam)^k <= 1, one source per episode:
2^-24 max (|gamma v| + |r~ + gamma v|) over the truncated steps (truncation_ref.boot_extra_bound)."""
import ctypes
import functools

import numpy as np
import pytest

import reward_norm_ref as rref
import truncation_ref as tr
from test_reward_norm_cpu import raw_rewards

pytestmark = pytest.mark.gpu

GAMMA, LAM, SCALE = 0.99, 0.95, 0.01
SEED = 3


# ---------------------------------------------------------------- the env layer
def _make(robot_name, n, report, integrator="euler"):
    from gym_roboy_amd.envs.robots import MsjRobot, UpperBodyRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    robot = MsjRobot() if robot_name == "msj" else UpperBodyRobot()
    return RoboyVecEnv(robot, n, seed=SEED, max_episode_length=tr.MAX_LEN, is_agent_getting_bonus_for_reaching_goal=True,
                       integrator=integrator, report_truncation=report)


def _prepare(vec, kernel):
    """reset, the scenario's goals and counters -> (actions, groups)"""
    if kernel is not None:
        vec.sim.select_kernel(kernel)
    obs0 = vec.reset()
    goal, step_num, actions, groups = tr.scenario(vec.num_envs, vec.n_q, vec.n_t, obs0[:, 2 * vec.n_q:])
    vec.set_goal(goal, step_num=step_num)
    return actions, groups


def _run_numpy(vec, kernel=None, form=None):
    """the scenario through step(): per step (obs, rew, done bools, the raw done words, truncated() or None)"""
    actions, groups = _prepare(vec, kernel)
    if form is not None:
        assert form in vec.sim.dispatch("env_step")["id"], vec.sim.dispatch("env_step")["id"]
    out = []
    for a in actions:
        obs, rew, done, info = vec.step(a)
        assert done.dtype == bool and info[0] == {}
        words = vec.sim.download(vec._d_done, (vec.num_envs,), np.uint32)
        out.append((obs, rew, done, words, vec.truncated() if vec.report_truncation else None))
    return out, groups


def _assert_twin(got, twin, groups, at_least=8):
    codes = []
    for t, ((obs, rew, done, words, trunc), (obs0, rew0, done0, words0, _)) in enumerate(zip(got, twin)):
        assert obs.tobytes() == obs0.tobytes() and rew.tobytes() == rew0.tobytes(), t
        assert np.array_equal(done, done0) and np.array_equal(words != 0, words0 != 0) and set(np.unique(words0)) <= {0, 1}
        want = tr.expected_codes(done0, rew0)
        assert np.array_equal(words, want), t                      # 1 <=> twin done and rew > 0, 2 <=> twin done and rew < 0
        assert not (done0 & (rew0 == 0)).any()
        assert np.array_equal(trunc, want == tr.TRUNCATED) and trunc.dtype == bool
        codes.append(words)
    tr.assert_every_code_occurs(np.stack(codes), groups, at_least)           # the coincidence envs read 1 (step 0, group 1)
    return np.stack(codes)


@pytest.mark.parametrize("case", ["env_per_lane_320", "lane_pair_320", "small_batch_200", "rk4_320", "upper_body_64"])
def test_codes_match_the_twin(case):
    robot, n, kernel, form, integ = {"env_per_lane_320": ("msj", 320, 1, "env_per_lane", "euler"),
                                     "lane_pair_320": ("msj", 320, 5, "lane_pair", "euler"),
                                     "small_batch_200": ("msj", 200, None, "tendon_per_lane", "euler"),
                                     "rk4_320": ("msj", 320, 1, "env_per_lane", "rk4"),
                                     "upper_body_64": ("upper", 64, None, None, "euler")}[case]
    runs = []
    for report in (True, False):
        vec = _make(robot, n, report, integ)
        try:
            runs.append(_run_numpy(vec, kernel, form))
            if report:
                stats = vec.stats()
        finally:
            vec.close()
    (got, groups), (twin, _) = runs
    codes = _assert_twin(got, twin, groups)
    assert stats["n_goal_reached"] == (codes == tr.TERMINATED).sum() and stats["n_episodes"] == (codes != 0).sum()


def test_sub_ranges_on_two_streams():
    """576 envs stepped as [0, 256) and [256, 576) on two streams: each range's codes are written behind its own env-step kernel"""
    import torch
    n = 576
    runs = []
    for report in (True, False):
        vec = _make("msj", n, report)
        try:
            actions, groups = _prepare(vec, 1)
            assert vec.range_capable()
            vec.sim.synchronize()
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            act = torch.from_numpy(actions).cuda()
            obs, rew = torch.empty(n, vec.obs_dim, device="cuda"), torch.empty(n, device="cuda")
            done = torch.zeros(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            out = []
            for t in range(tr.STEPS):
                for (lo, cnt), st in (((0, 256), s1), ((256, n - 256), s2)):
                    vec.step_range_dev(lo, cnt, st.cuda_stream, act[t].data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr())
                s1.synchronize(); s2.synchronize()
                words = done.cpu().numpy().astype(np.uint32)
                out.append((obs.cpu().numpy(), rew.cpu().numpy(), words != 0, words, vec.truncated() if report else None))
            runs.append(out)
        finally:
            vec.close()
    _assert_twin(runs[0], runs[1], groups)


def test_truncated_with_torch_inputs_and_the_kind_plane():
    import torch
    from gym_roboy_amd import _native as nat
    n = 320
    vec = _make("msj", n, True)
    try:
        actions, groups = _prepare(vec, 1)
        codes = []
        for a in actions:
            obs, rew, done, _ = vec.step(torch.from_numpy(a).cuda())
            trunc = vec.truncated()
            assert trunc.is_cuda and trunc.dtype == torch.bool and done.dtype == torch.bool
            kind = ctypes.c_void_p()
            nat.check(vec.sim._lib.rb_env_done_kind_ptr(vec.sim.handle, ctypes.byref(kind)))
            torch.cuda.synchronize()
            plane = vec.sim.download(kind.value, (n,), np.uint32)
            want = tr.expected_codes(done.cpu().numpy(), rew.cpu().numpy())
            assert np.array_equal(plane, want) and np.array_equal(trunc.cpu().numpy(), want == 2)
            codes.append(plane)
        tr.assert_every_code_occurs(np.stack(codes), groups)
    finally:
        vec.close()


def test_stats_reset_keeps_the_codes_right():
    """After stats(reset=True) - which zeroes the goal counters the codes are derived from - an env that then times out reads 2 and an
    env that then reaches its goal reads 1, for envs that had reached a goal before the reset and for envs that had not."""
    n = 320
    runs = []
    for report in (True, False):
        vec = _make("msj", n, report)
        try:
            actions, groups = _prepare(vec, 1)
            out = []
            obs, rew, done, _ = vec.step(actions[0])                 # groups 0 and 1 reach their goals: their counters stand at 1
            assert done[groups != 2].all() and (rew[groups != 2] > 0).all()
            assert vec.stats(reset=True)["n_goal_reached"] == (groups != 2).sum()
            # group 0 (one goal behind it) and half of group 2 (none) are put at their goal again, the others run into the limit
            again = (groups == 0) | ((groups == 2) & (np.arange(n) % 2 == 0))
            goal, q, qd = obs[:, 6:9].copy(), obs[:, 0:3].copy(), obs[:, 3:6].copy()
            goal[again] = 0.0; q[again] = 0.0; qd[again] = 0.0     # at rest in the zero pose, which is their goal
            acts = actions[1:7].copy()
            acts[0, again] = 0.0
            vec.sim.set_state(q, qd)
            vec.set_goal(goal, step_num=np.where(groups == 2, 2, 1).astype(np.uint32))
            for a in acts:
                o, r, d, _ = vec.step(a)
                out.append((o, r, d, vec.sim.download(vec._d_done, (n,), np.uint32), vec.truncated() if report else None))
            runs.append(out)
        finally:
            vec.close()
    got, twin = runs
    codes = []
    for (obs, rew, done, words, trunc), (obs0, rew0, done0, _, _) in zip(got, twin):
        assert obs.tobytes() == obs0.tobytes() and rew.tobytes() == rew0.tobytes() and np.array_equal(done, done0)
        assert np.array_equal(words, tr.expected_codes(done0, rew0)) and np.array_equal(trunc, words == 2)
        codes.append(words)
    codes = np.stack(codes)
    for had_goal in (groups != 2, groups == 2):
        assert ((codes == 1).any(axis=0) & had_goal).sum() >= 8 and ((codes == 2).any(axis=0) & had_goal).sum() >= 8
    assert (codes[0, again] == 1).all()


def test_a_disabled_handle_returns_an_error_code():
    from gym_roboy_amd import _native as nat
    vec = _make("msj", 64, False)
    try:
        lib, h = vec.sim._lib, vec.sim.handle
        kind = ctypes.c_void_p()
        assert lib.rb_env_done_kind_ptr(h, ctypes.byref(kind)) == nat.RB_EINVAL and b"not enabled" in lib.rb_last_error()
        assert lib.rb_env_done_kind_ptr(h, None) == nat.RB_EINVAL
        with pytest.raises(RuntimeError, match="report_truncation"):
            vec.truncated()
        # enabled and disabled again: the error again, and the done words are 0 / 1 as before
        assert lib.rb_env_done_kind_configure(h, 1) == nat.RB_OK and lib.rb_env_done_kind_ptr(h, ctypes.byref(kind)) == nat.RB_OK
        assert lib.rb_env_done_kind_configure(h, 0) == nat.RB_OK and lib.rb_env_done_kind_ptr(h, ctypes.byref(kind)) == nat.RB_EINVAL
        actions, _ = _prepare(vec, 1)
        words = []
        for a in actions[:6]:
            vec.step(a)
            words.append(vec.sim.download(vec._d_done, (64,), np.uint32))
        assert set(np.unique(np.stack(words))) == {0, 1}
    finally:
        vec.close()


# ---------------------------------------------------------------- the tail kernel
SHAPES = [(1, 1), (1, 65), (2, 64), (5, 257), (37, 1000), (128, 4097)]
CASES = [(T, N, dones, "half") for T, N in SHAPES for dones in rref.DONE_PATTERNS] + \
        [(T, N, "random", kind) for T, N in SHAPES for kind in tr.CODE_PATTERNS[1:]]


def _scratch(lib):
    import torch
    return torch.zeros(int(lib.rp_rollout_tail_scratch_doubles()), dtype=torch.float64, device="cuda")


def _call(fn, raw, code, val, last, carry, scratch, norm2=None, shift=None, clip=float("inf"), gamma=GAMMA, n_steps=None, outs=None):
    """one of the two tails (device tensors; None = a null pointer) -> (return code, rew, done, adv, ret, sums)"""
    import torch
    T, N = val.shape
    outs = outs or [torch.empty(T, N, device="cuda") for _ in range(4)]
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = fn(ptr(raw), ptr(code), ptr(val), ptr(last), SCALE, ptr(norm2), clip, ptr(shift), gamma, LAM, ptr(carry),
            *[ptr(o) for o in outs], ptr(sums), ptr(scratch), T if n_steps is None else n_steps, N,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (rc, *outs, sums)


def _inputs(T, N, dones, kind, seed):
    rng = np.random.default_rng(seed)
    raw, done = raw_rewards(rng, T, N), rref.done_pattern(dones, T, N, rng)
    val, last = rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    code = tr.codes_of(done, kind, rng)
    return raw, code, val, last, rng.normal(0.0, 3.0, N)


def _assert_adv_ret(adv, ret, r_tilde, val, code, last, what):
    import torch
    from gym_roboy_amd.ppo import gae_boot
    a64, r64 = tr.gae_boot64(r_tilde, val, code, last, GAMMA, LAM)
    a32, r32 = gae_boot(*[torch.from_numpy(np.ascontiguousarray(x)) for x in (r_tilde, val, code, last)], GAMMA, LAM)
    extra = tr.boot_extra_bound(r_tilde, val, code, GAMMA)
    for name, got, f32, want in (("adv", adv, a32, a64), ("ret", ret, r32, r64)):
        e32 = np.abs(f32.double().numpy() - want).max()
        err = np.abs(got.astype(np.float64) - want).max()
        bound = max(4.0 * e32, 1e-6 * np.abs(want).max()) + extra
        print("%s %s: fp32 loop %.3g, kernel %.3g, bound %.3g (extra %.3g), max |ref| %.3g" % (what, name, e32, err, bound, extra, np.abs(want).max()))
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("T,N,dones,kind", CASES)
def test_boot_tail_matches_float64_and_the_parent_tail(T, N, dones, kind):
    """With statistics (a shift, an rstd, a clamp that cuts) and without (null pointers, no clamp): adv / ret against the float64
    coded recurrence; rew, done, the sums and the carry bit-equal to rp_rollout_tail_dev's fed done = (code != 0)."""
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    raw, code, val, last, carry_in = _inputs(T, N, dones, kind, 7000 * T + N + len(dones) + 10 * len(kind))
    if kind.startswith("truncated") or (dones in ("all", "random") and T * N >= 1000):
        assert (code == 2).any()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_raw, d_code, d_val, d_last = dev(raw), dev(code), dev(val), dev(last)
    d_done01 = dev((code != 0).astype(np.int32))
    scratch = _scratch(lib)
    for stats in (True, False):
        rstd, clip = (np.float32(1.7), 0.05) if stats else (np.float32(1.0), float("inf"))
        kw = {"norm2": torch.tensor([[0.3], [float(rstd)]], device="cuda"), "shift": torch.tensor([0.3], dtype=torch.float64, device="cuda"),
              "clip": clip} if stats else {}
        c_boot, c_par = dev(carry_in), dev(carry_in)
        rc, rew, done, adv, ret, sums = _call(lib.rp_rollout_tail_boot_dev, d_raw, d_code, d_val, d_last, c_boot, scratch, **kw)
        rc_p, rew_p, done_p, adv_p, ret_p, sums_p = _call(lib.rp_rollout_tail_dev, d_raw, d_done01, d_val, d_last, c_par, scratch, **kw)
        assert rc == 0 and rc_p == 0
        assert torch.equal(rew, rew_p) and torch.equal(done, done_p) and torch.equal(sums, sums_p) and torch.equal(c_boot, c_par)
        r_tilde = rref.normalised(rref.scaled(raw, SCALE), rstd, clip) if stats else rref.scaled(raw, SCALE)
        assert np.array_equal(rew.cpu().numpy(), r_tilde) and np.array_equal(done.cpu().numpy(), (code != 0).astype(np.float32))
        if stats and T * N >= 1000:
            assert (np.abs(r_tilde) == np.float32(clip)).any() and (np.abs(r_tilde) < clip).any()
        _assert_adv_ret(adv.cpu().numpy(), ret.cpu().numpy(), r_tilde, val, code, last, "(%d, %d) %s %s stats=%s" % (T, N, dones, kind, stats))
        if (code == 2).any():                                       # the bootstrap is there: the parent's advantages differ
            assert not torch.equal(adv, adv_p)


@pytest.mark.parametrize("T,N,dones", [(1, 65, "all"), (5, 257, "random"), (37, 1000, "random"), (128, 4097, "random"), (37, 1000, "none")])
def test_without_a_truncation_the_boot_tail_is_the_parent_tail_to_the_bit(T, N, dones):
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    rng = np.random.default_rng(T * N)
    raw, done = raw_rewards(rng, T, N), rref.done_pattern(dones, T, N, rng)
    val, last = rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    carry_in = rng.normal(0.0, 3.0, N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [dev(raw), dev(done), dev(val), dev(last)]
    for kw in ({}, {"norm2": torch.tensor([[0.3], [1.7]], device="cuda"), "shift": torch.tensor([0.3], dtype=torch.float64, device="cuda"), "clip": 0.05}):
        ca, cb = dev(carry_in), dev(carry_in)
        a = _call(lib.rp_rollout_tail_boot_dev, *args, ca, _scratch(lib), **kw)
        b = _call(lib.rp_rollout_tail_dev, *args, cb, _scratch(lib), **kw)
        assert a[0] == 0 and b[0] == 0 and torch.equal(ca, cb)
        for x, y in zip(a[1:], b[1:]):
            assert torch.equal(x, y)


def test_boot_tail_argument_errors_are_codes():
    import torch
    from gym_roboy_amd import _policy_native as pn
    lib = pn.load()
    T, N = 5, 65
    raw, code, val, last, _ = _inputs(T, N, "random", "half", 9)
    raw, code, val, last = [torch.from_numpy(a).cuda() for a in (raw, code, val, last)]
    carry, scratch = torch.zeros(N, dtype=torch.float64, device="cuda"), _scratch(lib)
    marks = [torch.full((T, N), -7777.0, device="cuda") for _ in range(4)]
    fn = lib.rp_rollout_tail_boot_dev
    for kw, word in (({"clip": 0.0}, b"clip"), ({"clip": float("nan")}, b"clip"), ({"n_steps": 0}, b"n_steps"), ({"gamma": 1.5}, b"gamma"),
                     ({"gamma": -0.1}, b"gamma")):
        assert _call(fn, raw, code, val, last, carry, scratch, outs=marks, **kw)[0] == -1
        assert word in lib.rp_last_error()
    assert _call(fn, None, code, val, last, carry, scratch, outs=marks)[0] == -1 and b"null" in lib.rp_last_error()
    assert _call(fn, raw, None, val, last, carry, scratch, outs=marks)[0] == -1
    assert _call(fn, raw, code, val, last, carry, None, outs=marks)[0] == -1
    assert _call(fn, raw, code, val, last, None, scratch, outs=marks)[0] == -1
    assert all((m == -7777.0).all() for m in marks) and (carry == 0).all()               # nothing was launched
    assert _call(fn, raw, code, val, last, carry, scratch)[0] == 0                        # and the next call runs


# ---------------------------------------------------------------- PPO
PPO_T, PPO_N, PPO_MAX_LEN = 8, 512, 6
MODES = {"torch_eager": dict(use_graphs=False, fused_policy=False, fused_update=False),
         "fused_eager": dict(use_graphs=False, fused_policy=True, fused_update=True),
         "one_chain": dict(use_graphs=True, fused_policy=True, fused_update=True, rollout_chains=1),
         "two_chains": dict(use_graphs=True, fused_policy=True, fused_update=True, rollout_chains=2)}


@functools.lru_cache(maxsize=None)
def _rollouts(mode, normalize=False):
    """two collect()s of a fresh agent in that mode -> per rollout {name: numpy}, with the value of the last observation; computed
    once and shared by the tests below"""
    import torch
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env = RoboyVecEnv(MsjRobot(), PPO_N, seed=SEED, max_episode_length=PPO_MAX_LEN, report_truncation=True)
    try:
        agent = PPO(env, n_steps=PPO_T, seed=5, reward_scale=SCALE, bootstrap_timeouts=True, normalize_reward=normalize,
                    reward_norm_prime=False, **MODES[mode])
        out = []
        for _ in range(2):
            roll = agent.collect()
            torch.cuda.synchronize()
            with torch.no_grad():
                last = agent.policy.value(agent._obs)
            rec = {k: v.detach().cpu().numpy().copy() for k, v in roll.items()}
            rec["last"] = last.cpu().numpy()
            rec["chains"] = agent.rollout_chains
            out.append(rec)
        return out
    finally:
        env.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_ppo_rollout_bootstraps_truncated_episodes(mode):
    rolls = _rollouts(mode)
    assert rolls[0]["chains"] == (2 if mode == "two_chains" else 1)
    for k, rec in enumerate(rolls):
        trunc, done = rec["trunc"], rec["done"]
        assert trunc.shape == (PPO_T, PPO_N) and trunc.dtype == np.float32 and set(np.unique(trunc)) == {0.0, 1.0}
        assert set(np.unique(done)) == {0.0, 1.0} and (trunc <= done).all()
        assert trunc.sum() >= PPO_N // 2                             # the 6-step limit falls into every 8-step rollout
        code = (done + trunc).astype(np.int32)
        _assert_adv_ret(rec["adv"], rec["ret"], rec["rew"], rec["val"], code, rec["last"], "%s rollout %d" % (mode, k))


def test_fused_eager_and_graph_rollouts_agree_bit_for_bit():
    a, b, c = _rollouts("fused_eager"), _rollouts("one_chain"), _rollouts("two_chains")
    for k in range(2):
        for name in ("obs", "act", "logp", "val", "rew", "done", "trunc", "adv", "ret", "last"):
            assert a[k][name].tobytes() == b[k][name].tobytes(), (k, name)
            assert b[k][name].tobytes() == c[k][name].tobytes(), (k, name)


def test_ppo_with_reward_normalisation_and_bootstrap_in_one_launch():
    """normalize_reward and bootstrap_timeouts together: the boot tail runs with the running statistics; eager and captured agree"""
    a, b = _rollouts("fused_eager", True), _rollouts("one_chain", True)
    for k in range(2):
        for name in ("rew", "done", "trunc", "adv", "ret"):
            assert a[k][name].tobytes() == b[k][name].tobytes(), (k, name)
        code = (b[k]["done"] + b[k]["trunc"]).astype(np.int32)
        _assert_adv_ret(b[k]["adv"], b[k]["ret"], b[k]["rew"], b[k]["val"], code, b[k]["last"], "normalised rollout %d" % k)
    assert not np.array_equal(b[1]["rew"], _rollouts("one_chain")[1]["rew"])             # the second rollout ran under statistics


def test_ppo_needs_an_env_that_reports_truncation():
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    from gym_roboy_amd.ppo import PPO
    env = RoboyVecEnv(MsjRobot(), 64, max_episode_length=PPO_MAX_LEN)
    try:
        with pytest.raises(ValueError, match="report_truncation=True"):
            PPO(env, n_steps=4, bootstrap_timeouts=True)
    finally:
        env.close()
    env = RoboyVecEnv(MsjRobot(), 64, max_episode_length=PPO_MAX_LEN, report_truncation=True)
    try:
        with pytest.raises(ValueError, match="bootstrap_timeouts=True"):       # codes in a captured rollout that reads 0 / 1
            PPO(env, n_steps=4, use_graphs=True)
    finally:
        env.close()


def test_train_parallel_round_trip(tmp_path):
    import os
    import torch
    from gym_roboy_amd import train_parallel
    out = str(tmp_path / "results")
    argv = ["256", out, "--rounds", "1", "--steps-per-round", str(256 * 8 * 2), "--n-steps", "8", "--bootstrap-timeouts"]
    agent = train_parallel.main(argv)
    assert agent.bootstrap_timeouts and agent.env.report_truncation and agent._rollout_graph is not None
    ck = torch.load(os.path.join(out, "model.pkl"))
    assert ck["bootstrap_timeouts"] is True
    steps = agent.num_timesteps
    agent.env.close()
    again = train_parallel.main(argv)                                # resumes from the checkpoint
    assert again.num_timesteps == 2 * steps
    again.env.close()
    plain = train_parallel.main(argv[:-1])                           # loading does not depend on the flag
    assert not plain.bootstrap_timeouts and plain.num_timesteps == 3 * steps
    plain.env.close()
