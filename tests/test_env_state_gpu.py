"""GPU tests of the env's snapshot and restore (rb_env_state_*, RoboyVecEnv.state_dict / load_state_dict).  Every
comparison is bit for bit.  The statement throughout: an env that loads a snapshot IS the env that went on - every output of the next
13 steps, every accessor and every state plane at their end - whatever it held before the load.  The control (two continuous runs
are the same) makes that statement worth something."""
import ctypes

import numpy as np
import pytest

import env_state_util as esu

pytestmark = pytest.mark.gpu

ACT_SEED, OTHER_SEED, PROBE_SEED = 101, 202, 303


def _plant(name):
    """goals [n, n_q] for the scenario: every third env whose velocity after the FIRST step is inside the goal test's bound gets the pose
    it will be in after that step - read from a scout run of the same env - so the scenario has episodes that end at their goal; the other
    envs keep the goal the reset drew (the goal columns of the reset's rows are exact).  A goal does not move the robot, so the scout's
    first step is the scenario's."""
    env = esu.make_env(name)
    try:
        rows = env.reset()
        nq = env.n_q
        goal = rows[:, 2 * nq:3 * nq].copy()
        env.step(esu.actions(name, esu.LEG, ACT_SEED)[0])
        q, qd, feas = env.sim.read_state()
        slow = np.linalg.norm(qd.astype(np.float64), axis=1) < 0.9 * float(env._cfg.goal_vel_tol)
        planted = slow & feas & (np.arange(env.num_envs) % 3 == 0)
        assert planted.any()
        goal[planted] = q[planted]
        return goal
    finally:
        env.close()


def _first_leg(env, name, goal, cuda):
    env.reset()
    env.set_goal(goal)
    return esu.run_steps(env, esu.actions(name, 2 * esu.LEG, ACT_SEED)[:esu.LEG], cuda)


def _second_leg(env, name, cuda):
    recs = esu.run_steps(env, esu.actions(name, 2 * esu.LEG, ACT_SEED)[esu.LEG:], cuda)
    probe = esu.actions(name, 1, PROBE_SEED)[0]
    if cuda:
        import torch
        probe = torch.from_numpy(probe).cuda()
    return recs, esu.final_accessors(env, probe), esu.state_views(env)


def _qualify(env, recs, sd):
    """the first leg has moved every plane the options keep: both episode-end codes, a wrapped ring, a push, a start at a pool row"""
    done = np.array([r["done"] for r in recs])
    assert done.any()
    if env.report_truncation:
        trunc = np.array([r["truncated"] for r in recs])
        assert trunc.any() and (done & ~trunc).any(), "no env with each episode-end code"
    views = sd["views"]
    if "io.ring" in views:
        slots = views["io.ring"].shape[0]
        assert esu.LEG > 3 * slots and all(views["io.ring"][k].any() for k in range(slots)), "the ring has not wrapped"
    if env.push is not None:
        assert views["push.n"].sum() > 0
    if env.start_poses_size:
        assert (views["start.index"] != 0xFFFFFFFF).any() and (views["start.index"] == 0xFFFFFFFF).any()
    if env.episode_log_capacity:
        assert (views["elog.count"] == env.episode_log_capacity).any()
    if env.goal_curriculum is not None and env.goal_curriculum["levels"] > 1:
        assert len(np.unique(views["goals.level"])) > 1


def _continuous(name, goal, cuda):
    env = esu.make_env(name)
    try:
        first = _first_leg(env, name, goal, cuda)
        sd = env.state_dict(dict_view=True)
        _qualify(env, first, sd)
        return sd, first, _second_leg(env, name, cuda)
    finally:
        env.close()


def _same(a, b, what):
    diff = esu.first_difference(a, b, what)
    assert diff is None, diff


def _same_run(got, want, what):
    recs, final, (segs, views, rest) = got
    recs0, final0, (segs0, views0, rest0) = want
    for t, (r, r0) in enumerate(zip(recs, recs0)):
        _same(r, r0, "%s, step %d" % (what, t))
    _same(final, final0, what + ", accessors")
    assert segs == segs0
    for name in views0:
        _same(views[name], views0[name], "%s, segment %s" % (what, name))
    _same(rest, rest0, what + ", state_dict")


@pytest.mark.parametrize("cuda", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("name", list(esu.SETS))
def test_the_resumed_env_is_the_continuous_env(name, cuda):
    goal = _plant(name)
    sd, _, want = _continuous(name, goal, cuda)
    # the control: a second continuous run is the first, bit for bit - without it the comparison below would show nothing
    sd2, _, again = _continuous(name, goal, cuda)
    _same_run(again, want, "control")
    _same({k: v for k, v in sd2["views"].items()}, {k: v for k, v in sd["views"].items()}, "control, snapshot")
    # env B: the same constructor, another past - then the snapshot
    env = esu.make_env(name)
    try:
        env.reset()
        esu.run_steps(env, esu.actions(name, esu.OTHER, OTHER_SEED), cuda)
        before = env.state_dict(dict_view=True)["views"]
        moved = [k for k in before if esu.first_difference(before[k], sd["views"][k])]
        assert len(moved) > len(before) // 2, moved          # (B really held something else)
        env.load_state_dict(sd)
        _same_run(_second_leg(env, name, cuda), want, "resumed")
    finally:
        env.close()


def test_a_snapshot_survives_torch_save(tmp_path):
    import torch
    env = esu.make_env("msj_all")
    try:
        env.reset()
        esu.run_steps(env, esu.actions("msj_all", 3, ACT_SEED), False)
        sd = env.state_dict()
        torch.save(sd, str(tmp_path / "sd.pt"))
        back = torch.load(str(tmp_path / "sd.pt"), weights_only=False)
        _same(esu.to_np(back), esu.to_np(sd), "torch.save")
        env.load_state_dict(back)
    finally:
        env.close()


class _Graph:
    """one env step captured on a side stream (the pattern of tests/test_env_layer_model_gpu.py), replayed per action block"""

    def __init__(self, env):
        import torch
        self.env, n = env, env.num_envs
        dev = torch.device("cuda", 0)
        self.act = torch.zeros((n, env.n_t), device=dev)
        self.obs = torch.zeros((n, env.obs_dim), device=dev)
        self.rew, self.done = torch.zeros((n,), device=dev), torch.zeros((n,), dtype=torch.int32, device=dev)
        self.side = torch.cuda.Stream(device=dev)
        env.set_stream(self.side.cuda_stream)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.side, capture_error_mode="thread_local"):
            env.step_dev(self.act.data_ptr(), self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        torch.cuda.synchronize()

    def run(self, acts):
        import torch
        recs = []
        for a in acts:
            self.act.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
            torch.cuda.synchronize()
            self.graph.replay()
            torch.cuda.synchronize()
            self.env.note_replayed_steps(1)
            recs.append(esu.step_outputs(self.env, (self.obs, self.rew, self.done)))
        return recs


def test_a_captured_step_on_a_side_stream_continues_from_the_restored_state():
    """the planes are written in place and the graphs are kept: the SAME captured graph, replayed before the load and after it"""
    name = "msj_all"
    acts = esu.actions(name, 2 * esu.LEG, ACT_SEED)
    probe = esu.actions(name, 1, PROBE_SEED)[0]

    def continuous():
        env = esu.make_env(name)
        try:
            env.reset()
            g = _Graph(env)          # (the capture itself enqueues nothing: the first replay is the first step)
            g.run(acts[:esu.LEG])
            sd = env.state_dict(dict_view=True)
            return sd, (g.run(acts[esu.LEG:]), esu.final_accessors(env, probe), esu.state_views(env))
        finally:
            env.close()

    sd, want = continuous()
    _same_run(continuous()[1], want, "control")
    env = esu.make_env(name)
    try:
        env.reset()
        g = _Graph(env)
        g.run(esu.actions(name, esu.OTHER, OTHER_SEED))
        env.load_state_dict(sd)
        _same_run((g.run(acts[esu.LEG:]), esu.final_accessors(env, probe), esu.state_views(env)), want, "resumed")
    finally:
        env.close()


def test_a_live_permuted_pool_comes_back_permuted():
    """permute_goal_pool between reset and snapshot; restored into an env that holds the pool in its first order"""
    name = "msj_all"
    acts = esu.actions(name, 2 * esu.LEG, ACT_SEED)
    order = np.random.default_rng(5).permutation(esu.POOL_ROWS)
    a = esu.make_env(name)
    b = esu.make_env(name)
    try:
        a.reset()
        first_order = a.goal_pool()
        a.permute_goal_pool(order)
        assert np.array_equal(a.goal_pool(), first_order[order]) and not np.array_equal(a.goal_pool(), first_order)
        esu.run_steps(a, acts[:esu.LEG], False)
        a.goal_recipe = {"ordered": "custom", "m": esu.POOL_ROWS}          # (what a GoalPool's permutation leaves beside the rows)
        sd = a.state_dict()
        want = esu.run_steps(a, acts[esu.LEG:], False)
        b.reset()
        esu.run_steps(b, esu.actions(name, esu.OTHER, OTHER_SEED), False)
        assert np.array_equal(b.goal_pool(), first_order)
        b.load_state_dict(sd)
        assert np.array_equal(b.goal_pool(), first_order[order]) and b.goal_recipe == a.goal_recipe != {}
        got = esu.run_steps(b, acts[esu.LEG:], False)
        for t, (r, r0) in enumerate(zip(got, want)):
            _same(r, r0, "step %d" % t)            # (the goal columns of the rows: the later draws)
        _same(b.goal_index(), a.goal_index(), "goal index")
        _same(b.goal_pool(), a.goal_pool(), "goal pool")
        _same(b.goal_row_stats(), a.goal_row_stats(), "row counts")
    finally:
        a.close(); b.close()


def test_refusals_leave_the_env_as_it_was():
    from gym_roboy_amd import _native as nat
    name = "msj_all"
    env = esu.make_env(name)
    try:
        env.reset()
        esu.run_steps(env, esu.actions(name, 3, ACT_SEED), False)
        segs0, views0, rest0 = esu.state_views(env)
        # the library: a byte count that is not rb_env_state_bytes'
        nbytes = env.sim.state_bytes()
        d_blob = env.sim.malloc(nbytes + 16)
        lib, host = env.sim._lib, nat.StateHost()
        for call in (lib.rb_env_state_save_dev, lib.rb_env_state_load_dev):
            for wrong in (nbytes - 16, nbytes + 16, 0):
                assert call(env.sim.handle, ctypes.c_void_p(d_blob), wrong, ctypes.byref(host)) == nat.RB_EINVAL
                assert b"rb_env_state_bytes" in lib.rb_last_error()
            assert call(env.sim.handle, None, nbytes, ctypes.byref(host)) == nat.RB_EINVAL
        with pytest.raises(ValueError, match="bytes"):
            env.sim.load_state(np.zeros(nbytes - 16, np.uint8))
        # the env: states of envs that are not this one, each named by the first field or segment that differs
        others = (("n_envs", dict(n=256)), ("seed", dict(seed=15)), ("elog.ret", dict(episode_log=3)), ("io.ring", dict(action_delay=(0, 5))),
                  ("push.count", dict(push=None)), ("par.planes", dict(randomization=None, critic_obs=None)),
                  ("start.pool", dict(start_poses=esu.su.pool_of(esu._msj().get_description(), m=11))))
        for named, kw in others:
            other = esu.make_env(name, **kw)
            try:
                other.reset()
                sd = other.state_dict()
            finally:
                other.close()
            with pytest.raises(ValueError, match=named.replace(".", r"\.")):
                env.load_state_dict(sd)
        segs, views, rest = esu.state_views(env)
        assert segs == segs0
        _same(views, views0, "after the refusals")
        _same(rest, rest0, "after the refusals")
    finally:
        env.close()


@pytest.mark.parametrize("robot", ["msj", "upper"])
def test_a_handle_without_the_env_layer_has_the_core_segments_and_round_trips_them(robot):
    from gym_roboy_amd.envs.simulations import HipBatchSimulation
    make, n = (esu._msj, 300) if robot == "msj" else (esu._upper, 66)
    desc = make().get_description()
    sim = HipBatchSimulation(make(), n, seed=3)
    try:
        segs = sim.state_segments()
        assert [s[0] for s in segs] == ["core.q", "core.qd", "core.feas", "core.goal_count"]
        assert [s[2] * s[3] for s in segs] == [n * desc.n_q, n * desc.n_q, n, n] and all(s[4] % 16 == 0 for s in segs)
        rng = np.random.default_rng(0)
        q = rng.uniform(0.5 * desc.q_lo, 0.5 * desc.q_hi, (n, desc.n_q)).astype(np.float32)
        sim.set_state(q, np.zeros_like(q))
        sim.get_new_goal_joint_angles()                    # (moves the draw counters)
        blob, host = sim.save_state()
        want = sim.read_state()
        goals = sim.get_new_goal_joint_angles()
        for _ in range(3):
            sim.forward_step_command(rng.uniform(-0.3, 0.3, (n, desc.n_t)).astype(np.float32))
        assert not np.array_equal(sim.read_state()[0], want[0])
        sim.load_state(blob, host)
        for x, y in zip(sim.read_state(), want):
            assert np.array_equal(x, y)
        assert np.array_equal(sim.get_new_goal_joint_angles(), goals)      # the counter came back: the same draw again
        blob2, _ = sim.save_state()
        sim.load_state(blob, host)
        assert np.array_equal(sim.save_state()[0], blob) and not np.array_equal(blob2, blob)
    finally:
        sim.close()
