"""The composed host model of the env layer (tests/env_layer_model.py: EnvLayerModel) on the fp32 C oracle, without a GPU:
  1. with every option off it IS host_env_model.HostEnvModel, bit for bit - so it inherits that model's pin to the reference's golden
     vectors;
  2. with exactly one option on, the option's planes are those of the option's own restatement fed the same inputs;
  3. every case of CASES qualifies: its scenario makes every path run that the GPU comparison claims to cover;
  4. the model can SEE DESIGN.md §6's order: moving a behind-the-step stage in front of its neighbour changes a compared output,
     for each pair whose order §6 gives a reason for - but for 3 / 4, where no order is observable (see that test)."""
import numpy as np
import pytest

import env_layer_model as em
import env_io_util as iu
import env_obs_util as ou
import env_params_util as epu
import episode_log_util as eu
import goal_curriculum_util as gc
import goal_pool_util as gp
import push_util as pu
import shaping_util as shu
import start_pose_util as su
import truncation_ref as tr
from action_box_util import wide_actions
from action_obs_util import HistoryBook, clip_action
from host_env_model import COracleStepper, HostEnvModel

N, SEED, MAX_LEN, STEPS = 72, 7, 5, 30      # a full wave and a ragged one; wide_actions plants its specials in 72 envs


def _robot(which):
    return em._msj() if which == "msj" else em._upper()


# ---- 1. every option off ----
@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("which", ["msj", "upper"])
def test_with_every_option_off_it_is_the_host_env_model(which, auto_reset):
    robot = _robot(which)
    desc = robot.get_description()
    model = em.EnvLayerModel(robot, em.OracleStepper(robot, N), N, SEED, max_episode_length=MAX_LEN, auto_reset=auto_reset, joint_vel_penalty=True)
    host = HostEnvModel(robot, COracleStepper(robot, N), N, SEED, MAX_LEN, True, True, auto_reset)
    obs0 = model.reset()
    host.goal = host.draw(np.ones(N, bool))          # (RoboyEnv(...) then reset(): as every replay test mirrors it)
    assert not obs0[:, :2 * desc.n_q].any() and np.array_equal(obs0[:, 2 * desc.n_q:], host.goal)
    n_done = 0
    for act in wide_actions(N, desc.n_t, STEPS, SEED + 1):
        obs, rew, done, _ = model.step(act)
        h_obs, h_rew, h_done, _ = host.step(clip_action(act))      # (HostEnvModel takes actions inside the box)
        assert obs.tobytes() == h_obs.tobytes() and rew.tobytes() == h_rew.tobytes() and np.array_equal(done, h_done)
        assert np.array_equal(model.stats, host.stats) and np.array_equal(model.goal, host.goal)
        n_done += int(done.sum())
    assert n_done >= (STEPS // MAX_LEN) * N


# ---- 2. exactly one option on ----
def _pool(desc):
    return gp.small_pool(desc, m=7)


ONE_OPTION = {
    "goals": lambda d: dict(goals=_pool(d)),
    "goal_curriculum": lambda d: dict(goals=_pool(d), goal_curriculum=dict(levels=3, up=1, down=1, start=1)),
    "goal_row_stats": lambda d: dict(goals=_pool(d), goal_curriculum=dict(levels=1, up=1, down=1, start=0), goal_row_stats=True),
    "report_truncation": lambda d: dict(report_truncation=True),
    "critic_obs": lambda d: dict(critic_obs=("state", "age")),
    "reward_shaping": lambda d: dict(reward_shaping=shu.ALL),
    "push": lambda d: dict(push={"prob": 0.25, "sigma": pu.sigma_of(d)}),
    "episode_log": lambda d: dict(episode_log=2),
    "start_poses": lambda d: dict(start_poses=su.pool_of(d), start_prob=0.5),
    "action_delay": lambda d: dict(action_delay=(0, 3)),
    "sensor_noise": lambda d: dict(sensor_noise={"q": 0.01, "qd": 0.05}),
    "action_obs": lambda d: dict(action_obs=2),
    "tendon_obs": lambda d: dict(tendon_obs=("length", "force"), tendon_obs_scale={"force": 1 / 400}),
    "randomization": lambda d: dict(randomization=em._ranges(), critic_obs=("state", "params")),
}


@pytest.mark.parametrize("option", sorted(ONE_OPTION))
def test_with_one_option_on_its_planes_are_the_options_own_restatement(option):
    """MsjRobot, auto_reset, a reset and 12 steps.  The restatement is a second instance, fed what the option's kernel is fed: the
    done flags, the step's own reward, the goals-reached outcome - never the model's planes of that option."""
    robot = _robot("msj")
    desc = robot.get_description()
    nq = desc.n_q
    kw = ONE_OPTION[option](desc)
    stepper = em.ParamOracleStepper(robot, N) if option == "randomization" else em.OracleStepper(robot, N)
    model = em.EnvLayerModel(robot, stepper, N, SEED, max_episode_length=MAX_LEN, **kw)
    plain = em.EnvLayerModel(robot, em.OracleStepper(robot, N), N, SEED, max_episode_length=MAX_LEN)
    gids = np.arange(N, dtype=np.uint64)
    acts = wide_actions(N, desc.n_t, 12, SEED + 1)
    obs, p_obs = model.reset(), plain.reset()
    # the restatements' own state
    count = np.full(N, 2, np.int64)                              # goal counter: 1 behind construction, + 1 per reset
    level = np.full(N, kw.get("goal_curriculum", {}).get("start", 0), np.int64)
    index = None
    attempts = reached = None
    push_book = pu.Book(SEED, N, pu.threshold_of(0.25)) if option == "push" else None
    start_book = su.Book(SEED, N, su.threshold_of(0.5), su.M) if option == "start_poses" else None
    log = eu.EpisodeLogModel(N, 2)
    delay_book, history = iu.DelayBook(N, desc.n_t), HistoryBook(N, desc.n_t, 2)
    delay, delay_draws = iu.delay_draw(SEED, gids, 0, 0, 3), np.ones(N, np.uint32)
    colsig = iu.column_sigmas(nq, desc.n_t, (), {"q": 0.01, "qd": 0.05})
    if option == "sensor_noise":
        assert np.array_equal(obs, p_obs.astype(np.float64) + colsig * iu.sensor_noise64(SEED, gids, 0, 3 * nq))
    if option == "action_obs":
        assert obs.shape == (N, 3 * nq + 2 * desc.n_t) and not obs[:, 3 * nq:].any()
    if option == "tendon_obs":               # the zero pose, every set-point 0
        want = ou.expected_columns(robot, desc, p_obs[:, :nq], p_obs[:, nq:2 * nq], None, kw["tendon_obs"], kw["tendon_obs_scale"])[0]
        assert np.array_equal(obs[:, :3 * nq], p_obs) and np.array_equal(obs[:, 3 * nq:], want)
    if option == "randomization":            # env_params_util's own stepper, which draws by itself where the env resets, under HostEnvModel
        lo, hi = kw["randomization"].to_arrays(desc.n_t)
        par0 = epu.draw(SEED, gids, 0, lo, hi)
        assert model.par.tobytes() == par0.tobytes() and np.all(model.par_draws == 1)
        p_host = HostEnvModel(robot, epu.ParamOracleStepper(robot, N, SEED, lo, hi, par0, np.ones(N, np.uint32)), N, SEED, MAX_LEN, False, True, True)
        p_host.goal = p_host.draw(np.ones(N, bool))
    step_num = np.ones(N, np.int64)
    dones, rates = [], []
    if start_book:
        started = start_book.start(None)
        su.check_rows(obs, p_obs, started, start_book.index, kw["start_poses"], nq, "reset")
    if "goals" in kw:
        m, L = len(kw["goals"]), kw.get("goal_curriculum", {}).get("levels")
        index = gc.row(SEED, gids, 1, level, m, L) if L else gp.pool_row(SEED, gids, 1, m)
        attempts, reached = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
        assert np.array_equal(obs[:, 2 * nq:], kw["goals"][index])
    for t, act in enumerate(acts):
        q0, qd0, _ = model.state()
        fed = delay_book.shifted(act, delay)[0] if option == "action_delay" else act
        out, p_out = model.step(act), plain.step(fed)
        obs, rew, done = out[:3]
        hit = model.last_reached
        if option in ("report_truncation", "critic_obs", "episode_log", "goals", "goal_curriculum", "goal_row_stats", "reward_shaping"):
            assert np.array_equal(done, p_out[2]) and np.array_equal(obs[:, :2 * nq], p_out[0][:, :2 * nq])      # the state is the plain env's
        if option == "action_delay":          # the plain model fed the shifted sequence; a done env has drawn its next delay
            assert obs.tobytes() == p_out[0].tobytes() and rew.tobytes() == p_out[1].tobytes() and np.array_equal(done, p_out[2])
            delay_book.advance(done)
            delay[done] = iu.delay_draw(SEED, gids[done], delay_draws[done], 0, 3)
            delay_draws[done] += np.uint32(1)
            assert np.array_equal(model.delay, delay)
        if option == "sensor_noise":          # row number t + 1 (the reset's row was number 0); reward and done see the true state
            assert np.array_equal(obs, p_out[0].astype(np.float64) + colsig * iu.sensor_noise64(SEED, gids, t + 1, 3 * nq))
            assert rew.tobytes() == p_out[1].tobytes() and np.array_equal(done, p_out[2])
        if option == "tendon_obs":            # the plain row, then env_obs_util's columns at the state it reports under the step's actions
            want = ou.expected_columns(robot, desc, p_out[0][:, :nq], p_out[0][:, nq:2 * nq], act, kw["tendon_obs"], kw["tendon_obs_scale"])[0]
            assert np.array_equal(obs[:, :3 * nq], p_out[0]) and np.array_equal(obs[:, 3 * nq:], want) and want.shape == (N, 2 * desc.n_t)
            assert rew.tobytes() == p_out[1].tobytes() and np.array_equal(done, p_out[2])
        if option == "action_obs":
            assert obs[:, :3 * nq].tobytes() == p_out[0].tobytes() and np.array_equal(obs[:, 3 * nq:], history.blocks(act, done))
        if option == "randomization":
            h_obs, h_rew, h_done, _ = p_host.step(clip_action(act))
            assert obs.tobytes() == h_obs.tobytes() and rew.tobytes() == h_rew.tobytes() and np.array_equal(done, h_done)
            assert model.par.tobytes() == p_host.stepper.par.tobytes() and np.array_equal(model.par_draws, p_host.stepper.draws)
            assert model.critic_rows[:, 3 * nq:].tobytes() == model.par.tobytes()
        if option == "report_truncation":
            assert np.array_equal(model.kind, tr.expected_codes(done, rew)) and np.array_equal(model.truncated(), done & ~hit)
        if option == "critic_obs":
            step_num = np.where(done, 1, step_num + 1)
            q, qd, _ = model.state()
            want = np.concatenate([q, qd, obs[:, 2 * nq:], (step_num.astype(np.float32) / np.float32(MAX_LEN))[:, None]], axis=1)
            assert model.critic_rows.tobytes() == want.tobytes()
        if option == "reward_shaping":
            prev = acts[t - 1] if t else None
            first = np.ones(N, bool) if t == 0 else dones[-1]
            q1, qd1, _ = model.state()
            cost = shu.cost64(desc, robot, q0.astype(np.float64), qd0.astype(np.float64), act, prev, first, shu.ALL)
            assert np.array_equal(model.cost, cost) and np.array_equal(rew, p_out[1] - cost)
            rates.append(shu.terms64(desc, robot, q0.astype(np.float64), qd0.astype(np.float64), act, prev, first)[0][0])
        if option == "episode_log":
            log.step_outcome(rew.astype(np.float32), done, hit)
            assert eu.same_log(model.episode_log(), log.log()) and model.log.full == log.full
        if push_book:
            pushed, m_at = push_book.step()
            b = model.push_book
            assert np.array_equal(b.count, push_book.count) and np.array_equal(b.last, push_book.last) and np.array_equal(b.n_pushes, push_book.n_pushes)
            want = (np.asarray(pu.sigma_of(desc))[None, :] * pu.z64(SEED, gids[pushed], m_at[pushed], nq)).astype(np.float32)
            assert np.array_equal(model.impulse[pushed], want) and np.array_equal(model.last_push()[0], pushed)
        if start_book:
            started = start_book.start(done)
            assert np.array_equal(model.start_book.count, start_book.count) and np.array_equal(model.start_book.index, start_book.index)
            q, qd, feas = model.state()
            pose = kw["start_poses"][start_book.index[started].astype(np.int64)]
            assert np.array_equal(q[started], pose) and not qd[started].any() and feas[started].all()
            assert np.array_equal(obs[started, :nq], pose) and not obs[started, nq:2 * nq].any()
            assert not obs[done & ~started, :2 * nq].any()
        if "goals" in kw and done.any():
            if option == "goal_row_stats":
                np.add.at(attempts, index[done], np.uint64(1))
                np.add.at(reached, index[done & hit], np.uint64(1))
            count[done] += 2
            if L:
                level[done] = gc.next_level(level[done], hit[done], 1, 1, L)
                index[done] = gc.row(SEED, gids[done], (count[done] - 1).astype(np.uint32), level[done], m, L)
                assert np.array_equal(model.level, level) and np.array_equal(model.goal_index, index)
            else:
                index[done] = gp.pool_row(SEED, gids[done], (count[done] - 1).astype(np.uint32), m)
            if option == "goal_row_stats":
                assert np.array_equal(model.attempts, attempts) and np.array_equal(model.row_reached, reached)
        if "goals" in kw:
            assert np.array_equal(obs[:, 2 * nq:], kw["goals"][index]) and np.array_equal(model.goal, kw["goals"][index])
        dones.append(done)
    assert np.array(dones).sum(axis=0).min() >= 2
    if option == "reward_shaping":
        assert np.array_equal(np.array(rates), shu.rate64(acts, np.array(dones)))
    if option == "goal_row_stats":
        assert attempts.sum() == np.array(dones).sum()


# ---- 3. the cases qualify ----
_runs = {}


def _run(name, auto_reset, order=em.STEP_STAGES):
    """one scenario on the C oracle -> (model, record, every compared output per step); the §6 order's runs are shared"""
    key = (name, auto_reset, tuple(order))
    if key not in _runs:
        stepper = em.case_stepper(name)
        if ("goals", name) not in _runs:
            _runs[("goals", name)] = em.case_goals(name, stepper)
        goals = _runs[("goals", name)]
        model = em.case_model(name, stepper(), auto_reset, goals, behind_step_order=order)
        outs = []

        class Keep:                      # (run_scenario's device hook, used here to keep the model's own outputs)
            reset = staticmethod(lambda: None)
            step = staticmethod(lambda act: (None, None))

            @staticmethod
            def compare(where, dev, out):
                log = model.episode_log()
                outs.append({"obs": out[0].copy(), "reward": None if len(out) == 1 else out[1].copy(), "critic": None if not model.critic_names else
                             model.critic_rows.copy(), "log_return": log["return"].copy(), "log_kind": log["kind"].copy(), "kind": model.kind.copy()})
        rec = em.run_scenario(model, em.case_actions(name), Keep)
        _runs[key] = (model, rec, outs)
    return _runs[key]


@pytest.mark.parametrize("name,auto_reset", [(name, a) for name in sorted(em.CASES) for a in (True, False) if a or name in em.BOTH_WAYS])
def test_every_case_makes_every_path_run(name, auto_reset):
    model, rec, _ = _run(name, auto_reset)
    assert model.margin_min > 4 * em.MARGIN      # (what CASES promises of its seeds)
    em.qualify(model, rec)
    done = np.array(rec.done)
    assert len(done) == em.LEG1 + em.LEG2 and rec.resets[0] == 0 and em.LEG1 in rec.resets
    if not auto_reset:
        assert len(rec.resets) > 2           # stage 1a never ran, the loop's own resets did
    n = model.n
    assert n > 64 and n % 64 != 0            # whole waves plus a ragged one
    if model.gid0:                           # the ids cross 2^32: on EACH side envs are pushed, start from the pool, go up and down
        assert int(model.ids[0]) < 2 ** 32 <= int(model.ids[-1])
        for side in (model.ids < 2 ** 32, model.ids >= 2 ** 32):
            assert model.push_book.n_pushes[side].any() and model.start_book.count[side].any()
            assert (model.level[side] > em.START_LEVEL).any() and (model.level[side] < em.START_LEVEL).any()


# ---- 4. the order ----
def _moved(later, earlier):
    """§6's order with stage `later` moved directly in front of stage `earlier`"""
    order = [s for s in em.STEP_STAGES if s != later]
    order.insert(order.index(earlier), later)
    return tuple(order)


def _differs(a, b):
    """the compared outputs in which two runs differ"""
    keys = set()
    for x, y in zip(a, b):
        keys |= {k for k in x if x[k] is not None and x[k].tobytes() != y[k].tobytes()}
    return keys


@pytest.mark.parametrize("name,earlier,later,seen_in", [
    ("msj_all", "0", "3", "log_return"),        # the log adds up the reward as shaping apply left it
    ("upper_all", "0", "3", "log_return"),
    ("msj_all", "1", "2", "critic"),            # the goal kernel stands in front of everything that reads the goal
    ("msj_all", "1a", "2", "critic"),           # the critic rows report the planes as the start-pose kernel left them
])
def test_a_stage_moved_in_front_of_its_neighbour_changes_a_compared_output(name, earlier, later, seen_in):
    right, wrong = _run(name, True)[2], _run(name, True, _moved(later, earlier))[2]
    assert seen_in in _differs(right, wrong)


def test_no_output_tells_the_log_in_front_of_the_codes_from_the_log_behind_them():
    """§6 places the episode log in front of the episode-end codes 'while the done words are still flags'.  Both kernels test the done
    word against 0 and tell the outcome from the goals-reached counter against a `seen` plane of their own (csrc/env_episode_log.hpp,
    done_kind_kernel), so a log behind the codes records the same: this order is a convention, not an observable - stated here so
    that nobody takes the cases for blind to it."""
    right, wrong = _run("msj_all", True)[2], _run("msj_all", True, _moved("4", "3"))[2]
    assert not _differs(right, wrong)
