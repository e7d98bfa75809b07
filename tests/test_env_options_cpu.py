"""``gym_roboy_amd/envs/options.py`` without a GPU and without the library: the command line against the keyword arguments
``train_parallel.main`` hands to ``RoboyVecEnv`` (written out from the main that declared and parsed every flag itself), the one
``KEY=VALUE`` parser, what a checkpoint records about an env, what ``load()`` checks and ``visualize_agent`` replays, and the
named segments of the statistics block the ranks sum."""
import itertools
import types
import warnings

import numpy as np
import pytest
import torch

from env_options_util import same
from gym_roboy_amd.envs import options
from gym_roboy_amd.sharding import STAT_KEYS, join_segments, split_segments


# ---- 1. the command line ----
class FakePool:
    def __init__(self, m, ordered=False):
        self.m, self.is_ordered, self.recipe = m, ordered, {"kind": "reachable", "m": m, "ordered": "rest_distance" if ordered else None}

    def ordered(self):
        return FakePool(self.m, True)

    def __eq__(self, other):
        return isinstance(other, FakePool) and (self.m, self.is_ordered) == (other.m, other.is_ordered)


BASE = dict(seed=0, device=0, integrator="euler", goals=None, env_id_offset=0, tendon_obs=None, tendon_obs_scale=None, sensor_noise=None,
            action_delay=None, report_truncation=False, action_obs=None, critic_obs=None, goal_curriculum=None)
ABSENT_WHEN_OFF = ("goal_row_stats", "reward_shaping", "push")
POOL = ["--goals", "reachable:64"]
LEVELS = POOL + ["--goal-levels", "4"]
STAIRS = {"levels": 4, "up": 1, "down": 1, "start": 0}
ALL_FLAGS = ["--seed", "5", "--tendon-obs", "length,force", "--tendon-obs-scale", "force=0.0025,length=4", "--sensor-noise", "q=0.01,force=2",
             "--action-delay", "0:2", "--action-obs", "2", "--critic-obs", "state,age,delay,actions", "--goals", "reachable:256",
             "--goal-levels", "4", "--goal-up", "2", "--goal-down", "0", "--goal-order", "reach_rate", "--goal-reorder-every", "3",
             "--reward-shaping", "action_rate=0.05", "--push", "prob=0.02,sigma=0.5", "--bootstrap-timeouts"]
COMMAND_LINES = [
    ([], {}),
    (["--seed", "3"], dict(seed=3)),
    (["--tendon-obs", "length,force"], dict(tendon_obs=("length", "force"))),
    (["--tendon-obs-scale", "force=0.0025,length=4"], dict(tendon_obs_scale={"force": 0.0025, "length": 4.0})),
    (["--sensor-noise", "q=0.01,qd=0.05,force=2"], dict(sensor_noise={"q": 0.01, "qd": 0.05, "force": 2.0})),
    (["--action-delay", "2"], dict(action_delay=2)),
    (["--action-delay", "0:3"], dict(action_delay=(0, 3))),
    (["--action-obs", "2"], dict(action_obs=2)),
    (["--critic-obs", "state,age"], dict(critic_obs=("state", "age"))),
    (["--goals", "reachable"], dict(goals=FakePool(16384))),
    (POOL, dict(goals=FakePool(64))),
    (LEVELS, dict(goals=FakePool(64, True), goal_curriculum=STAIRS)),
    (LEVELS + ["--goal-up", "2"], dict(goals=FakePool(64, True), goal_curriculum=dict(STAIRS, up=2))),
    (LEVELS + ["--goal-down", "0"], dict(goals=FakePool(64, True), goal_curriculum=dict(STAIRS, down=0))),
    (LEVELS + ["--goal-order", "rest_distance"], dict(goals=FakePool(64, True), goal_curriculum=STAIRS)),
    (LEVELS + ["--goal-order", "reach_rate"], dict(goals=FakePool(64, True), goal_curriculum=STAIRS, goal_row_stats=True)),
    (LEVELS + ["--goal-order", "reach_rate", "--goal-reorder-every", "2"],
     dict(goals=FakePool(64, True), goal_curriculum=STAIRS, goal_row_stats=True)),
    (["--bootstrap-timeouts"], dict(report_truncation=True)),
    (["--reward-shaping", "action_rate=0.05,tension=0.01"], dict(reward_shaping={"action_rate": 0.05, "tension": 0.01})),
    (["--reward-shaping", "action_rate=0"], dict(reward_shaping={"action_rate": 0.0})),      # (all zeros: passed on, the env turns it off)
    (["--push", "prob=0.02,sigma=0.5"], dict(push={"prob": 0.02, "sigma": 0.5})),
    (["--normalize-obs", "--symmetry", "loss", "--lr-schedule", "adaptive"], {}),  # (the agent's flags leave the env's call alone)
    (ALL_FLAGS, dict(seed=5, tendon_obs=("length", "force"), tendon_obs_scale={"force": 0.0025, "length": 4.0},
                     sensor_noise={"q": 0.01, "force": 2.0}, action_delay=(0, 2), action_obs=2,
                     critic_obs=("state", "age", "delay", "actions"), goals=FakePool(256, True),
                     goal_curriculum={"levels": 4, "up": 2, "down": 0, "start": 0}, goal_row_stats=True, report_truncation=True,
                     reward_shaping={"action_rate": 0.05}, push={"prob": 0.02, "sigma": 0.5})),
]


def _run_main(argv, monkeypatch, tmp_path):
    """the fake-constructor idiom of tests/test_critic_obs_cpu.py: main up to the agent, the env's call recorded"""
    import gym_roboy_amd.envs.goals as envgoals
    import gym_roboy_amd.envs.vec_env as vec_env
    import gym_roboy_amd.ppo as ppo
    import gym_roboy_amd.train_parallel as tp
    seen = {}

    class Stop(Exception):
        pass

    def fake_env(*a, **kw):
        seen["env_args"], seen["env"] = a, kw
        return object()

    def fake_ppo(env, **kw):
        seen["ppo"] = kw
        raise Stop

    def fake_pool(robot, m, seed=0, integrator=None, device=0):
        seen["pool"] = dict(m=m, seed=seed, integrator=integrator, device=device)
        return FakePool(m)

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(vec_env, "RoboyVecEnv", fake_env)
    monkeypatch.setattr(ppo, "PPO", fake_ppo)
    monkeypatch.setattr(envgoals, "reachable_goals", fake_pool)
    with pytest.raises(Stop):
        tp.main(["4", str(tmp_path)] + list(argv))
    return seen


@pytest.mark.parametrize("argv,changed", COMMAND_LINES, ids=[" ".join(a) or "no flags" for a, _ in COMMAND_LINES])
def test_the_command_line_becomes_exactly_these_keyword_arguments(argv, changed, monkeypatch, tmp_path, capsys):
    seen = _run_main(argv, monkeypatch, tmp_path)
    want = dict(BASE, **changed)
    assert seen["env"] == want
    for key in ABSENT_WHEN_OFF:
        assert (key in seen["env"]) == (key in changed), key
    assert len(seen["env_args"]) == 2 and type(seen["env_args"][0]).__name__ == "MsjRobot" and seen["env_args"][1] == 4
    assert seen["ppo"]["asymmetric_critic"] is bool(want["critic_obs"]) and seen["ppo"]["bootstrap_timeouts"] is want["report_truncation"]
    if want["goals"] is not None:
        assert seen["pool"] == dict(m=want["goals"].m, seed=want["seed"], integrator="euler", device=0)


def test_rank_and_device_reach_the_env(monkeypatch, tmp_path):
    monkeypatch.setenv("RANK", "2")
    monkeypatch.setenv("LOCAL_RANK", "1")
    seen = _run_main(["--push", "prob=0.5,sigma=1"], monkeypatch, tmp_path)
    assert seen["env"] == dict(BASE, device=1, env_id_offset=8, push={"prob": 0.5, "sigma": 1.0})


def test_env_kwargs_from_args_alone_leaves_out_what_the_process_knows():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("num_envs", type=int)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bootstrap-timeouts", action="store_true")
    options.add_env_arguments(ap)
    options.add_env_arguments(ap, late=True)
    static = {k: v for k, v in BASE.items() if k not in ("goals", "device", "env_id_offset")}
    assert options.env_kwargs_from_args(ap.parse_args(["4"])) == static
    assert options.env_kwargs_from_args(ap.parse_args(["4", "--goals", "reachable:8", "--action-delay", "1"])) == dict(static, action_delay=1)


def test_the_moved_names_stay_importable():
    import gym_roboy_amd.envs.vec_env as vec_env
    import gym_roboy_amd.train_parallel as tp
    for name in ("TENDON_OBS_CHANNELS", "SENSOR_NOISE_KEYS", "tendon_obs_mask", "tendon_obs_scales", "sensor_noise_sigmas", "action_delay_range",
                 "action_obs_rows", "action_obs_bounds", "critic_obs_spec", "reward_shaping_weights", "push_spec", "parse_reward_shaping",
                 "parse_push"):
        assert getattr(vec_env, name) is getattr(options, name), name
    for name in ("parse_goals", "parse_goal_curriculum", "parse_goal_order", "DEFAULT_GOAL_POOL", "GOAL_ORDERS", "ENV_INTEGRATOR"):
        assert getattr(tp, name) is getattr(options, name), name


# ---- 2. the one KEY=VALUE parser ----
@pytest.mark.parametrize("flag,key,match_missing,match_twice", [
    ("--tendon-obs-scale", "force", "tendon obs scale: expected CHANNEL=FACTOR, got 'force'", "tendon obs scale: 'force' given twice"),
    ("--sensor-noise", "q", "sensor noise: expected KEY=SIGMA, got 'q'", "sensor noise: 'q' given twice"),
    ("--reward-shaping", "action_rate", "reward shaping: expected TERM=WEIGHT, got 'action_rate'", "reward shaping: 'action_rate' given twice"),
    ("--push", "prob", "push: expected KEY=VALUE, got 'prob'", "push: 'prob' given twice")])
def test_every_key_value_flag_refuses_a_missing_sign_and_a_repeated_key(flag, key, match_missing, match_twice, tmp_path):
    import gym_roboy_amd.train_parallel as tp
    with pytest.raises(ValueError, match=match_missing):
        tp.main(["4", str(tmp_path), flag, "%s,other=1" % key])
    with pytest.raises(ValueError, match=match_twice):
        tp.main(["4", str(tmp_path), flag, "%s=1,%s=0.5" % (key, key)])
    with pytest.raises(ValueError):
        tp.main(["4", str(tmp_path), flag, "%s=much" % key])


def test_bad_flags_are_reported_in_the_order_main_always_parsed_them(tmp_path):
    import gym_roboy_amd.train_parallel as tp
    with pytest.raises(ValueError, match="sensor noise"):            # (before the goal flags' SystemExit)
        tp.main(["4", str(tmp_path), "--sensor-noise", "q", "--goals", "bogus"])
    with pytest.raises(ValueError, match="invalid literal"):         # (--action-delay before --tendon-obs-scale)
        tp.main(["4", str(tmp_path), "--action-delay", "soon", "--tendon-obs-scale", "force"])
    with pytest.raises(SystemExit, match="--goals takes"):           # (the goal flags before --reward-shaping and --push)
        tp.main(["4", str(tmp_path), "--goals", "bogus", "--push", "prob"])


def test_the_parser_itself():
    assert options.parse_key_values("", "x") is None and options.parse_key_values(None, "x") is None
    assert options.parse_key_values("a=1,,b=2.5,", "x") == {"a": 1.0, "b": 2.5}
    with pytest.raises(ValueError):
        options.parse_key_values("a=1=2", "x")
    with pytest.raises(ValueError, match="the option: expected K=V, got 'a'"):
        options.parse_key_values("a", "the option", "K=V")
    # the two callers that also validate, as before
    assert options.parse_reward_shaping("action_rate=0.05,tension=0.01") == {"action_rate": 0.05, "tension": 0.01}
    assert options.parse_push("prob=0.02,sigma=0.5") == {"prob": 0.02, "sigma": 0.5}
    with pytest.raises(ValueError, match="unknown term"):
        options.parse_reward_shaping("jerk=1")
    with pytest.raises(ValueError, match="needs both"):
        options.parse_push("prob=0.5")


# ---- 3. the checkpoint ----
DEFAULT_RECORD = {"tendon_obs": {"channels": [], "scale": [1.0, 1.0, 1.0, 1.0]}, "env_io": {"sensor_noise": {}, "action_delay": None}}
ROWS = np.arange(9, dtype=np.float32).reshape(3, 3) / 16
SCALE = [4.0, 1.0, 1.0, float(np.float32(0.0025))]


def _full_env(**over):
    env = types.SimpleNamespace(
        num_envs=2, tendon_obs=("length", "force"), tendon_obs_scale=np.array([4, 1, 1, 0.0025], np.float32), sensor_noise={"q": 0.01, "force": 2.0},
        action_delay=(0, 2), action_obs=2, critic_obs_names=("state", "age", "delay", "actions"), critic_obs_dim=27, report_truncation=True,
        goal_pool_size=3, goal_pool=lambda: ROWS.copy(), goal_recipe={"kind": "reachable", "ordered": "reach_rate"},
        goal_curriculum={"levels": 4, "up": 1, "down": 1, "start": 0}, goal_levels=lambda: np.array([0, 3], np.uint32),
        goal_row_stats_enabled=True, goal_row_stats=lambda reset=False: {"attempts": np.array([5, 4, 3], np.uint64), "reached": np.array([5, 2, 0], np.uint64)},
        reward_shaping={"action_rate": float(np.float32(0.05)), "tension": 0.0, "activation": 0.0},
        push={"prob": 0.02, "sigma": [0.5, 0.5, 0.5], "threshold": 335544}, randomization=None, obs_dim=41)
    env.levels_set = []
    env.set_goal_levels = env.levels_set.append
    vars(env).update(over)
    return env


FULL_RECORD = {
    "tendon_obs": {"channels": ["length", "force"], "scale": SCALE},
    "env_io": {"sensor_noise": {"q": 0.01, "force": 2.0}, "action_delay": [0, 2], "action_obs": 2},
    "critic_obs": ["state", "age", "delay", "actions"],
    "goals": {"q": torch.from_numpy(ROWS), "recipe": {"kind": "reachable", "ordered": "reach_rate"}},
    "goal_curriculum": {"levels": 4, "up": 1, "down": 1, "level": torch.tensor([0, 3], dtype=torch.int64)},
    "goal_row_stats": {"attempts": torch.tensor([5, 4, 3], dtype=torch.int64), "reached": torch.tensor([5, 2, 0], dtype=torch.int64)},
    "reward_shaping": {"action_rate": float(np.float32(0.05)), "tension": 0.0, "activation": 0.0},
    "env_push": {"prob": 0.02, "sigma": [0.5, 0.5, 0.5], "threshold": 335544},
}


def test_the_record_of_an_env():
    assert same(options.env_checkpoint_record(object()), DEFAULT_RECORD)
    assert same(options.env_checkpoint_record(types.SimpleNamespace()), DEFAULT_RECORD)
    assert same(options.env_checkpoint_record(None), DEFAULT_RECORD)
    assert same(options.env_checkpoint_record(_full_env()), FULL_RECORD)
    # the critic rows' names are the agent's to record: PPO names its asymmetric_critic, whatever the env writes
    assert same(options.env_checkpoint_record(_full_env(), critic=False), {k: v for k, v in FULL_RECORD.items() if k != "critic_obs"})
    assert same(options.env_checkpoint_record(object(), critic=True), dict(DEFAULT_RECORD, critic_obs=[]))
    # a fixed delay is a number, a torch step's levels are a tensor already, no action rows leave no key
    env = _full_env(action_delay=3, action_obs=0, goal_levels=lambda: torch.tensor([1, 2]))
    rec = options.env_checkpoint_record(env)
    assert rec["env_io"] == {"sensor_noise": {"q": 0.01, "force": 2.0}, "action_delay": 3}
    assert same(rec["goal_curriculum"]["level"], torch.tensor([1, 2], dtype=torch.int64))
    # channels off: the scales of an env without channels are not recorded
    assert options.env_checkpoint_record(_full_env(tendon_obs=()))["tendon_obs"] == DEFAULT_RECORD["tendon_obs"]


def test_the_constructor_arguments_of_a_checkpoint():
    kw, needs_vec_env = options.env_kwargs_from_checkpoint(DEFAULT_RECORD)
    assert needs_vec_env is False
    assert kw == dict(tendon_obs=None, tendon_obs_scale=None, sensor_noise=None, action_delay=None, action_obs=None, goals=None, push=None)
    assert options.env_kwargs_from_checkpoint({"policy": {}}) == (kw, False)          # a checkpoint older than every option
    kw, needs_vec_env = options.env_kwargs_from_checkpoint(FULL_RECORD)
    assert needs_vec_env is True
    goals = kw.pop("goals")
    assert isinstance(goals, np.ndarray) and goals.dtype == np.float32 and np.array_equal(goals, ROWS)
    assert kw == dict(tendon_obs=["length", "force"], tendon_obs_scale=dict(zip(("length", "rate", "activation", "force"), SCALE)),
                      sensor_noise={"q": 0.01, "force": 2.0}, action_delay=(0, 2), action_obs=2, push={"prob": 0.02, "sigma": [0.5, 0.5, 0.5]})
    assert isinstance(kw["action_delay"], tuple)
    # one option at a time decides whether a RoboyVecEnv is needed; a goal pool alone does not (RoboyEnv's client takes the rows)
    for rec, needed in ((dict(DEFAULT_RECORD, goals=FULL_RECORD["goals"]), False),
                        (dict(DEFAULT_RECORD, env_push=FULL_RECORD["env_push"]), True),
                        (dict(DEFAULT_RECORD, env_io={"sensor_noise": {}, "action_delay": 2}), True),
                        (dict(DEFAULT_RECORD, env_io={"sensor_noise": {}, "action_delay": 0}), False),
                        (dict(DEFAULT_RECORD, env_io={"sensor_noise": {"q": 0.1}, "action_delay": None}), True),
                        (dict(DEFAULT_RECORD, env_io={"sensor_noise": {}, "action_delay": None, "action_obs": 1}), True),
                        (dict(DEFAULT_RECORD, reward_shaping=FULL_RECORD["reward_shaping"], goal_curriculum=FULL_RECORD["goal_curriculum"]), False)):
        assert options.env_kwargs_from_checkpoint(rec)[1] is needed, rec


def _quiet(call):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = call()
    assert not seen, [str(w.message) for w in seen]
    return out


def test_what_load_checks_on_the_env_side():
    ck = dict(FULL_RECORD, critic_obs_dim=27)
    env = _full_env()
    kept = _quiet(lambda: options.check_env_checkpoint(env, ck, critic_dim=27))
    # the levels went into the env (as many levels, as many envs); pool, counts and pushes are kept aside
    assert len(env.levels_set) == 1 and np.array_equal(env.levels_set[0], [0, 3])
    assert sorted(kept) == ["env_push", "goal_curriculum", "goal_row_stats", "goals"] and kept["goal_curriculum"] is None
    assert kept["goals"] is ck["goals"] and kept["goal_row_stats"] is ck["goal_row_stats"] and kept["env_push"] is ck["env_push"]
    # a plain env against a plain checkpoint, and against one older than every key
    for plain in (DEFAULT_RECORD, {}):
        assert _quiet(lambda: options.check_env_checkpoint(object(), plain)) == dict.fromkeys(("goals", "goal_row_stats", "goal_curriculum", "env_push"))
    # other rows: refused
    for other in (_full_env(tendon_obs=("length",)), _full_env(tendon_obs_scale=np.ones(4, np.float32)), object()):
        with pytest.raises(ValueError, match="the checkpoint was trained on the observation .* this env gives"):
            options.check_env_checkpoint(other, ck)
    with pytest.raises(ValueError, match="trained on the observation"):
        options.check_env_checkpoint(_full_env(), DEFAULT_RECORD)
    with pytest.raises(ValueError, match=r"critic was trained on the rows \['state', 'age', 'delay', 'actions'\] \(27 columns\), this env writes "
                                         r"\['state', 'age'\] \(27;"):
        options.check_env_checkpoint(_full_env(critic_obs_names=("state", "age")), ck, critic_dim=27)
    with pytest.raises(ValueError, match=r"\(27 columns\), this env writes .* \(19;"):
        options.check_env_checkpoint(_full_env(), ck, critic_dim=19)
    _quiet(lambda: options.check_env_checkpoint(_full_env(critic_obs_names=("state",)), ck))      # an agent that reads no critic rows
    # other weights: a warning, and the env's hold
    for other in (_full_env(reward_shaping=None), _full_env(reward_shaping=dict(FULL_RECORD["reward_shaping"], tension=0.5))):
        with pytest.warns(UserWarning, match="the checkpoint was trained with reward_shaping=.* this env runs reward_shaping="):
            options.check_env_checkpoint(other, ck)
    with pytest.warns(UserWarning, match="reward_shaping=None, this env runs"):
        options.check_env_checkpoint(_full_env(), {k: v for k, v in ck.items() if k != "reward_shaping"})
    # levels that do not fit stay aside: other number of levels, other number of envs, no curriculum
    for other in (_full_env(goal_curriculum=dict(levels=8, up=1, down=1, start=0)), _full_env(num_envs=3), _full_env(goal_curriculum=None)):
        kept = _quiet(lambda: options.check_env_checkpoint(other, ck))
        assert kept["goal_curriculum"] is ck["goal_curriculum"] and other.levels_set == []
    # other pushes, another pool: conditions of a run, no layout - nothing is said
    _quiet(lambda: options.check_env_checkpoint(_full_env(push=None, goal_pool_size=0), ck))


# ---- 4. the statistics block ----
OPTIONAL = {"levels": torch.tensor([3, 0, 1, 252]), "row_counts": np.arange(12, dtype=np.uint64).astype(np.float64),
            "pushes": [41, 2048.0], "shaping": [0.125, 2048.0]}


@pytest.mark.parametrize("present", [c for k in range(5) for c in itertools.combinations(OPTIONAL, k)], ids=lambda c: "+".join(c) or "none")
def test_segments_come_back_by_name_behind_the_sum(present):
    stats = [float(i) + 0.5 for i in range(len(STAT_KEYS))]
    segments = [("statistics", stats)] + [(name, OPTIONAL[name]) for name in present]
    block, layout = join_segments(segments)
    assert block.dtype == torch.float64 and block.ndim == 1
    flat = stats + [float(x) for name in present for x in OPTIONAL[name]]
    assert block.tolist() == flat                                  # the order given, nothing between
    summed = block * 2                                             # what two ranks with the same numbers sum to
    total = split_segments(summed, layout)
    assert list(total) == ["statistics"] + list(present)
    assert total["statistics"].tolist() == [2 * x for x in stats]
    for name in present:
        assert total[name].tolist() == [2 * float(x) for x in OPTIONAL[name]], name
    for name in OPTIONAL:
        if name not in present:
            with pytest.raises(KeyError):
                total[name]


def test_counts_are_exact_in_the_block():
    assert join_segments([("n", [2 ** 53 - 1])])[0].tolist() == [float(2 ** 53 - 1)]      # counts are exact in the block
