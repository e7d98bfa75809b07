"""Start poses without a GPU (include/roboy_sim.h: rb_env_start_poses_*; csrc/env_start.hpp): the rule restated in
tests/start_pose_util.py against the host program built from the function the kernel calls; the GPU tests' seed, probability and pool
size qualified on the restated rule alone; the command line, the checkpoint record and its replay as literal dicts; every ValueError
and SystemExit of the validator and the parsers; the new symbols of the header in the library."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import start_pose_util as su
from env_options_util import same
from gym_roboy_amd import _native as nat
from gym_roboy_amd.envs import options
from start_pose_util import M, MAX_LEN, N, PROB, SEED, STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym_roboy_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()


# ---- 1. the restated rule against the shared function ----
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("start_pose_host") / "start_pose_host")
    src = os.path.join(ROOT, "tests", "hostmath", "start_pose_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, src])
    return exe


def _grid():
    rows = []
    for seed in (0, SEED, 2 ** 40 + 5):
        for threshold in (0, 1, su.threshold_of(PROB), 2 ** 24 - 1, 2 ** 24):
            for m in (1, M, 4096, 2 ** 32 - 1):
                for gid in (0, 1, 199, 2 ** 33 + 7):
                    for d in (0, 1, 2, 3, 5, 255, 2 ** 32 - 1):
                        rows.append((seed, gid, d, threshold, m))
    return rows


def test_the_host_program_equals_the_restatement(host_program):
    rows = _grid()
    assert len(rows) > 1500
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    out = subprocess.run([host_program], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)
    assert got.shape == (len(rows), 2)
    for (seed, gid, d, threshold, m), (index, count) in zip(rows, got):
        assert index == int(su.index_of(seed, [gid], d, threshold, m)[0]), (seed, gid, d, threshold, m)
        assert count == (d + 1) % 2 ** 32
    # the edges: threshold 0 never, 2^24 always, m = 1 row 0
    by = {r: g for r, g in zip(rows, got)}
    assert all(g[0] == su.INDEX_REST for r, g in by.items() if r[3] == 0)
    assert all(g[0] < r[4] for r, g in by.items() if r[3] == 2 ** 24)
    assert all(g[0] == 0 for r, g in by.items() if r[3] == 2 ** 24 and r[4] == 1)
    assert {g[0] == su.INDEX_REST for r, g in by.items() if r[3] == su.threshold_of(PROB)} == {True, False}


def test_several_thousand_pairs_of_one_env_batch(host_program):
    gids, ds = np.meshgrid(np.arange(386), np.arange(12), indexing="ij")
    gids, ds = gids.reshape(-1), ds.reshape(-1)
    threshold = su.threshold_of(PROB)
    text = "".join("%d %d %d %d %d\n" % (SEED, g, d, threshold, M) for g, d in zip(gids, ds))
    out = subprocess.run([host_program], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)
    assert got.shape == (386 * 12, 2)
    assert np.array_equal(got[:, 0], su.index_of(SEED, gids, ds, threshold, M).astype(np.int64))
    assert np.array_equal(got[:, 1], ds + 1)


def test_the_restatement_itself():
    assert su.threshold_of(0) == 0 and su.threshold_of(1) == 2 ** 24 and su.threshold_of(0.5) == 2 ** 23
    gids = np.arange(4096)
    from_pool, row = su.draw(SEED, gids, 0, 2 ** 23, M)
    assert 0.45 < from_pool.mean() < 0.55 and row.min() == 0 and row.max() == M - 1
    # decision and row come from different words of the block: the row's distribution does not depend on the decision
    assert set(row[from_pool]) == set(row[~from_pool]) == set(range(M))
    book = su.Book(SEED, 8, 2 ** 24, M)
    assert book.start().all() and np.all(book.count == 1)
    who = np.arange(8) % 2 == 0
    first = book.index.copy()
    book.start(who)
    assert np.array_equal(book.count, 1 + who) and np.array_equal(book.index[~who], first[~who])
    assert np.array_equal(book.index[who], su.index_of(SEED, np.arange(8), 1, 2 ** 24, M)[who])


# ---- 2. the GPU tests' inputs, on the restated rule alone ----
def test_the_gpu_inputs_exercise_every_row_and_both_outcomes():
    """An env whose episodes are MAX_LEN = 5 steps long starts at the reset (d = 0) and, over STEPS = 12 steps, at least twice more
    (d = 1, 2; an env that reaches a goal early starts more often): the draws d = 0 .. 2 of the N = 200 envs are a lower bound on what
    a run exercises."""
    assert STEPS // MAX_LEN == 2
    threshold = su.threshold_of(PROB)
    gids = np.arange(N)
    at_reset = su.index_of(SEED, gids, 0, threshold, M)
    assert (at_reset == su.INDEX_REST).any() and (at_reset != su.INDEX_REST).any()           # both outcomes at the reset
    in_steps = np.concatenate([su.index_of(SEED, gids, d, threshold, M) for d in (1, 2)])
    assert (in_steps == su.INDEX_REST).any() and (in_steps != su.INDEX_REST).any()           # ... and among the starts of the run
    every = np.concatenate((at_reset, in_steps))
    assert set(every[every != su.INDEX_REST].tolist()) == set(range(M))                      # every one of the 7 rows is drawn
    # the two shards of 193 envs and the 386-env batch: both outcomes in either half
    for lo in (0, 193):
        half = su.index_of(SEED, np.arange(lo, lo + 193), 0, threshold, M)
        assert (half == su.INDEX_REST).any() and (half != su.INDEX_REST).any()


# ---- 3. the command line, the record, the replay ----
class FakePool:
    def __init__(self, m, seed):
        self.m, self.seed, self.recipe = m, seed, {"kind": "reachable", "m": m, "seed": seed}
        self.q = np.zeros((m, 3), np.float32)

    def __eq__(self, other):
        return isinstance(other, FakePool) and (self.m, self.seed) == (other.m, other.seed)


BASE = dict(seed=0, device=0, integrator="euler", goals=None, env_id_offset=0, tendon_obs=None, tendon_obs_scale=None, sensor_noise=None,
            action_delay=None, report_truncation=False, action_obs=None, critic_obs=None, goal_curriculum=None)
COMMAND_LINES = [
    ([], {}),
    (["--start-poses", "reachable"], dict(start_poses=FakePool(4096, 1), start_prob=1.0)),
    (["--start-poses", "reachable:64", "--start-prob", "0.5"], dict(start_poses=FakePool(64, 1), start_prob=0.5)),
    (["--seed", "4", "--start-poses", "reachable:8", "--start-prob", "0"], dict(seed=4, start_poses=FakePool(8, 5), start_prob=0.0)),
    (["--push", "prob=0.02,sigma=0.5"], dict(push={"prob": 0.02, "sigma": 0.5})),
]


def _run_main(argv, monkeypatch, tmp_path):
    import gym_roboy_amd.envs.goals as envgoals
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
        raise Stop

    def fake_pool(robot, m, seed=0, integrator=None, device=0):
        seen.setdefault("pools", []).append(dict(m=m, seed=seed, integrator=integrator, device=device))
        return FakePool(m, seed)

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
    assert seen["env"] == dict(BASE, **changed)
    for key in ("start_poses", "start_prob"):
        assert (key in seen["env"]) == (key in changed), key
    if "start_poses" in changed:                                    # the run's seed + 1: not the goal pool
        assert seen["pools"] == [dict(m=changed["start_poses"].m, seed=seen["env"]["seed"] + 1, integrator="euler", device=0)]
    else:
        assert "pools" not in seen


def test_the_goal_pool_and_the_start_pool_are_two_pools(monkeypatch, tmp_path, capsys):
    seen = _run_main(["--goals", "reachable:32", "--start-poses", "reachable:16"], monkeypatch, tmp_path)
    assert seen["pools"] == [dict(m=32, seed=0, integrator="euler", device=0), dict(m=16, seed=1, integrator="euler", device=0)]


def test_env_kwargs_from_args_names_the_request():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bootstrap-timeouts", action="store_true")
    options.add_env_arguments(ap)
    options.add_env_arguments(ap, late=True)
    static = {k: v for k, v in BASE.items() if k not in ("goals", "device", "env_id_offset")}
    assert options.env_kwargs_from_args(ap.parse_args([])) == static
    assert options.env_kwargs_from_args(ap.parse_args(["--start-poses", "reachable:9", "--start-prob", "0.25"])) == \
        dict(static, start_poses={"m": 9, "prob": 0.25})
    assert options.env_kwargs_from_args(ap.parse_args(["--start-poses", "reachable"])) == dict(static, start_poses={"m": 4096, "prob": 1.0})


ROWS = np.arange(6, dtype=np.float32).reshape(2, 3) / 16
DEFAULT_RECORD = {"tendon_obs": {"channels": [], "scale": [1.0, 1.0, 1.0, 1.0]}, "env_io": {"sensor_noise": {}, "action_delay": None}}
START_RECORD = {"q": torch.from_numpy(ROWS), "prob": 0.5, "threshold": 2 ** 23, "recipe": {"kind": "reachable", "m": 2}}


def _env(**over):
    env = types.SimpleNamespace(start_poses_size=2, start_prob=0.5, start_pose_pool=lambda: ROWS.copy(), start_recipe={"kind": "reachable", "m": 2})
    vars(env).update(over)
    return env


def test_the_record_and_its_replay():
    assert same(options.env_checkpoint_record(_env()), dict(DEFAULT_RECORD, env_start_poses=START_RECORD))
    # an env without the option writes exactly what it wrote
    assert same(options.env_checkpoint_record(_env(start_poses_size=0)), DEFAULT_RECORD)
    assert same(options.env_checkpoint_record(object()), DEFAULT_RECORD)
    # start_prob 0 stays a configured option
    rec = options.env_checkpoint_record(_env(start_prob=0.0))["env_start_poses"]
    assert rec["prob"] == 0.0 and rec["threshold"] == 0
    # load(): a condition of the run, kept aside; absent when the checkpoint has none
    ck = dict(DEFAULT_RECORD, env_start_poses=START_RECORD)
    kept = options.check_env_checkpoint(object(), ck)
    assert sorted(kept) == ["env_push", "env_start_poses", "goal_curriculum", "goal_row_stats", "goals"] and kept["env_start_poses"] is START_RECORD
    assert options.check_env_checkpoint(object(), DEFAULT_RECORD) == dict.fromkeys(("goals", "goal_row_stats", "goal_curriculum", "env_push"))
    # the replay
    plain = dict(tendon_obs=None, tendon_obs_scale=None, sensor_noise=None, action_delay=None, action_obs=None, goals=None, push=None)
    assert options.env_kwargs_from_checkpoint(DEFAULT_RECORD) == (plain, False)
    kw, needs_vec_env = options.env_kwargs_from_checkpoint(ck)
    assert needs_vec_env is False                                   # (the single RoboyEnv plays from rest)
    rows = kw.pop("start_poses")
    assert isinstance(rows, np.ndarray) and rows.dtype == np.float32 and np.array_equal(rows, ROWS)
    assert kw == dict(plain, start_prob=0.5)


def test_evaluate_agent_replaces_the_condition():
    from gym_roboy_amd import evaluate_agent as ev
    ck = dict(DEFAULT_RECORD, env_start_poses=START_RECORD)
    for argv, want in (([], ("rows", 0.5)), (["--start-poses", "reachable:64"], ({"m": 64, "prob": 1.0}, None)),
                       (["--start-poses", "reachable:64", "--start-prob", "0.25"], ({"m": 64, "prob": 0.25}, None)),
                       (["--start-prob=0.5", "--start-poses=reachable"], ({"m": 4096, "prob": 0.5}, None))):
        argv = ["model.pkl"] + argv
        kw, given = ev.env_conditions(ck, ev.parser().parse_args(argv), argv)
        assert given == [f for f in ("--start-poses", "--start-prob") if any(w.startswith(f) for w in argv)]
        if want[0] == "rows":
            assert np.array_equal(kw["start_poses"], ROWS) and kw["start_prob"] == want[1]
        else:
            assert kw["start_poses"] == want[0] and "start_prob" not in kw
    kw, _ = ev.env_conditions(DEFAULT_RECORD, ev.parser().parse_args(["model.pkl"]), ["model.pkl"])
    assert "start_poses" not in kw and "start_prob" not in kw


def test_the_statistics_segment():
    from gym_roboy_amd.sharding import STAT_KEYS, join_segments, split_segments
    block, layout = join_segments([("statistics", [0.5] * len(STAT_KEYS)), ("pushes", [3, 10.0]), ("start_poses", [96, 200.0])])
    total = split_segments(block * 2, layout)
    assert total["start_poses"].tolist() == [192.0, 400.0] and list(total) == ["statistics", "pushes", "start_poses"]


# ---- 4. every ValueError and SystemExit ----
def test_the_validator():
    lo, hi = -np.ones(3, np.float32), np.ones(3, np.float32)
    assert options.start_pose_spec(None, 1.0, 3, lo, hi) is None
    spec = options.start_pose_spec(ROWS, 0.5, 3, lo, hi)
    assert sorted(spec) == ["prob", "q", "recipe", "threshold"] and spec["prob"] == 0.5 and spec["threshold"] == 2 ** 23 and spec["recipe"] == {}
    assert spec["q"].dtype == np.float32 and spec["q"].flags.c_contiguous and np.array_equal(spec["q"], ROWS)
    assert options.start_pose_spec(ROWS, 0, 3, lo, hi)["threshold"] == 0 and options.start_pose_spec(ROWS, 1, 3, lo, hi)["threshold"] == 2 ** 24
    from gym_roboy_amd.envs.goals import GoalPool
    assert options.start_pose_spec(GoalPool(ROWS, {"m": 2}), 1.0, 3, lo, hi)["recipe"] == {"m": 2}
    for prob in (-0.1, 1.5, float("nan"), float("inf"), True, "0.5", None, [0.5]):
        with pytest.raises(ValueError, match="start_prob must be in"):
            options.start_pose_spec(ROWS, prob, 3, lo, hi)
    with pytest.raises(ValueError, match="start_prob needs start_poses"):
        options.start_pose_spec(None, 0.5, 3, lo, hi)
    bad = ROWS.copy()
    bad[1, 2] = 1.5
    for rows, match in ((bad, "start_poses: goals must lie inside"), (ROWS[:, :2], r"start_poses: goals must have shape \(m, 3\)"),
                        (np.zeros((0, 3), np.float32), "start_poses: goals must have shape"), (ROWS * np.nan, "start_poses: goals must be finite")):
        with pytest.raises(ValueError, match=match):
            options.start_pose_spec(rows, 0.5, 3, lo, hi)
    with pytest.raises(ValueError, match="has 5 rows"):
        options.start_pose_spec(ROWS, 0.5, 3, lo, hi, m=5)


def test_the_parsers():
    assert options.parse_start_poses("") == (0, 1.0) and options.parse_start_poses("", None) == (0, 1.0)
    assert options.parse_start_poses("reachable") == (4096, 1.0) and options.parse_start_poses("reachable:7", 0.25) == (7, 0.25)
    for text in ("bogus", "reachable:0", "reachable:x", "reachable:-3", "box:4"):
        with pytest.raises(SystemExit, match="--start-poses takes"):
            options.parse_start_poses(text)
    for prob in (-0.5, 1.01, float("nan")):
        with pytest.raises(SystemExit, match="--start-prob takes"):
            options.parse_start_poses("reachable", prob)
    with pytest.raises(SystemExit, match="--start-prob needs --start-poses"):
        options.parse_start_poses("", 0.5)


def test_bad_flags_end_main_before_a_gpu_is_touched(tmp_path):
    import gym_roboy_amd.train_parallel as tp
    with pytest.raises(SystemExit, match="--start-poses takes"):
        tp.main(["4", str(tmp_path), "--start-poses", "everywhere"])
    with pytest.raises(SystemExit, match="--start-prob needs"):
        tp.main(["4", str(tmp_path), "--start-prob", "0.5"])
    with pytest.raises(SystemExit, match="--start-prob takes"):
        tp.main(["4", str(tmp_path), "--start-poses", "reachable", "--start-prob", "2"])


# ---- 5. the header and the library ----
def test_the_new_symbols_are_declared_and_the_abi_number_stands():
    lib = nat.load()
    for name in ("rb_env_start_poses_configure", "rb_env_start_poses_set", "rb_env_start_poses_ptr"):
        assert re.search(r"\bint %s\(rb_sim \*sim" % name, HEADER) and name in nat.SIGNATURES and hasattr(lib, name)
    assert int(re.search(r"#define RB_ABI_VERSION (\d+)", HEADER).group(1)) == 6 == lib.rb_abi_version()
    assert int(re.search(r"#define RB_START_INDEX_REST 0x([0-9A-F]+)u", HEADER).group(1), 16) == nat.RB_START_INDEX_REST == su.INDEX_REST
    src = open(os.path.join(CSRC, "env_start.hpp")).read()
    assert int(re.search(r"STREAM_START = (\d+)", src).group(1)) == su.STREAM_START == 7
