"""The episode log and the batched evaluation without a GPU: the option's validator, flag, checkpoint key and rule
(gym_roboy_amd/envs/options.py), ``evaluate_agent``'s command line, the summary's arithmetic, and the lane rule itself - the function
the kernel calls (csrc/env_episode_log.hpp: rbel::lane_step), built for the host with AddressSanitizer and UBSan as a program of its
own (tests/hostmath/episode_log_host.cpp) and held bit for bit to tests/episode_log_util.py's numpy restatement."""
import argparse
import os
import subprocess
import types

import numpy as np
import pytest

import episode_log_util as elu
from conftest import ROOT, build_dir
from gym_roboy_amd import _native as nat
from gym_roboy_amd.envs import options

CSRC = os.path.join(ROOT, "gym_roboy_amd", "csrc")


# ---- 1. the option's Python half ----
def test_the_validator():
    assert options.episode_log_capacity(None) == 0
    assert [options.episode_log_capacity(e) for e in (1, 3, np.int64(64))] == [1, 3, 64]
    assert nat.RB_EPISODE_LOG_MAX == 64
    for bad in (0, 65, -1, True, 2.0, "3", (1,)):
        with pytest.raises(ValueError, match="episode_log: an int, 1 <= E <= 64"):
            options.episode_log_capacity(bad)


def _parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("num_envs", type=int)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bootstrap-timeouts", action="store_true")
    options.add_env_arguments(ap)
    options.add_env_arguments(ap, late=True)
    return ap


def test_the_flag():
    assert [row[0] for row in options.ENV_FLAGS].count("--episode-log") == 1
    ap = _parser()
    assert "episode_log" not in options.env_kwargs_from_args(ap.parse_args(["4"]))
    assert options.env_kwargs_from_args(ap.parse_args(["4", "--episode-log", "5"]))["episode_log"] == 5
    off = options.env_kwargs_from_args(ap.parse_args(["4"]))
    assert options.env_kwargs_from_args(ap.parse_args(["4", "--episode-log", "5"])) == dict(off, episode_log=5)
    with pytest.raises(ValueError, match="episode_log"):
        options.env_kwargs_from_args(ap.parse_args(["4", "--episode-log", "65"]))


def test_the_checkpoint_key_and_its_absence():
    plain = options.env_checkpoint_record(types.SimpleNamespace())
    assert "episode_log" not in plain and "episode_log" not in options.env_checkpoint_record(types.SimpleNamespace(episode_log_capacity=0))
    assert options.env_checkpoint_record(types.SimpleNamespace(episode_log_capacity=7)) == dict(plain, episode_log=7)
    # a condition of the run, not a layout: not taken over
    kw, needs_vec_env = options.env_kwargs_from_checkpoint(dict(plain, episode_log=7))
    assert "episode_log" not in kw and needs_vec_env is False
    assert (kw, needs_vec_env) == options.env_kwargs_from_checkpoint(plain)


def test_the_rule_of_check_env_checkpoint():
    plain = options.env_checkpoint_record(types.SimpleNamespace())
    aside = options.check_env_checkpoint(types.SimpleNamespace(), plain)
    # any capacity of this env against any capacity of the checkpoint: nothing is said, nothing is taken over
    for own in (0, 2):
        for saved in (None, 1, 64):
            ck = dict(plain) if saved is None else dict(plain, episode_log=saved)
            assert options.check_env_checkpoint(types.SimpleNamespace(episode_log_capacity=own), ck) == aside
    for bad in (0, 65, "many"):
        with pytest.raises(ValueError, match="episode_log"):
            options.check_env_checkpoint(types.SimpleNamespace(), dict(plain, episode_log=bad))


# ---- 2. the summary's arithmetic ----
def test_the_figures_against_numpy_on_hand_made_planes():
    rng = np.random.default_rng(3)
    n, cap = 37, 5
    count = rng.integers(0, cap + 1, n)
    count[:3] = (0, cap, 1)
    log = {"count": count.astype(np.int64), "return": rng.normal(-40, 25, (n, cap)).astype(np.float32),
           "length": rng.integers(1, 400, (n, cap)).astype(np.int64), "kind": rng.integers(1, 3, (n, cap)).astype(np.int64)}
    for first_k in (1, 3, cap, cap + 1):
        sums, _, _ = elu.summary_np(log, first_k)
        got = options.episode_log_figures([sums[k] for k in elu.SUMS] + [0.0], n)
        live = np.arange(cap)[None, :] < np.minimum(count, first_k)[:, None]
        r = log["return"].astype(np.float64)[live]
        assert got["n_records"] == live.sum() and {k: got[k] for k in elu.SUMS} == sums
        assert got["mean_return"] == pytest.approx(r.mean(), rel=1e-13) and got["std_return"] == pytest.approx(r.std(), rel=1e-10)
        assert got["mean_length"] == pytest.approx(log["length"][live].mean(), rel=1e-13)
        assert got["success_rate"] == pytest.approx((log["kind"][live] == 1).mean(), rel=1e-13)
        assert got["success_rate"] + got["truncated_rate"] == pytest.approx(1.0, rel=1e-13)
        assert got["complete"] is bool((count >= first_k).all()) is False
    full = dict(log, count=np.full(n, cap, np.int64))
    assert options.episode_log_figures([elu.summary_np(full, cap)[0][k] for k in elu.SUMS], n)["complete"] is True
    empty = options.episode_log_figures([0.0] * 8, n)
    assert empty["n_records"] == 0 and all(np.isnan(empty[k]) for k in ("mean_return", "std_return", "mean_length", "success_rate")) \
        and empty["complete"] is False


def test_the_model_on_a_sequence_worked_by_hand():
    m = elu.EpisodeLogModel(2, 2)
    third = np.float32(1) / np.float32(3)
    for rew, done, term in (((third, 1.0), (0, 1), (0, 1)), ((third, 2.0), (0, 0), (0, 0)), ((third, 3.0), (1, 1), (0, 0)),
                            ((1.0, 1.0), (1, 1), (1, 0))):
        m.step_outcome(np.array(rew, np.float32), np.array(done), np.array(term))
    log = m.log()
    assert log["count"].tolist() == [2, 2] and m.full == 2
    assert log["return"][0, 0] == np.float32(np.float32(third + third) + third) and log["return"][0, 1] == 1.0
    assert log["return"][1].tolist() == [1.0, 5.0] and log["length"].tolist() == [[3, 1], [1, 2]]
    assert log["kind"].tolist() == [[2, 1], [1, 2]]                # env 1's third episode (truncated, return 1) found the log full
    assert m.acc.tolist() == [0.0, 0.0] and m.age.tolist() == [0, 0]


# ---- 3. the lane rule built for the host, under the sanitizers ----
@pytest.fixture(scope="module")
def host_program():
    exe = os.path.join(build_dir(), "episode_log_host_san")
    src = os.path.join(ROOT, "tests", "hostmath", "episode_log_host.cpp")
    deps = [src, os.path.join(CSRC, "env_episode_log.hpp"), os.path.join(ROOT, "include", "roboy_sim.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                               "-I", CSRC, "-o", exe, src])
    return exe


def _sequences(n, T, seed, wrap):
    """rewards of mixed magnitude (the fp32 sum's order matters), done rates from 0.05 to 1 per env, counters that move on half of the
    episode ends - from just below 2^32 where ``wrap``"""
    rng = np.random.default_rng(seed)
    reward = (rng.normal(0, 1, (T, n)) * 10.0 ** rng.integers(-3, 4, (T, n))).astype(np.float32)
    p_done = np.linspace(0.05, 1.0, n)[rng.permutation(n)]
    done = rng.random((T, n)) < p_done
    moved = done & (rng.random((T, n)) < 0.5)
    start = np.full(n, 2 ** 32 - 3 if wrap else 0, np.uint64) + rng.integers(0, 3, n).astype(np.uint64)
    reached = ((start[None, :] + np.cumsum(moved, axis=0).astype(np.uint64)) % np.uint64(2 ** 32)).astype(np.uint32)
    return reward, done, reached, (start % np.uint64(2 ** 32)).astype(np.uint32)


@pytest.mark.parametrize("capacity,T,wrap", [(1, 12, False), (3, 40, True), (64, 96, True), (64, 30, False)])
def test_host_program_equals_the_model_bit_for_bit(host_program, capacity, T, wrap):
    n = 1500
    reward, done, reached, seen0 = _sequences(n, T, 100 + capacity + T, wrap)
    model = elu.EpisodeLogModel(n, capacity, reached=seen0)
    for t in range(T):
        model.step(reward[t], done[t], reached[t])
    # the cases this run is for
    if T >= capacity:
        assert (model.count == capacity).sum() >= 8 and ((done.sum(axis=0) > capacity) & (model.count == capacity)).sum() >= 8      # saturation
    else:
        assert model.count.max() < capacity
    if wrap:
        wrapped = reached[-1] < seen0
        assert wrapped.sum() >= 100 and (model.kind[:, wrapped] == elu.TERMINATED).any() and (model.kind[:, wrapped] == elu.TRUNCATED).any()
    words = np.stack((reward.view(np.uint32), done.astype(np.uint32), reached), axis=2).reshape(-1, 3)
    text = "%d %d %d\n%s\n%s\n" % (n, capacity, T, " ".join(map(str, seen0)), "\n".join("%d %d %d" % tuple(w) for w in words))
    run = subprocess.run([host_program], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split("\n")
    state = np.array([line.split() for line in lines[:n]], dtype=np.uint32)
    records = np.array([line.split() for line in lines[n:n + capacity * n]], dtype=np.uint32).reshape(capacity, n, 3)
    assert int(lines[n + capacity * n]) == model.full == int((model.count == capacity).sum())
    assert np.array_equal(state[:, 0], model.count) and np.array_equal(state[:, 1], model.acc.view(np.uint32))
    assert np.array_equal(state[:, 2], model.age) and np.array_equal(state[:, 3], model.seen)
    assert np.array_equal(records[:, :, 0], model.ret.view(np.uint32)) and np.array_equal(records[:, :, 1], model.len)
    assert np.array_equal(records[:, :, 2], model.kind)
    assert set(np.unique(model.kind)) <= {0, elu.TERMINATED, elu.TRUNCATED} and (model.kind != 0).sum() == model.count.sum()


# ---- 4. evaluate_agent's command line ----
CK_RECORD = {
    "tendon_obs": {"channels": ["length", "force"], "scale": [4.0, 1.0, 1.0, 0.0025]},
    "env_io": {"sensor_noise": {"q": 0.01}, "action_delay": [0, 2], "action_obs": 2},
    "env_push": {"prob": 0.02, "sigma": [0.5, 0.5, 0.5], "threshold": 335544},
    "reward_shaping": {"action_rate": 0.05, "tension": 0.0, "activation": 0.0}, "episode_log": 9,
}


def _conditions(argv, ck=CK_RECORD):
    from gym_roboy_amd import evaluate_agent as ea
    args = ea.parser().parse_args(["model.pkl"] + argv)
    return ea.env_conditions(ck, args, argv)


def test_evaluate_agent_parser():
    from gym_roboy_amd import evaluate_agent as ea
    args = ea.parser().parse_args(["m.pkl"])
    assert (args.model, args.envs, args.episodes, args.seed, args.max_episode_length, args.json) == ("m.pkl", 4096, 1, 1, 400, None)
    args = ea.parser().parse_args(["m.pkl", "--envs", "256", "--episodes", "3", "--seed", "5", "--max-episode-length", "50", "--json", "o.json",
                                   "--push", "prob=0.05,sigma=0.5"])
    assert (args.envs, args.episodes, args.seed, args.max_episode_length, args.json, args.push) == (256, 3, 5, 50, "o.json", "prob=0.05,sigma=0.5")
    # every env flag is taken, and every one has its keys
    assert set(ea.FLAG_KEYS) == {row[0] for row in options.ENV_FLAGS}
    assert ea.given_flags(["m.pkl", "--push=prob=1,sigma=1", "--envs", "4", "--action-delay", "2"]) == ["--action-delay", "--push"]
    for bad in (["--episodes", "0"], ["--episodes", "65"], ["--envs", "0"]):
        with pytest.raises(SystemExit):
            ea.main(["m.pkl"] + bad)


def test_evaluate_agent_takes_the_checkpoints_conditions():
    kw, given = _conditions(["--episodes", "2", "--seed", "4", "--max-episode-length", "30"])
    assert given == []
    assert kw == dict(tendon_obs=["length", "force"], tendon_obs_scale=dict(zip(("length", "rate", "activation", "force"), CK_RECORD["tendon_obs"]["scale"])),
                      sensor_noise={"q": 0.01}, action_delay=(0, 2), action_obs=2, goals=None, push={"prob": 0.02, "sigma": [0.5, 0.5, 0.5]},
                      seed=4, integrator=options.ENV_INTEGRATOR, max_episode_length=30, episode_log=2)
    # a plain checkpoint: a plain env with the evaluation's own log (the checkpoint's capacity is not taken over)
    kw, _ = _conditions([], ck={})
    assert kw["episode_log"] == 1 and kw["push"] is None and kw["tendon_obs"] is None and kw["seed"] == 1


def test_evaluate_agent_flags_replace_the_checkpoints_conditions():
    base, _ = _conditions([])
    kw, given = _conditions(["--push", "prob=0.05,sigma=0.5"])
    assert given == ["--push"] and kw == dict(base, push={"prob": 0.05, "sigma": 0.5})
    kw, _ = _conditions(["--push", ""])                                   # given and empty: no pushes
    assert "push" not in kw and {k: v for k, v in base.items() if k != "push"} == kw
    kw, given = _conditions(["--sensor-noise", "q=0.1,qd=0.2", "--action-delay", "3"])
    assert given == ["--sensor-noise", "--action-delay"] and kw == dict(base, sensor_noise={"q": 0.1, "qd": 0.2}, action_delay=3)
    kw, _ = _conditions(["--goals", "reachable:64"])
    assert kw["goals"] is True                                            # a pool to be made; without the flag the checkpoint's rows (none here)
    kw, _ = _conditions(["--reward-shaping", "action_rate=0.5"])
    assert kw["reward_shaping"] == {"action_rate": 0.5}
    # the layout flags are taken like the others - the width check in main() then says which to drop
    kw, given = _conditions(["--action-obs", "1"])
    assert kw["action_obs"] == 1 and given == ["--action-obs"]
    # --episode-log is not the evaluation's capacity: --episodes is
    kw, _ = _conditions(["--episode-log", "7", "--episodes", "2"])
    assert kw["episode_log"] == 2
    with pytest.raises(ValueError, match="push"):
        _conditions(["--push", "prob=2,sigma=1"])
