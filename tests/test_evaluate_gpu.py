"""Batched policy evaluation over the episode log (gym_roboy_amd/ppo.py: PPO.evaluate, evaluate_policy; gym_roboy_amd/evaluate_agent.py;
train_parallel --eval-every) on the GPU.

``evaluate`` is held, bit for bit, to a loop written out here: the same ``act_into(deterministic=True)`` and a twin env with the same
seed give the same planes and the same summary - nothing in it is approximate, so nothing here has a tolerance.  Training is held
untouched the same way: of two agents with the same seed, the one that evaluates between its rounds collects the same next rollout."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRAIN, N_EVAL, T, MAX_LEN, E = 256, 300, 8, 8, 2


def _env(n, seed, **kw):
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    return RoboyVecEnv(MsjRobot(), n, seed=seed, **kw)


def _agent(env, **kw):
    import torch
    from gym_roboy_amd.ppo import PPO
    torch.manual_seed(0)
    return PPO(env, n_steps=T, reward_scale=0.01, seed=0, device="cuda", **kw)


def _planes(env):
    d_count, d_ret, d_len, d_kind, d_full = env._episode_log_planes()
    env.sim.synchronize()
    n, cap = env.num_envs, env.episode_log_capacity
    return (env.sim.download(d_count, (n,), np.uint32), env.sim.download(d_ret, (cap, n)), env.sim.download(d_len, (cap, n), np.uint32),
            env.sim.download(d_kind, (cap, n), np.uint32), env.sim.download(d_full, (1,), np.uint32))


@pytest.mark.parametrize("case", ["plain", "normalize_obs", "asymmetric_critic"])
def test_evaluate_equals_the_loop_written_out(case):
    import torch
    train_kw = dict(critic_obs=("state", "age")) if case == "asymmetric_critic" else {}
    agent_kw = {"plain": {}, "normalize_obs": dict(normalize_obs=True), "asymmetric_critic": dict(asymmetric_critic=True)}[case]
    train = _env(N_TRAIN, 0, **train_kw)
    env, twin = (_env(N_EVAL, 9, max_episode_length=MAX_LEN, episode_log=E) for _ in range(2))
    try:
        agent = _agent(train, **agent_kw)
        assert agent._fused is not None
        agent.update(agent.collect())
        if case == "normalize_obs":
            assert agent.obs_norm.count > 0
        got = agent.evaluate(env, episodes_per_env=E, poll_every=4)
        assert got["complete"] is True and got["n_records"] == N_EVAL * E and got["n_complete"] == N_EVAL
        assert got["steps"] % 4 == 0 and got["steps"] <= E * MAX_LEN
        assert got["n_terminated"] + got["n_truncated"] == N_EVAL * E and got["sum_length"] <= N_EVAL * got["steps"]
        # the loop, written out
        dev = torch.device("cuda")
        obs = torch.as_tensor(twin.reset(), dtype=torch.float32, device=dev)
        twin.clear_episode_log()
        act, logp, val = torch.empty((N_EVAL, twin.n_t), device=dev), torch.empty(N_EVAL, device=dev), torch.empty(N_EVAL, device=dev)
        cobs = torch.zeros((N_EVAL, agent.cobs_dim), device=dev) if case == "asymmetric_critic" else None      # (the env writes no critic rows)
        packed = agent._fused.pack()
        for _ in range(got["steps"]):
            agent._fused.act_into(obs, act, logp, val, packed=packed, deterministic=True, norm=agent.obs_norm, cobs=cobs, cnorm=agent.cobs_norm)
            obs = twin.step(act)[0]
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(_planes(env), _planes(twin))):
            assert x.tobytes() == y.tobytes(), k
        want = twin.episode_log_summary(first_k=E)
        assert {k: np.float64(v).tobytes() for k, v in got.items() if k != "steps"} == {k: np.float64(v).tobytes() for k, v in want.items()}
        # a second evaluation on the same env starts over: reset, log cleared
        again = agent.evaluate(env, episodes_per_env=1, poll_every=1)
        assert again["n_records"] == N_EVAL and again["complete"] is True and again["steps"] <= MAX_LEN
    finally:
        train.close(); env.close(); twin.close()


@pytest.mark.parametrize("use_graphs", [False, True])
def test_training_is_untouched_by_an_evaluation_between_rounds(use_graphs):
    import torch
    rolls, counters = [], []
    for evaluates in (True, False):
        train = _env(N_TRAIN, 0)
        env = _env(N_EVAL, 9, max_episode_length=MAX_LEN, episode_log=1)
        try:
            agent = _agent(train, use_graphs=use_graphs)
            agent.update(agent.collect())
            before = (agent.num_timesteps, int(agent._step_base.item()), agent._epoch)
            if evaluates:
                assert agent.evaluate(env)["complete"] is True
                assert (agent.num_timesteps, int(agent._step_base.item()), agent._epoch) == before
            roll = agent.collect()
            torch.cuda.synchronize()
            rolls.append({k: roll[k].detach().cpu().numpy().copy() for k in ("obs", "act", "logp")})
            counters.append((agent.num_timesteps, int(agent._step_base.item()), agent._epoch))
        finally:
            train.close(); env.close()
    for k in ("obs", "act", "logp"):
        assert rolls[0][k].tobytes() == rolls[1][k].tobytes(), k
    assert counters[0] == counters[1] and np.isfinite(rolls[0]["logp"]).all()


def test_what_evaluate_refuses():
    train = _env(N_TRAIN, 0)
    wide, small, none = _env(64, 9, action_obs=1, episode_log=2), _env(64, 9, episode_log=1), _env(64, 9)
    try:
        agent = _agent(train)
        with pytest.raises(ValueError, match="an env of its own"):
            agent.evaluate(train)
        with pytest.raises(ValueError, match="reads 9 observation columns, this env gives 17"):
            agent.evaluate(wide, episodes_per_env=2)
        with pytest.raises(ValueError, match="episode_log >= 2, this one has episode_log=1"):
            agent.evaluate(small, episodes_per_env=2)
        with pytest.raises(ValueError, match="episode_log >= 1, this one has episode_log=None"):
            agent.evaluate(none)
        for bad in (dict(episodes_per_env=0), dict(poll_every=0)):
            with pytest.raises(ValueError, match="must be >= 1"):
                agent.evaluate(small, **bad)
    finally:
        for e in (train, wide, small, none):
            e.close()


def test_the_torch_path_evaluates_too():
    """an agent without the fused policy step: ``policy.act(deterministic=True)`` and the clamp the rollout applies"""
    train = _env(N_TRAIN, 0)
    env = _env(N_EVAL, 9, max_episode_length=MAX_LEN, episode_log=E)
    try:
        agent = _agent(train, fused_policy=False, fused_update=False)
        assert agent._fused is None
        got = agent.evaluate(env, episodes_per_env=E)
        assert got["complete"] is True and got["n_records"] == N_EVAL * E and got["steps"] == E * MAX_LEN
    finally:
        train.close(); env.close()


def test_train_parallel_evaluates_and_evaluate_agent_replays_the_checkpoint(tmp_path):
    results = tmp_path / "results"
    run = lambda *argv: subprocess.run([sys.executable, "-m"] + list(argv), cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = run("gym_roboy_amd.train_parallel", "256", str(results), "--rounds", "2", "--steps-per-round", str(256 * 8), "--n-steps", "8",
              "--eval-every", "1", "--eval-envs", "256", "--eval-episodes", "1", "--push", "prob=0.01,sigma=0.25")
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("episode statistics")]
    assert len(lines) == 2, out.stdout
    for line in lines:
        keys = {k: float(v) for k, v in re.findall(r"'(eval_[a-z_]+)': ([0-9.e+-]+|nan)", line)}
        assert sorted(keys) == ["eval_mean_length", "eval_mean_return", "eval_success_rate"], line
        assert 0.0 <= keys["eval_success_rate"] <= 1.0 and 1.0 <= keys["eval_mean_length"] <= 400.0
    model = str(results / "model.pkl")
    for name, flags, push in (("same", [], {"prob": 0.01, "sigma": [0.25] * 3}), ("pushed", ["--push", "prob=0.05,sigma=0.5"], {"prob": 0.05, "sigma": 0.5})):
        path = str(tmp_path / (name + ".json"))
        out = run("gym_roboy_amd.evaluate_agent", model, "--envs", "256", "--episodes", "1", "--max-episode-length", "40", "--json", path, *flags)
        assert out.returncode == 0, out.stdout + out.stderr
        printed = json.loads(out.stdout.strip().splitlines()[-1])
        with open(path) as f:
            saved = json.load(f)
        assert saved["summary"] == printed and printed["n_records"] == 256 and printed["complete"] is True and printed["steps"] <= 40
        assert saved["conditions"]["push"] == push and saved["conditions"]["episode_log"] == 1 and saved["conditions"]["max_episode_length"] == 40
        assert saved["flags"] == [f for f in flags if f.startswith("--")] and saved["timesteps"] == 2 * 256 * 8
