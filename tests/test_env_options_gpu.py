"""``gym_roboy_amd/envs/options.py`` end to end on the GPU: one short ``train_parallel`` run with every env option on, its checkpoint
against ``env_checkpoint_record``, a one-env ``RoboyVecEnv`` rebuilt from ``env_kwargs_from_checkpoint``, and ``visualize_agent`` on it."""
import os

import numpy as np
import pytest

from env_options_util import same

pytestmark = pytest.mark.gpu

EVERY_OPTION = ["--tendon-obs", "length,force", "--sensor-noise", "q=0.01,force=2", "--action-delay", "0:2", "--action-obs", "2",
                "--critic-obs", "state,age,delay,actions", "--goals", "reachable:256", "--goal-levels", "4", "--goal-order", "reach_rate",
                "--reward-shaping", "action_rate=0.05", "--push", "prob=0.02,sigma=0.5", "--bootstrap-timeouts"]
ENV_KEYS = ["critic_obs", "env_io", "env_push", "goal_curriculum", "goal_row_stats", "goals", "reward_shaping", "tendon_obs"]


def test_a_run_with_every_option_writes_the_record_and_plays_back_from_it(tmp_path, capsys):
    import torch
    from gym_roboy_amd import train_parallel, visualize_agent
    from gym_roboy_amd.envs.options import env_checkpoint_record, env_kwargs_from_checkpoint
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    out = str(tmp_path / "results")
    model = os.path.join(out, "model.pkl")
    agent = train_parallel.main(["256", out, "--rounds", "2", "--steps-per-round", str(256 * 8), "--n-steps", "8"] + EVERY_OPTION)
    try:
        text = capsys.readouterr().out
        rounds = [l for l in text.splitlines() if l.startswith("episode statistics (all ranks):")]
        assert len(rounds) == 2, text
        for line in rounds:
            for name in ("pushes_per_step", "shaping_cost_per_step", "mean_level", "reach_rate_whole_pool"):
                assert "'%s'" % name in line, (name, line)
        ck = torch.load(model)
        record = env_checkpoint_record(agent.env)
        assert sorted(record) == ENV_KEYS
        for key in ENV_KEYS:
            assert same(ck[key], record[key]), key
        assert ck["env_io"] == {"sensor_noise": {"q": 0.01, "force": 2.0}, "action_delay": [0, 2], "action_obs": 2}
        assert ck["critic_obs"] == ["state", "age", "delay", "actions"] and tuple(ck["goals"]["q"].shape) == (256, 3)
        assert agent.env.obs_dim == 41 and agent.env.goal_pool_size == 256
        kwargs, needs_vec_env = env_kwargs_from_checkpoint(ck)
        assert needs_vec_env
        one = RoboyVecEnv(MsjRobot(), 1, **kwargs)
        try:
            assert one.obs_dim == agent.env.obs_dim == 41 and one.reset().shape == (1, 41)
            assert one.tendon_obs == agent.env.tendon_obs and one.action_delay == agent.env.action_delay == (0, 2)
            assert one.push == agent.env.push and np.array_equal(one.goal_pool(), agent.env.goal_pool())
        finally:
            one.close()
    finally:
        agent.env.close()
    total = visualize_agent.main([model, "--steps", "3", "--pause", "0"])
    steps = [l for l in capsys.readouterr().out.splitlines() if l.startswith("step ")]
    assert len(steps) == 3 and np.isfinite(total)
