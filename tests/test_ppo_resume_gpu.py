"""GPU tests of a checkpoint that continues the run (PPO.save(path, resume=True) / PPO.load; train_parallel --exact-resume; DESIGN.md
§31).  On the fused paths the agent and its env are deterministic, so the statement is exact: a run that was stopped at a backup and
continued from it IS the run that went on - policy, optimiser, statistics, noise step base, rollouts and env state, bit for bit.  Each
case carries its control (the continuous run twice), and the comparison is shown once to fail where the record is ignored."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import env_state_util as esu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, MAX_LEN = 256, 16, 12          # episodes end inside a rollout of 16 steps: truncations are bootstrapped, delays redrawn

ENV_ALL = dict(sensor_noise={"q": 0.01, "qd": 0.05}, action_delay=(0, 3), action_obs=2, critic_obs=("state", "age", "delay", "actions"),
               report_truncation=True)
CASES = {
    # name: (env options, agent options)
    "eager_plain": ({}, dict(use_graphs=False)),
    # every agent option that keeps something between calls, on an env with noise, delay and critic rows; normalize_obs /
    # normalize_reward put the priming rollout in front of the first one - the step base then runs ahead of num_timesteps
    "graph_all": (ENV_ALL, dict(use_graphs=True, normalize_obs=True, normalize_reward=True, bootstrap_timeouts=True, lr_schedule="adaptive",
                                asymmetric_critic=True)),
    "graph_symmetry_loss": ({}, dict(use_graphs=True, symmetry="loss")),
}


def _env(case, seed=3):
    from gym_roboy_amd.envs.robots import MsjRobot
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    return RoboyVecEnv(MsjRobot(), N, seed=seed, max_episode_length=MAX_LEN, **CASES[case][0])


def _agent(env, case, **kw):
    from gym_roboy_amd.ppo import PPO
    return PPO(env, **dict(dict(n_steps=T, nminibatches=2, noptepochs=2, reward_scale=0.01, seed=0, device="cuda", fused_policy=True,
                                fused_update=True), **CASES[case][1], **kw))


def _round(agent):
    """one collect() + update(); the rollout as numpy copies (graph mode hands out views of the graph's buffers)"""
    roll = agent.collect()
    kept = {k: v.detach().cpu().numpy().copy() for k, v in roll.items()}
    agent.update(roll)
    return kept


def _snapshot(agent):
    """everything the issue names, as numpy / numbers"""
    import torch
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu().numpy().copy()
    snap = {"policy": {k: cpu(v) for k, v in agent.policy.state_dict().items()},
            "adam": {"m": cpu(agent._fadam.m), "v": cpu(agent._fadam.v), "t": int(agent._fadam.t)},
            "lr": float(agent.learning_rate), "num_timesteps": int(agent.num_timesteps), "step_base": int(agent._step_base.item()),
            "epoch": int(agent._epoch), "obs": cpu(agent._obs), "cobs": None if agent._cobs is None else cpu(agent._cobs)}
    for name in ("obs_norm", "cobs_norm", "reward_norm"):
        n = getattr(agent, name)
        snap[name] = None if n is None else {"state": cpu(n.state), "norm": cpu(n.norm)}
    snap["ret_carry"] = None if agent.reward_norm is None else cpu(agent.reward_norm.ret_carry)
    sd = agent.env.state_dict(dict_view=True)
    snap["env"] = esu.to_np({k: v for k, v in sd.items() if k != "blob"})
    return snap


def _continuous(case, rounds=3):
    env = _env(case)
    try:
        agent = _agent(env, case)
        rolls = [_round(agent) for _ in range(rounds)]
        return rolls, _snapshot(agent)
    finally:
        env.close()


def _same(a, b, what):
    diff = esu.first_difference(a, b, what)
    assert diff is None, diff


@pytest.mark.parametrize("case", list(CASES))
def test_a_resumed_run_is_the_continuous_run(case, tmp_path):
    path = str(tmp_path / "model.pkl")
    rolls, want = _continuous(case)
    # the control: the continuous run twice
    rolls2, again = _continuous(case)
    _same(rolls2, rolls, "control, rollouts")
    _same(again, want, "control")
    if case == "graph_all":           # the priming rollout is in: the step base runs one rollout ahead of the counted timesteps
        assert want["step_base"] == 4 * T and want["num_timesteps"] == 3 * T * N
    # B: one round, then the backup
    env = _env(case)
    try:
        b = _agent(env, case)
        first = _round(b)
        _same(first, rolls[0], "B's first rollout")
        b.save(path, resume=True)
    finally:
        env.close()
    # C: a fresh env, a fresh agent, the backup, two more rounds
    env = _env(case)
    try:
        c = _agent(env, case)
        c.load(path)
        for k in (1, 2):
            _same(_round(c), rolls[k], "resumed, rollout %d" % k)
        _same(_snapshot(c), want, "resumed")
    finally:
        env.close()


def test_without_the_record_the_comparison_fails_at_the_first_rollout(tmp_path):
    """what the parent did, and what load(resume=False) still does: the envs restart, so the next rollout is another one"""
    case, path = "eager_plain", str(tmp_path / "model.pkl")
    rolls, _ = _continuous(case, rounds=2)
    env = _env(case)
    try:
        b = _agent(env, case)
        _round(b)
        b.save(path, resume=True)
    finally:
        env.close()
    env = _env(case)
    try:
        d = _agent(env, case)
        d.load(path, resume=False)
        got = _round(d)
        for k in ("obs", "act", "rew", "adv", "ret"):
            assert esu.first_difference(got[k], rolls[1][k]) is not None, k
        assert d._obs is not None and int(d.env.stats()["n_env_steps"]) == T * N          # (its envs began at their reset)
    finally:
        env.close()


def test_old_checkpoints_are_untouched_and_a_record_of_another_env_is_refused(tmp_path):
    import torch
    case = "eager_plain"
    plain, full = str(tmp_path / "plain.pkl"), str(tmp_path / "full.pkl")
    env = _env(case)
    try:
        a = _agent(env, case)
        _round(a)
        a.save(plain)
        a.save(full, resume=True)
        ck, ck_full = torch.load(plain), torch.load(full)          # (both load as checkpoints always did: tensors, numbers, strings)
        assert "resume" not in ck and set(ck_full) == set(ck) | {"resume"}
        _same(esu.to_np({k: v for k, v in ck_full.items() if k != "resume"}), esu.to_np(ck), "the keys a checkpoint always had")
        with pytest.raises(ValueError, match="no resume record"):
            a.load(plain, resume=True)
    finally:
        env.close()
    # load() of a checkpoint without the record leaves the env as it is
    env = _env(case)
    try:
        c = _agent(env, case)
        env.reset()
        esu.run_steps(env, esu.actions("msj_all", 3, 1)[:, :N], False)
        before = esu.state_views(env)
        c.load(plain)
        after = esu.state_views(env)
        assert before[0] == after[0]
        _same(after[1], before[1], "the env's planes")
        _same(after[2], before[2], "the env's state_dict")
        assert c._obs is None
    finally:
        env.close()
    # a record of an env that is not this agent's: ValueError, the agent and the env as they were
    env = _env(case, seed=4)
    try:
        c = _agent(env, case)
        params = esu.to_np(dict(c.policy.state_dict()))
        before = esu.state_views(env)
        with pytest.raises(ValueError, match="seed = 3, this env has seed = 4"):
            c.load(full)
        _same(esu.to_np(dict(c.policy.state_dict())), params, "the policy")
        _same(esu.state_views(env)[1], before[1], "the env's planes")
        assert c.num_timesteps == 0
        c.load(full, resume=False)                     # (ignoring the record, the checkpoint loads as one without it)
        assert c.num_timesteps == T * N and c._obs is None
    finally:
        env.close()
    # an agent option load() has always refused is refused before the record's env state is written
    env = _env(case)
    try:
        c = _agent(env, case, normalize_obs=True)
        before = esu.state_views(env)
        with pytest.raises(ValueError, match="observation normalisation"):
            c.load(full)
        _same(esu.state_views(env)[1], before[1], "the env's planes")
        assert c.num_timesteps == 0
    finally:
        env.close()


def test_the_torch_path_restores_its_generators_and_goes_on(tmp_path):
    """no bit-for-bit claim there (torch's kernels): the record is written, read and the run continues"""
    import torch
    case, path = "eager_plain", str(tmp_path / "model.pkl")
    env = _env(case)
    try:
        a = _agent(env, case, fused_policy=False, fused_update=False)
        _round(a)
        a.save(path, resume=True)
        rng = torch.get_rng_state().clone()
        steps = int(env.stats()["n_env_steps"])
    finally:
        env.close()
    env = _env(case)
    try:
        c = _agent(env, case, fused_policy=False, fused_update=False)
        torch.manual_seed(12345)
        c.load(path)
        assert torch.equal(torch.get_rng_state(), rng) and c._obs is not None and int(env.stats()["n_env_steps"]) == steps
        roll = _round(c)
        assert np.isfinite(roll["adv"]).all() and c.num_timesteps == 2 * T * N
    finally:
        env.close()


# ---- the trainer, as child processes with a time limit each ----
CHILD_LIMIT = 240
TRAIN = ["--exact-resume", "--goals", "reachable:64", "--eval-envs", "256", "--push", "prob=0.1,sigma=0.5",
         "--n-steps", "8", "--steps-per-round", str(2 * 8 * N)]


def _train(results, rounds, world=1, eval_every=1):
    """train_parallel as ``world`` fresh child processes (gloo on the one GPU where there are two); -> rank 0's stdout"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    argv = [sys.executable, "-m", "gym_roboy_amd.train_parallel", str(N), str(results), "--rounds", str(rounds), "--eval-every", str(eval_every)] + TRAIN
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        if world > 1:
            env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        procs.append(subprocess.Popen(argv + (["--backend", "gloo"] if world > 1 else []), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            try:
                outs.append(p.communicate(timeout=CHILD_LIMIT))
            except subprocess.TimeoutExpired:
                for q in procs:                      # its peers wait for it in a collective: none of them goes on
                    if q.poll() is None:
                        q.kill()
                outs.append(p.communicate())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for rank, (p, (out, err)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d ended %r\n%s\n%s" % (rank, p.returncode, out[-2000:], err[-3000:])
    return outs[0][0]


def _statistics_lines(stdout):
    return [line for line in stdout.splitlines() if line.startswith("episode statistics")]


def _backup(results, world):
    import torch
    from gym_roboy_amd.ppo import unpack_arrays
    model = torch.load(os.path.join(str(results), "model.pkl"), map_location="cpu")
    ranks = [torch.load(os.path.join(str(results), "resume.rank%d.pt" % r), map_location="cpu") for r in range(world)]
    return ({k: v.numpy() for k, v in model["policy"].items()}, esu.to_np(model["optimizer"]),
            [unpack_arrays(r["resume"]["env"]) for r in ranks], [unpack_arrays(r["eval_env"]) for r in ranks])


@pytest.mark.parametrize("world, eval_every", [(1, 1), (2, 1), (1, 2)], ids=["one_rank", "two_ranks_gloo", "one_rank_eval_every_2"])
def test_the_trainer_stopped_and_started_is_the_trainer_that_went_on(world, eval_every, tmp_path):
    """eval_every 2: the cadence counts the rounds of the whole run, not of this start - the second start's only round is round 2 and
    evaluates, its first did not"""
    d1, d2 = tmp_path / "d1", tmp_path / "d2"
    through = _statistics_lines(_train(d1, 2, world, eval_every))
    first = _statistics_lines(_train(d2, 1, world, eval_every))
    second = _statistics_lines(_train(d2, 1, world, eval_every))
    assert len(through) == 2 and len(first) == len(second) == 1
    assert first[0] == through[0] and ("'eval_success_rate': " in first[0]) == (eval_every == 1)
    assert not [f for f in os.listdir(str(d2)) if f.endswith(".tmp")] and os.path.exists(os.path.join(str(d2), "resume.rank0.pt.prev"))
    assert second[0] == through[1], (second[0], through[1])          # the second round's line, character for character
    assert re.search(r"'eval_success_rate': ", second[0]) and re.search(r"'pushes_per_step': ", second[0])
    policy1, adam1, envs1, evals1 = _backup(d1, world)
    policy2, adam2, envs2, evals2 = _backup(d2, world)
    _same(policy2, policy1, "model.pkl's policy")
    _same(adam2, adam1, "model.pkl's optimiser")
    for rank in range(world):                      # every rank wrote, and restored, its own shard
        assert envs1[rank]["identity"]["env_id_offset"] == rank * N
        assert np.array_equal(envs2[rank]["blob"], envs1[rank]["blob"]), "rank %d's env blob" % rank
        assert np.array_equal(evals2[rank]["blob"], evals1[rank]["blob"]), "rank %d's evaluation env blob" % rank
        _same(esu.to_np(envs2[rank]["host"]), esu.to_np(envs1[rank]["host"]), "rank %d's host counters" % rank)
