"""Play a trained agent back in one environment and print its rewards.

Counterpart of ``/root/reference/gym_roboy/visualize_agent.py``
(``python -m gym_roboy_amd.visualize_agent <model.pkl>``): the reference loads a
stable_baselines ``PPO2`` model, steps a single ROS-backed ``RoboyEnv`` with it
and logs each reward with a 30 ms pause (:18-25,28-43).  Here the model is the
checkpoint written by ``gym_roboy_amd.train_parallel`` and the env is a
``RoboyEnv`` over the in-process ``HipSimulationClient``.
"""
import argparse
import time


class Logger:
    """Prints the step reward and paces the loop (reference :18-25)."""

    def __init__(self, pause_secs: float = 0.03):
        self.pause_secs = pause_secs
        self.total = 0.0

    def log(self, step: int, reward: float):
        self.total += reward
        print("step %4d  reward %10.4f  return %12.4f" % (step, reward, self.total))
        if self.pause_secs > 0:
            time.sleep(self.pause_secs)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("model", help="model.pkl written by gym_roboy_amd.train_parallel")
    ap.add_argument("--steps", type=int, default=400, help="the reference loops forever; one episode by default")
    ap.add_argument("--pause", type=float, default=0.03)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from .envs import RoboyEnv
    from .envs.options import env_kwargs_from_checkpoint
    from .envs.robots import MsjRobot
    from .envs.simulations import HipSimulationClient
    from .ppo import MlpPolicy

    ck = torch.load(args.model, map_location="cpu")
    env_kw, needs_vec_env = env_kwargs_from_checkpoint(ck)
    if needs_vec_env:
        # trained with tendon channels or the last actions in the observation, under sensor noise, an action delay or random pushes: the
        # same row, under the same conditions, comes from a RoboyVecEnv of one env, which resets itself on done and returns the reset row
        from .envs.vec_env import RoboyVecEnv
        vec = RoboyVecEnv(MsjRobot(), 1, **env_kw)
        reset = lambda: vec.reset()[0]

        def step(a):
            o, r, d, _ = vec.step(a[None])
            return o[0], float(r[0]), False
        n_obs, n_act = vec.observation_space.shape[0], vec.action_space.shape[0]
    else:
        # (start poses: the single RoboyEnv plays from the rest pose; only the one-env RoboyVecEnv above replays env_kw["start_poses"])
        env = RoboyEnv(simulation_client=HipSimulationClient(robot=MsjRobot(), goals=env_kw["goals"]))
        reset = env.reset

        def step(a):
            o, r, d, _ = env.step(a)
            return o, r, d
        n_obs, n_act = env.observation_space.shape[0], env.action_space.shape[0]
    # (a checkpoint of PPO's asymmetric_critic: the value net has its own input width and is not evaluated - the actor alone is played
    # back, and no critic row is needed)
    policy = MlpPolicy(n_obs, n_act, critic_obs_dim=ck.get("critic_obs_dim"))
    if ck["policy"]["pi.0.weight"].shape[1] != n_obs:
        raise SystemExit("%s holds a policy over %d observation columns, this env gives %d: it was not written by this "
                         "train_parallel" % (args.model, ck["policy"]["pi.0.weight"].shape[1], n_obs))
    policy.load_state_dict(ck["policy"])
    if ck.get("obs_norm") is not None:          # trained with PPO's normalize_obs: the policy reads the observation through them
        from .ppo import ObsNorm
        stats = ObsNorm(n_obs)
        stats.load_state_dict(ck["obs_norm"])
        policy.set_obs_norm(stats)
    logger = Logger(args.pause)
    obs = reset()
    for i in range(args.steps):
        with torch.no_grad():
            action, _, _ = policy.act(torch.as_tensor(obs, dtype=torch.float32)[None], deterministic=True)
        obs, reward, done = step(np.clip(action[0].numpy(), -1.0, 1.0).astype(np.float32))
        logger.log(i, reward)
        if done:
            obs = reset()
    return logger.total


if __name__ == "__main__":
    main()
