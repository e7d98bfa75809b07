"""TEST HELPER for the mirror-symmetry augmentation (gym_roboy_amd/envs/symmetry.py, ppo.py: PPO(symmetry="augment")):
the maps of MsjRobot written down by hand, random involution maps for the streaming kernel, a stub env with a ``mirror_map`` for the
CPU tests of PPO, and the numpy / torch concatenation ``augment`` is held to."""
import numpy as np

from gym_roboy_amd._gymcompat import spaces
from gym_roboy_amd.envs.symmetry import mirror_rows, row_mirror_map

# MsjRobot: the x-z plane, tendon 7 - k is tendon k reflected; the rotated robot of tests/test_mirror_pairs.py: the y-z plane
JOINT_SIGN = {0: np.array([-1, 1, -1]), 1: np.array([1, -1, -1])}
MSJ_IMAGE = np.arange(8)[::-1].copy()
AUGMENTED = ("obs", "act", "adv", "logp", "val", "ret")


def random_involution_map(width, rng):
    """A random column map of `width` columns that is an involution - random disjoint pairs, the rest fixed - with random signs that
    agree inside a pair (so that applying the map twice is the identity): (src int32, sign float32)"""
    order = rng.permutation(width)
    src = np.arange(width)
    n_pairs = rng.integers(0, width // 2 + 1)
    for a, b in order[:2 * n_pairs].reshape(-1, 2):
        src[a], src[b] = b, a
    sign = rng.choice(np.float32([-1.0, 1.0]), width)
    sign = np.where(src < np.arange(width), sign[src], sign).astype(np.float32)
    return src.astype(np.int32), sign


def is_involution(src, sign):
    src = np.asarray(src, np.int64)
    return bool(np.array_equal(src[src], np.arange(len(src))) and np.all(np.asarray(sign)[src] * np.asarray(sign) == 1))


class MirrorToyEnv:
    """A numpy env of MsjRobot's bare row layout (9 observation columns, 8 actions) with a ``mirror_map``; its dynamics do not matter
    to the tests, which check what PPO does with the rollout"""

    def __init__(self, n, seed=0, with_map=True, plane=0):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.num_envs = n
        self.observation_space = spaces.Box(low=-10, high=10, shape=(9,), dtype="float32")
        self.action_space = spaces.Box(low=-1, high=1, shape=(8,), dtype="float32")
        self.W = self.rng.standard_normal((9, 8)).astype(np.float32) * 0.5
        if with_map:
            self.mirror_map = lambda: row_mirror_map(3, 8, JOINT_SIGN[plane], MSJ_IMAGE)

    def reset(self):
        self.obs = self.rng.standard_normal((self.n, 9)).astype(np.float32)
        return self.obs

    def step(self, a):
        rew = -np.square(np.asarray(a) - np.tanh(self.obs @ self.W)).sum(1).astype(np.float32)
        done = self.rng.random(self.n) < 0.05
        return self.reset(), rew, done, [{}] * self.n


def twin_case(msj_robot, n=321):
    """The equivariance tests' envs: states 0.5 x random_states(desc, n, 7), three actions per env in [-1, 1], goals on the far side of
    the box joint by joint (no env is done), all float32: (desc, q, qd, acts [3, n, n_t], goal)"""
    from conftest import random_states
    desc = msj_robot.get_description()
    q, qd, _ = random_states(desc, n, 7)
    q, qd = (0.5 * q).astype(np.float32), (0.5 * qd).astype(np.float32)
    rng = np.random.default_rng(9)
    acts = rng.uniform(-1, 1, (3, n, desc.n_t)).astype(np.float32)
    goal = (0.9 * np.where(q >= 0, desc.q_lo, desc.q_hi)).astype(np.float32)
    return desc, q, qd, acts, goal


def concatenated(roll, maps):
    """The rollout and its mirror image as a [1, 2 n, ...] rollout dict (torch tensors, or numpy arrays for numpy input): what an
    agent WITHOUT the option is fed so that it runs the update the option runs"""
    obs_src, obs_sign, act_src = maps
    out = {}
    for k in AUGMENTED:
        x = roll[k].reshape(-1, *roll[k].shape[2:])
        if k == "obs":
            image = mirror_rows(x, obs_src, obs_sign)
        elif k == "act":
            image = mirror_rows(x, act_src)
        else:
            image = x
        if isinstance(x, np.ndarray):
            out[k] = np.concatenate([x, image])[None]
        else:
            import torch
            out[k] = torch.cat([x, image])[None]
    return out


def bits(x):
    """the int32 view of float32 values (numpy array or torch tensor), so that -0 and +0 differ"""
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, np.float32).view(np.int32)
    import torch
    return x.detach().contiguous().view(torch.int32).cpu().numpy()
