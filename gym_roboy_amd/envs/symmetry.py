"""Row maps of the robot's mirror symmetry: pure Python, no GPU.

A robot with a mirror plane (``rb_mirror_info``: MsjRobot's is x-z, tendon ``7 - k`` is tendon ``k`` reflected) seen in the mirror
is the same robot in the state ``(S q, S qd)`` under the set-points ``P sp``: ``S`` flips the two joints whose axes lie in the plane,
``P`` exchanges every tendon with its image.  Every transition ``(s, a, r, s')`` of ``RoboyVecEnv`` therefore has a twin
``(M s, P a, r, M s')`` that is as valid as the original; ``M`` is what ``S`` and ``P`` do to the env's observation row.

``row_mirror_map`` writes ``M`` and ``P`` as a column source and a column sign per row layout; ``mirror_rows`` applies such a map and
is the statement the HIP kernel (``rp_mirror_rows_dev``) is held to, bit for bit.
"""
import numpy as np

# the tendon channels of the observation in row order (RoboyVecEnv's TENDON_OBS_CHANNELS): all four are scalars of the tendon - a
# length, its rate, an activation, a force - so the mirror exchanges partner columns and changes no sign
TENDON_CHANNELS = ("length", "rate", "activation", "force")


def row_mirror_map(n_q, n_t, joint_sign, tendon_image, tendon_obs=(), action_obs=0):
    """The mirror image of ``RoboyVecEnv``'s observation row ``[q, qd, goal | n_t columns per tendon channel | K action blocks]`` and of
    its action row, as ``(obs_src int32[obs_dim], obs_sign float32[obs_dim], act_src int32[n_t])``:
    ``M obs = obs[..., obs_src] * obs_sign`` and ``P act = act[..., act_src]``.

    ``joint_sign`` [n_q] (+-1) and ``tendon_image`` [n_t] (an involution without fixed points) are ``rb_mirror_info``'s;
    ``tendon_obs``: the env's channel names (any order: the row holds them in the fixed channel order); ``action_obs``: K."""
    n_q, n_t, rows = int(n_q), int(n_t), int(action_obs or 0)
    sign = np.asarray(joint_sign, np.int64).reshape(-1)
    image = np.asarray(tendon_image, np.int64).reshape(-1)
    if sign.shape != (n_q,) or not np.all(np.abs(sign) == 1):
        raise ValueError("joint_sign: %d entries of +-1, got %r" % (n_q, joint_sign))
    if image.shape != (n_t,) or sorted(image.tolist()) != list(range(n_t)) or not np.array_equal(image[image], np.arange(n_t)) \
            or np.any(image == np.arange(n_t)):
        raise ValueError("tendon_image: an involution of [0, %d) without fixed points, got %r" % (n_t, tendon_image))
    names = [tendon_obs] if isinstance(tendon_obs, str) else list(tendon_obs or ())
    if [c for c in names if c not in TENDON_CHANNELS] or len(set(names)) != len(names):
        raise ValueError("tendon_obs takes distinct names out of %s, got %r" % (TENDON_CHANNELS, tendon_obs))
    if rows < 0:
        raise ValueError("action_obs must be >= 0")
    blocks = len(names) + rows                                   # blocks of n_t columns behind [q, qd, goal]
    src = [np.arange(3 * n_q)] + [3 * n_q + b * n_t + image for b in range(blocks)]
    sgn = [np.tile(sign, 3).astype(np.float32), np.ones(blocks * n_t, np.float32)]
    return np.concatenate(src).astype(np.int32), np.concatenate(sgn), image.astype(np.int32)


def mirror_rows(x, src, sign=None):
    """``x[..., src] * sign`` for a numpy array or a torch tensor (``sign`` None: the permutation alone): one IEEE multiply per
    element, so a flipped 0 is -0."""
    if isinstance(x, np.ndarray):
        out = x[..., np.asarray(src, np.int64)]
        return out if sign is None else out * np.asarray(sign, x.dtype)
    import torch
    out = x[..., torch.as_tensor(src, dtype=torch.int64, device=x.device)]
    return out if sign is None else out * torch.as_tensor(sign, dtype=x.dtype, device=x.device)
