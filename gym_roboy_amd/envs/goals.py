"""Goal pools: env goals drawn from poses the robot can hold.

The reference asks its simulator for a *feasible* goal pose (``ros_simulation_client.py:73-81``); a goal that is only uniform in a box
need not be a pose the tendons can hold still.  ``reachable_goals`` makes such poses with the physics the env itself steps: it drives a
batch from rest under constant random set-points until it has settled and keeps the poses that stayed feasible.  ``RoboyVecEnv(...,
goals=pool)``, ``HipSimulationClient(..., goals=pool)`` and ``gym_roboy_amd.make(..., goals=pool)`` then draw every goal as a row of the
pool (``rb_env_goal_pool_set``: which row is a pure function of seed, global env id and draw number).
"""
import numpy as np

from . import reward as rw

MAX_BATCHES = 4
MAX_LEVELS = 256      # RB_GOAL_LEVELS_MAX: the most levels of a goal curriculum


def _count_array(x, name):
    """counts as Python-int-exact numpy: a 1-d array of non-negative integers -> object array of Python ints"""
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError("%s must be a 1-d array of counts, got shape %s" % (name, a.shape))
    if a.dtype.kind not in "iu" and not (a.dtype.kind == "O" and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in a)):
        raise ValueError("%s must be integers, got dtype %s" % (name, a.dtype))
    vals = [int(v) for v in a]
    if any(v < 0 for v in vals):
        raise ValueError("%s must be >= 0" % name)
    return vals


def reach_rate_order(attempts, reached, prior=(1, 2)):
    """The permutation ``[m]`` (int64) that sorts pool rows from the most often reached to the least: by descending
    ``(reached + a) / (attempts + b)`` with ``prior = (a, b)``, ``0 <= a <= b``, ``b > 0`` - the counts of
    ``RoboyVecEnv.goal_row_stats()`` smoothed by ``b`` imagined attempts of which ``a`` reached.  Rates are compared as
    exact rationals (``fractions.Fraction`` over Python ints, never floats: counts near 2^40 hold rates a float64 merges).  Ties keep
    their current order; rows nobody has tried all tie at ``a / b``.  ``ValueError`` for mismatched shapes, negative counts,
    ``reached > attempts`` or a prior outside the above."""
    from fractions import Fraction
    att, rch = _count_array(attempts, "attempts"), _count_array(reached, "reached")
    if len(att) != len(rch):
        raise ValueError("attempts and reached must have the same length, got %d and %d" % (len(att), len(rch)))
    if any(r > t for r, t in zip(rch, att)):
        raise ValueError("reached must not exceed attempts")
    try:
        a, b = prior
        a, b = Fraction(a), Fraction(b)
    except (TypeError, ValueError):
        raise ValueError("prior is a pair (a, b) of numbers, got %r" % (prior,))
    if a < 0 or b <= 0 or a > b:
        raise ValueError("prior (a, b) needs 0 <= a <= b and b > 0, got %r" % (prior,))
    rate = [(r + a) / (t + b) for r, t in zip(rch, att)]
    return np.asarray(sorted(range(len(att)), key=lambda j: -rate[j]), dtype=np.int64)       # (sorted is stable)


class GoalPool:
    """``q``: the poses ``[m, n_q]`` float32; ``recipe``: how they were made (``reachable_goals``' arguments plus the yield), or ``{}``;
    ``source``: ``[m, 2]`` ints, the (batch, env) whose set-points (``settle_setpoints``) hold row j, or None; ``order``: on a pool
    made by ``ordered``, the permutation it applied (row j is row ``order[j]`` of the pool it was called on), else None."""

    def __init__(self, q, recipe=None, source=None):
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[0] < 1 or q.shape[1] < 1:
            raise ValueError("a goal pool is an array [m, n_q] with m >= 1, got shape %s" % (q.shape,))
        self.q = q
        self.recipe = dict(recipe or {})
        self.source = None if source is None else np.asarray(source, dtype=np.int64).reshape(q.shape[0], 2)
        self.order = None

    def __len__(self):
        return self.q.shape[0]

    def ordered(self, key="rest_distance", attempts=None, reached=None, prior=(1, 2)):
        """A new ``GoalPool`` with the rows sorted from easiest to hardest, which is what a goal curriculum (``RoboyVecEnv(...,
        goal_curriculum=...)``) takes row order for.  ``"rest_distance"``: by ``|q|_2`` from the zero pose every episode
        starts from, formed in float64; a stable sort, so ties keep pool order.  ``"reach_rate"``: by how often a policy reached each
        row, ``reach_rate_order(attempts, reached, prior)`` over counts ``[m]`` as ``RoboyVecEnv.goal_row_stats()`` gives them
        (DESIGN.md §24).  ``source`` is permuted with the rows, the recipe gains ``"ordered": key`` and ``order`` holds the
        permutation."""
        if key == "rest_distance":
            if attempts is not None or reached is not None:
                raise ValueError("attempts and reached belong to key='reach_rate'")
            order = np.argsort(np.sqrt(np.sum(np.square(self.q.astype(np.float64)), axis=1)), kind="stable")
        elif key == "reach_rate":
            if attempts is None or reached is None:
                raise ValueError("key='reach_rate' needs attempts= and reached= (counts per row)")
            order = reach_rate_order(attempts, reached, prior)
            if len(order) != len(self):
                raise ValueError("the pool has %d rows, the counts have %d" % (len(self), len(order)))
        else:
            raise ValueError("a goal pool is ordered by 'rest_distance' or 'reach_rate', got %r" % (key,))
        recipe = dict(self.recipe)
        recipe["ordered"] = key
        pool = GoalPool(self.q[order], recipe, None if self.source is None else self.source[order])
        pool.order = np.asarray(order, dtype=np.int64)
        return pool


def goal_curriculum_spec(goal_curriculum, m=None):
    """``goal_curriculum``: None, an int ``L`` or ``dict(levels=, up=1, down=1, start=0)`` -> None or the dict with all four keys as
    ints, checked as ``rb_env_goal_curriculum_configure`` checks them: ``1 <= levels <= min(m, 256)`` (``m``: the pool's rows, where
    known), ``up, down >= 0``, ``0 <= start < levels``.  ``ValueError`` otherwise."""
    if goal_curriculum is None:
        return None
    spec = {"levels": None, "up": 1, "down": 1, "start": 0}
    if isinstance(goal_curriculum, dict):
        unknown = sorted(set(goal_curriculum) - set(spec))
        if unknown:
            raise ValueError("goal_curriculum: unknown keys %s (levels, up, down, start)" % unknown)
        spec.update(goal_curriculum)
    elif isinstance(goal_curriculum, (int, np.integer)) and not isinstance(goal_curriculum, bool):
        spec["levels"] = goal_curriculum
    else:
        raise ValueError("goal_curriculum is None, an int (the number of levels) or a dict(levels=, up=1, down=1, start=0), got %r"
                         % (goal_curriculum,))
    for k, v in spec.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("goal_curriculum: %s must be an int, got %r" % (k, v))
        spec[k] = int(v)
    most = MAX_LEVELS if m is None else min(int(m), MAX_LEVELS)
    if not 1 <= spec["levels"] <= most:
        raise ValueError("goal_curriculum: levels must be in 1..%d (at most the pool's rows and %d), got %d" % (most, MAX_LEVELS, spec["levels"]))
    if spec["up"] < 0 or spec["down"] < 0:
        raise ValueError("goal_curriculum: up and down must be >= 0")
    if not 0 <= spec["start"] < spec["levels"]:
        raise ValueError("goal_curriculum: start must be in 0..levels - 1, got %d" % spec["start"])
    return spec


def goal_rows(goals, n_q: int, low, high, m=None) -> np.ndarray:
    """A ``GoalPool`` or an array -> contiguous float32 rows ``[m, n_q]``, checked as ``rb_env_goal_pool_set`` checks them: the shape,
    every value finite and inside ``[low, high]`` (the env's angle box), and - ``m`` given: the size of the pool the env already holds -
    the same number of rows.  ``ValueError`` otherwise."""
    rows = goals.q if isinstance(goals, GoalPool) else goals
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] != int(n_q) or rows.shape[0] < 1:
        raise ValueError("goals must have shape (m, %d) with m >= 1, got %s" % (int(n_q), rows.shape))
    if m is not None and rows.shape[0] != int(m):
        raise ValueError("the env's goal pool has %d rows, fixed when it was first set; got %d" % (int(m), rows.shape[0]))
    if not np.all(np.isfinite(rows)):
        raise ValueError("goals must be finite")
    lo, hi = np.broadcast_to(np.asarray(low, np.float32), (int(n_q),)), np.broadcast_to(np.asarray(high, np.float32), (int(n_q),))
    if np.any(rows < lo) or np.any(rows > hi):
        raise ValueError("goals must lie inside the angle box [%s, %s]" % (lo.tolist(), hi.tolist()))
    return rows


def default_settle_tol(robot) -> float:
    """``goal_vel_tol / 20`` with ``goal_vel_tol = |vel.high - vel.low|_2 / 5`` exactly as ``RoboyVecEnv`` forms it: a goal must be
    holdable well inside the velocity tolerance that "reached" uses."""
    vels = robot.get_joint_vels_space()
    return float(rw.l2_distance(vels.low, vels.high) / 5) / 20.0


def settle_batch_size(m: int) -> int:
    """``B = 2 m`` envs per batch, rounded up to a multiple of 256."""
    return -(-2 * int(m) // 256) * 256


def settle_setpoints(robot, seed: int, batch: int, n_envs: int) -> np.ndarray:
    """The constant set-points ``[n_envs, n_t]`` of batch number ``batch``: uniform in the robot's action box."""
    act = robot.get_action_space()
    return np.random.default_rng([int(seed), int(batch)]).uniform(act.low, act.high, (int(n_envs), act.shape[0])).astype(np.float32)


def reachable_goals(robot, m: int, seed: int = 0, integrator="euler", n_substeps: int = 1, settle_steps: int = 100,
                    settle_tol=None, device: int = 0) -> GoalPool:
    """``m`` poses the robot holds under constant set-points, as a ``GoalPool``.

    Batches of ``B = 2 m`` envs (rounded up to a multiple of 256) start at rest, each env under its own set-points
    ``default_rng([seed, batch]).uniform(act.low, act.high)``, uploaded once as a one-row action ring, and run ``settle_steps`` steps in
    one ``rollout_dev`` call - the env's own step kernels, no per-step download.  A row is kept when its feasibility flag reads feasible
    after the last step and ``|qd|_2 <= settle_tol`` (None: ``default_settle_tol``); the first ``m`` kept rows in env order, batch after
    batch, are the pool.  At most 4 batches: a ``RuntimeError`` with the measured yield after that.  The same arguments give the same
    pool bit for bit, so every rank of a multi-GPU run that calls this with the run's seed holds the same pool."""
    from .simulations.hip_simulation_client import HipBatchSimulation
    m = int(m)
    if m < 1:
        raise ValueError("m must be >= 1")
    if int(settle_steps) < 1:
        raise ValueError("settle_steps must be >= 1")
    tol = default_settle_tol(robot) if settle_tol is None else float(settle_tol)
    if not tol > 0:
        raise ValueError("settle_tol must be > 0")
    n_envs = settle_batch_size(m)
    kept, source, tried, batches = [], [], 0, 0
    sim = HipBatchSimulation(robot, n_envs, integrator=integrator, n_substeps=n_substeps, device=device, seed=seed)
    try:
        d_ring = sim.malloc(4 * n_envs * sim.n_t)
        while sum(len(k) for k in kept) < m and batches < MAX_BATCHES:
            if batches:
                sim.forward_reset_command()
            sim.upload(d_ring, settle_setpoints(robot, seed, batches, n_envs))
            sim.rollout_dev(d_ring, 1, int(settle_steps))
            q, qd, feasible = sim.read_state()
            keep = feasible & (np.sqrt(np.sum(np.square(qd, dtype=np.float32), axis=1, dtype=np.float32)) <= np.float32(tol))
            kept.append(q[keep])
            source.append(np.stack((np.full(int(keep.sum()), batches), np.nonzero(keep)[0]), axis=1))
            tried += n_envs
            batches += 1
    finally:
        sim.close()
    rows = np.concatenate(kept, axis=0)
    if rows.shape[0] < m:
        raise RuntimeError("reachable_goals: %d of %d envs settled feasibly within %d steps (yield %.1f %%), %d poses were asked for"
                           % (rows.shape[0], tried, int(settle_steps), 100.0 * rows.shape[0] / tried, m))
    recipe = {"robot": type(robot).__name__, "m": m, "seed": int(seed), "integrator": str(integrator), "n_substeps": int(n_substeps),
              "settle_steps": int(settle_steps), "settle_tol": tol, "batch_envs": n_envs, "batches": batches,
              "yield": float(rows.shape[0]) / float(tried)}
    return GoalPool(rows[:m], recipe, np.concatenate(source, axis=0)[:m])
