"""TEST HELPER for the per-env physical parameters (include/roboy_sim.h: rb_params_*): the descriptions the oracle steps an env
with, random parameter sets, the numpy restatement of the on-device draw, and a stepper over the oracle with each env on its own
description (importable without a GPU: tests/test_env_params_gpu.py and the composed model of tests/env_layer_model.py share it)."""
import numpy as np

from oracle import philox_np as ph

STREAM_PARAMS = 3


def perturbed(desc, par):
    """desc with parameters par [P] applied: f_max *= force_scale, every link's mass and inertia *= mass_scale,
    damping *= damping_scale (the set-point offset is the caller's: it adds to the set-points)."""
    from gym_roboy_amd.envs.robots.description import RobotDescription
    nt = desc.n_t
    d = RobotDescription(desc.to_dict())
    d.f_max = desc.f_max * np.asarray(par[:nt], np.float64)
    d.mass = desc.mass * float(par[2 * nt])
    d.inertia = desc.inertia * float(par[2 * nt])
    d.damping = desc.damping * np.asarray(par[2 * nt + 1:2 * nt + 4], np.float64)
    return d


def random_params(rng, nt, n):
    """n random parameter sets [n][P]: force scales 0.5-1.5, offsets +-0.05 m, mass scale 0.5-2 (never 1), damping 0-3"""
    P = 2 * nt + 4
    p = np.empty((n, P))
    p[:, :nt] = rng.uniform(0.5, 1.5, (n, nt))
    p[:, nt:2 * nt] = rng.uniform(-0.05, 0.05, (n, nt))
    p[:, 2 * nt] = np.where(rng.random(n) < 0.5, rng.uniform(0.5, 0.9, n), rng.uniform(1.1, 2.0, n))
    p[:, 2 * nt + 1:] = rng.uniform(0.0, 3.0, (n, 3))
    return p


def draw(seed, env_ids, d, lo, hi):
    """[len(env_ids)][P] float32: draw number d[i] of env env_ids[i] - block b = philox_draw(seed, g, d, 3, b), parameter p takes
    word p mod 4 of block p / 4, value lo_p + (hi_p - lo_p) * u01(word) with two roundings (fp32)."""
    env_ids = np.asarray(env_ids, np.uint64)
    d = np.broadcast_to(np.asarray(d, np.uint32), env_ids.shape)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    P = lo.shape[0]
    out = np.empty((env_ids.shape[0], P), np.float32)
    # one philox call per distinct counter value (the counter's index word varies per env)
    for dv in np.unique(d):
        sel = d == dv
        words = np.concatenate([ph.draw(seed, env_ids[sel], int(dv), STREAM_PARAMS, b) for b in range((P + 3) // 4)], axis=-1)[:, :P]
        u = ph.u01(words)
        out[sel] = (hi - lo) * u + lo          # fp32: product rounded, then sum rounded (numpy does not contract)
    return out


class PerEnvOracle:
    """the fp64 oracle with each env on its own description (its parameters par [n, P]); states kept in float32.  The base of the
    two steppers below and of tests/env_layer_model.py's, which is handed its parameters instead of drawing them."""

    def __init__(self, robot, n, par0, integrator="euler"):
        from oracle.c_oracle import COracle
        self.COracle = COracle
        self.desc = robot.get_description()
        self.n, self.integ = n, 0 if integrator == "euler" else 1
        self.par = par0.astype(np.float32).copy()
        self.q = np.zeros((n, 3), np.float32)
        self.qd = np.zeros((n, 3), np.float32)
        self.f = np.ones(n, bool)
        self.orc = [COracle(perturbed(self.desc, self.par[i].astype(np.float64)), "f64") for i in range(n)]

    def step(self, sp):
        nt = self.desc.n_t
        for i in range(self.n):
            qo, qdo, fo = self.orc[i].step(self.q[i:i + 1].astype(np.float64), self.qd[i:i + 1].astype(np.float64),
                                           sp[i:i + 1].astype(np.float64) + self.par[i, nt:2 * nt].astype(np.float64), integrator=self.integ)
            self.q[i], self.qd[i], self.f[i] = qo[0], qdo[0], fo[0]
        return self.q.copy(), self.qd.copy(), self.f.copy()

    def zero(self, mask):
        self.q[mask] = 0.0
        self.qd[mask] = 0.0
        self.f[mask] = True

    def set_params(self, mask, par):
        for i in np.nonzero(mask)[0]:
            self.par[i] = par[i]
            self.orc[i] = self.COracle(perturbed(self.desc, self.par[i].astype(np.float64)), "f64")


class ParamOracleStepper(PerEnvOracle):
    """host_env_model's stepper interface over the fp64 oracle, each env on its own description; on reset(mask) the masked
    envs' parameters become the next draw of the restatement (what the kernel draws where it redraws the goal)"""

    def __init__(self, robot, n, seed, lo, hi, par0, draws0):
        PerEnvOracle.__init__(self, robot, n, par0)
        self.seed, self.lo, self.hi = seed, lo, hi
        self.draws = draws0.astype(np.uint32).copy()

    def reset(self, mask):
        idx = np.nonzero(mask)[0]
        self.zero(idx)
        new = self.par.copy()
        new[idx] = draw(self.seed, idx.astype(np.uint64), self.draws[idx], self.lo, self.hi)
        self.draws[idx] += 1
        self.set_params(np.asarray(mask, bool), new)
