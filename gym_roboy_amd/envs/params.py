"""Per-env physical parameters of ball-joint robots (include/roboy_sim.h: rb_params_*).

Planes [P][n_envs], P = 2 n_t + 4: force_scale[n_t], setpoint_offset[n_t], mass_scale, damping_scale[3].  ``ParamRanges`` holds the
uniform box each parameter is drawn from on the device; a name left out keeps its nominal value (lo = hi).
"""
import numpy as np

NAMES = ("force_scale", "setpoint_offset", "mass_scale", "damping_scale")
NOMINAL = {"force_scale": 1.0, "setpoint_offset": 0.0, "mass_scale": 1.0, "damping_scale": 1.0}


def n_params(n_t: int) -> int:
    return 2 * int(n_t) + 4


def widths(n_t: int) -> dict:
    return {"force_scale": int(n_t), "setpoint_offset": int(n_t), "mass_scale": 1, "damping_scale": 3}


def plane_slices(n_t: int) -> dict:
    """name -> slice of the plane axis"""
    out, p = {}, 0
    for name in NAMES:
        w = widths(n_t)[name]
        out[name] = slice(p, p + w)
        p += w
    return out


class ParamRanges:
    """``ParamRanges(force_scale=(0.8, 1.2), damping_scale=([0.5, 0.5, 0.5], [2, 2, 2]))``: each value a (lo, hi) pair of scalars or
    of per-tendon / per-joint arrays."""

    def __init__(self, force_scale=None, setpoint_offset=None, mass_scale=None, damping_scale=None):
        self.ranges = {}
        for name, v in zip(NAMES, (force_scale, setpoint_offset, mass_scale, damping_scale)):
            if v is None:
                continue
            if len(v) != 2:
                raise ValueError("%s: expected a (lo, hi) pair" % name)
            self.ranges[name] = (np.asarray(v[0], dtype=np.float64), np.asarray(v[1], dtype=np.float64))

    def to_arrays(self, n_t: int):
        """(lo [P], hi [P]) float32, validated as rb_params_set_ranges validates them."""
        w, sl = widths(n_t), plane_slices(n_t)
        P = n_params(n_t)
        lo, hi = np.empty(P, np.float32), np.empty(P, np.float32)
        for name in NAMES:
            if name in self.ranges:
                a, b = self.ranges[name]
                try:
                    a = np.broadcast_to(a, (w[name],))
                    b = np.broadcast_to(b, (w[name],))
                except ValueError:
                    raise ValueError("%s: expected a scalar or %d values per bound" % (name, w[name]))
            else:
                a = b = np.full(w[name], NOMINAL[name])
            lo[sl[name]], hi[sl[name]] = a, b
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
            raise ValueError("range bounds must be finite")
        if np.any(lo > hi):
            raise ValueError("lo > hi")
        if np.any(lo[sl["mass_scale"]] <= 0):
            raise ValueError("mass_scale must stay > 0")
        if np.any(lo[sl["force_scale"]] < 0) or np.any(lo[sl["damping_scale"]] < 0):
            raise ValueError("force_scale and damping_scale must stay >= 0")
        return lo, hi

    def __repr__(self):
        return "ParamRanges(%s)" % ", ".join("%s=(%s, %s)" % (k, a, b) for k, (a, b) in self.ranges.items())


def planes_to_dict(planes: np.ndarray, n_t: int) -> dict:
    """[P][N] planes -> {'force_scale': [N, n_t], 'setpoint_offset': [N, n_t], 'mass_scale': [N], 'damping_scale': [N, 3]}"""
    sl = plane_slices(n_t)
    out = {name: np.ascontiguousarray(planes[sl[name]].T) for name in NAMES}
    out["mass_scale"] = out["mass_scale"][:, 0].copy()
    return out
