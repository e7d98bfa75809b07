"""The tendon-state readout (include/roboy_sim.h: rb_tendon_state_dev / rb_tendon_state, ABI 6) without a GPU: the ABI, error
handling on a null handle, the resources of the new kernels in the shipped code objects, and the ball-joint class's per-tendon
function (csrc/msj_math.hpp: MsjModel::tendon_state) compiled for the host in fp64 against the oracle's tendon geometry and
muscle model.  The GPU file (test_tendon_state_gpu.py) checks the kernels themselves."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gym_roboy_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from build_dir import build_dir  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()
LIB = os.path.join(ROOT, "gym_roboy_amd", "csrc", "libroboy_sim.so")
NEW_KERNELS = ("rbts::msj_tendon_state8<256>", "rbts::msj_tendon_state_nt<256>",
               "rbt::tree_tendon_state<2, true>", "rbt::tree_tendon_state<2, false>")


def test_abi_6_declares_and_exports_both_entry_points():
    assert int(re.search(r"#define RB_ABI_VERSION (\d+)", HEADER).group(1)) == 6
    lib = nat.load()
    assert lib.rb_abi_version() == 6
    assert re.search(r"RB_SP_SCALED = 0\b", HEADER) and re.search(r"RB_SP_ENV = 1\b", HEADER)
    assert (nat.RB_SP_SCALED, nat.RB_SP_ENV) == (0, 1)
    for name in ("rb_tendon_state_dev", "rb_tendon_state"):
        assert name in nat.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8


@pytest.mark.parametrize("name", ["rb_tendon_state_dev", "rb_tendon_state"])
def test_null_handle_is_an_error_not_an_abort(name):
    lib = nat.load()
    rc = getattr(lib, name)(None, None, nat.RB_SP_SCALED, 1.0, None, None, None, None)
    assert rc == nat.RB_EINVAL
    assert b"null" in lib.rb_last_error()


def test_readout_kernels_are_shipped_without_scratch_or_spills():
    import code_object_meta as com
    meta = {com.short(k): v for k, v in com.kernel_metadata(LIB).items()}
    for name in NEW_KERNELS:
        assert name in meta, (name, sorted(k for k in meta if "tendon" in k))
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


# ---- the per-tendon function in fp64 against the oracle ----
@pytest.fixture(scope="module")
def ts_lib():
    so = os.path.join(build_dir(), "libtendon_state_host.so")
    src = os.path.join(ROOT, "tests", "hostmath", "tendon_state_host.cpp")
    deps = [src] + [os.path.join(ROOT, "gym_roboy_amd", "csrc", f) for f in ("msj_math.hpp", "msj_build.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.ts_eval.restype = ctypes.c_int
    lib.ts_eval.argtypes = [ctypes.c_void_p, ctypes.c_long] + [dp] * 7
    return lib


def _host_readout(lib, desc, q, qd, sp):
    n, nt = q.shape[0], desc.n_t
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in (q, qd, sp)]
    out = [np.empty((n, nt)) for _ in range(4)]
    c = desc.as_c_struct()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.ts_eval(ctypes.addressof(c), n, *[a.ctypes.data_as(dp) for a in args + out])
    assert rc == 0
    return dict(zip(("length", "rate", "activation", "force"), out))


def _oracle_readout(desc, q, qd, sp):
    from oracle.physics_np import TendonRobotOracle
    o = TendonRobotOracle(desc)
    length, L = o.tendon_geometry(q)
    rate = np.einsum("nkj,nj->nk", L, qd)
    act = np.clip(o.kp * (length - o.l0 - o.sigma * sp) / o.l0, 0.0, 1.0)
    return {"length": length, "rate": rate, "activation": act, "force": o.muscle_force(length, rate, sp)}, o


def _states(desc, n, seed):
    """n random states in four groups: inside the boxes; set-points far above the box (every tendon slack: activation
    clamped to 0); far below (activation saturated at 1); joint speeds 60x the limit (shortening faster than v_max l0:
    the f_V clamp at v = -1)."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.98 * desc.q_lo, 0.98 * desc.q_hi, (n, desc.n_q))
    qd = rng.uniform(-desc.qd_max, desc.qd_max, (n, desc.n_q))
    sp = rng.uniform(-0.3, 0.3, (n, desc.n_t))
    g = n // 4
    sp[g:2 * g] = rng.uniform(5.0, 10.0, (g, desc.n_t))
    sp[2 * g:3 * g] = rng.uniform(-10.0, -5.0, (g, desc.n_t))
    qd[3 * g:] *= 60.0
    return q, qd, sp


def _robots():
    from gym_roboy_amd.envs.robots import MsjRobot
    from random_robots import random_ball_joint_robot
    out = [("msj", MsjRobot.get_description())]
    for n_t in (1, 5, 16):
        out.append(("ball%d" % n_t, random_ball_joint_robot(40 + n_t, n_t)[1]))
    return out


@pytest.mark.parametrize("which", ["msj", "ball1", "ball5", "ball16"])
def test_ball_joint_readout_function_matches_the_oracle_in_fp64(ts_lib, which):
    desc = dict(_robots())[which]
    q, qd, sp = _states(desc, 10000, 7)
    got = _host_readout(ts_lib, desc, q, qd, sp)
    ref, o = _oracle_readout(desc, q, qd, sp)
    # the edges are really visited
    g = q.shape[0] // 4
    assert np.all(ref["activation"][g:2 * g] == 0.0) and np.all(ref["activation"][2 * g:3 * g] == 1.0)
    v = ref["rate"] / (o.v_max * o.l0)
    assert np.sum(v < -1.0) > 100
    assert np.all(got["activation"][g:2 * g] == 0.0) and np.all(got["activation"][2 * g:3 * g] == 1.0)
    # fp64 closed form against the fp64 generic formulation: rounding differences only
    scale = {"length": np.abs(ref["length"]).max(), "rate": np.abs(ref["rate"]).max(), "activation": 1.0,
             "force": float(np.max(o.f_max))}
    for k in ("length", "rate", "activation", "force"):
        err = np.abs(got[k] - ref[k]).max() / scale[k]
        assert err < 1e-10, (which, k, err)
    assert np.all(got["force"] >= 0.0) and np.all((got["activation"] >= 0.0) & (got["activation"] <= 1.0))
