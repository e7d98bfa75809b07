"""The pair form of the "rolled stages" step (msj_math.hpp: AccelPaired / tendon_pair, the headline RK4 kernel's acceleration)
computes what the one-tendon-at-a-time form (AccelPinned) computes, BIT FOR BIT: the same expressions and the same order of
the torque sums, only the order of independent instructions differs.  Both are compiled in one host translation unit
(tests/hostmath/accel_paired_host.cpp) and compared on seeded states and actions inside the joint limits: the acceleration alone,
and whole env steps (Euler, RK4; one and several substeps), in fp32 and fp64, for MsjRobot and a random 8-tendon ball-joint robot."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import random_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from build_dir import build_dir  # noqa: E402

N = 4096


@pytest.fixture(scope="module")
def ap_lib():
    so = os.path.join(build_dir(), "libaccel_paired_host.so")
    src = os.path.join(ROOT, "tests", "hostmath", "accel_paired_host.cpp")
    deps = [src] + [os.path.join(ROOT, "gym_roboy_amd", "csrc", f) for f in ("msj_math.hpp", "msj_build.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    return ctypes.CDLL(so)


def _desc(which):
    from gym_roboy_amd.envs.robots import MsjRobot
    from random_robots import random_ball_joint_robot
    return MsjRobot.get_description() if which == "msj" else random_ball_joint_robot(31, 8)[1]


def _both(lib, desc, dtype, mode, nsub, seed):
    q, qd, sp = (np.ascontiguousarray(a, dtype) for a in random_states(desc, N, seed))
    fn = lib.ap_run_f32 if dtype == np.float32 else lib.ap_run_f64
    out = [np.zeros((N, 3), dtype), np.zeros((N, 3), dtype), np.zeros(N, np.uint8),
           np.zeros((N, 3), dtype), np.zeros((N, 3), dtype), np.zeros(N, np.uint8)]
    rc = fn(ctypes.byref(desc.as_c_struct()), ctypes.c_double(0.1), nsub, mode, ctypes.c_long(N),
            *[ctypes.c_void_p(a.ctypes.data) for a in (q, qd, sp)], *[ctypes.c_void_p(a.ctypes.data) for a in out])
    assert rc == 0
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("which", ["msj", "ball8"])
def test_paired_acceleration_is_bit_identical_to_the_pinned_one(ap_lib, which, dtype):
    qa, _, _, qb, _, _ = _both(ap_lib, _desc(which), dtype, 0, 1, 5)
    assert np.isfinite(qa).all() and np.abs(qa).max() > 0
    assert qa.tobytes() == qb.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nsub", [1, 4])
@pytest.mark.parametrize("mode", [1, 2], ids=["euler", "rk4"])
@pytest.mark.parametrize("which", ["msj", "ball8"])
def test_paired_step_is_bit_identical_to_the_pinned_one(ap_lib, which, mode, nsub, dtype):
    q0 = random_states(_desc(which), N, 6 + nsub)[0]
    qa, va, fa, qb, vb, fb = _both(ap_lib, _desc(which), dtype, mode, nsub, 6 + nsub)
    assert np.isfinite(qa).all() and not np.array_equal(qa.astype(np.float32), q0)       # the step moved the state
    assert qa.tobytes() == qb.tobytes() and va.tobytes() == vb.tobytes() and np.array_equal(fa, fb)
