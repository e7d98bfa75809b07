"""Tendon channels in the fused env step's observation (include/roboy_sim.h: rb_env_obs_*; csrc/env_obs.hpp)
without a GPU: the ABI, the pure column count, error handling on a null handle, the new kernel instances in the shipped code
objects (no scratch, no spills, their last argument where the kernels read it late), and the host restatement of the expected
columns (tests/env_obs_util.py) against the conventions of tests/test_tendon_state_cpu.py and the per-env descriptions of
tests/env_params_util.py.  The GPU file (test_env_obs_gpu.py) checks the kernels themselves."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from gym_roboy_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()
LIB = os.path.join(ROOT, "gym_roboy_amd", "csrc", "libroboy_sim.so")
NAMES = ("rb_env_obs_configure", "rb_env_obs_dim", "rb_env_obs_count")
C8, CX = "rb::MsjConst<float, 8>", "rb::MsjConst<float, 16>"
# Euler / RK4 each: baked MsjRobot (the unroll factors of the large-batch env-per-lane rows: 8 / rolled stages = 9), kernarg Const8
# (2), kernarg ConstX (0); each again in parameter form; and the two row kernels of rb_env_reset_dev
NEW_KERNELS = ["rbo::msj_obs_env_step<0, 256, 8, %s, true>" % C8, "rbo::msj_obs_env_step<1, 256, 9, %s, true>" % C8] + \
    ["rbo::msj_obs_env_step<%d, 256, 2, %s, false>" % (i, C8) for i in (0, 1)] + \
    ["rbo::msj_obs_env_step<%d, 256, 0, %s, false>" % (i, CX) for i in (0, 1)] + \
    ["rbo::msj_obs_params_env_step<%d, 256, %s, %s>" % (i, c, bk) for i in (0, 1) for c, bk in ((C8, "true"), (C8, "false"), (CX, "false"))] + \
    ["rbo::msj_obs_rows<256, %s >" % c for c in (C8, CX)]


def test_the_three_entry_points_are_declared_exported_and_mirrored():
    lib = nat.load()
    for name in NAMES:
        assert re.search(r"\b(int|int32_t) %s\(" % name, HEADER), name
        assert name in nat.SIGNATURES
        assert hasattr(lib, name)
    assert lib.rb_env_obs_configure.restype is ctypes.c_int and lib.rb_env_obs_count.restype is ctypes.c_int32
    for bit, name in ((1, "LENGTH"), (2, "RATE"), (4, "ACTIVATION"), (8, "FORCE"), (15, "ALL")):
        assert re.search(r"RB_OBS_%s = %d\b" % (name, bit), HEADER)


def test_obs_count_is_pure_and_counts_the_selected_channels():
    lib = nat.load()
    for n_q, n_t in ((3, 8), (3, 1), (3, 16), (20, 38)):
        for mask in range(16):
            assert lib.rb_env_obs_count(n_q, n_t, mask) == 3 * n_q + bin(mask).count("1") * n_t
    assert lib.rb_env_obs_count(3, 8, 1 | 8) == 25 and lib.rb_env_obs_count(3, 8, 15) == 41
    assert lib.rb_env_obs_count(3, 8, 16) == -1 and lib.rb_env_obs_count(-1, 8, 1) == -1


def test_null_handle_is_an_error_not_an_abort():
    lib = nat.load()
    dim = ctypes.c_int32()
    assert lib.rb_env_obs_configure(None, 1, None) == nat.RB_EINVAL
    assert lib.rb_env_obs_dim(None, ctypes.byref(dim)) == nat.RB_EINVAL
    assert lib.rb_last_error()


def test_python_mask_and_scale_helpers():
    from gym_roboy_amd.envs.vec_env import TENDON_OBS_CHANNELS, tendon_obs_mask, tendon_obs_scales
    from env_obs_util import BITS, CHANNELS
    assert TENDON_OBS_CHANNELS == CHANNELS
    assert tendon_obs_mask(("force", "length")) == BITS["length"] | BITS["force"] == 9
    assert tendon_obs_mask("rate") == 2 and tendon_obs_mask(CHANNELS) == 15
    for bad in (("torque",), ("force", "force")):
        with pytest.raises(ValueError):
            tendon_obs_mask(bad)
    assert np.array_equal(tendon_obs_scales({"force": 0.25}), np.float32([1, 1, 1, 0.25]))
    for bad in ({"force": np.inf}, {"pull": 1.0}):
        with pytest.raises(ValueError):
            tendon_obs_scales(bad)


def test_new_kernels_are_shipped_without_scratch_or_spills():
    import code_object_meta as com
    meta = {com.short(k): v for k, v in com.kernel_metadata(LIB).items()}
    assert sorted(k for k in meta if k.startswith("rbo::")) == sorted(NEW_KERNELS)
    for name in NEW_KERNELS:
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)


def test_the_late_obs_argument_sits_where_the_kernels_read_it():
    """env_obs.hpp: the kernarg instances read their ObsArgs argument - the LAST one, behind MsjEnvArgs (and ParamArgs) - through the
    kernel-argument segment at obs_args_offset(end of the argument in front) = that end rounded up to 8 bytes."""
    import code_object_meta as com
    notes = []
    for image in com.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as fh:
            fh.write(image)
            fh.flush()
            notes.append(subprocess.run([os.path.join(com.LLVM, "llvm-readelf"), "--notes", fh.name], capture_output=True, text=True, check=True).stdout)
    checked = 0
    for block in "\n".join(notes).split("\n  - .agpr_count:")[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        if not m or "msj_obs_" not in m.group(1) or "env_step" not in m.group(1):
            continue
        args = []
        for entry in re.split(r"\n      - ", block.split(".args:", 1)[1].split("\n    .group_segment_fixed_size", 1)[0])[1:]:
            f = {k: v for k, v in re.findall(r"\.(offset|size|value_kind):\s+(\w+)", entry)}
            if not f["value_kind"].startswith("hidden"):
                args.append((int(f["offset"]), int(f["size"]), f["value_kind"]))
        assert len(args) == (4 if "params" in m.group(1) else 3) and all(a[2] == "by_value" for a in args), (m.group(1), args)
        last, prev = args[-1], args[-2]
        nt = 16 if "MsjConstIfLi16" in m.group(1) else 8
        assert last[1] == 16 + 16 + 16 * nt, (m.group(1), last)                  # mask, obs_dim, staged, pad, scale[4], units[nt]
        assert last[0] == (prev[0] + prev[1] + 7) // 8 * 8, (m.group(1), args)
        assert args[1][0] == (args[0][1] + 7) // 8 * 8                             # MsjEnvArgs, as in the plain env kernels
        checked += 1
    assert checked == 12


# ---- the host restatement ----
def _robots():
    from gym_roboy_amd.envs.robots import MsjRobot
    from random_robots import random_ball_joint_robot
    return [("msj", MsjRobot(), MsjRobot.get_description())] + \
        [("ball%d" % nt,) + tuple(random_ball_joint_robot(40 + nt, nt)) for nt in (5, 12)]


@pytest.mark.parametrize("which", ["msj", "ball5", "ball12"])
def test_restatement_follows_the_readout_tests_conventions(which):
    """readout64 without parameters IS test_tendon_state_cpu._oracle_readout (same oracle calls, same signs and units)"""
    from env_obs_util import readout64
    from test_tendon_state_cpu import _oracle_readout, _states
    desc = {n: d for n, _, d in _robots()}[which]
    q, qd, sp = _states(desc, 2000, 5)
    got, _ = readout64(desc, q, qd, sp)
    ref, _ = _oracle_readout(desc, q, qd, sp)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert np.all(got["force"] >= 0) and np.all(got["length"] > 0)


@pytest.mark.parametrize("which", ["msj", "ball12"])
def test_restatement_with_parameters_is_each_envs_own_description(which):
    """vectorised force scale and set-point offset against the oracle on env_params_util.perturbed(desc, par[i]), env by env"""
    from env_obs_util import readout64
    from env_params_util import perturbed, random_params
    from test_tendon_state_cpu import _oracle_readout, _states
    desc = {n: d for n, _, d in _robots()}[which]
    nt, n = desc.n_t, 48
    q, qd, sp = _states(desc, n, 9)
    par = random_params(np.random.default_rng(3), nt, n)
    got, _ = readout64(desc, q, qd, sp, par)
    for i in range(n):
        ref, _ = _oracle_readout(perturbed(desc, par[i]), q[i:i + 1], qd[i:i + 1], sp[i:i + 1] + par[i, nt:2 * nt])
        for k in ref:
            np.testing.assert_allclose(got[k][i], ref[k][0], rtol=1e-13, atol=1e-13 * float(np.max(desc.f_max)), err_msg=k)


def test_expected_columns_order_scale_and_zero_set_points():
    from env_obs_util import column_tolerances, env_rescale64, expected_columns, readout64
    _, robot, desc = _robots()[0]
    rng = np.random.default_rng(1)
    q = rng.uniform(0.9 * desc.q_lo, 0.9 * desc.q_hi, (16, 3))
    qd = rng.uniform(-desc.qd_max, desc.qd_max, (16, 3))
    act = rng.uniform(-1.2, 1.2, (16, 8))
    box = robot.get_action_space()
    sp = env_rescale64(robot, act)
    assert sp.min() >= box.low[0] - 1e-12 and sp.max() <= box.high[0] + 1e-12 and np.any(sp == box.low[0])     # clamped
    ref, o = readout64(desc, q, qd, sp)
    cols, _ = expected_columns(robot, desc, q, qd, act, ("force", "length"), {"force": 0.5})
    assert cols.shape == (16, 16)
    assert np.array_equal(cols[:, :8], ref["length"]) and np.array_equal(cols[:, 8:], 0.5 * ref["force"])      # row order, not argument order
    zero, _ = expected_columns(robot, desc, q, qd, None, ("activation",))
    assert np.array_equal(zero, readout64(desc, q, qd, np.zeros((16, 8)))[0]["activation"])
    tol = column_tolerances(o, ("length", "force"), {"force": -0.5})
    assert tol.shape == (16,) and np.all(tol > 0) and np.allclose(tol[8:], 0.5 * 2e-5 * np.max(o.f_max))
