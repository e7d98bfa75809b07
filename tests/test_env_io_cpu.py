"""Action latency and sensor noise of the fused env step (include/roboy_sim.h: rb_env_io_*; csrc/env_io.hpp) without a
GPU: the two restated draws (tests/env_io_util.py), the ABI, the Python-side validation, and the new kernel instances in the shipped
code objects - no scratch, no spills, the late arguments where the device code reads them.  The GPU file (test_env_io_gpu.py) checks
the kernels themselves."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from env_io_util import STREAM_DELAY, STREAM_SENSOR, DelayBook, delay_draw, sensor_noise64
from gym_roboy_amd import _native as nat
from oracle import philox_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()
LIB = os.path.join(ROOT, "gym_roboy_amd", "csrc", "libroboy_sim.so")
NAMES = ("rb_env_io_configure", "rb_env_io_ptr", "rb_env_io_sample_delay_dev")
C8, CX = "rb::MsjConst<float, 8>", "rb::MsjConst<float, 16>"
# Euler / RK4 each: baked MsjRobot (unroll 8 / rolled stages = 9), kernarg Const8 (2), kernarg ConstX (0); each again in parameter
# form; the small-batch instances that stand in for MsjRobot's 64-thread env-per-lane rows (tendons and stages written out); the reset
# rows' noise and the delay draw
NEW_KERNELS = ["rbio::msj_io_env_step<%d, 64, 8, %s, true>" % (i, C8) for i in (0, 1)] + \
    ["rbio::msj_io_env_step<0, 256, 8, %s, true>" % C8, "rbio::msj_io_env_step<1, 256, 9, %s, true>" % C8] + \
    ["rbio::msj_io_env_step<%d, 256, 2, %s, false>" % (i, C8) for i in (0, 1)] + \
    ["rbio::msj_io_env_step<%d, 256, 0, %s, false>" % (i, CX) for i in (0, 1)] + \
    ["rbio::msj_io_params_env_step<%d, 256, %s, %s>" % (i, c, bk) for i in (0, 1) for c, bk in ((C8, "true"), (C8, "false"), (CX, "false"))] + \
    ["rbio::io_noise_rows", "rbio::io_sample_delay"]
IO_ARGS_SIZE = 8 * 4 + 8 + 6 * 4 + 4 * 76        # three planes and the ring, slot stride, six ints, colsig[76]


# ---- the restated draws ----
def test_sensor_noise_is_standard_normal_and_independent_across_columns_rows_and_envs():
    ids = np.arange(100_000, dtype=np.uint64) + np.uint64(777)
    z = sensor_noise64(5, ids, 3, 25)                                    # 2.5e6 draws
    assert z.shape == (100_000, 25) and z.dtype == np.float64
    assert abs(z.mean()) < 0.005 and abs(z.var() - 1.0) < 0.005 and abs((z ** 4).mean() - 3.0) < 0.05
    assert np.abs(np.corrcoef(z.T) - np.eye(25)).max() < 0.015           # columns
    assert abs(np.corrcoef(z[:-1, 0], z[1:, 0])[0, 1]) < 0.01            # neighbouring envs
    z4 = sensor_noise64(5, ids, 4, 25)
    assert abs(np.corrcoef(z[:, 0], z4[:, 0])[0, 1]) < 0.01 and np.abs(z4 - z).max() > 1.0      # the next row
    z32 = sensor_noise64(5, ids, 3, 25, dtype=np.float32)
    assert z32.dtype == np.float32 and np.abs(z32.astype(np.float64) - z).max() < 1e-5
    # the layout: column c = component c & 3 of block c >> 2, whatever the row's width; per-env row numbers
    wide = sensor_noise64(5, ids[:1000], 3, 73)
    assert np.array_equal(wide[:, :25], z[:1000]) and np.array_equal(sensor_noise64(5, ids[:1000], 3, 9), z[:1000, :9])
    w = philox_np.draw(5, ids[:1000], 3, STREAM_SENSOR, 18)
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) / 2.0 ** 24
    u2 = (w[:, 1] >> np.uint32(8)).astype(np.float64) / 2.0 ** 24
    assert np.allclose(wide[:, 72], np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2), rtol=0, atol=1e-14)
    rows = np.where(np.arange(1000) % 2 == 0, 3, 4)
    mixed = sensor_noise64(5, ids[:1000], rows, 25)
    assert np.array_equal(mixed[0::2], z[:1000][0::2]) and np.array_equal(mixed[1::2], z4[:1000][1::2])
    # it is not the policy's stream, and another seed or the id's high word give other draws
    from oracle import policy_ref
    assert STREAM_SENSOR != policy_ref.STREAM_POLICY and np.abs(policy_ref.policy_noise(5, ids[:1000], 3, 25) - z[:1000]).max() > 1.0
    for other in (sensor_noise64(6, ids[:1000], 3, 25), sensor_noise64(5, ids[:1000] + (np.uint64(1) << np.uint64(32)), 3, 25)):
        assert np.abs(other - z[:1000]).max() > 1.0


def test_delay_draw_covers_its_range_exactly_uniformly_and_does_not_move_with_the_sharding():
    ids = np.arange(200_000, dtype=np.uint64)
    for lo, hi in ((0, 3), (1, 3), (2, 7), (0, 7), (4, 4), (0, 0)):
        d = delay_draw(9, ids, 0, lo, hi)
        assert d.dtype == np.int64 and d.min() == lo and d.max() == hi
        counts = np.bincount(d - lo, minlength=hi - lo + 1)
        assert np.abs(counts / len(ids) - 1.0 / (hi - lo + 1)).max() < 0.005
    # exactly uniform in the 24-bit word: value v takes the words [ceil(v 2^24 / R), ceil((v + 1) 2^24 / R)), whose counts differ by
    # at most one - checked on the map itself, over every boundary word
    for lo, hi in ((0, 3), (1, 3), (0, 6), (2, 7)):
        R = hi - lo + 1
        edges = [-(-v * (1 << 24) // R) for v in range(R + 1)]
        sizes = np.diff(edges)
        assert edges[0] == 0 and edges[-1] == 1 << 24 and sizes.max() - sizes.min() <= 1
        for v in range(R):
            for u, want in ((edges[v], v), (edges[v + 1] - 1, v)):
                assert lo + ((u * R) >> 24) == lo + want
    # the word is word 0 of block 0 of stream 5 at index = the draw number
    w = philox_np.draw(9, ids[:100], 2, STREAM_DELAY, 0)[:, 0].astype(np.int64)
    assert np.array_equal(delay_draw(9, ids[:100], 2, 1, 3), 1 + (((w >> 8) * 3) >> 24))
    # keyed by the global env id: a shard sees the draws of its envs wherever it starts; per-env draw counters
    whole = delay_draw(9, ids[:4096], 1, 0, 7)
    assert np.array_equal(delay_draw(9, ids[:1024] + np.uint64(1000), 1, 0, 7), whole[1000:2024])
    m = np.arange(4096) % 3
    mixed = delay_draw(9, ids[:4096], m, 0, 7)
    for k in range(3):
        assert np.array_equal(mixed[m == k], delay_draw(9, ids[:4096], k, 0, 7)[m == k])
    assert np.mean(delay_draw(9, ids[:4096], 2, 0, 7) != whole) > 0.5


def test_delay_book_feeds_the_shifted_sequence_and_the_rest_command():
    book = DelayBook(4, 2)
    d = np.array([0, 1, 2, 3])
    acts = [np.full((4, 2), t + 1.0, np.float32) for t in range(5)]
    fed = []
    for t, a in enumerate(acts):
        out, rest = book.shifted(a, d)
        fed.append((out[:, 0].copy(), rest.copy()))
        book.advance(np.array([False, False, t == 2, False]))
    assert np.array_equal(fed[0][1], [False, True, True, True]) and np.array_equal(fed[0][0], [1, 0, 0, 0])
    assert np.array_equal(fed[2][0], [3, 2, 1, 0]) and np.array_equal(fed[2][1], [False, False, False, True])
    # env 2 was done at the third step: its episode restarts, the old episode's actions are not used again
    assert np.array_equal(fed[3][0], [4, 3, 0, 1]) and np.array_equal(fed[3][1], [False, False, True, False])
    assert np.array_equal(fed[4][0], [5, 4, 0, 2])


# ---- the ABI ----
def test_the_three_entry_points_are_declared_exported_and_mirrored():
    lib = nat.load()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, HEADER), name
        assert name in nat.SIGNATURES
        assert hasattr(lib, name) and getattr(lib, name).restype is ctypes.c_int
    assert re.search(r"#define RB_IO_MAX_DELAY 7\b", HEADER) and nat.RB_IO_MAX_DELAY == 7
    assert re.search(r"#define RB_ABI_VERSION 6\b", HEADER)
    # the struct as the header lays it out: six floats, four int32
    assert ctypes.sizeof(nat.EnvIoConfig) == 40
    assert [f[0] for f in nat.EnvIoConfig._fields_] == ["sigma_q", "sigma_qd", "sigma_tendon", "delay_lo", "delay_hi", "resample_on_reset", "_pad"]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct rb_env_io_config \{(.*?)\} rb_env_io_config;", HEADER, re.S).group(1))
    assert re.findall(r"\b([a-z_]+)(?:\[4\])?[,;]", body) == [f[0] for f in nat.EnvIoConfig._fields_]


def test_null_handle_is_an_error_not_an_abort():
    lib = nat.load()
    cfg = nat.EnvIoConfig()
    assert lib.rb_env_io_configure(None, ctypes.byref(cfg)) == nat.RB_EINVAL
    assert lib.rb_env_io_configure(None, None) == nat.RB_EINVAL
    assert lib.rb_env_io_ptr(None, None, None, None, None, None) == nat.RB_EINVAL
    assert lib.rb_env_io_sample_delay_dev(None, None) == nat.RB_EINVAL
    assert lib.rb_last_error()


def test_python_side_validation():
    from gym_roboy_amd.envs.vec_env import SENSOR_NOISE_KEYS, action_delay_range, sensor_noise_sigmas
    assert SENSOR_NOISE_KEYS == ("q", "qd", "length", "rate", "activation", "force")
    s = sensor_noise_sigmas({"q": 0.01, "qd": 0.05, "length": 5e-4, "force": 2.0}, ("length", "force"))
    assert s.dtype == np.float32 and np.array_equal(s, np.float32([0.01, 0.05, 5e-4, 0, 0, 2.0]))
    assert not sensor_noise_sigmas(None).any() and not sensor_noise_sigmas({}).any()
    for bad, ch in (({"q": -0.01}, ()), ({"q": np.nan}, ()), ({"qd": np.inf}, ()),          # negative, not finite
                    ({"torque": 1.0}, ()), ({"goal": 0.1}, ()),                            # unknown key
                    ({"force": 2.0}, ("length",)), ({"rate": 0.1}, ())):                   # a channel that is not selected
        with pytest.raises(ValueError):
            sensor_noise_sigmas(bad, ch)
    assert action_delay_range(None) == (0, 0, False) and action_delay_range(2) == (2, 2, False)
    assert action_delay_range((0, 3)) == (0, 3, True) and action_delay_range((7, 7)) == (7, 7, True) and action_delay_range(0) == (0, 0, False)
    for bad in (8, (0, 8), (3, 1), -1, (-1, 2)):                                           # delay > 7, lo > hi, negative
        with pytest.raises(ValueError):
            action_delay_range(bad)


def test_checkpoint_helpers_record_both_settings():
    from gym_roboy_amd.ppo import _env_io_of

    class Env:
        sensor_noise = {"q": 0.01, "force": 2}
        action_delay = (0, 3)
    assert _env_io_of(Env()) == {"sensor_noise": {"q": 0.01, "force": 2.0}, "action_delay": [0, 3]}
    Env.action_delay = 2
    assert _env_io_of(Env())["action_delay"] == 2
    assert _env_io_of(None) == {"sensor_noise": {}, "action_delay": None}


# ---- the shipped code objects ----
def test_new_kernels_are_shipped_without_scratch_or_spills():
    import code_object_meta as com
    meta = {com.short(k): v for k, v in com.kernel_metadata(LIB).items()}
    assert sorted(k for k in meta if k.startswith("rbio::")) == sorted(NEW_KERNELS)
    for name in NEW_KERNELS:
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)


def test_the_late_arguments_sit_where_the_kernels_read_them():
    """env_io.hpp: every io env-step instance reads its ObsArgs and its IoArgs - the last two arguments, behind MsjEnvArgs (and
    ParamArgs) - through the kernel-argument segment, each at the end of the argument in front rounded up to 8 bytes; the reset
    rows' kernel reads its IoArgs 16 bytes into the segment."""
    import code_object_meta as com
    notes = []
    for image in com.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as fh:
            fh.write(image)
            fh.flush()
            notes.append(subprocess.run([os.path.join(com.LLVM, "llvm-readelf"), "--notes", fh.name], capture_output=True, text=True, check=True).stdout)
    checked = rows = 0
    for block in "\n".join(notes).split("\n  - .agpr_count:")[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        if not m or "4rbio" not in m.group(1):
            continue
        args = []
        for entry in re.split(r"\n      - ", block.split(".args:", 1)[1].split("\n    .group_segment_fixed_size", 1)[0])[1:]:
            f = {k: v for k, v in re.findall(r"\.(offset|size|value_kind):\s+(\w+)", entry)}
            if not f["value_kind"].startswith("hidden"):
                args.append((int(f["offset"]), int(f["size"]), f["value_kind"]))
        if "io_noise_rows" in m.group(1):
            assert [a[:2] for a in args[:3]] == [(0, 8), (8, 4), (16, IO_ARGS_SIZE)], args
            rows += 1
            continue
        if "env_step" not in m.group(1):
            continue
        assert len(args) == (5 if "params" in m.group(1) else 4) and all(a[2] == "by_value" for a in args), (m.group(1), args)
        io, obs, prev = args[-1], args[-2], args[-3]
        nt = 16 if "MsjConstIfLi16" in m.group(1) else 8
        assert obs[1] == 16 + 16 + 16 * nt and obs[0] == (prev[0] + prev[1] + 7) // 8 * 8, (m.group(1), args)
        assert io[1] == IO_ARGS_SIZE and io[0] == (obs[0] + obs[1] + 7) // 8 * 8, (m.group(1), args)
        assert args[1][0] == (args[0][1] + 7) // 8 * 8                             # MsjEnvArgs, as in the plain env kernels
        checked += 1
    assert checked == 14 and rows == 1
