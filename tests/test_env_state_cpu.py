"""CPU tests of the env's snapshot and restore: the pure comparison of a state against an env's identity and segment
table, the argument errors that are raised before any library call, the C ABI's declarations, and the guard that keeps the next
option from forgetting its planes - every device-pointer member of the handle and of its option records is classified exactly once."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_roboy_amd import _native as nat
from gym_roboy_amd.envs import options as opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "roboy_sim.h")).read()
SOURCE = open(os.path.join(ROOT, "gym_roboy_amd", "csrc", "roboy_sim.hip")).read()
HOST = open(os.path.join(ROOT, "gym_roboy_amd", "csrc", "env_host.hpp")).read()

IDENTITY = {"n_envs": 300, "n_q": 3, "n_t": 8, "seed": 14, "env_id_offset": 0, "integrator": 1, "n_substeps": 1, "step_size": 0.1}


def _table(*planes):
    """a segment table as the library lays it out: each segment at the next multiple of 16"""
    table, at = [], 0
    for name, dtype, rows, cols in planes:
        table.append((name, dtype, rows, cols, at))
        at += (np.dtype(dtype).itemsize * rows * cols + 15) // 16 * 16
    return table, at


PLANES = (("core.q", "float32", 3, 300), ("core.feas", "uint32", 1, 300), ("env.ep_sum", "float64", 2, 300), ("io.ring", "float32", 4, 2400),
          ("goals.row_stats", "uint64", 2, 37), ("elog.ret", "float32", 2, 300), ("elog.full", "uint32", 1, 1))


def _state(planes=PLANES, **identity):
    table, nbytes = _table(*planes)
    return {"version": opt.ENV_STATE_VERSION, "identity": dict(IDENTITY, **identity), "segments": table, "blob": np.zeros(nbytes, np.uint8),
            "host": {"env_steps": 0.0}, "env": {}, "markers": {"last_actions": None},
            "slabs": {k: np.zeros(1, np.float32) for k in opt.ENV_STATE_SLABS}}


def test_equal_tables_pass_and_each_kind_of_difference_is_named():
    own, _ = _table(*PLANES)
    opt.compare_env_state(IDENTITY, own, _state())
    opt.compare_env_state(IDENTITY, [list(s) for s in own], _state())          # (a table that went through a file: lists)
    for field, other in (("n_envs", 256), ("seed", 15), ("env_id_offset", 300), ("integrator", 0), ("n_substeps", 2), ("step_size", 0.05),
                         ("n_t", 12), ("n_q", 20)):
        with pytest.raises(ValueError, match=r"\b%s = " % field):
            opt.compare_env_state(IDENTITY, own, _state(**{field: other}))
    # identity is looked at first, and the first field in its fixed order is the one named
    with pytest.raises(ValueError, match="n_envs"):
        opt.compare_env_state(IDENTITY, own, _state(planes=PLANES[:2], n_envs=256, seed=1))

    def swap(k, **kw):
        p = dict(zip(("name", "dtype", "rows", "cols"), PLANES[k]), **kw)
        return PLANES[:k] + ((p["name"], p["dtype"], p["rows"], p["cols"]),) + PLANES[k + 1:]

    cases = ((swap(3, rows=8), r"'io\.ring' has shape \[8\]\[2400\] in the state, \[4\]\[2400\]"),        # another ring size
             (swap(5, rows=3), r"'elog\.ret' has shape \[3\]\[300\]"),                                      # another log capacity
             (swap(4, cols=11), r"'goals\.row_stats' has shape \[2\]\[11\]"),                               # another pool
             (swap(1, dtype="float32"), r"'core\.feas' is float32 in the state, uint32 in this env"),
             (PLANES[:3] + PLANES[4:], r"this env has the segment 'io\.ring', the state has none"),         # the saved env lacked an option
             (PLANES[:-1], r"this env has the segment 'elog\.full', the state has none"),
             (PLANES[:3] + (("par.planes", "float32", 20, 300),) + PLANES[3:], r"the state has the segment 'par\.planes', this env has none"),
             (PLANES + (("start.pool", "float32", 37, 3),), r"the state has the segment 'start\.pool', this env has none"),
             (PLANES[:2] + (PLANES[3], PLANES[2]) + PLANES[4:], r"'env\.ep_sum' stands at another place"))
    for planes, message in cases:
        with pytest.raises(ValueError, match=message):
            opt.compare_env_state(IDENTITY, own, _state(planes=planes))
    # the same planes at other offsets
    moved = _state()
    moved["segments"] = [s if k < 2 else s[:4] + (s[4] + 16,) for k, s in enumerate(moved["segments"])]
    with pytest.raises(ValueError, match=r"'env\.ep_sum' lies at offset"):
        opt.compare_env_state(IDENTITY, own, moved)


def test_a_dict_that_is_no_state_is_refused_by_its_own_content():
    opt.check_env_state_dict(_state())
    for bad in (None, [], "state", 3):
        with pytest.raises(ValueError, match="a dict from RoboyVecEnv.state_dict"):
            opt.check_env_state_dict(bad)
    for key in opt.ENV_STATE_KEYS:
        sd = _state()
        del sd[key]
        with pytest.raises(ValueError, match="has no %r" % key):
            opt.check_env_state_dict(sd)
    sd = _state(); sd["version"] = 99
    with pytest.raises(ValueError, match="version"):
        opt.check_env_state_dict(sd)
    sd = _state(); sd["blob"] = sd["blob"][:-16]
    with pytest.raises(ValueError, match="the blob has"):
        opt.check_env_state_dict(sd)
    sd = _state(); sd["blob"] = sd["blob"].astype(np.float32)
    with pytest.raises(ValueError, match="uint8"):
        opt.check_env_state_dict(sd)
    sd = _state(); sd["segments"][2] = ("env.ep_sum", "float16", 2, 300, sd["segments"][2][4])
    with pytest.raises(ValueError, match="is no segment"):
        opt.check_env_state_dict(sd)
    sd = _state(); sd["segments"][2] = sd["segments"][2][:4] + (8,)
    with pytest.raises(ValueError, match="offset"):
        opt.check_env_state_dict(sd)
    sd = _state(); del sd["slabs"]["rew"]
    with pytest.raises(ValueError, match="'rew' slab"):
        opt.check_env_state_dict(sd)
    sd = _state(); del sd["host"]["env_steps"]
    with pytest.raises(ValueError, match="env_steps"):
        opt.check_env_state_dict(sd)


def test_argument_errors_come_before_any_library_call():
    """an env object without a simulation: whatever reached the library would raise AttributeError, not ValueError"""
    from gym_roboy_amd.envs.vec_env import RoboyVecEnv
    env = RoboyVecEnv.__new__(RoboyVecEnv)
    assert not hasattr(env, "sim")
    for bad in (None, {}, {"version": 1}, _state() | {"version": 0}, dict(_state(), blob=np.zeros(3, np.uint8))):
        with pytest.raises(ValueError):
            env.load_state_dict(bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="dict_view"):
            env.state_dict(dict_view=bad)
    with pytest.raises(AttributeError):          # (and a well-formed dict does go on to the env)
        env.load_state_dict(_state())
    env._pending_actions = np.zeros((4, 8), np.float32)          # between step_async and step_wait: no state to take
    with pytest.raises(RuntimeError, match="step_async"):
        env.state_dict()


def test_views_are_views_of_the_blob():
    sd = _state()
    views = opt.env_state_views(sd["segments"], sd["blob"])
    assert list(views) == [p[0] for p in PLANES]
    for (name, dtype, rows, cols, offset) in sd["segments"]:
        assert views[name].dtype == np.dtype(dtype) and views[name].shape == (rows, cols)
    views["env.ep_sum"][1, 7] = 2.5
    at = sd["segments"][2][4] + 8 * (300 + 7)
    assert sd["blob"][at:at + 8].view(np.float64)[0] == 2.5


def test_the_c_abi_declares_and_exports_the_four_calls():
    lib = nat.load()
    for name in ("rb_env_state_segments", "rb_env_state_bytes", "rb_env_state_save_dev", "rb_env_state_load_dev"):
        assert re.search(r"\bint %s\(rb_sim \*sim" % name, HEADER) and name in nat.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int
    assert int(re.search(r"#define RB_ABI_VERSION (\d+)", HEADER).group(1)) == 6 == lib.rb_abi_version()
    # the structs as the header lays them out
    assert ctypes.sizeof(nat.StateSegment) == 48 + 4 + 4 + 3 * 8 and nat.StateSegment.offset.offset == 72
    assert ctypes.sizeof(nat.StateHost) == 64
    fields = re.search(r"typedef struct rb_state_segment \{(.*?)\} rb_state_segment;", HEADER, re.S).group(1)
    assert re.findall(r"\b(?:char|uint32_t|int64_t)\s+([a-z_, ]+)(?:\[48\])?;", fields) == ["name", "dtype", "reserved", "rows, cols", "offset"]
    enum = re.search(r"enum rb_state_dtype \{(.*?)\}", HEADER).group(1)
    assert [x.strip() for x in enum.split(",")] == ["RB_STATE_F32 = 0", "RB_STATE_U32 = 1", "RB_STATE_F64 = 2", "RB_STATE_U64 = 3"]
    assert [nat.STATE_DTYPES[k] for k in range(4)] == ["float32", "uint32", "float64", "uint64"]
    # null handles are refused, not fatal
    count, nbytes = ctypes.c_int32(), ctypes.c_int64()
    assert lib.rb_env_state_segments(None, None, 0, ctypes.byref(count)) == nat.RB_EINVAL
    assert lib.rb_env_state_bytes(None, ctypes.byref(nbytes)) == nat.RB_EINVAL
    assert lib.rb_env_state_save_dev(None, None, 0, None) == nat.RB_EINVAL
    assert lib.rb_env_state_load_dev(None, None, 0, None) == nat.RB_EINVAL


def test_load_keeps_the_graphs_and_says_why():
    """the preamble's convention: an entry point that opens with reconfigure() and keeps the graphs carries a comment that says why"""
    body = HOST[HOST.index("int rb_env_state_load_dev("):]
    body = body[:body.index("\n}\n")]
    assert "reconfigure(s, KEEP_GRAPHS" in body and "DROP_GRAPHS" not in body
    comment = " ".join(re.findall(r"//(.*)", body[:body.index("reconfigure(")]))
    assert "graphs stay" in comment and "IN PLACE" in comment
    save = HOST[HOST.index("int rb_env_state_save_dev("):HOST.index("int rb_env_state_load_dev(")]
    assert "hipMemcpyDeviceToDevice, s->stream" in save and "Synchronize" not in save and "reconfigure(" not in save
    assert "hipLaunchKernelGGL" not in HOST[HOST.index("int rb_env_state_segments("):]          # no kernel: copies


# ---- the guard: every device pointer of the handle and of its option records is state or on the "not state" list, never both ----
def _struct_body(name):
    start = SOURCE.index("struct %s {" % name)
    depth, k = 0, SOURCE.index("{", start)
    for k in range(k, len(SOURCE)):
        depth += {"{": 1, "}": -1}.get(SOURCE[k], 0)
        if depth == 0:
            return SOURCE[start:k]
    raise AssertionError(name)


def _device_pointer_members(body):
    """the names d_... declared as pointers in a struct body: `float *d_a = nullptr, *d_b = nullptr;`, comments dropped"""
    code = re.sub(r"//.*", "", body)
    return re.findall(r"\*\s*(d_\w+)\s*(?:=|;|,)", code)


def _classification():
    records = ["rb_sim"] + sorted(set(re.findall(r"^struct (Opt\w+) \{", SOURCE, re.M)))
    members = {rec: _device_pointer_members(_struct_body(rec)) for rec in records}
    # which member of rb_sim holds which record: `OptParams par; OptChannels chan; ...`
    holder = {}
    for line in re.sub(r"//.*", "", _struct_body("rb_sim")).splitlines():
        for rec, name in re.findall(r"\b(Opt\w+)\s+(\w+)\s*;", line):
            holder[name] = rec
    fn = SOURCE[SOURCE.index("std::vector<StateSeg> state_segments(rb_sim *s) {"):]
    fn = re.sub(r"//.*", "", fn[:fn.index("\n}\n")])
    state = []
    for field, member in re.findall(r"\bs->(?:(\w+)\.)?(d_\w+)", fn):
        state.append("%s.%s" % (holder[field] if field else "rb_sim", member))
    head = SOURCE[SOURCE.index("// ---- the handle's state"):SOURCE.index("struct StateSeg {")]
    listed = re.findall(r"\b(rb_sim|Opt\w+)\.(d_\w+)", " ".join(re.findall(r"//(.*)", head[head.index("// not state"):])))
    return members, holder, state, ["%s.%s" % x for x in listed]


def test_every_device_pointer_is_state_or_listed_as_not_state_exactly_once():
    members, holder, state, not_state = _classification()
    everything = ["%s.%s" % (rec, m) for rec, names in members.items() for m in names]
    assert len(everything) == len(set(everything)) and len(everything) > 50
    assert set(holder.values()) == set(members) - {"rb_sim"}, "an option record that is no member of the handle (or the other way round)"
    assert len(state) == len(set(state)), sorted(x for x in state if state.count(x) > 1)
    assert len(not_state) == len(set(not_state))
    assert not set(state) & set(not_state), sorted(set(state) & set(not_state))
    missing = sorted(set(everything) - set(state) - set(not_state))
    assert not missing, "neither in state_segments() nor on its 'not state' list: %s" % missing
    unknown = sorted((set(state) | set(not_state)) - set(everything))
    assert not unknown, "classified, but no device pointer of the handle: %s" % unknown
    # what the list is there for: the planes the options' Open items named
    for plane in ("OptPush.d_count", "OptEpisodeLog.d_acc", "OptStart.d_count", "OptStart.d_index", "OptGoals.d_pool", "OptGoals.d_level",
                  "OptGoals.d_row_stats", "OptIo.d_ring", "OptParams.d_draws", "rb_sim.d_goal_count", "rb_sim.d_ep_cnt"):
        assert plane in state


def test_the_guard_sees_a_forgotten_plane():
    """the parser, held to a struct it has not seen: a plane added to a record shows up as a member"""
    assert _device_pointer_members("bool on; uint32_t *d_a = nullptr, *d_b = nullptr;  // *d_not\n float *d_c; int n; double *d_e = nullptr; "
                                   "unsigned long long *d_total = nullptr; rb::MsjTendon<float> *d_ten = nullptr;") == \
        ["d_a", "d_b", "d_c", "d_e", "d_total", "d_ten"]
    members, _, state, not_state = _classification()
    assert "d_total" in members["OptPush"] and "d_ten" in members["rb_sim"] and "d_hist" in members["OptGoals"]


def test_segment_names_are_unique_and_stable():
    fn = SOURCE[SOURCE.index("std::vector<StateSeg> state_segments(rb_sim *s) {"):]
    names = re.findall(r'seg\("([a-z_.0-9]+)"', fn[:fn.index("\n}\n")])
    assert len(names) == len(set(names)) and all(len(n) < 48 and re.fullmatch(r"[a-z]+\.[a-z_]+", n) for n in names)
    assert names[:4] == ["core.q", "core.qd", "core.feas", "core.goal_count"]
    for n in ("io.ring", "goals.row_stats", "goals.pool", "start.pool", "elog.full", "push.impulse", "shaping.sums", "par.planes", "critic.rows"):
        assert n in names
