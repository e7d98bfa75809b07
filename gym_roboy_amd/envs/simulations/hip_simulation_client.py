"""In-process MI355X simulation clients (replace the ROS -> CARDSflow round-trip).

``HipBatchSimulation`` owns N environments in HBM and is the throughput path:
``forward_step_command(actions[N, n_t])`` is one kernel launch.
``HipSimulationClient`` is the single-env drop-in for the reference's
``RosSimulationClient`` (``gym_roboy/envs/simulations/ros_simulation_client.py:12-81``):
same constructor convention ``Client(robot, process_idx=1, ...)``, same four
methods, same return types.  Both call ``libroboy_sim.so`` through ctypes and
raise if it is missing or no GPU is visible; there is no CPU fallback.
"""
import ctypes

import numpy as np

from ... import _native as nat
from ..robots import RobotState, RoboyRobot
from .simulation_client import SimulationClient
from .. import params as envparams

TENDON_STATE_KEYS = ("length", "rate", "activation", "force")


class HipBatchSimulation:
    """N lock-step environments of one robot on one GPU."""

    def __init__(self, robot: RoboyRobot, n_envs: int, integrator="euler", step_size: float = 0.1,
                 n_substeps: int = 1, device: int = 0, seed: int = 0, env_id_offset: int = 0):
        self.robot = robot
        self._h = None
        self._lib = nat.load()
        self._desc = robot.get_description()
        if integrator not in nat.INTEGRATORS:
            raise ValueError("integrator must be 'euler' or 'rk4'")
        handle = ctypes.c_void_p()
        nat.check(self._lib.rb_create(
            ctypes.byref(self._desc.as_c_struct()), int(n_envs), nat.INTEGRATORS[integrator],
            float(step_size), int(n_substeps), int(device), int(seed), int(env_id_offset),
            ctypes.byref(handle)))
        self._h = handle
        self.n_envs = int(n_envs)
        self.n_q, self.n_t = self._desc.n_q, self._desc.n_t
        self.step_size = float(step_size)
        self._owned = []
        self._stream = None            # what set_stream last handed to the library (None: the handle's own stream)
        self.n_params = 0              # P while per-env parameters are enabled
        self._d_param_mask = None      # sample_params(mask): device copy of the mask (first use)
        self._goal_pool_m = 0          # rows of the goal pool set through set_goal_pool (0: none)
        self._d_state = None           # save_state / load_state: (device buffer, bytes) of the blob (first use)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            for ptr in self._owned:
                self._lib.rb_free(self._h, ptr)
            self._owned = []
            self._lib.rb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        info = nat.SimInfo()
        nat.check(self._lib.rb_info(self._h, ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in nat.SimInfo._fields_}

    def dispatch(self, entry="step") -> dict:
        """The row of the library's dispatch table the next launch of `entry` ('step', 'env_step', 'fused_rollout') takes on this
        handle: ``{'id': 'ball8/step/env_per_lane/rk4/b256/table/v0', 'kernel': 1, 'block': 256, ...}``."""
        row = nat.DispatchRow()
        nat.check(self._lib.rb_dispatch_current(self._h, nat.ENTRIES[entry] if isinstance(entry, str) else int(entry), ctypes.byref(row)))
        return dict(row.as_dict(), id=row.row_id())

    def specialization(self) -> str:
        """'kernarg', 'table' (MsjRobot's ahead-of-time instances) or 'jit' (hiprtc instances on this robot's constants)."""
        return {0: "kernarg", 1: "table", 2: "jit"}[self._lib.rb_specialization(self._h)]

    def select_kernel(self, kernel: int):
        nat.check(self._lib.rb_select_kernel(self._h, int(kernel)))

    def mirror_info(self) -> dict:
        """The robot's mirror symmetry (``rb_mirror_info``): ``{'plane': 0 (x-z) or 1 (y-z), 'joint_sign': int32 [n_q], 'tendon_image':
        int32 [n_t]}``.  ``NativeError`` for a robot without a mirror plane."""
        plane = ctypes.c_int32(-1)
        sign, image = np.zeros(self.n_q, np.int32), np.zeros(self.n_t, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        nat.check(self._lib.rb_mirror_info(self._h, ctypes.byref(plane), sign.ctypes.data_as(i32p), image.ctypes.data_as(i32p)))
        return {"plane": int(plane.value), "joint_sign": sign, "tendon_image": image}

    def set_stream(self, stream_ptr):
        """``None``: the handle's own stream; ``0``: the device's default (null) stream, which is
        what ``torch.cuda.current_stream().cuda_stream`` is unless another stream was made
        current; otherwise a ``hipStream_t`` value."""
        if stream_ptr is None:
            arg = ctypes.c_void_p(0)
        elif int(stream_ptr) == 0:
            arg = ctypes.c_void_p(nat.STREAM_DEVICE_DEFAULT)
        else:
            arg = ctypes.c_void_p(int(stream_ptr))
        nat.check(self._lib.rb_set_stream(self._h, arg))
        self._stream = stream_ptr

    def synchronize(self):
        nat.check(self._lib.rb_synchronize(self._h))

    # -- host-array interface (numpy in, numpy out) -----------------------
    def _out(self):
        return (np.empty((self.n_envs, self.n_q), np.float32),
                np.empty((self.n_envs, self.n_q), np.float32),
                np.empty(self.n_envs, np.uint8))

    def forward_reset_command(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        nat.check(self._lib.rb_reset(self._h, nat.u8ptr(m)))
        return self.read_state()

    def read_state(self):
        q, qd, f = self._out()
        nat.check(self._lib.rb_read_state(self._h, nat.fptr(q), nat.fptr(qd), nat.u8ptr(f)))
        return q, qd, f.astype(bool)

    def set_state(self, q, qd, feasible=None):
        q = nat.as_f32(q, (self.n_envs, self.n_q), "q")
        qd = nat.as_f32(qd, (self.n_envs, self.n_q), "qd")
        f = None if feasible is None else np.ascontiguousarray(feasible, dtype=np.uint8)
        nat.check(self._lib.rb_set_state(self._h, nat.fptr(q), nat.fptr(qd), nat.u8ptr(f)))

    def forward_step_command(self, actions, act_scale: float = 1.0):
        """actions: [N, n_t] tendon set-points (``act_scale=1``) or raw policy
        actions in [-1, 1] (``act_scale`` = the robot's set-point bound)."""
        a = nat.as_f32(actions, (self.n_envs, self.n_t), "actions")
        q, qd, f = self._out()
        nat.check(self._lib.rb_step(self._h, nat.fptr(a), float(act_scale),
                                    nat.fptr(q), nat.fptr(qd), nat.u8ptr(f)))
        return q, qd, f.astype(bool)

    def tendon_state(self, set_points=None, act_scale: float = 1.0):
        """Per-tendon state of every env at the current state: ``{'length', 'rate', 'activation', 'force'}``, each ``[N, n_t]``
        float32 (m, m/s with > 0 lengthening, [0, 1], N).  ``set_points`` ``[N, n_t]`` are read as ``forward_step_command``
        reads its actions (set-point = ``act_scale * set_points``); ``None`` = all set-points 0.  Activation and force are what
        the next step's first acceleration evaluation would use with these set-points; the state is not modified.
        A numpy array (or None) gives numpy arrays (synchronous); a CUDA ``torch.Tensor`` gives tensors on its device,
        computed on torch's current stream without a host copy."""
        return self._tendon_state(set_points, nat.RB_SP_SCALED, act_scale)

    def _tendon_state(self, act, sp_mode, act_scale, torch_device=None):
        if _is_cuda_tensor(act) or (act is None and torch_device is not None):
            return self._tendon_state_torch(act, sp_mode, act_scale, torch_device)
        a = None if act is None else nat.as_f32(act, (self.n_envs, self.n_t), "set_points")
        out = {k: np.empty((self.n_envs, self.n_t), np.float32) for k in TENDON_STATE_KEYS}
        nat.check(self._lib.rb_tendon_state(self._h, None if a is None else nat.fptr(a), int(sp_mode), float(act_scale),
                                            *[nat.fptr(out[k]) for k in TENDON_STATE_KEYS]))
        return out

    def _tendon_state_torch(self, act, sp_mode, act_scale, device=None):
        import torch
        if act is not None:
            if act.dtype != torch.float32 or tuple(act.shape) != (self.n_envs, self.n_t) or not act.is_contiguous():
                raise ValueError("set_points must be a contiguous float32 CUDA tensor of shape (%d, %d)" % (self.n_envs, self.n_t))
            device = act.device
        # torch's current stream: ordered behind the kernels that produced the set-points, no host sync
        stream = torch.cuda.current_stream(device).cuda_stream
        if stream != self._stream:
            self.set_stream(stream)
        out = {k: torch.empty((self.n_envs, self.n_t), dtype=torch.float32, device=device) for k in TENDON_STATE_KEYS}
        self.tendon_state_dev(0 if act is None else act.data_ptr(), sp_mode, act_scale,
                              *[out[k].data_ptr() for k in TENDON_STATE_KEYS])
        return out

    def get_new_goal_joint_angles(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        goals = np.empty((self.n_envs, self.n_q), np.float32)
        nat.check(self._lib.rb_sample_goals(self._h, nat.u8ptr(m), nat.fptr(goals)))
        return goals

    # -- per-env physical parameters (rb_params_*; ball-joint robots) -----
    def enable_params(self) -> int:
        """Give every env its own force scales, set-point offsets, mass scale and damping scales, all nominal; returns P.  The step
        and env-step entries then launch the parameter kernels.  Calling it again resets planes, draw counters and ranges."""
        p = ctypes.c_int32()
        nat.check(self._lib.rb_params_enable(self._h, ctypes.byref(p)))
        self.n_params = int(p.value)
        return self.n_params

    def disable_params(self):
        nat.check(self._lib.rb_params_disable(self._h))
        self.n_params = 0

    def params_ptr(self):
        """(device planes [P][N] float32, device draw counters [N] uint32)"""
        d_p, d_d = ctypes.c_void_p(), ctypes.c_void_p()
        nat.check(self._lib.rb_params_ptr(self._h, ctypes.byref(d_p), ctypes.byref(d_d)))
        return d_p.value, d_d.value

    def get_param_planes(self) -> np.ndarray:
        d_p, _ = self.params_ptr()
        return self.download(d_p, (self.n_params, self.n_envs))

    def get_param_draws(self) -> np.ndarray:
        _, d_d = self.params_ptr()
        return self.download(d_d, (self.n_envs,), np.uint32)

    def get_params(self) -> dict:
        """{'force_scale': [N, n_t], 'setpoint_offset': [N, n_t], 'mass_scale': [N], 'damping_scale': [N, 3]} (numpy)"""
        return envparams.planes_to_dict(self.get_param_planes(), self.n_t)

    def set_params(self, **partial):
        """Overwrite some parameters of every env: ``set_params(mass_scale=m[N], force_scale=f[N, n_t])``; a scalar or a per-tendon /
        per-joint row broadcasts over the envs."""
        unknown = set(partial) - set(envparams.NAMES)
        if unknown:
            raise ValueError("unknown parameter(s): %s" % sorted(unknown))
        planes = self.get_param_planes()
        sl, w = envparams.plane_slices(self.n_t), envparams.widths(self.n_t)
        for name, v in partial.items():
            v = np.asarray(v, dtype=np.float32)
            if name == "mass_scale" and v.ndim == 1:
                v = v[:, None]                    # [N] -> [N, 1]
            v = np.broadcast_to(v, (self.n_envs, w[name]))
            planes[sl[name]] = v.T
        d_p, _ = self.params_ptr()
        self.upload(d_p, np.ascontiguousarray(planes))

    def set_param_ranges(self, ranges, resample_on_reset: bool = True):
        """``ranges``: an ``envs.params.ParamRanges``; ``resample_on_reset``: the fused env step redraws an env's parameters when it
        auto-resets."""
        lo, hi = ranges.to_arrays(self.n_t)
        nat.check(self._lib.rb_params_set_ranges(self._h, nat.fptr(lo), nat.fptr(hi), int(bool(resample_on_reset))))

    def sample_params(self, mask=None):
        """Redraw the parameters of the masked envs (``mask`` [N] bool, None = all) from the ranges; synchronous."""
        if mask is None:
            nat.check(self._lib.rb_params_sample_dev(self._h, None))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (self.n_envs,):
                raise ValueError("mask must have shape (%d,)" % self.n_envs)
            if self._d_param_mask is None:
                self._d_param_mask = self.malloc(self.n_envs)
            self.upload(self._d_param_mask, m)
            nat.check(self._lib.rb_params_sample_dev(self._h, ctypes.c_void_p(self._d_param_mask)))
        self.synchronize()

    # -- action latency and sensor noise of the fused env step (rb_env_io_*; ball-joint robots) -----
    def configure_io(self, cfg):
        """``cfg``: a ``_native.EnvIoConfig``, or None to switch the extension off.  Needs the env layer configured; resets the
        delay plane, the counters and the action history."""
        nat.check(self._lib.rb_env_io_configure(self._h, None if cfg is None else ctypes.byref(cfg)))

    def io_ptrs(self) -> dict:
        """device pointers: 'delay', 'delay_draws', 'rows' ([N] uint32 each), 'history' ([slots][N][n_t] float32 or None), 'slots'"""
        p = [ctypes.c_void_p() for _ in range(4)]
        slots = ctypes.c_int32()
        nat.check(self._lib.rb_env_io_ptr(self._h, *[ctypes.byref(x) for x in p], ctypes.byref(slots)))
        return dict(zip(("delay", "delay_draws", "rows", "history"), (x.value for x in p)), slots=int(slots.value))

    def sample_io_delay(self, mask=None):
        """Redraw the action delay of the masked envs (``mask`` [N] bool, None = all) from the configured range; synchronous."""
        if mask is None:
            nat.check(self._lib.rb_env_io_sample_delay_dev(self._h, None))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (self.n_envs,):
                raise ValueError("mask must have shape (%d,)" % self.n_envs)
            if self._d_param_mask is None:
                self._d_param_mask = self.malloc(self.n_envs)
            self.upload(self._d_param_mask, m)
            nat.check(self._lib.rb_env_io_sample_delay_dev(self._h, ctypes.c_void_p(self._d_param_mask)))
        self.synchronize()

    # -- the last K commanded actions as observation columns (rb_env_action_obs_*; ball-joint robots) -----
    def configure_action_obs(self, rows: int):
        """``rows`` = K action rows behind the env step's observation (0 switches them off).  Needs the env layer configured; a
        change of the action history's slot count resets it (and an io configuration's planes and counters)."""
        nat.check(self._lib.rb_env_action_obs_configure(self._h, int(rows)))

    def action_obs_rows(self) -> int:
        rows = ctypes.c_int32()
        nat.check(self._lib.rb_env_action_obs_rows(self._h, ctypes.byref(rows)))
        return int(rows.value)

    # -- device-pointer interface (no host copies) ------------------------
    def state_ptrs(self):
        q, qd, f = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nat.check(self._lib.rb_state_ptrs(self._h, ctypes.byref(q), ctypes.byref(qd), ctypes.byref(f)))
        return q.value, qd.value, f.value

    def malloc(self, nbytes: int) -> int:
        ptr = ctypes.c_void_p()
        nat.check(self._lib.rb_malloc(self._h, int(nbytes), ctypes.byref(ptr)))
        self._owned.append(ptr)
        return ptr.value

    def upload(self, d_ptr: int, array: np.ndarray):
        a = np.ascontiguousarray(array)
        nat.check(self._lib.rb_memcpy_h2d(self._h, ctypes.c_void_p(d_ptr),
                                          a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    def download(self, d_ptr: int, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        nat.check(self._lib.rb_memcpy_d2h(self._h, out.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.c_void_p(d_ptr), out.nbytes))
        return out

    # -- the handle's state as one blob (rb_env_state_*) -----
    def state_segments(self) -> list:
        """The handle's state planes as configured now, in blob order: tuples ``(name, dtype, rows, cols, offset)`` - ``dtype`` a
        numpy type name, ``offset`` the segment's byte offset in the blob."""
        count = ctypes.c_int32()
        nat.check(self._lib.rb_env_state_segments(self._h, None, 0, ctypes.byref(count)))
        segs = (nat.StateSegment * max(count.value, 1))()
        nat.check(self._lib.rb_env_state_segments(self._h, segs, count.value, ctypes.byref(count)))
        return [(s.name.decode("ascii"), nat.STATE_DTYPES[s.dtype], int(s.rows), int(s.cols), int(s.offset)) for s in segs[:count.value]]

    def state_bytes(self) -> int:
        nbytes = ctypes.c_int64()
        nat.check(self._lib.rb_env_state_bytes(self._h, ctypes.byref(nbytes)))
        return int(nbytes.value)

    def _state_blob(self, nbytes: int) -> int:
        """the device buffer a snapshot passes through (kept: a trainer takes one per backup)"""
        if self._d_state is None or self._d_state[1] < nbytes:
            self._d_state = (self.malloc(max(nbytes, 16)), nbytes)
        return self._d_state[0]

    def save_state(self):
        """``(blob, host)``: every state plane of the handle, copied out on its stream behind whatever is in flight there, as one
        ``uint8`` numpy array laid out as ``state_segments()`` says, and the host members ``{"env_steps": float}``."""
        nbytes, host = self.state_bytes(), nat.StateHost()
        d_blob = self._state_blob(nbytes)
        nat.check(self._lib.rb_env_state_save_dev(self._h, ctypes.c_void_p(d_blob), nbytes, ctypes.byref(host)))
        blob, end = self.download(d_blob, (nbytes,), np.uint8), 0
        for _, dtype, rows, cols, offset in self.state_segments() + [("", "uint8", 0, 0, nbytes)]:
            blob[end:offset] = 0           # the padding between segments: the same state gives the same bytes
            end = offset + np.dtype(dtype).itemsize * rows * cols
        return blob, {"env_steps": float(host.env_steps)}

    def load_state(self, blob, host=None):
        """Write every state plane back in place from ``blob`` (``save_state``'s, of a handle configured like this one: the library
        checks the byte count alone, ``ValueError``) and set the host members.  No pointer moves and no graph is dropped."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        if blob.nbytes != self.state_bytes():
            raise ValueError("env state: the handle's state has %d bytes, the blob has %d" % (self.state_bytes(), blob.nbytes))
        d_blob = self._state_blob(blob.nbytes)
        if blob.nbytes:
            self.upload(d_blob, blob)
        h = None
        if host is not None:
            h = nat.StateHost()
            h.env_steps = float(host["env_steps"])
        nat.check(self._lib.rb_env_state_load_dev(self._h, ctypes.c_void_p(d_blob), blob.nbytes, None if h is None else ctypes.byref(h)))

    def step_dev(self, d_act: int, act_scale: float = 1.0):
        nat.check(self._lib.rb_step_dev(self._h, ctypes.c_void_p(d_act), float(act_scale)))

    def tendon_state_dev(self, d_act: int, sp_mode: int, act_scale: float, d_length: int, d_rate: int, d_activation: int,
                         d_force: int):
        """Raw form of ``tendon_state`` (``rb_tendon_state_dev``): device pointers, 0 = NULL (set-points 0 / output not written);
        ``sp_mode`` ``nat.RB_SP_SCALED`` or ``nat.RB_SP_ENV`` (the env layer's rescale; needs ``rb_env_configure``).
        Asynchronous on the handle's stream."""
        nat.check(self._lib.rb_tendon_state_dev(self._h, ctypes.c_void_p(d_act or 0), int(sp_mode), float(act_scale),
                                                *[ctypes.c_void_p(p or 0) for p in (d_length, d_rate, d_activation, d_force)]))

    def range_capable(self, env_layer: bool = False) -> bool:
        """True if this handle's kernel form steps sub-ranges of the batch (``rb_range_capable``): the plain step, or
        (env_layer) the fused env step."""
        return bool(int(self._lib.rb_range_capable(self._h)) & (2 if env_layer else 1))

    def step_range_dev(self, first_env: int, n_envs: int, stream_ptr, d_act: int, act_scale: float = 1.0):
        """Envs [first_env, first_env + n_envs) on the stream ``stream_ptr`` (None / 0: the handle's); ``d_act`` is the WHOLE batch's slab."""
        nat.check(self._lib.rb_step_range_dev(self._h, int(first_env), int(n_envs), ctypes.c_void_p(int(stream_ptr or 0)),
                                              ctypes.c_void_p(d_act), float(act_scale)))

    def rollout_dev(self, d_act_ring: int, ring: int, n_steps: int, act_scale: float = 1.0,
                    use_graph: bool = False):
        nat.check(self._lib.rb_rollout_dev(self._h, ctypes.c_void_p(d_act_ring), int(ring),
                                           int(n_steps), float(act_scale), int(bool(use_graph))))

    def rollout_chains(self) -> int:
        """1: rollout_dev's graphs launch once per step over the whole batch; 2: the two halves step as two independent chains."""
        return int(self._lib.rb_rollout_chains(self._h))

    def set_rollout_chains(self, chains: int):
        """0: the library's choice; 1..4: that many chains of launches per step in graph rollouts (``rb_set_rollout_chains``)."""
        nat.check(self._lib.rb_set_rollout_chains(self._h, int(chains)))

    def rollout_fused_dev(self, d_act_ring: int, ring: int, n_steps: int, act_scale: float = 1.0):
        """Open-loop rollout in one launch (state in registers across the steps)."""
        nat.check(self._lib.rb_rollout_fused_dev(self._h, ctypes.c_void_p(d_act_ring), int(ring),
                                                 int(n_steps), float(act_scale)))

    def fill_actions_dev(self, d_act: int, step: int):
        nat.check(self._lib.rb_fill_actions_dev(self._h, ctypes.c_void_p(d_act), int(step)))

    def sample_goals_dev(self, d_goal: int, d_mask: int = 0):
        nat.check(self._lib.rb_sample_goals_dev(self._h, ctypes.c_void_p(d_mask or 0),
                                                ctypes.c_void_p(d_goal)))

    # -- goal pool (rb_env_goal_pool_*) --------------------
    def set_goal_pool(self, goals):
        """Draw goals from the rows of ``goals`` (an ``envs.goals.GoalPool`` or an array ``[m, n_q]`` inside the robot's joint limits)
        instead of the box: ``get_new_goal_joint_angles`` / ``sample_goals_dev`` then return pool rows.  The first call fixes m; a
        later one replaces the rows in place."""
        from ..goals import goal_rows
        rows = goal_rows(goals, self.n_q, self._desc.q_lo, self._desc.q_hi, m=self._goal_pool_m or None)
        nat.check(self._lib.rb_env_goal_pool_set(self._h, nat.fptr(rows), rows.shape[0]))
        self._goal_pool_m = int(rows.shape[0])

    def goal_pool(self) -> np.ndarray:
        """The pool's rows ``[m, n_q]`` as the device holds them."""
        d_pool, m = ctypes.c_void_p(), ctypes.c_int64()
        nat.check(self._lib.rb_env_goal_pool_ptr(self._h, ctypes.byref(d_pool), ctypes.byref(m)))
        self.synchronize()
        return self.download(d_pool.value, (int(m.value), self.n_q))


class HipSimulationClient(SimulationClient):
    """Single-env ``SimulationClient`` backed by a batch of one on the GPU."""

    def __init__(self, robot: RoboyRobot, process_idx: int = 1, timeout_secs: int = 2,
                 integrator="euler", n_substeps: int = 1, device: int = 0, seed: int = 0, goals=None, goal_curriculum=None):
        # process_idx plays the role it has in the reference (which simulator
        # instance, ros_simulation_client.py:27-30): here, the global env id
        # that keys this env's random streams.  timeout_secs is accepted for
        # signature compatibility; an in-process call cannot time out.
        # goals: an envs.goals.GoalPool or rows [m, n_q] - get_new_goal_joint_angles returns rows of that pool (the reference's
        # simulator hands out FEASIBLE poses, ros_simulation_client.py:73-81), by the rule the vectorised env uses.
        if goal_curriculum is not None:
            raise ValueError("goal_curriculum is an option of the vectorised env (RoboyVecEnv): a single-env client draws goals without "
                             "an episode outcome that could move a level")
        self.robot = robot
        self._timeout_secs = timeout_secs
        self._step_size = 0.1   # ros_simulation_client.py:22
        self._sim = HipBatchSimulation(robot, 1, integrator=integrator, step_size=self._step_size,
                                       n_substeps=n_substeps, device=device, seed=seed,
                                       env_id_offset=int(process_idx))
        self._n_t = robot.get_action_space().shape[0]
        if goals is not None:
            try:
                self._sim.set_goal_pool(goals)
            except Exception:
                self._sim.close()
                raise

    def _state(self, q, qd, feasible) -> RobotState:
        # float64 arrays like the reference's (ROS float lists -> np.array)
        return self.robot.new_state(joint_angle=q[0].astype(np.float64),
                                    joint_vel=qd[0].astype(np.float64),
                                    is_feasible=bool(feasible[0]))

    def read_state(self) -> RobotState:
        return self._state(*self._sim.read_state())

    def forward_step_command(self, action) -> RobotState:
        action = np.asarray(action, dtype=np.float32)
        if action.shape != (self._n_t,):
            raise TypeError("action must be a sequence of %d floats" % self._n_t)
        return self._state(*self._sim.forward_step_command(action[None, :]))

    def forward_reset_command(self) -> RobotState:
        return self._state(*self._sim.forward_reset_command())

    def get_new_goal_joint_angles(self) -> np.ndarray:
        return self._sim.get_new_goal_joint_angles()[0].astype(np.float64)

    def read_tendon_state(self, action=None) -> dict:
        """Per-tendon state of the env (no counterpart in the reference): ``{'length', 'rate', 'activation', 'force'}``, each
        ``[n_t]`` float64, under the set-points ``action`` (as ``forward_step_command`` takes them; None = all 0)."""
        if action is not None:
            action = np.asarray(action, dtype=np.float32)
            if action.shape != (self._n_t,):
                raise TypeError("action must be a sequence of %d floats" % self._n_t)
            action = action[None, :]
        return {k: v[0].astype(np.float64) for k, v in self._sim.tendon_state(action).items()}

    def close(self):
        self._sim.close()


def _is_cuda_tensor(x):
    return x is not None and type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)
