/* roboy_sim.h - C ABI of the MI355X batched tendon-robot physics step.
 *
 * Drop-in boundary for gym-roboy's SimulationClient plugin interface
 * (reference: gym_roboy/envs/simulations/simulation_client.py:6-23).  In the
 * reference every method of that interface is one ROS service round-trip into
 * the external CARDSflow simulator (ros_simulation_client.py:32-81); here each
 * is one in-process call that advances / reads N independent environments
 * whose state lives in HBM.  Plain pointers and sizes only; no torch types.
 *
 *   reference method (file:line)                         entry point here
 *   ---------------------------------------------------  ----------------------
 *   RosSimulationClient.__init__        (ros_..py:16-30)  rb_create
 *   forward_step_command(action)        (ros_..py:48-60)  rb_step / rb_step_dev
 *   forward_reset_command()             (ros_..py:32-38)  rb_reset
 *   read_state()                        (ros_..py:66-71)  rb_read_state
 *   get_new_goal_joint_angles()         (ros_..py:73-81)  rb_sample_goals
 *   _check_service_available_or_timeout (ros_..py:62-64)  return codes + rb_last_error
 *   RoboyEnv.step env layer             (roboy_env.py:51-70,92-134)  rb_env_step_dev
 *   (no counterpart: per-tendon state, the motor boards' readings)         rb_tendon_state_dev
 *
 * Layouts.  Host-facing arrays are row-major [n_envs][n] float32 (what numpy
 * and a policy network produce).  Device state is struct-of-arrays: joint
 * angle plane j is q[j*n_envs .. (j+1)*n_envs), same for velocities, plus one
 * uint32 feasibility word per env.  Device action slabs are row-major
 * [n_envs][n_t] float32 (one 32-byte record per MsjRobot env: two 16-byte
 * loads per lane, contiguous across the wave).
 *
 * Threading: a handle owns one device and one stream; calls on one handle
 * must be serialised by the caller; handles are independent (one process per
 * GPU for the multi-GPU configuration).  All functions return RB_OK (0) or an
 * error code, never abort; rb_last_error() gives the message (thread-local).
 */
#ifndef ROBOY_SIM_H
#define ROBOY_SIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_ABI_VERSION 6

enum rb_status {
    RB_OK = 0,
    RB_EINVAL = 1,       /* bad argument / malformed robot description      */
    RB_EUNSUPPORTED = 2, /* robot structure has no HIP kernel (yet)         */
    RB_EHIP = 3,         /* HIP runtime error (no device, launch failure)   */
    RB_ENOMEM = 4
};

enum rb_integrator { RB_EULER = 0, RB_RK4 = 1 };

/* kernel variants (rb_select_kernel): */
enum rb_kernel {
    RB_KERNEL_AUTO = 0,
    RB_KERNEL_ENV_PER_LANE = 1,    /* one env per lane: throughput form        */
    RB_KERNEL_TENDON_PER_LANE = 2, /* 8 lanes per env + DPP reductions: latency form */
    RB_KERNEL_ENV_PER_WAVE = 3,    /* generic joint-tree robots: a few envs per wave, eight lanes per link, LDS */
    RB_KERNEL_ENV_PER_LANE_SPLIT = 4,/* joint trees, small batches: one env per lane, but several waves per group of 64
                                      envs - one per set of branches of the tree - so that a step waits for a part of
                                      the instruction stream only */
    RB_KERNEL_ENV_PER_LANE_SPLIT2 = 6,/* joint trees, batches between "one workgroup of form 4 per CU" and "a wave on every SIMD"
                                      (the upper body: 16 384 < n <= 32 768 envs): the same code in TWO part waves per 64 envs
                                      with a workgroup lean enough in LDS for two per CU; the library's own choice in that
                                      range for the committed upper body, built by hiprtc on request for other robots */
    RB_KERNEL_LANE_PAIR = 5          /* ball-joint robots with a mirror plane (MsjRobot): two lanes per env - the odd lane
                                      steps the env's mirror image with the same code and constants, four tendons each,
                                      torque sums swapped by DPP: twice the waves of the env-per-lane form for the same
                                      batch, a per-wave instruction chain 0.64x as long */
};

/* Robot description, format "roboy-tendon-robot/1" (Python
 * mirror: gym_roboy_amd/envs/robots/description.py).  All arrays are owned by
 * the caller and only read during rb_create. */
typedef struct rb_robot_desc {
    int32_t n_q;             /* joints = moving links                         */
    int32_t n_t;             /* tendons                                       */
    int32_t n_vp;            /* total via-points                              */
    int32_t _pad;
    const int32_t *parent;   /* [n_q] parent link, -1 = base                  */
    const double *axis;      /* [n_q][3] unit joint axis, parent frame        */
    const double *origin;    /* [n_q][3] joint origin, parent frame           */
    const double *mass;      /* [n_q]                                         */
    const double *com;       /* [n_q][3] centre of mass, link frame           */
    const double *inertia;   /* [n_q][6] xx,yy,zz,xy,xz,yz about COM          */
    const double *armature;  /* [n_q] reflected actuator inertia              */
    const double *damping;   /* [n_q] viscous joint damping                   */
    const double *q_lo;      /* [n_q] feasible region, lower                  */
    const double *q_hi;      /* [n_q] feasible region, upper                  */
    const double *qd_max;    /* [n_q] joint speed limit                       */
    double gravity[3];
    const int32_t *vp_offset;/* [n_t+1] CSR offsets into the via-point arrays */
    const int32_t *vp_link;  /* [n_vp] link of each via-point, -1 = base      */
    const double *vp_pos;    /* [n_vp][3] position in that link's frame       */
    const double *f_max;     /* [n_t] maximum isometric muscle force          */
    double kp, setpoint_scale, v_max, fl_width, kpe, e0, fv_a, fv_n;
} rb_robot_desc;

typedef struct rb_sim rb_sim;

typedef struct rb_sim_info {
    int64_t n_envs;
    int32_t n_q, n_t;
    int32_t integrator, n_substeps;
    int32_t kernel;             /* rb_kernel actually in use                  */
    int32_t device;
    double step_size;
    int64_t bytes_per_env_step; /* algorithmic HBM bytes: 4*(4 n_q + n_t + 1) */
    int64_t env_id_offset;
} rb_sim_info;

/* env-layer configuration for rb_env_* (reference RoboyEnv.__init__ kwargs and
 * constants, roboy_env.py:12-28) */
typedef struct rb_env_config {
    int32_t joint_vel_penalty;      /* roboy_env.py:13                        */
    int32_t goal_bonus;             /* is_agent_getting_bonus_for_reaching_goal */
    int32_t max_episode_length;     /* 400, roboy_env.py:28                   */
    int32_t auto_reset;             /* 1: on done also reset the env, as the
                                       reference's SubprocVecEnv workers do
                                       (train_parallel.py:29); 0: RoboyEnv.step
                                       alone (goal resampled only, :67-68)    */
    float penalty_boundary;         /* 1,    roboy_env.py:26                  */
    float bonus_goal;               /* 1000, roboy_env.py:27                  */
    float angle_lo, angle_hi;       /* joint-angle box (msj_robot.py:9)       */
    float vel_lo, vel_hi;           /* joint-velocity box (msj_robot.py:10)   */
    float action_lo, action_hi;     /* tendon set-point box (msj_robot.py:16) */
    float goal_angle_tol;           /* _MAX_DISTANCE_JOINT_ANGLE / 200 (:127) */
    float goal_vel_tol;             /* _MAX_DISTANCE_JOINT_VELS / 5    (:130) */
} rb_env_config;

const char *rb_last_error(void);
int rb_abi_version(void);
int rb_device_count(int *count);

/* rb_create: build a batch of n_envs environments on `device`.
 * env_id_offset shards one logical batch over several handles/GPUs: all
 * counter-based random streams are keyed by (seed, env_id_offset + i), so
 * results do not depend on how the batch is split.
 * The robot decides the kernels: one body on an x-y-z ball joint with 8 tendons
 * (MsjRobot) gets the specialised closed-form kernels; the same class with 1..16
 * tendons the closed form with a run-time tendon count (env-per-lane only); any
 * other joint tree (up to 32 joints / 64 tendons) the joint-tree kernels (articulated-body
 * algorithm): one env per lane running code generated for the robot (the committed upper
 * body ahead of time - with a several-waves-per-env-group form for small batches - any
 * other robot through hiprtc) or, without such code, octets of lanes per link. */
int rb_create(const rb_robot_desc *robot, int64_t n_envs, int integrator,
              double step_size, int n_substeps, int device, uint64_t seed,
              int64_t env_id_offset, rb_sim **out);
void rb_destroy(rb_sim *sim);
int rb_info(const rb_sim *sim, rb_sim_info *info);
/* rb_select_kernel: pin the kernel form (RB_KERNEL_*), or hand the choice back to the library (RB_KERNEL_AUTO, the default).
 * What is bit-equal to what: every form evaluates the same model (each passes the same parity tests against the fp64 oracle,
 * 2e-5), but the forms order their floating-point sums differently, so results are BIT-identical only within one form -
 *   - across batch splits (env_id_offset shards, sub-ranges, rollout chains): bit-identical as long as every piece runs the
 *     same form.  RB_KERNEL_AUTO chooses by the HANDLE's batch size (ball joints with a mirror plane: eight lanes per env up to
 *     4 096 / 12 288 envs for Euler / RK4, two lanes per env up to 16 384 / 32 768, one env per lane above), so shards on either
 *     side of a threshold agree to ~1 ulp per step, not bit for bit: pin the form (the same rb_select_kernel on every
 *     handle) where bit equality across shard sizes is wanted;
 *   - rb_env_step_dev against rb_step_dev + the reference's env arithmetic: bit-identical states when the handle's form is
 *     pinned to 1, 2 or 5.  Under RB_KERNEL_AUTO the env layer chooses by its own thresholds: eight lanes per env up to 8 192 envs,
 *     two lanes per env up to 24 576 / 32 768 envs (robots with a mirror plane), one env per lane otherwise;
 *   - the env-per-lane form itself has two instances by the handle's batch size: up to 65 536 envs (64-thread workgroups,
 *     tendon loop written out) and above (256-thread workgroups; RK4: the stages as a rolled loop over running sums) - equal to
 *     ~1 ulp, bit-identical only among handles on the same side of 65 536 envs. */
int rb_select_kernel(rb_sim *sim, int kernel);
/* The robot's mirror symmetry, as rb_create found it in the robot's constants (the two-lanes-per-env kernels step "the env's mirror
 * image" by it; a learner can use it to double its data: DESIGN.md §25).  Seen in the mirror the robot is the same robot in the state
 * (joint_sign * q, joint_sign * qd) with the set-points of tendon k and tendon tendon_image[k] exchanged.
 *   plane         0: the x-z plane, 1: the y-z plane (as rb_dispatch_row.variant numbers them)
 *   joint_sign    [n_q = 3]: (-1, +1, -1) for plane 0, (+1, -1, -1) for plane 1 - the joints whose axes lie in the plane change sign
 *   tendon_image  [n_t = 8]: the partner of every tendon, an involution without fixed points
 * Whatever kernel form is selected.  RB_EUNSUPPORTED for a robot without a mirror plane: every joint tree, every other tendon count,
 * asymmetric ball-joint robots.  Added by name: the ABI version stays 6. */
int rb_mirror_info(const rb_sim *sim, int32_t *plane, int32_t *joint_sign /* [n_q] */, int32_t *tendon_image /* [n_t] */);
/* How the env-per-lane kernels of this handle get the robot's constants: RB_SPEC_NONE = through the kernarg
 * (scalar loads); RB_SPEC_TABLE = instances compiled ahead of time on the reference's MsjRobot (the handle's
 * constants equal that table bit for bit); RB_SPEC_JIT = instances compiled with hiprtc on this robot's own
 * constants (8-tendon ball-joint robots, batches above 65 536 envs; built by the first call that needs them, or
 * by this one; ROBOY_SIM_JIT=0 disables it).  All three are the same source and pass the same parity tests;
 * the specialised ones run ~6 % faster.  Returns -1 for a null handle; after RB_SPEC_NONE rb_last_error() says why. */
enum { RB_SPEC_NONE = 0, RB_SPEC_TABLE = 1, RB_SPEC_JIT = 2 };
int rb_specialization(rb_sim *sim);
/* The code objects hiprtc builds are kept on disk (ROBOY_SIM_JIT_CACHE = a directory; default $XDG_CACHE_HOME/gym_roboy_amd or
 * ~/.cache/gym_roboy_amd; "0" = no cache), keyed by source text (robot constants included), architecture and library build:
 * a second process on the same robot loads in milliseconds what took hiprtc 1-80 s.  Process-wide counts since load:
 * hits = builds served from the cache, compiles = hiprtc compilations, stores = files written.  Any pointer may be NULL. */
void rb_jit_cache_stats(int64_t *hits, int64_t *compiles, int64_t *stores);
/* The stream every launch, copy and synchronisation of this handle uses.  NULL = the
 * handle's own (non-blocking) stream; RB_STREAM_DEVICE_DEFAULT = the device's default
 * (null) stream, which is what a framework's "current stream" is unless the caller made
 * another one current (its handle is 0 and cannot be told from NULL, hence the
 * sentinel); anything else = that hipStream_t.  Drains the previous stream first. */
#define RB_STREAM_DEVICE_DEFAULT ((void *)(intptr_t)-1)
int rb_set_stream(rb_sim *sim, void *hip_stream);
int rb_synchronize(rb_sim *sim);

/* ---- host-buffer entry points (synchronous; plumbing, not the hot loop) ---- */
int rb_reset(rb_sim *sim, const uint8_t *mask /* [n_envs] or NULL = all */);
int rb_set_state(rb_sim *sim, const float *q, const float *qd,
                 const uint8_t *feasible /* NULL = all feasible */);
int rb_read_state(rb_sim *sim, float *q, float *qd, uint8_t *feasible);
/* set-point = act_scale * act; act_scale = 1 when the caller has already
 * rescaled to the robot's set-point box (roboy_env.py:54-57) */
int rb_step(rb_sim *sim, const float *act, float act_scale,
            float *q, float *qd, uint8_t *feasible);
int rb_sample_goals(rb_sim *sim, const uint8_t *mask, float *goal_q);

/* ---- device-pointer entry points (asynchronous on the handle's stream) ---- */
/* The library's own state buffers, in place.  Layout by kernel class: ball-joint robots keep SoA planes
 * q[n_q][n_envs], qd[n_q][n_envs] (one env per lane reads a plane element each); joint-tree robots keep
 * env-major rows q[n_envs][n_q], qd[n_envs][n_q] (a wave owns a few whole envs).  feasible[n_envs] either way. */
int rb_state_ptrs(rb_sim *sim, float **d_q, float **d_qd, uint32_t **d_feasible);
int rb_step_dev(rb_sim *sim, const float *d_act, float act_scale);
/* n_steps steps, one kernel boundary per step; step t reads slab (t % ring) of d_act_ring
 * ([ring][n_envs][n_t]).  use_graph != 0 replays the launches from captured hipGraphs -
 * for large batches as rb_rollout_chains() independent chains, i.e. one launch per step
 * and HALF of the batch (below); use_graph = 0 launches once per step over the whole batch. */
int rb_rollout_dev(rb_sim *sim, const float *d_act_ring, int ring, int n_steps,
                   float act_scale, int use_graph);
/* How rb_rollout_dev (use_graph = 1) steps this handle: 1 = one launch over the whole batch per step; 2 = the two halves of the batch
 * as two independent chains of launches, each a linear graph on its own stream (large batches - ball joints from 98 304 envs RK4 /
 * 262 144 envs Euler, the one-wave joint-tree form from 32 768 / 65 536: one half's launch gaps and load / store phases lie under the
 * other half's arithmetic - MsjRobot RK4 at 262 144 envs 16.6 -> 13.0 us per step; envs are independent, the results are the same
 * bit for bit; ROBOY_SIM_CHAINS=1 switches it off, 2-4 force a count).  Eager rollouts (use_graph = 0) and rb_step_dev launch once. */
int rb_rollout_chains(rb_sim *sim);
/* 0 = the library's choice (above), 1..4 = that many chains for the kernel forms that can be stepped in sub-ranges (others keep 1):
 * what bench.py uses to time the one-launch-per-step form beside the default one. */
int rb_set_rollout_chains(rb_sim *sim, int chains);
/* Open-loop rollout fused into ONE launch: every env advances n_steps steps, the
 * state stays in registers in between and only the action of each step is read
 * (slab t % ring of d_act_ring).  For action sequences that are known up front
 * (random-action rollouts, sampling-based planning); NOT the per-step contract of
 * rb_step_dev / rb_rollout_dev (no policy can sit between steps), so bench.py
 * reports it separately and never as the headline.  Bit-identical to n_steps
 * calls of rb_step_dev with the env-per-lane kernel form selected (the
 * tendon-per-lane form RB_KERNEL_AUTO picks for small batches sums the tendon
 * torques in another order: same result to ~1e-6).  Ball-joint robots only. */
int rb_rollout_fused_dev(rb_sim *sim, const float *d_act_ring, int ring, int n_steps, float act_scale);
/* synthetic i.i.d. U[-1,1) actions: Philox4x32-10, key = seed,
 * counter = (env id, step, stream 0) */
int rb_fill_actions_dev(rb_sim *sim, float *d_act, uint32_t step);
int rb_sample_goals_dev(rb_sim *sim, const uint8_t *d_mask, float *d_goal_q /* [n_q][n_envs] */);

/* ---- fused env layer (next row of the scope table) ---- */
int rb_env_configure(rb_sim *sim, const rb_env_config *cfg);
int rb_env_reset_dev(rb_sim *sim, float *d_obs /* [n_envs][3 n_q] */);
/* Host-buffer entry (synchronous): overwrite every env's goal ([n_envs][n_q]) and,
 * if step_num is not NULL, its episode step counter - what assigning
 * RoboyEnv._goal_state / .step_num does in the reference's own tests
 * (gym_roboy/envs/tests/test_roboy_env.py:62-66,172-176); lets a caller replay recorded
 * (state, goal, counter) triples through rb_env_step_dev. */
int rb_env_set_goal(rb_sim *sim, const float *goal_q, const uint32_t *step_num /* [n_envs] or NULL */);
/* Actions: the reference asserts that an action lies in [-1, 1] (roboy_env.py:52); a batched kernel cannot raise, so every kernel
 * form of the fused env step clamps every non-NaN action to [-1, 1] itself before rescaling it into the set-point box of
 * rb_env_configure, +-inf included: an action outside the box gives, bit for bit, what its clipped value gives (a policy's raw
 * Gaussian samples may be handed in as they are; tests/test_action_box_gpu.py pins this for every form).  NaN is the caller's to
 * avoid: what a NaN action does is not specified. */
int rb_env_step_dev(rb_sim *sim, const float *d_act /* [n_envs][n_t], clamped to [-1,1] */,
                    float *d_obs, float *d_reward, uint32_t *d_done);
/* ---- sub-ranges: envs [first_env, first_env + n_envs) on a stream of the caller's choice ----
 * The per-step entry points above launch ONCE per step over the whole batch - which, for a large batch, leaves the launch
 * gap and the load / store phases of a single generation of waves uncovered (rb_rollout_dev's chains exist for that).  A
 * closed-loop caller gets the same overlap by running its loop as two independent chains over the two halves of the batch
 * on two streams - its policy kernel and this step per half (gym_roboy_amd/ppo.py does: the reference's consumer,
 * train_parallel.py:28-35) - forked and joined by the caller, once per rollout.  (Forking and joining inside every step
 * call does not pay: a join costs ~8 us on this stack, profiles/r4_a/region_timeline.log.)  Envs are independent, so
 * disjoint ranges may run concurrently and the results do not depend on the split.  The array arguments are those of the
 * WHOLE batch (the library applies the offsets); first_env is a multiple of 256; hip_stream NULL = the handle's stream.
 * rb_range_capable(): bit 0 = rb_step_range_dev takes sub-ranges with the handle's kernel form (ball joints with 8 tendons
 * except the tendon-per-lane form; joint trees in the one-wave-per-64-envs form), bit 1 = rb_env_step_range_dev does (ball
 * joints always; joint trees in that form); a clear bit = whole batches only: a WHOLE batch (first_env = 0, n_envs = all) is taken
 * by every form on the caller's stream, a true sub-range is refused with RB_EUNSUPPORTED.  (The `ranges` field of the dispatch
 * table's rows, below, says the same per kernel instance.)
 * Lifetime: the handle remembers every distinct caller stream it has launched a range on (an event behind the last launch;
 * 8 entries, least recently used reused after a wait), and rb_destroy / rb_select_kernel / rb_set_stream wait for that work
 * like for the handle's own streams - the caller need not join before closing.  The caller's stream may already be
 * destroyed by then (the event is waited for, not the stream).  During a stream CAPTURE of the caller's stream nothing is
 * in flight and nothing is remembered: run-time kernel builds are deferred (a form that has no kernel yet is refused with
 * RB_EUNSUPPORTED rather than built inside the capture), and whoever replays the captured graph keeps the handle alive and
 * its kernel form unchanged while replays are in flight. */
int rb_range_capable(rb_sim *sim);
int rb_step_range_dev(rb_sim *sim, int64_t first_env, int64_t n_envs, void *hip_stream, const float *d_act, float act_scale);
int rb_env_step_range_dev(rb_sim *sim, int64_t first_env, int64_t n_envs, void *hip_stream,
                          const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done);
/* episode statistics summed over this handle's envs since the last reset of
 * the accumulators: [sum episode return, sum return^2, n_episodes, sum episode
 * length, n_goal_reached, n_infeasible_env_steps, n_env_steps, sum reward]
 * (fp64).  [7] is the finished episodes' returns plus the running ones: what an episode that rb_env_reset_dev abandoned in
 * mid-episode had collected is in neither, so [7] is the sum of every reward handed out only while no reset falls inside an
 * episode.  Without rb_env_configure only [5] (envs flagged infeasible at the
 * time of the call) and [6] are non-zero.  The _dev form copies them into caller-owned device memory (e.g. a
 * torch tensor that is then all-reduced over RCCL); the host form synchronises. */
int rb_env_stats(rb_sim *sim, double *stats8, int reset);
int rb_env_stats_dev(rb_sim *sim, double *d_stats8, int reset);

/* ---- tendon state readout (ABI 6) ----
 * Length, length rate, activation and force of every tendon of every env: the quantities the step computes and consumes
 * internally, at the handle's CURRENT state under the given set-points; the state is not modified.  Outputs are row-major
 * [n_envs][n_t] float32; any output pointer may be NULL (not written).  d_act NULL = all set-points 0 (either mode).
 *   length     m, the whole tendon (every segment, the ones that do not move included)
 *   rate       dl/dt in m/s, > 0 lengthening
 *   activation in [0, 1]
 *   force      N, >= 0: the Hill-type force of DESIGN.md §2, i.e. the force the next step's first acceleration
 *              evaluation would apply with these set-points
 * The set-points are formed as the step forms them: RB_SP_SCALED as the plain step does (set-point = act_scale * act,
 * act_scale > 0), RB_SP_ENV as the fused env layer does (act in [-1, 1] rescaled into the action box of rb_env_configure,
 * which must have been called).  Pointers 16-byte aligned.  These kernels are NOT rows of the dispatch table below, which keys
 * the three step entry kinds only (like rb_sample_goals_dev and rb_fill_actions_dev): one kernel per robot class, whichever
 * step form the handle uses.  The device form is asynchronous on the handle's stream; the host form takes host arrays and
 * synchronises. */
enum rb_setpoint_mode {
    RB_SP_SCALED = 0,   /* set-point = act_scale * act (the plain step's convention)                                          */
    RB_SP_ENV = 1       /* the env layer's rescale into the action box (needs rb_env_configure): non-NaN act clamped to [-1, 1] */
};
int rb_tendon_state_dev(rb_sim *sim, const float *d_act, int sp_mode, float act_scale,
                        float *d_length, float *d_rate, float *d_activation, float *d_force);
int rb_tendon_state(rb_sim *sim, const float *act, int sp_mode, float act_scale,
                    float *length, float *rate, float *activation, float *force);

/* ---- per-env parameters (ABI 6, additive) ----
 * Ball-joint robots (1..16 tendons) only; a joint tree is refused with RB_EUNSUPPORTED.  Per env, fp32, struct-of-arrays planes
 * [P][n_envs] with P = 2 n_t + 4, in this order:
 *   planes 0 .. n_t-1          force_scale[k]      multiplies tendon k's f_max (the passive term too: F = f_max (a f_L f_V + f_PE))   nominal 1
 *   planes n_t .. 2 n_t-1      setpoint_offset[k]  m, added to tendon k's set-point after the step's own rescale                    nominal 0
 *   plane  2 n_t               mass_scale          multiplies every link's mass and inertia (I_O and m c; not the armature)           nominal 1
 *   planes 2 n_t+1 .. 2 n_t+3  damping_scale[j]    multiplies joint j's viscous damping                                               nominal 1
 * Env i with parameters p steps like the robot whose description has f_max[k] *= force_scale[k], every link's mass and inertia
 * *= mass_scale, damping[j] *= damping_scale[j], on the set-points sp + setpoint_offset.
 * While enabled, the step entries (rb_step, rb_step_dev, rb_step_range_dev, rb_rollout_dev) and the env-step entries
 * (rb_env_step_dev, rb_env_step_range_dev) launch the parameter kernels, one env per lane, whatever rb_select_kernel chose; the
 * fused rollout, the tendon-state readout and rb_dispatch_current are refused with RB_EUNSUPPORTED.  Enabling and disabling evict the
 * handle's cached rollout graphs.
 * Redraws: Philox4x32-10 stream 3.  Draw d of the env with global id g takes, for block b = 0 .. ceil(P/4)-1, the words of the
 * generator at counter (g low, g high, d, 3 << 8 | b) and key (seed low, seed high); parameter p takes word p mod 4 of block p / 4
 * and becomes lo_p + (hi_p - lo_p) * u01(word) with two roundings.  d is the env's draw counter, which each draw advances by one;
 * the values do not depend on how the batch is sharded (env_id_offset).  The fused env step redraws an env's parameters on done
 * with auto_reset when the ranges were set with resample_on_reset, where it redraws the goal: the step that ended the episode used
 * the old parameters, the first step of the new episode uses the new ones.
 *   enable:      allocates the planes and a uint32 draw-counter plane [n_envs], fills them with the nominal values and zero counts,
 *                sets the ranges to lo = hi = nominal without redraw on reset; writes P to *n_params unless NULL.  Calling it
 *                again resets planes, counters and ranges.
 *   disable:     frees them; the handle steps with its usual kernels again.
 *   ptr:         the device planes and counters (the caller may write the planes; asynchronous users order on the handle's stream).
 *   set_ranges:  host arrays lo[P], hi[P]; RB_EINVAL for a bound that is not finite, lo > hi, a mass_scale lo <= 0, a force_scale
 *                or damping_scale lo < 0.
 *   sample_dev:  redraws the envs with d_mask[i] != 0 (d_mask: device [n_envs], NULL = all), asynchronous on the handle's stream. */
int rb_params_enable(rb_sim *sim, int32_t *n_params);
int rb_params_disable(rb_sim *sim);
int rb_params_ptr(rb_sim *sim, float **d_params, uint32_t **d_draws);
int rb_params_set_ranges(rb_sim *sim, const float *lo, const float *hi, int resample_on_reset);
int rb_params_sample_dev(rb_sim *sim, const uint8_t *d_mask);

/* ---- tendon channels in the fused env step's observation (ABI 6, additive) ----
 * Ball-joint robots (1..16 tendons) only; a joint tree is refused with RB_EUNSUPPORTED.  With a channel mask set, the rows that
 * rb_env_step_dev, rb_env_step_range_dev and rb_env_reset_dev write are
 *   [q (n_q), qd (n_q), goal (n_q), then per selected channel in the order length, rate, activation, force: n_t values],
 * obs_dim = 3 n_q + C n_t floats (C = the number of selected channels; MsjRobot with length and force: 25), row stride obs_dim: the
 * caller's observation array holds n_envs * obs_dim floats, and rb_env_step_range_dev applies first_env * obs_dim to it.  The first
 * 3 n_q columns and every other output of the step are what they are without the mask.
 * The tendon columns are the quantities of the tendon state readout above (m, m/s, [0, 1], N) at the state the row reports, under
 * the set-points the step has just applied, held, and - on a handle with per-env parameters - under the parameters the env's NEXT
 * step will use: what that step's first acceleration evaluation sees if the action is repeated.  On a handle without parameters
 * that is what rb_tendon_state_dev returns behind the step for the same actions under RB_SP_ENV; an env that was done and
 * auto-reset reports the zero pose under the last actions, with resample_on_reset under its REDRAWN parameters.  rb_env_reset_dev
 * writes the columns of the zero pose with every set-point 0 (plus the env's set-point offset, on a handle with parameters).
 * Each channel is multiplied by its scale (scale[4] in channel order, NULL = ones; one rounded fp32 multiply, no shift).
 * While a mask is set, the env-step entries launch the extended kernels (csrc/env_obs.hpp), one env per lane in the nominal or the
 * parameter form, whatever rb_select_kernel chose, and rb_dispatch_current refuses RB_ENTRY_ENV_STEP with RB_EUNSUPPORTED; the
 * step entries are untouched.
 *   configure: needs rb_env_configure; mask 0 switches the extension off (the handle's own kernels again); evicts the cached
 *              rollout graphs; RB_EINVAL for unknown bits and for a scale that is not finite.
 *   obs_dim:   the row width of the handle as configured (3 n_q without a mask).
 *   obs_count: 3 n_q + popcount(mask) n_t, without a handle or a device; -1 for unknown bits or negative counts.
 * RB_ABI_VERSION is still 6 (nothing that existed changed), so the number does not tell a consumer whether these three functions
 * are there: look the symbol up (dlsym of the configure function) before relying on them. */
enum rb_obs_channel {
    RB_OBS_LENGTH = 1,
    RB_OBS_RATE = 2,
    RB_OBS_ACTIVATION = 4,
    RB_OBS_FORCE = 8,
    RB_OBS_ALL = 15
};
int rb_env_obs_configure(rb_sim *sim, uint32_t channel_mask, const float *scale);
int rb_env_obs_dim(rb_sim *sim, int32_t *obs_dim);
int32_t rb_env_obs_count(int32_t n_q, int32_t n_t, uint32_t channel_mask);

/* ---- per-env action latency and sensor noise in the fused env step (ABI 6, additive) ----
 * Ball-joint robots (1..16 tendons) only; a joint tree is refused with RB_EUNSUPPORTED.  Opt-in per handle; composes with per-env
 * parameters and with tendon channels (either, both or neither, a channel mask of 0 included).
 * Latency.  Env i has an integer delay d_i in [0, RB_IO_MAX_DELAY], a uint32 plane [n_envs] the caller may read and write.  With k the
 * episode step a launch computes (the env's step counter on entry: 1 behind a reset or an auto-reset), the step is driven by the action row the caller passed at
 * episode step k - d_i of the same episode, clamped and rescaled like a direct one; while k - d_i < 1 by the rest command: every
 * set-point 0 m, plus the env's set-point offset on a handle with parameters - what the env-reset rows' tendon columns assume.
 * Everything behind the step sees the command that was applied: the tendon columns ("the set-points just applied, held") and the
 * parameter form's columns of an auto-reset env.  The rows are kept in a device ring history[S][n_envs][n_t] of raw action rows,
 * S the smallest power of two above delay_hi; every step stores the row it was handed into slot k mod S, an env with 0 < d_i < k
 * reads slot (k - d_i) mod S.  No ring exists and the delay plane is not read with delay_hi = 0.  An auto-reset clears nothing (k
 * restarts at 1); without auto_reset the counter and the history run on.  The ring is indexed by the step counter: a caller that
 * rewrites the counters (the step_num argument of the set-goal call) steps with whatever those slots hold.  A delay written into
 * the plane by hand must not exceed delay_hi.
 * Delay draws: Philox4x32-10 stream 5.  Draw m of the env with global id g is word 0 of the generator at counter (g low, g high, m,
 * 5 << 8) and key (seed low, seed high): d = delay_lo + (((word >> 8) * (delay_hi - delay_lo + 1)) >> 24), in integers.  m is the
 * env's own draw counter (a uint32 plane), advanced by one per draw; independent of sharding (env_id_offset).  configure draws every
 * env once.  With resample_on_reset the fused env step redraws d_i on done with auto_reset, where the goal and the parameters are
 * redrawn: the episode that ended used the old delay, the new episode uses the new one.
 * Sensor noise.  Standard deviations in physical units, finite and >= 0: sigma_q (the n_q angle columns), sigma_qd (the n_q
 * velocity columns), sigma_tendon[4] per tendon channel in channel order (m, m/s, activation, N); the goal columns are never
 * noised.  A noised column reports (value + sigma z) x its channel scale, evaluated as one fused multiply-add on the scaled value.
 * Reward, done, state, statistics, goal and parameter redraws use the true state: with noise on and off they are bit-identical.
 * Row number r of the env with global id g takes for the column at row position c (0 .. obs_dim-1, goal columns counted) component
 * c & 3 of block c >> 2 of the generator at counter (g low, g high, r, 4 << 8 | block), Box-Muller on the pairs (0,1) and (2,3):
 * u1 = ((w >> 8) + 1) / 2^24, u2 = (w >> 8) / 2^24, z = sqrt(-2 ln u1) cos(2 pi u2) for the even component, sin for the odd.
 * r is a per-env uint32 row counter, zeroed by configure and advanced by one for every row the env-step or the env-reset entry
 * writes for that env while any sigma is set (an auto-reset row is still one row per step).  The env-reset rows are noised too.
 * Nothing is clipped to an observation box.
 * While configured, the env-step entries (step, step-range, reset) run the io kernels (csrc/env_io.hpp), one env per lane in the
 * nominal or the parameter form, whatever rb_select_kernel chose, and rb_dispatch_current refuses RB_ENTRY_ENV_STEP with
 * RB_EUNSUPPORTED; the plain step entries are untouched.  A sub-range shifts the history by first_env n_t inside each slot (slot
 * stride n_envs n_t floats) and the three planes by first_env.
 *   configure:        needs rb_env_configure; drains the handle's streams and evicts the cached rollout graphs; calling it again
 *                     resets planes, counters and ring; NULL switches it off (buffers freed, the handle's previous kernels again).
 *                     RB_EINVAL for a negative or non-finite sigma or a delay range outside 0 <= lo <= hi <= RB_IO_MAX_DELAY.
 *   ptr:              the device planes (delay, delay draw counters, row counters), the ring (NULL without one) and its slot
 *                     count S (0 without one); any output may be NULL.  Asynchronous users order on the handle's stream.
 *   sample_delay_dev: redraws the envs with d_mask[i] != 0 (d_mask: device [n_envs], NULL = all), asynchronous on the handle's stream.
 * RB_ABI_VERSION is still 6, for the reason given above: look the configure function up before relying on these three. */
#define RB_IO_MAX_DELAY 7
typedef struct rb_env_io_config {
    float sigma_q, sigma_qd, sigma_tendon[4];
    int32_t delay_lo, delay_hi;          /* 0 <= lo <= hi <= RB_IO_MAX_DELAY */
    int32_t resample_on_reset, _pad;
} rb_env_io_config;
int rb_env_io_configure(rb_sim *sim, const rb_env_io_config *cfg);
int rb_env_io_ptr(rb_sim *sim, uint32_t **d_delay, uint32_t **d_delay_draws, uint32_t **d_rows, float **d_history, int32_t *slots);
int rb_env_io_sample_delay_dev(rb_sim *sim, const uint8_t *d_mask);

/* ---- the last K commanded actions as observation columns of the fused env step (ABI 6, additive) ----
 * Ball-joint robots (1..16 tendons) only; a joint tree is refused with RB_EUNSUPPORTED.  Opt-in per handle; composes with per-env
 * parameters, tendon channels, sensor noise and action latency (any subset, none of them included).  What a memoryless policy
 * needs to compensate a latency: the commands that are still on their way.
 * Row.  With rows = K, 1 <= K <= RB_ACTION_OBS_MAX, the rows that the env-step, env-step-range and env-reset entries write are
 *   [q, qd, goal | the tendon channels as above | K blocks of n_t action columns, the newest block first],
 * obs_dim = 3 n_q + C n_t + K n_t floats, which is what the obs_dim query reports and the stride the range entry applies to
 * first_env.  The first 3 n_q + C n_t columns and every other output of the step (reward, done, codes, state, statistics, goal,
 * parameter and delay redraws, the noise counters) are bit for bit what the same handle gives without the option.
 * Blocks.  With s the env's step counter as the step leaves it (the counter on entry + 1, or 1 behind an auto-reset), block j
 * (0-based) holds, per component, the action row the caller HANDED IN at episode step s - 1 - j of the same episode, clamped to
 * [-1, 1] as the step clamps it: the handed row, not the one a delay applied.  Where s - 1 - j < 1 the block is all 0.0f: the row of
 * an env that was auto-reset carries K zero blocks, so do the env-reset rows, and the first step behind a reset reports the handed
 * row in block 0 and zeros behind it.  Without auto_reset the counter and the history run on, as the delay's do.  The action columns
 * are never noised and never scaled; the noise on the other columns keeps its generator blocks numbered by row position, so it
 * gives the same noised leading columns with and without the option.
 * Ring.  The rows come from the latency's device ring history[S][n_envs][n_t], with S the smallest power of two above
 * max(delay_hi, K - 1) here: it exists whenever K > 0, also without an io configuration, and the io pointer query reports it
 * (and S) then too, with NULL planes.  Every env reads only slots it wrote itself in the running episode; an auto-reset clears
 * nothing.  The ring is indexed by the step counter: a caller that rewrites the counters (the step_num argument of the set-goal
 * call) reads whatever those slots hold.
 * While K > 0 the env-step entries run the history kernels (csrc/env_hist.hpp), one env per lane in the nominal or the parameter
 * form, whatever rb_select_kernel chose, and rb_dispatch_current refuses RB_ENTRY_ENV_STEP with RB_EUNSUPPORTED.
 * "Bit for bit" above therefore holds against a handle that runs the same step text: one with parameters, channels or an io
 * configuration (their kernels are one env per lane too), or - without any of them - one whose env step is its env-per-lane row
 * (RB_KERNEL_ENV_PER_LANE selected).  A bare handle under RB_KERNEL_AUTO may step with another form (octets, lane pairs), which
 * rounds differently: against that the state agrees within the forms' parity tolerance, not to the bit - as for the two
 * extensions above.
 *   configure: needs rb_env_configure; 0 switches the option off (the handle's previous kernels and rows again); drains the
 *              handle's streams and evicts the cached rollout graphs.  Callable before or after the io configure call: whichever
 *              of the two changes S rebuilds the ring, zeroed, and leaves the io planes and counters as a fresh io configuration
 *              does - reset the envs before stepping on.  RB_EINVAL outside 0..RB_ACTION_OBS_MAX, RB_EUNSUPPORTED for a joint tree.
 *   rows:      K as configured (0: off).
 *   count:     3 n_q + popcount(mask) n_t + rows n_t, without a handle or a device; -1 for unknown bits, negative counts or
 *              rows outside 0..RB_ACTION_OBS_MAX.
 * RB_ABI_VERSION is still 6, for the reason given above: look the configure function up before relying on these three. */
#define RB_ACTION_OBS_MAX 8
int rb_env_action_obs_configure(rb_sim *sim, int32_t rows);
int rb_env_action_obs_rows(rb_sim *sim, int32_t *rows);
int32_t rb_env_action_obs_count(int32_t n_q, int32_t n_t, uint32_t channel_mask, int32_t rows);

/* ---- episode-end codes: which episodes ended at the time limit ----
 * The fused env step ends an episode when the goal is reached or when the episode is max_episode_length steps old, and reports
 * both as done = 1.  While enabled, every env-step entry (rb_env_step_dev, rb_env_step_range_dev; every kernel form, both robot
 * classes, every extension) is followed on the same stream, over the same envs, by one small kernel that rewrites the step's done
 * words into codes: RB_DONE_NONE, RB_DONE_TERMINATED (the goal was reached) or RB_DONE_TRUNCATED (the time limit alone ended the
 * episode).  Terminated wins: an env that reaches its goal on its last permitted step reads RB_DONE_TERMINATED.  `done != 0` is
 * exactly the done of a handle without the option; observations, rewards, state and statistics are untouched.  A consumer that
 * bootstraps the value of truncated episodes (rp_rollout_tail_boot_dev in roboy_policy.h) reads the codes from d_done.
 * How: an env reached its goal iff its goal counter (the n_goal_reached term of rb_env_stats) moved since its last episode end;
 * the handle keeps that counter's last seen value per env.  Enabling reads the counters as they stand; rb_env_configure and the
 * reset of rb_env_stats / rb_env_stats_dev, which zero the counters, zero the seen values on the same stream, and rb_env_reset_dev
 * re-reads them.  rb_rollout_fused_dev (the open-loop benchmark entry) reports no codes.
 *   configure: needs rb_env_configure; drains the handle's streams and evicts the cached rollout graphs, so call it before a
 *              caller captures env steps into a graph of its own.  enable = 0 frees the planes: the handle launches exactly what
 *              it launched before.  Off by default.
 *   ptr:       the last step's codes, a device plane [n_envs] (zero until the first step); RB_EINVAL while not enabled.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_done_kind_configure up before relying on it. */
#define RB_DONE_NONE 0
#define RB_DONE_TERMINATED 1
#define RB_DONE_TRUNCATED 2
int rb_env_done_kind_configure(rb_sim *sim, int enable);
int rb_env_done_kind_ptr(rb_sim *sim, uint32_t **d_kind);

/* ---- privileged critic rows: the exact state and the env's hidden parameters, for an asymmetric critic ----
 * §12-§18 make the observation row noisy, late and blind to the env's own parameters on purpose.  A value net that is only trained
 * and never deployed may see what the simulator knows.  While a mask is set, every env-step entry (rb_env_step_dev,
 * rb_env_step_range_dev and the two entries below; every ball-joint kernel form and extension) is followed on the same stream, over
 * the same envs, by one small kernel that writes a second row per env; rb_env_reset_dev is followed by it too.  It reads the planes as
 * the step left them - after any auto-reset and redraw - so the row describes the state, goal, parameters and delay that the returned
 * observation row belongs to.  Blocks, in this order, each present only if its bit is set:
 *   RB_CRITIC_STATE    3 n_q   q, qd, goal from the planes: the observation's first 3 n_q columns without noise.  Always selected:
 *                              a non-zero mask implies it
 *   RB_CRITIC_AGE      1       float(step_num) / float(max_episode_length), one fp32 division (1 / max_len behind a reset)
 *   RB_CRITIC_PARAMS   np      the parameter planes in plane order (rb_params_ptr), unscaled; needs rb_params_enable
 *   RB_CRITIC_DELAY    1       float(delay) (rb_env_io_ptr); needs rb_env_io_configure
 *   RB_CRITIC_ACTIONS  K n_t   a bitwise copy of the observation row's K action blocks (never noised, zeros behind a reset); needs
 *                              rb_env_action_obs_configure(K > 0)
 * Tendon channels are not offered: their exact values are in no plane, and the observation row's copies may be noised.
 * Observations, rewards, done words, state and statistics are those of a handle without the option.  Ball-joint robots; a joint
 * tree is refused with RB_EUNSUPPORTED.
 *   configure: after rb_env_configure and after the options the mask depends on (RB_EINVAL otherwise, and RB_EINVAL for a row wider
 *              than RB_CRITIC_OBS_MAX_DIM, the PPO gradient kernels' input limit).  Drains the handle's streams and evicts the cached
 *              rollout graphs: call it before a caller captures env steps.  mask = 0 frees the plane: the handle launches exactly
 *              what it launched before.  Changing an option the mask depends on afterwards makes the env-step entries fail with
 *              RB_EINVAL until the rows are configured again.
 *   dim:       Dc, the row width (0 while off).  count: the same from the numbers alone, -1 for an unknown bit.
 *   ptr:       the handle's own plane [n_envs][Dc], written by rb_env_step_dev, rb_env_step_range_dev and rb_env_reset_dev;
 *              RB_EINVAL while off.  rb_env_set_goal does not rewrite it.
 *   rb_env_step_critic_dev / rb_env_step_range_critic_dev: the same steps with the rows written to d_cobs ([n_envs][Dc] of the
 *              WHOLE batch; a range writes its own rows) instead of the handle's plane - a captured rollout writes its [t + 1] slice
 *              directly.  Full waves store float4 runs where d_cobs is 16-byte aligned, one row per lane where it is not.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_critic_obs_configure up before relying on it. */
#define RB_CRITIC_STATE 1u
#define RB_CRITIC_AGE 2u
#define RB_CRITIC_PARAMS 4u
#define RB_CRITIC_DELAY 8u
#define RB_CRITIC_ACTIONS 16u
#define RB_CRITIC_ALL 31u
#define RB_CRITIC_OBS_MAX_DIM 63
int rb_env_critic_obs_configure(rb_sim *sim, uint32_t mask);
int rb_env_critic_obs_dim(rb_sim *sim, int32_t *dim);
int32_t rb_env_critic_obs_count(int32_t n_q, int32_t n_t, uint32_t mask, int32_t n_params, int32_t action_rows);
int rb_env_critic_obs_ptr(rb_sim *sim, float **d_rows);
int rb_env_step_critic_dev(rb_sim *sim, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done, float *d_cobs);
int rb_env_step_range_critic_dev(rb_sim *sim, int64_t first_env, int64_t n_envs, void *hip_stream,
                                 const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done, float *d_cobs);

/* ---- goal pool: env goals drawn from a set of poses the robot can hold instead of the goal box ----
 * The reference asks its simulator for a FEASIBLE goal pose (ros_..py:73-81); a goal uniform in a box need not be one the tendons can
 * hold.  While a handle holds a pool of m rows [m][n_q], goal number `draw` of the env with global id gid = env_id_offset + i is row
 *     k = (uint64(w) * uint64(m)) >> 32,   w = word 0 of Philox4x32-10(key = seed, counter = (gid, draw, stream 4 << 8 | 0))
 * of the pool, bit for bit: one multiply-shift and no rejection loop, so a row's probability is off 1 / m by at most 2^-32 (a relative
 * bias of at most m / 2^32).  Keyed by the global env id: goals do not depend on sharding.  `draw` is the env's goal counter, which
 * advances as without a pool (+1 at a reset; at an episode end +1, or +2 with auto_reset, where the row is the one of the second draw).
 * Where it applies:
 *   - every env-step entry, every kernel form, every robot class: one small kernel directly behind the step kernel (same stream, same
 *     envs, in front of the critic rows and the episode-end codes) gives each env that is done its row, in the goal plane and in
 *     columns [2 n_q, 3 n_q) of its observation row - with and without auto_reset.  Envs that are not done are untouched.  Reward,
 *     done and statistics of the step that ended the episode used the old goal, as without a pool;
 *   - rb_env_reset_dev: every env's goal, in the plane and (d_obs != NULL) in the observation row;
 *   - rb_sample_goals and rb_sample_goals_dev: rows of the pool by the same rule, so a single-env client draws what the batched env does.
 * rb_rollout_fused_dev redraws goals inside one kernel and returns RB_EUNSUPPORTED while a pool is set.  rb_env_set_goal still
 * overrides everything.  A handle without a pool launches exactly what it launched before.
 *   set: goal_q is a host array [m][n_q], m >= 1; every value finite and inside the angle box of rb_env_configure (without an env layer:
 *        inside the robot's own box, which rb_sample_goals draws from), else RB_EINVAL before anything is enqueued or changed.  The
 *        first call fixes m for the handle's lifetime and allocates the device copy; a later call with the same m overwrites the rows
 *        IN PLACE - the pointer never moves, so a graph captured earlier reads the new rows on its next replay - and one with another
 *        m is refused with RB_EINVAL.  Drains the handle's streams and copies synchronously: call the first one before a caller
 *        captures env steps, later ones between steps.  The first call on a handle with an env layer also replaces every env's
 *        current goal, drawn from the box, by the pool row of that same draw (counters untouched): from then on every goal of the
 *        handle is a row of the pool.  After a later call, goals already drawn stay until their env draws again.
 *   ptr: the device rows and m; RB_EINVAL while no pool is set.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_goal_pool_set up before relying on it. */
int rb_env_goal_pool_set(rb_sim *sim, const float *goal_q /* host, [m][n_q] */, int64_t m);
int rb_env_goal_pool_ptr(rb_sim *sim, float **d_pool, int64_t *m);

/* ---- goal curriculum: a difficulty level per env over an ORDERED goal pool ----
 * A one-up / one-down staircase per env on top of a goal pool whose rows the caller has ordered from easiest to hardest (the library
 * never sorts: row order is difficulty order).  Every env carries a level l in [0, L).  An env at level l draws from the rows
 *     [0, hi(l)),   hi(l) = uint32((uint64(l + 1) * m) / L)
 * so hi(L - 1) = m, hi(0) >= 1, and the windows are cumulative: easy goals keep occurring.  The draw is the pool's, scaled by the window:
 *     k = (uint64(w) * uint64(hi(l))) >> 32,   w = word 0 of Philox4x32-10(key = seed, counter = (gid, draw, stream 4 << 8 | 0))
 * with draw = goal counter - 1 after the step, as above.  An env at level L - 1 draws exactly the row a handle with the plain pool
 * draws, and L = 1 is the plain pool plus the index plane.
 * An episode end in a step (done word non-zero) decides the outcome first: "reached" iff the env's goals-reached counter (the
 * statistics' n_goal_reached, per env) differs from the value the curriculum saw at the env's last episode end - the rule of the
 * episode-end codes, on a plane of the curriculum's own, so the codes may be off.  Reached: l <- min(l + up, L - 1); not reached:
 * l <- l - min(l, down).  Then the value seen becomes the counter, the row is drawn at the NEW level, its number goes into the index
 * plane and its values into the goal plane and the observation row's goal columns, as the pool writes them.  Envs that are not done
 * are untouched.  One kernel, launched IN PLACE of the pool's behind every env-step launch: the launches per step are a pool handle's.
 *   - rb_env_reset_dev: levels do not move; the value seen becomes every env's counter; every env draws within its window.
 *   - rb_env_configure again and rb_env_stats(_dev) with reset clear the value seen with the counters they clear.
 *   - rb_env_set_goal: the index plane reads RB_GOAL_INDEX_NONE for every env until it draws again.
 *   - rb_env_goal_pool_set in place (same m): levels and indices stay; the new rows must be ordered again, which is the caller's business.
 *   - rb_rollout_fused_dev refuses while a pool is set; rb_sample_goals and rb_sample_goals_dev return RB_EUNSUPPORTED on a handle
 *     with a curriculum (without an env layer there is no outcome to move a level).
 *   configure: needs rb_env_configure and rb_env_goal_pool_set.  1 <= levels <= min(m, RB_GOAL_LEVELS_MAX), up >= 0, down >= 0,
 *        0 <= level0 < levels, else RB_EINVAL before anything is enqueued or changed.  ONCE per handle - the arguments travel by value
 *        in the kernel's argument block and a captured graph freezes them - a second call is RB_EINVAL.  Drains the handle's streams,
 *        allocates the planes (level = level0 everywhere), then redraws every env's goal once by the rule above (draw counters
 *        untouched: they stay those of a handle without a curriculum).  Call it before a caller captures env steps.
 *   level_ptr, index_ptr: the device planes uint32 [n]; RB_EINVAL without a curriculum.
 *   levels_set: host uint32 [n], every value < levels or RB_EINVAL before anything changes; drains the streams, copies, does not redraw.
 *   level_hist_dev: d_out[levels] uint64 = how many envs sit at each level, on `hip_stream` (NULL: the handle's): a memset of d_out
 *        and one kernel, capturable.  level_hist: the same into host memory, synchronous.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_goal_curriculum_configure up before relying on it. */
#define RB_GOAL_LEVELS_MAX 256
#define RB_GOAL_INDEX_NONE 0xFFFFFFFFu
int rb_env_goal_curriculum_configure(rb_sim *sim, int32_t levels, int32_t up, int32_t down, int32_t level0);
int rb_env_goal_level_ptr(rb_sim *sim, uint32_t **d_level);
int rb_env_goal_index_ptr(rb_sim *sim, uint32_t **d_index);
int rb_env_goal_levels_set(rb_sim *sim, const uint32_t *host_levels /* [n] */);
int rb_env_goal_level_hist_dev(rb_sim *sim, uint64_t *d_out /* [levels] */, void *hip_stream);
int rb_env_goal_level_hist(rb_sim *sim, uint64_t *out /* host, [levels] */);

/* ---- outcome counts per pool row, and re-ordering a live pool by them ----
 * The curriculum takes row order for difficulty order; these counts measure it.  Two planes uint64 [2][m] behind one pointer:
 * attempts[m], then reached[m], zero when enabled.  The rule, in an env-step launch (every env-step entry, every kernel form), for an
 * env whose done word is non-zero, BEFORE its level, the value seen and its index are written:
 *     k0  = index[i]                                 (the row the ended episode was aimed at)
 *     hit = goals-reached counter[i] != value seen[i] (the outcome the level rule uses)
 *     k0 < m:  attempts[k0] += 1;  hit: reached[k0] += 1
 * Everything else the env does is the curriculum's contract above, bit for bit.  Nothing is counted for an env whose index reads
 * RB_GOAL_INDEX_NONE (behind rb_env_set_goal), nor by rb_env_reset_dev: the episodes a reset abandons are not attempts.  While
 * enabled, one kernel (the curriculum's lane text plus the adds) is launched IN PLACE of the curriculum's: the launches per step stay
 * a pool handle's.  The adds are global integer atomics whose result is unused: exact in any order, so ranges of one handle stepped
 * on two streams (rb_env_step_range_dev) add into the same planes safely.
 *   - rb_env_configure again, rb_env_stats(_dev) with reset, rb_env_reset_dev, rb_env_goal_levels_set and rb_env_goal_pool_set in
 *     place do nothing to the counts: they are the caller's to clear (read with clear, or set).
 *   - L = 1 ("the plain pool plus the index plane") is the way to count without a staircase; a handle without a curriculum has no
 *     index plane and cannot count.  A handle that does not enable the counts launches exactly what it launched before.
 *   enable: needs rb_env_goal_curriculum_configure, else RB_EINVAL.  ONCE per handle - it switches the kernel a captured graph would
 *        have frozen - a second call is RB_EINVAL.  Drains the handle's streams, then allocates and zeroes the planes.  Call it before
 *        a caller captures env steps.
 *   ptr: the device planes and m.  read: the planes into host memory [2][m], synchronous, behind a drain of the handle's streams;
 *        clear != 0 zeroes them after the copy.  set: host [2][m] into the planes, synchronous, behind a drain; a row with
 *        reached > attempts is RB_EINVAL before anything changes.  All three: RB_EINVAL while the counts are not enabled.
 *   rb_env_goal_pool_permute: new row j of the pool is old row order[j].  Any handle with a pool.  `order` is a host array [m] and must
 *        be a permutation of 0..m-1, else RB_EINVAL before anything is enqueued or changed.  Drains the handle's streams and permutes
 *        the device rows IN PLACE - the pointer never moves, so a graph captured earlier reads the new order on its next replay.  With a
 *        curriculum the index plane is remapped (index <- new number of the row it held; RB_GOAL_INDEX_NONE stays), with counts both
 *        planes are permuted the same way.  Levels, the values seen, the goal planes, the observation rows and every draw counter are
 *        left alone.  Invariant before and after: for every env with an index, pool row index[i] equals the env's goal plane bit for
 *        bit.  Synchronous; call it between steps.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_goal_row_stats_enable up before relying on it. */
int rb_env_goal_row_stats_enable(rb_sim *sim);
int rb_env_goal_row_stats_ptr(rb_sim *sim, uint64_t **d_counts /* [2][m] */, int64_t *m);
int rb_env_goal_row_stats_read(rb_sim *sim, uint64_t *host /* [2][m] */, int clear);
int rb_env_goal_row_stats_set(rb_sim *sim, const uint64_t *host /* [2][m] */);
int rb_env_goal_pool_permute(rb_sim *sim, const uint32_t *order /* host, [m] */);

/* ---- reward shaping: an action-rate term and two effort terms around the fused env step ----
 * Every robot, every kernel form, every env-step entry: no env-step kernel changes; one kernel is launched in front of it and one
 * behind it, on its stream, over its envs.  With weights w_r = action_rate, w_f = tension, w_a = activation (finite, >= 0), the reward
 * an env step returns is
 *     reward[i] = fl32( r_step[i] - cost[i] )                 r_step: the reward of a handle without the option, bit for bit
 *     cost[i]   = w_r c_rate + w_f c_tension + w_a c_activation
 * at the state s_t the env is in BEFORE the step and the action row a_t handed to this step (an auto-reset inside the step does not
 * disturb it):
 *     c_rate       = mean over tendons of (â_k - p_k)^2: â = clamp(a_t, -1, 1) as the step clamps, p = the clamped row of the same
 *                    episode's previous step; 0 on an episode's first step (the step entered with step counter 1, which a reset and an
 *                    auto-reset leave there).  p lives in a plane of its own, [n][n_t].
 *     c_tension    = mean over tendons of (F_k / F_max,k)^2
 *     c_activation = mean over tendons of act_k^2       F, act: what rb_tendon_state_dev(RB_SP_ENV) reports for s_t and a_t
 * Each mean is summed over k ascending in fp32 by one lane: a cost does not depend on the batch size, the launch range or the kernel
 * form.  Observations, done words, the state, rb_env_stats (which keeps reporting the task's return) and every random draw are those
 * of a handle without the option.
 *   configure: needs rb_env_configure.  NULL or all-zero weights: off, the planes are freed, the handle launches exactly what it
 *        launched before.  Drains the handle's streams and drops its graphs; call it before a caller captures env steps.  Zeroes the
 *        statistics below.  RB_EINVAL for a negative or non-finite weight; RB_EUNSUPPORTED for tension or activation while per-env
 *        parameters are enabled (the readout has no parameter form) or while the action-delay range reaches above 0 (the row applied
 *        is then not the row handed) - in either order of the two calls; action_rate alone combines with both.  A refusal leaves the
 *        handle as it was.  rb_rollout_fused_dev is RB_EUNSUPPORTED while the option is on.
 *   cost_ptr: the device plane [n] of the last step's costs.
 *   stats: {sum of finished episodes' costs, finished episodes, sum of all step costs, steps} since these sums were last cleared
 *        (reset != 0 clears them behind the read; rb_env_configure clears them; rb_env_stats(reset) does not).  fp64, a fixed order
 *        of additions: bit-reproducible.  Synchronous.  rb_env_reset_dev zeroes the running episode costs and the cost plane; the
 *        episodes it abandons are not counted.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_shaping_configure up before relying on it. */
typedef struct rb_env_shaping_config {
    float action_rate, tension, activation;
    float _pad;
} rb_env_shaping_config;
int rb_env_shaping_configure(rb_sim *sim, const rb_env_shaping_config *cfg);
int rb_env_shaping_cost_ptr(rb_sim *sim, float **d_cost /* [n] */);
int rb_env_shaping_stats(rb_sim *sim, double out[4], int reset);

/* ---- random velocity pushes: an external disturbance in front of the fused env step ----
 * Every robot, every kernel form, every env-step entry, every option above: no env-step kernel changes; ONE kernel is launched in
 * front of every env-step launch over envs [i0, i0 + cnt), on its stream, over the same envs.  The step that follows integrates,
 * clamps, writes the row, adds noise, accounts reward and done and auto-resets as it always did, from the state it finds.
 * A handle with the option holds four planes: count, last, n_pushes (uint32 [n]) and impulse (float [n][n_q], env-major for every
 * robot class).  For env i of the handle, global id g = env_id_offset + i, the kernel does:
 *   1. m = count[i]; count[i] = m + 1.  The counter wraps as a uint32; nothing but rb_env_push_configure resets it (neither a reset
 *      nor an episode end does).
 *   2. w = philox_draw(seed, g, m, STREAM_PUSH = 6, block 0).v[0] (csrc/philox.hpp).  The env is PUSHED iff (w >> 8) < threshold:
 *      integer arithmetic only, P(push per env step) = threshold / 2^24.
 *   3. pushed: for every joint j < n_q, z_j is component j & 3 of block 1 + (j >> 2) of the same draw (same seed, g, m, stream),
 *      turned into a normal deviate by the sensor noise's Box-Muller expression (pairs (0,1) and (2,3); u1 = ((w >> 8) + 1) / 2^24,
 *      u2 = (w >> 8) / 2^24; radius sqrt(-2 ln u1), angle 2 pi u2; cosine to the even component, sine to the odd), in fp32;
 *          impulse[i][j] = fl32(sigma_j z_j)
 *          qd_j          = clamp(fl32(qd_j + impulse[i][j]), -qd_max_j, +qd_max_j)       qd_max: the description's, the bound every
 *                                                                                        step kernel clamps to
 *      - product and sum are two roundings, never one fused multiply-add: the stored impulse is exactly what was added.  Then
 *      last[i] = m + 1 and n_pushes[i] += 1.  The velocity lives in the handle's own layout; q is not touched.
 *   4. not pushed: nothing but count[i] is touched; the env's impulse row keeps its old content.
 * After a step, "env i was pushed in this step" reads last[i] == count[i].
 * Order in front of the step: the push kernel, then the reward-shaping cost (the cost of the state the step really starts from),
 * then the env-step kernel.  All of a step's own refusals (a whole-batch-only form given a sub-range, the critic rows' and the
 * shaping checks) are tested BEFORE the push kernel is enqueued: a refused step has moved neither velocities nor counters.
 * rb_env_reset_dev leaves the four planes alone; rb_step* and rb_rollout_dev never push (pushes belong to the env layer).
 *   configure: needs rb_env_configure (RB_EINVAL without).  NULL, threshold == 0 or all of the first n_q sigmas zero: off, the
 *        planes are freed, the handle launches exactly what it launched before.  RB_EINVAL for threshold > 2^24 and for a negative
 *        or non-finite sigma among the first n_q.  RB_ENOMEM when the planes cannot be allocated.  A refusal leaves the handle as it
 *        was.  A successful call zeroes all four planes.  Drains the handle's streams and drops its graphs; call it before a caller
 *        captures env steps.  rb_rollout_fused_dev is RB_EUNSUPPORTED while the option is on.
 *   ptr: the four device planes (any argument may be NULL); RB_EINVAL without the option.
 *   count: the sum of n_pushes over the handle's envs; reset != 0 zeroes that plane behind the read.  Synchronous.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_push_configure up before relying on it. */
typedef struct rb_env_push_config {
    uint32_t threshold;                  /* 0 .. 2^24: P(push per env step) = threshold / 2^24 */
    uint32_t _pad;
    float sigma[32];                     /* rad/s per joint, the first n_q are read */
} rb_env_push_config;
int rb_env_push_configure(rb_sim *sim, const rb_env_push_config *cfg);
int rb_env_push_ptr(rb_sim *sim, uint32_t **d_count, uint32_t **d_last, uint32_t **d_n_pushes, float **d_impulse);
int rb_env_push_count(rb_sim *sim, uint64_t *pushes, int reset);

/* ---- episode log: each env's first E finished episodes - return, length, outcome - behind the fused env step ----
 * Every robot, every kernel form, every env-step entry, every option above: no env-step kernel changes; ONE kernel is launched
 * behind every env-step launch over envs [i0, i0 + cnt), on its stream, over the same envs - behind the reward-shaping apply (the
 * reward is the one the caller receives) and the goal pool, in front of the episode-end codes (the done words are read as flags,
 * != 0, so the records are the same with and without the codes).
 * A handle with capacity E holds, all indexed by the env's index in the handle (never by the position in a launch):
 *   acc   float  [n]     running return of the env's current episode        age   uint32 [n]     steps seen in the current episode
 *   seen  uint32 [n]     the goals-reached counter at the env's last episode end (a plane of the log's own)
 *   count uint32 [n]     records written, saturates at E                     full  uint32 one     number of envs with count == E
 *   ret   float  [E][n]  per-record return      len  uint32 [E][n]  per-record length      kind  uint32 [E][n]  per-record outcome
 * For env i the kernel does, with r = reward[i] and g = the env's goals-reached counter:
 *     a = fl32(acc[i] + r);  t = age[i] + 1
 *     done[i] == 0:  acc[i] = a; age[i] = t
 *     done[i] != 0:  k = (g != seen[i]) ? RB_DONE_TERMINATED : RB_DONE_TRUNCATED;  seen[i] = g;  c = count[i]
 *                    c < E: ret[c][i] = a; len[c][i] = t; kind[c][i] = k; count[i] = c + 1; c + 1 == E: full += 1 (one atomic add)
 *                    acc[i] = 0; age[i] = 0
 * rb_env_reset_dev zeroes acc and age of every env: the abandoned episode is not recorded; records and counts stay.  Wherever
 * the episode counters are cleared (rb_env_stats with reset, rb_env_configure) `seen` is cleared with them.
 *   configure: capacity 0 switches the option off (the planes are freed, the handle launches exactly what it launched before);
 *        1 .. RB_EPISODE_LOG_MAX switches it on.  Needs rb_env_configure.  RB_EINVAL outside 0 .. RB_EPISODE_LOG_MAX, RB_ENOMEM
 *        when the planes cannot be allocated; either leaves the handle as it was.  A successful call leaves every plane zero and
 *        `seen` equal to the counters as they stand.  Drains the handle's streams and drops its graphs; call it before a caller
 *        captures env steps.  rb_rollout_fused_dev is RB_EUNSUPPORTED while the option is on.
 *   ptr: the device planes and the capacity (any argument may be NULL); RB_EINVAL without the option.
 *   clear: count, full, acc and age to zero, `seen` to the counters as they stand.  Enqueued on the handle's stream, nothing is
 *        drained and no graph dropped: it may be called between replays of a captured env step.
 *   summary: over the records k < min(count[i], first_k) of every env (first_k >= 1, may exceed E), eight doubles:
 *        [records, sum of returns, sum of squared returns, sum of lengths, terminated, truncated, envs with count >= first_k, 0].
 *        A two-stage reduction in a fixed order (block partials, then the last block adds them in block order): the same planes
 *        give the same bits; the counts are exact.  summary is synchronous; summary_dev is enqueued on the handle's stream and
 *        writes d_out8 (device memory, may be NULL: the result stays in the handle).
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_episode_log_configure up before relying on it. */
#define RB_EPISODE_LOG_MAX 64
int rb_env_episode_log_configure(rb_sim *sim, int32_t capacity);
int rb_env_episode_log_ptr(rb_sim *sim, uint32_t **d_count, float **d_ret, uint32_t **d_len, uint32_t **d_kind, uint32_t **d_full, int32_t *capacity);
int rb_env_episode_log_clear(rb_sim *sim);
int rb_env_episode_log_summary(rb_sim *sim, int32_t first_k, double out8[8]);
int rb_env_episode_log_summary_dev(rb_sim *sim, int32_t first_k, double *d_out8);

/* ---- start poses: episodes begin at a row of a pool instead of the zero pose ----
 * Every robot, every kernel form, every env-step entry, every option above but tendon channels: no env-step kernel changes; ONE
 * kernel is launched behind every reset kernel (in front of everything else rb_env_reset_dev enqueues: row kernels, sensor noise and
 * critic rows work from what it left) and, on a handle configured with auto_reset, behind every env-step launch over envs
 * [i0, i0 + cnt), on its stream, over the same envs - directly behind the goal kernel, in front of the critic rows, the episode log
 * and the episode-end codes (the done words are read as flags, != 0).  Nothing of the option is enqueued in front of a step.
 * A handle with the option holds the pool (float [m][n_q]) and two planes: count and index (uint32 [n]).  For env i of the handle,
 * global id g = env_id_offset + i, at a reset or where done[i] != 0 behind a step (an env whose done word is 0 is not touched):
 *   1. d = count[i]; count[i] = d + 1.  The counter wraps as a uint32, does not depend on the goal counter, and nothing but
 *      rb_env_start_poses_configure resets it (neither a reset, an episode end nor rb_env_stats does).
 *   2. w = philox_draw(seed, g, d, STREAM_START = 7, block 0) (csrc/philox.hpp).  The env starts FROM THE POOL iff
 *      (w.v[1] >> 8) < threshold, threshold = round-half-even(prob 2^24): integer arithmetic only, 2^24 always, 0 never.
 *   3. from the pool: k = (uint64(w.v[0]) m) >> 32; q = pool[k] bit for bit, qd = 0, feas = 1, index[i] = k, and columns [0, 2 n_q)
 *      of the env's observation row become [pool[k], 0].  Behind a step of a handle with sensor noise on q / qd those columns get the
 *      noise of the row the step has just written (row number rows[i] - 1, the sensor noise's own blocks and expression): the row is
 *      what the step would have written had it reset to the pose.
 *   4. otherwise the env stays at the zero pose the kernel in front wrote: index[i] = RB_START_INDEX_REST, nothing else is touched.
 * The start pose does not change the reward or the done word of the step that ended the previous episode.  A pose that coincides
 * with the env's goal ends the new episode at its first step as reached; nothing keeps poses and goals apart.
 *   configure: needs rb_env_configure.  m == 0 (rows may be NULL): off, pool and planes are freed, the handle launches exactly what
 *        it launched before.  RB_EINVAL for m < 0, prob outside [0, 1] (or NaN), a row that is not finite or outside the robot's joint
 *        limits; RB_EUNSUPPORTED while tendon channels are in the observation (rb_env_obs_configure; that call refuses likewise while
 *        start poses are configured); RB_ENOMEM when pool or planes cannot be allocated.  A refusal leaves the handle as it was.  A
 *        successful call zeroes count and sets every index to RB_START_INDEX_REST; the envs keep the state they have until they
 *        start again.  Drains the handle's streams and drops its graphs; call it before a caller captures env steps.
 *        rb_rollout_fused_dev is RB_EUNSUPPORTED while the option is on.
 *   set: replaces the rows in place by as many others (RB_EINVAL for another m, a bad row, or without the option).  Neither the
 *        pointer nor m moves, so a captured graph reads the new rows at its next replay; poses already started from stay.
 *   ptr: pool, m and the two device planes (any argument may be NULL); RB_EINVAL without the option.
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_start_poses_configure up before relying on it. */
#define RB_START_INDEX_REST 0xFFFFFFFFu
int rb_env_start_poses_configure(rb_sim *sim, const float *rows /* [m][n_q] */, int64_t m, double prob);
int rb_env_start_poses_set(rb_sim *sim, const float *rows /* [m][n_q] */, int64_t m);
int rb_env_start_poses_ptr(rb_sim *sim, float **d_pool, int64_t *m, uint32_t **d_count, uint32_t **d_index);

/* ---- the handle's state as one blob: snapshot and restore ----
 * State is everything a later step, reset, statistic or accessor reads that an earlier one wrote: the core planes (q, qd, the
 * feasibility words, the goal draw counters), the env layer's planes and counters, and every plane of every option that is configured
 * - draw counters, delays, the action ring, the goal and start pools as they stand (they are permuted and rewritten while live),
 * levels, indices, row counts, shaping sums, push planes, the episode log.  Staging buffers, reduction scratch and the constants of
 * the robot or the configuration are not state.  ONE function of the library lists the segments of the handle as it is configured
 * now; the four calls below walk that list.
 *   segments: the table, in blob order.  `name` is a stable string ("core.q", "io.ring", "goals.row_stats", ...), `dtype` the element
 *        type, rows x cols the plane as it lies in memory (row-major [rows][cols]), `offset` the segment's byte offset in the blob,
 *        16-byte aligned.  *count receives the number of segments (also where capacity is smaller, or `out` NULL with capacity 0:
 *        the first min(capacity, *count) entries are written).
 *   bytes: the blob's size (the last segment's end, rounded up to 16).
 *   save_dev: enqueues one device-to-device copy per segment on the handle's stream, behind whatever is in flight there, into d_blob
 *        (device memory, 16-byte aligned), and fills *host (may be NULL).  It synchronises nothing: the blob is complete when the
 *        stream has reached the copies (rb_synchronize, or work enqueued behind them on the same stream).
 *   load_dev: waits until nothing of the handle is in flight, then copies every segment back IN PLACE and sets the host members from
 *        *host (NULL leaves them).  No pointer moves and no graph is dropped, so a captured graph's next replay continues from the
 *        restored state.  The blob must come from a handle of the same configuration (batch size, robot, options and their sizes):
 *        the table is the caller's means to check that - the library checks the byte count alone.
 *   Both return RB_EINVAL for a null blob or a byte count other than rb_env_state_bytes', and a refused call leaves the handle as it
 *   was.  Both work on a handle without rb_env_configure: its segments are the four core planes.
 * Configuration is not state: seed, env id offset, the option records' settings, parameter ranges.  A caller restores into a handle
 * it has configured the same way (RoboyVecEnv.load_state_dict compares identity and table first).
 * RB_ABI_VERSION is still 6 (nothing that existed changed): look rb_env_state_segments up before relying on these four. */
enum rb_state_dtype { RB_STATE_F32 = 0, RB_STATE_U32 = 1, RB_STATE_F64 = 2, RB_STATE_U64 = 3 };
typedef struct rb_state_segment {
    char name[48];
    uint32_t dtype;        /* rb_state_dtype                                            */
    uint32_t reserved;
    int64_t rows, cols;    /* as it lies in memory: [rows][cols]                        */
    int64_t offset;        /* byte offset in the blob, 16-byte aligned                  */
} rb_state_segment;
typedef struct rb_state_host {
    double env_steps;      /* env steps issued since the statistics were reset - the one host member that moves after configuration */
    double reserved[7];
} rb_state_host;
int rb_env_state_segments(rb_sim *sim, rb_state_segment *out, int32_t capacity, int32_t *count);
int rb_env_state_bytes(rb_sim *sim, int64_t *bytes);
int rb_env_state_save_dev(rb_sim *sim, void *d_blob, int64_t bytes, rb_state_host *host);
int rb_env_state_load_dev(rb_sim *sim, const void *d_blob, int64_t bytes, const rb_state_host *host);

/* ---- which kernel instance a call launches: the library's dispatch table, readable (ABI 5) ----
 * Every launch of the three entry kinds goes through ONE table of kernel instances keyed by (robot class, entry kind, kernel form,
 * integrator, workgroup size, constants source, variant); RB_KERNEL_AUTO's thresholds are a list of rules (first match wins).  Both
 * are static data of the library: readable without a GPU, so tests enumerate them instead of restating them. */
enum rb_robot_class { RB_CLASS_BALL8 = 0,   /* one body on an x-y-z ball joint, 8 tendons (MsjRobot's class)         */
                      RB_CLASS_BALLX = 1,   /* the same with 1..16 tendons (run-time count)                           */
                      RB_CLASS_TREE = 2 };  /* any other joint tree                                                   */
enum rb_entry_kind { RB_ENTRY_STEP = 0,           /* rb_step, rb_step_dev, rb_step_range_dev, rb_rollout_dev         */
                     RB_ENTRY_ENV_STEP = 1,       /* rb_env_step_dev, rb_env_step_range_dev                          */
                     RB_ENTRY_FUSED_ROLLOUT = 2 };/* rb_rollout_fused_dev                                            */
typedef struct rb_dispatch_row {
    int32_t robot_class;   /* rb_robot_class                                                                          */
    int32_t entry;         /* rb_entry_kind                                                                           */
    int32_t kernel;        /* an rb_kernel value, never RB_KERNEL_AUTO                                                      */
    int32_t integrator;    /* rb_integrator                                                                           */
    int32_t block;         /* threads per workgroup; 0 = decided by the robot (octet waves, split parts)              */
    int32_t constants;     /* RB_SPEC_NONE (kernarg) / RB_SPEC_TABLE (ahead-of-time instances) / RB_SPEC_JIT (hiprtc) */
    int32_t variant;       /* two lanes per env: mirror plane (0 x-z, 1 y-z); octet joint-tree kernels: single-pass tables; else 0 */
    int32_t ranges;        /* 1: takes sub-ranges of the batch (rb_*_range_dev, rollout chains); 0: whole batches only */
} rb_dispatch_row;
/* what a handle must offer for an AUTO rule to apply (rb_auto_rule.needs, a bit set) */
enum { RB_NEED_MIRROR = 1,        /* ball joints: the robot has a mirror plane (two-lanes-per-env form possible)       */
       RB_NEED_NO_MIRROR = 2,     /* ball joints: it has none                                                          */
       RB_NEED_SPLIT_TABLE = 4,   /* joint trees: ahead-of-time instances of the five-wave split form (the committed upper body) */
       RB_NEED_SPLIT2_TABLE = 8,  /* ... of the lean two-part split form                                               */
       RB_NEED_LANE = 16 };       /* joint trees: one-wave-per-64-envs kernels at hand (ahead of time) or worth building (hiprtc: batch
                                     >= 16 384 envs, generated code within the register file; ROBOY_SIM_JIT) */
typedef struct rb_auto_rule {
    int32_t robot_class;          /* rb_robot_class                                                                    */
    int32_t entry;                /* rb_entry_kind, -1 = any                                                           */
    int32_t integrator;           /* rb_integrator, -1 = any                                                           */
    int32_t needs;                /* RB_NEED_* bits that must all be set                                               */
    int64_t min_envs_exclusive;   /* applies to handles with min_envs_exclusive < n_envs <= max_envs                   */
    int64_t max_envs;
    int32_t kernel;               /* the rb_kernel AUTO picks                                                          */
    int32_t _pad;
} rb_auto_rule;
/* batch-size thresholds of the launch configuration that are not kernel forms */
typedef struct rb_launch_thresholds {
    int64_t small_batch;          /* ball joints, one env per lane: 64-thread workgroups up to here, 256 above (and hiprtc / baked large-batch instances) */
    int64_t pair_small_batch;     /* two lanes per env: the same switch                                                */
    int64_t chain_batch_rk4, chain_batch_euler;             /* rb_rollout_dev: two chains from here on (ball joints)  */
    int64_t chain_batch_tree_rk4, chain_batch_tree_euler;   /* ... joint trees in the one-wave form                   */
    int64_t eager_head_batch_rk4; /* rb_rollout_dev: one ring turn of plain launches in front of the graphs (ball joints, RK4) */
    int64_t tree_jit_batch;       /* joint trees without ahead-of-time instances: AUTO builds the one-wave kernels from here on */
} rb_launch_thresholds;
int rb_dispatch_rows(const rb_dispatch_row **rows);     /* returns the row count; *rows = the library's static table */
int rb_auto_rules(const rb_auto_rule **rules);          /* returns the rule count; first match wins               */
int rb_get_launch_thresholds(rb_launch_thresholds *out);
/* The row the NEXT launch of `entry` over the whole batch takes on this handle (RB_EUNSUPPORTED + message if none).  Builds the
 * run-time kernels that launch would build (hiprtc; never inside a stream capture - then the row of what is at hand). */
int rb_dispatch_current(rb_sim *sim, int entry, rb_dispatch_row *out);

/* device memory helpers so a ctypes caller needs no HIP binding of its own */
int rb_malloc(rb_sim *sim, int64_t bytes, void **d_ptr);
int rb_free(rb_sim *sim, void *d_ptr);
int rb_memcpy_h2d(rb_sim *sim, void *d_dst, const void *h_src, int64_t bytes);
int rb_memcpy_d2h(rb_sim *sim, void *h_dst, const void *d_src, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* ROBOY_SIM_H */
