// roboy_sim.hip - MI355X (gfx950) implementation of include/roboy_sim.h.
//
// Replaces the per-step ROS round-trip of the reference's RosSimulationClient
// (gym_roboy/envs/simulations/ros_simulation_client.py:32-81) by kernels that
// advance N independent environments in lock-step.  Ball-joint robots: state
// struct-of-arrays in HBM, one env per lane (msj_kernels.hpp; one tendon per lane
// for small batches, below), robot constants wave-uniform - through the kernarg
// (scalar loads -> SGPRs), or folded into the code: MsjRobot's table ahead of time
// (msj_baked.hpp), any other 8-tendon robot's by hiprtc at run time (msj_jit.hpp);
// LDS holds only what is indexed at run time (the set-points of the rolled tendon
// loop).  Generic joint trees: one env per lane running straight-line code generated
// for the robot (tree_lane_gen.hpp, tree_lane.hpp: the committed upper body ahead of
// time, other robots by hiprtc) or, without that specialisation, two envs per wave,
// eight lanes per link, working set in LDS (tree_aba.hpp).  DESIGN.md §4-§5.
// Which kernel instance a call launches is ONE table (roboy_dispatch.hpp, included below): rows keyed by robot class / entry kind /
// kernel form / integrator / workgroup size / constants source / variant, RB_KERNEL_AUTO's thresholds as a list of rules - but for a
// handle with per-env parameters, tendon channels, an io configuration or action rows, whose kernels (env_params.hpp, env_obs.hpp,
// env_io.hpp, env_hist.hpp) one launch path chooses (extension_launch, env_host.hpp).  This file holds the kernels that are not in a
// header of their own, the handle, the run-time builds, the streams, chains and graphs, the core C ABI (rb_create, rb_step*,
// rb_rollout*), the tendon-state readout and the dispatch exports; the fused env layer's host side - rb_env_*, rb_params_*, the
// statistics - is env_host.hpp, included behind the dispatch table.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/roboy_sim.h"
#include "msj_build.hpp"
#include "msj_kernels.hpp"
#include "msj_jit.hpp"
#include "tree_aba.hpp"
// env-per-lane form of the joint-tree kernels: generated per robot (tree_lane_gen.hpp); the committed upper body's
// instances are compiled here ahead of time, any other robot's by hiprtc (tree_lane_jit.hpp)
#include "tree_lane_defs.hpp"
#define RBL_NS rbl_baked
#include "tree_lane_baked.hpp"
#include "tree_lane.hpp"
#undef RBL_NS
// ... and its split form (several waves per group of 64 envs, for small batches): tree_lane_split.hpp
#define RBL_NS rbl_split_baked
#include "tree_lane_split_baked.hpp"
#include "tree_lane_split.hpp"
#undef RBL_NS
#include "tree_lane_jit.hpp"
#include "tree_lane_split2.hpp"      // the lean two-part split instances: a translation unit of their own (roboy_sim_split2.hip)
#include "tendon_state.hpp"           // the tendon-state readout (rb_tendon_state_dev)
#include "env_params.hpp"             // per-env physical parameters (rb_params_*)
#include "env_obs.hpp"                // tendon channels in the fused env step's observation (rb_env_obs_*)
#include "env_io.hpp"                 // per-env action latency and sensor noise in the fused env step (rb_env_io_*)
#include "env_hist.hpp"               // the last K commanded actions as observation columns (rb_env_action_obs_*)
#include "env_critic.hpp"             // privileged critic rows behind the fused env step (rb_env_critic_obs_*)
#include "env_goal.hpp"               // goals drawn from a pool of poses (rb_env_goal_pool_*)
#include "env_shaping.hpp"            // action-rate and effort reward terms around the fused env step (rb_env_shaping_*)
#include "env_push.hpp"               // random velocity pushes in front of the fused env step (rb_env_push_*)
#include "env_episode_log.hpp"        // per-env episode records behind the fused env step (rb_env_episode_log_*)
#include "env_start.hpp"              // episodes that begin at a pose from a pool (rb_env_start_poses_*)

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define RB_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(RB_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
    } while (0)

#ifndef RB_SMALL_BATCH
#define RB_SMALL_BATCH 65536   // <= this many envs: latency-oriented launch configuration
#endif
// AUTO picks the tendon-per-lane form up to this many envs (measured crossover,
// profiles/r1_b/sweep.log: Euler 2.9 vs 3.5 us at 8 192 and a tie at 16 384; RK4
// 6.2 vs 7.0 us at 16 384 and 10.2 vs 7.1 us at 32 768)
// (round 4, robots with a mirror plane: the two-lanes-per-env form takes over from 4 096 / 12 288 envs - roboy_dispatch.hpp: AUTO_RULES)
#ifndef RB_TENDON_LANE_BATCH_EULER
#define RB_TENDON_LANE_BATCH_EULER 8192
#endif
#ifndef RB_TENDON_LANE_BATCH_RK4
#define RB_TENDON_LANE_BATCH_RK4 16384
#endif
#ifndef RB_TENDON_LANE_BATCH_PAIR_EULER
#define RB_TENDON_LANE_BATCH_PAIR_EULER 4096
#endif
#ifndef RB_TENDON_LANE_BATCH_PAIR_RK4
#define RB_TENDON_LANE_BATCH_PAIR_RK4 12288
#endif
// launch configuration of the env-per-lane form above RB_SMALL_BATCH envs: workgroup size and
// unroll factor of the tendon loop, per integrator (A/B: profiles/r2_a/kernel_ab_experiments.log)
#ifndef RB_BIG_BLOCK_EULER
#define RB_BIG_BLOCK_EULER 256
#endif
#ifndef RB_BIG_UNROLL_EULER
#define RB_BIG_UNROLL_EULER 2
#endif
#ifndef RB_BIG_BLOCK_RK4
#define RB_BIG_BLOCK_RK4 256
#endif
#ifndef RB_BIG_UNROLL_RK4
#define RB_BIG_UNROLL_RK4 2
#endif
// kernels instantiated on MsjRobot's baked constant table (msj_baked.hpp) unroll the tendon loop by this much, per integrator
// (round 2, U = 2 / 4 / 8: RK4 16.96 / 16.63 / 16.77 us, Euler 2M 36.9 / 35.2 / 35.3 us; round 3, U = 4 / 8: RK4 262 144 envs
// 16.58 / 16.92 us and 2 M envs 97.8 / 110.9 us, Euler 262 144 envs 7.01 / 6.88 us and 2 M envs 35.29 / 34.63 us - fully
// unrolled, the robot's constants are literals instead of scalar-register operands, which issue at half rate (profiles/r3_a:
// issue_forms_probe.log); RK4 pays more for the registers of the longer body than it gains)
#ifndef RB_BAKED_UNROLL_EULER
#define RB_BAKED_UNROLL_EULER 8
#endif
// (round 4: RK4 = RS, the "rolled stages" form - msj_math.hpp: step_rs, msj_kernels.hpp: msj_step_env_per_lane_rs - the four
// stages as a loop over running sums, the eight tendons written out inside it: a quarter of the code and 64 registers, so
// the constants are literals without the register bill that sank U = 8; 262 144 envs 16.6 -> 15.9 us per step with one launch,
// 12.9 -> 12.0 us in two chains, 131 072 envs 9.5 -> 8.6 / 7.4 us; profiles/r4_a/rs_sweep.log)
#ifndef RB_BAKED_UNROLL_RK4
#define RB_BAKED_UNROLL_RK4 RS
#endif
// (the fused open-loop rollout is instantiated with the SAME unroll factor as the step kernel - its results are bit-identical to
// single steps only then: the fully unrolled body contracts its products differently - although it loses to it: it keeps its
// state in registers across steps, 2 M envs Euler 8.6e10 env-steps/s at U = 4, 7.4e10 at U = 8)
// joint-tree robots without ahead-of-time instances: AUTO builds the env-per-lane kernels with hiprtc (~10 s each)
// from this many envs on (ROBOY_SIM_JIT=2: at any batch size, =0: never); below it the octet kernels run
#ifndef RB_TREE_JIT_BATCH
#define RB_TREE_JIT_BATCH 16384
#endif
// ... and only for robots whose generated code keeps at most this many values alive at once (rblg::Generated::max_live;
// the upper body: 332): beyond it the kernel spills to scratch - minutes to build, and every reload a full memory
// latency on a SIMD with one wave - and the octets are the better form.  An explicit rb_select_kernel(1) builds anyway.
#ifndef RB_TREE_LANE_MAX_LIVE
#define RB_TREE_LANE_MAX_LIVE 400
#endif
// joint-tree robots with split-form instances (several waves per 64 envs): AUTO uses them up to this many envs - while
// the waves of a launch still find a SIMD each (measured crossover against the one-wave form: profiles/r3_a)
#ifndef RB_TREE_SPLIT_BATCH
#define RB_TREE_SPLIT_BATCH 16384
#endif
// The lean two-part split form (tree_lane_gen.hpp: SPLIT2_FORM; roboy_sim_split2.hip): AUTO uses it up to this many envs
#ifndef RB_TREE_SPLIT2_BATCH
#define RB_TREE_SPLIT2_BATCH 32768
#endif
// the two-lanes-per-env form launches one-wave workgroups up to this many envs (spread over the CUs), 256-thread ones above
#ifndef RB_PAIR_SMALL_BATCH
#define RB_PAIR_SMALL_BATCH 65536
#endif
// AUTO picks the two-lanes-per-env form (robots with a mirror plane) above the tendon-per-lane range up to this many envs
// (0: never; set from the sweep in profiles/r4_a)
#ifndef RB_PAIR_BATCH_EULER
#define RB_PAIR_BATCH_EULER 16384
#endif
#ifndef RB_PAIR_BATCH_RK4
#define RB_PAIR_BATCH_RK4 32768
#endif
// The fused env layer of an 8-tendon ball-joint robot has its own AUTO thresholds (the accounting behind the step shifts the
// crossovers): two lanes per env up to here where the robot has a mirror plane (profiles/r5_a/env_pairs_sweep.log) ...
#ifndef RB_PAIR_ENV_BATCH_EULER
#define RB_PAIR_ENV_BATCH_EULER 24576
#endif
#ifndef RB_PAIR_ENV_BATCH_RK4
#define RB_PAIR_ENV_BATCH_RK4 32768
#endif
// ... and eight lanes per env below that (any 8-tendon ball-joint robot; profiles/r5_a/env_octets_sweep.log)
#ifndef RB_OCTET_ENV_BATCH_EULER
#define RB_OCTET_ENV_BATCH_EULER 8192
#endif
#ifndef RB_OCTET_ENV_BATCH_RK4
#define RB_OCTET_ENV_BATCH_RK4 8192
#endif
using namespace rbk;    // the env-per-lane kernels (msj_kernels.hpp), EnvParams, GoalBox, ...

// ------------------------------------------------------------------ kernels

// Env-per-lane step for ball-joint robots with 1..NTX tendons (count in c.nt): the rolled
// tendon loop of the large-batch form with a run-time trip count; actions are rows of
// c.nt floats, staged (scaled) as the lane's LDS column.
template <int INTEG, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
msj_step_env_per_lane_nt(const ConstX c, float *__restrict__ q, float *__restrict__ qd,
                         uint32_t *__restrict__ feas, const float *__restrict__ act, float act_scale, long n) {
    const long i = long(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    __shared__ float lds_sp[NTX][BLOCK];
    const int nt = c.nt;
    const float *row = act + i * nt;
    for (int k = 0; k < nt; ++k) lds_sp[k][threadIdx.x] = row[k] * (act_scale * c.ten[k].ksg);
    float qq[3], vv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + i]; vv[j] = qd[j * n + i]; }
    const bool ok = rb::MsjModel<float, NTX>::template step_sp<INTEG, 0>(c, qq, vv, SpLds{&lds_sp[0][threadIdx.x], BLOCK});
#pragma unroll
    for (int j = 0; j < 3; ++j) { q[j * n + i] = qq[j]; qd[j * n + i] = vv[j]; }
    feas[i] = ok ? 1u : 0u;
}

// ---------------------------------------------------------------------------
// Tendon-per-lane form for small batches.  8 consecutive lanes share one env:
// lane k evaluates tendon k (routing, Hill force, torque contribution), the 3
// torque components are summed over the 8 lanes with DPP adds (no LDS), and
// every lane then carries the (cheap, redundant) rigid-body solve.  A wave
// advances 8 envs with ~1/3 of the per-wave instruction chain of the
// env-per-lane form, and a 4 096-env batch becomes 512 waves instead of 64:
// what a latency-bound launch needs.  The per-tendon record is lane-dependent
// here, so it is read from a small device table (one 64-byte record per lane,
// L1/L2-resident) instead of SGPRs.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over the 8 lanes of an env group, result in every lane:
// quad_perm(1,0,3,2), quad_perm(2,3,0,1), then row_half_mirror (lane i <-> 7-i)
__device__ __forceinline__ float sum8(float v) {
    v += dpp_move<0xB1>(v);
    v += dpp_move<0x4E>(v);
    v += dpp_move<0x141>(v);
    return v;
}

struct AccelOneTendon {
    const Const8 &c;
    const rb::MsjTendon<float> &t;
    float spk;
    __device__ __forceinline__ void operator()(const float q[3], const float qd[3], float qdd[3]) const {
        using M = rb::MsjModel<float, NT8>;
        const M::Frame f = M::frame(q, qd);
        float tx = 0.0f, ty = 0.0f, tz = 0.0f;
        M::tendon(c, f, t, spk, tx, ty, tz);
        tx = sum8(tx); ty = sum8(ty); tz = sum8(tz);
        M::rigid_body(c, f, qd, tx, ty, tz, qdd);
    }
};

// XCD-aware block -> env-group map of the two kernels below.  A wave touches only 32 bytes of each
// state plane, so four consecutive waves share every 128-byte line; workgroups
// are dealt round-robin over the 8 XCDs (private L2s), which made each line
// travel to four L2s (PMC: 2.5x the algorithmic read bytes).  Blocks that share
// an XCD (equal blockIdx % 8) now take one contiguous range of env groups
// (bijective form of cdna_hip_programming.md T1; affects traffic only).
__device__ __forceinline__ unsigned xcd_block() {
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7u, qn = nb >> 3, rn = nb & 7u;
    return (xcd < rn ? xcd * (qn + 1u) : rn * (qn + 1u) + (xcd - rn) * qn) + (blockIdx.x >> 3);
}

template <int INTEG>
__global__ void __launch_bounds__(64)
msj_step_tendon_per_lane(const Const8 c, const rb::MsjTendon<float> *__restrict__ ten,
                         float *__restrict__ q, float *__restrict__ qd, uint32_t *__restrict__ feas,
                         const float *__restrict__ act, float act_scale, long n) {
    const long t = long(xcd_block()) * 64 + threadIdx.x;
    const int k = threadIdx.x & 7;
    long e = t >> 3;
    const bool live = e < n;          // whole 8-lane groups are live or not; dead groups
    if (!live) e = n - 1;             // shadow the last env so every DPP partner is active
    const rb::MsjTendon<float> rec = ten[k];
    const float spk = act[e * NT8 + k] * (act_scale * rec.ksg);   // activation offset of the own tendon
    float qq[3], vv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + e]; vv[j] = qd[j * n + e]; }
    const bool ok = rb::MsjModel<float, NT8>::template integrate<INTEG>(c, qq, vv, AccelOneTendon{c, rec, spk});
    // lanes 0-2 store q, 3-5 store qd, 6 stores the feasibility word: one store each
    if (live && k < 6) {
        const float val = k == 0 ? qq[0] : k == 1 ? qq[1] : k == 2 ? qq[2] : k == 3 ? vv[0] : k == 4 ? vv[1] : vv[2];
        float *plane = (k < 3 ? q : qd) + long(k < 3 ? k : k - 3) * n;
        plane[e] = val;
    }
    if (live && k == 6) feas[e] = ok ? 1u : 0u;
}


// The fused env layer in the eight-lanes-per-env form (round 5): the step as above - lane k rescales and evaluates tendon k - and
// behind the integrator lane 0 of each group does RoboyEnv.step's accounting (rbk::env_account, shared with the other two forms).
// For small batches, where a launch is one wave's dependent chain: the chain of this form is a third of the env-per-lane kernel's.
// n: the handle's envs (plane stride); cnt: the envs of this launch (a sub-range arrives on shifted pointers, env0 = its global id).
template <int INTEG>
__global__ void __launch_bounds__(64)
msj_env_step_tendon_per_lane(const Const8 c, const rb::MsjTendon<float> *__restrict__ ten, const MsjEnvArgs a) {
    const float *__restrict__ q = a.q, *__restrict__ qd = a.qd, *__restrict__ goal = a.goal, *__restrict__ act = a.act;
    const long n = a.n, cnt = a.cnt;
    const float slope = a.e.slope, act_hi = a.e.act_hi;
    const long t = long(xcd_block()) * 64 + threadIdx.x;
    const int k = threadIdx.x & 7;
    long e = t >> 3;
    const bool live = e < cnt;
    if (!live) e = cnt - 1;           // dead groups shadow the last env so every DPP partner is active
    const rb::MsjTendon<float> rec = ten[k];
    // action -> set-point (rbe::action_setpoint), then set-point -> activation offset
    const float x = act[e * NT8 + k];
    const float spk = rbe::action_setpoint(slope, x, act_hi) * rec.ksg;
    float qq[3], vv[3], gg[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + e]; vv[j] = qd[j * n + e]; gg[j] = goal[j * n + e]; }
    const bool ok = rb::MsjModel<float, NT8>::template integrate<INTEG>(c, qq, vv, AccelOneTendon{c, rec, spk});
    // (kernarg constants: the accounting reads its arguments late - msj_kernels.hpp, MsjEnvArgs)
    if (live && k == 0) rbk::env_account(rbk::late_env_args(rbk::msj_env_args_offset(int(sizeof(Const8) + sizeof(void *)))), e, qq, vv, gg, ok);
}


// State layout: SoA planes [n_q][n] for the env-per-lane / tendon-per-lane kernels, env-major rows
// [n][n_q] for the joint-tree kernels (rows != 0), tree_aba.hpp.
__device__ __forceinline__ long state_index(long i, int j, int n_q, long n, int rows) { return rows ? i * n_q + j : long(j) * n + i; }

__global__ void reset_kernel(float *q, float *qd, uint32_t *feas, const uint8_t *mask, int n_q, long n, int rows) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    for (int j = 0; j < n_q; ++j) { q[state_index(i, j, n_q, n, rows)] = 0.0f; qd[state_index(i, j, n_q, n, rows)] = 0.0f; }
    feas[i] = 1u;
}

// read-back staging: [n][n_q] q rows | [n][n_q] qd rows | [n] feasibility bytes in
// one buffer: one kernel, one device-to-host copy, one synchronisation
__global__ void pack_state_kernel(const float *q, const float *qd, const uint32_t *feas, float *rows, int n_q, long n, int src_rows) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float *rq = rows + i * n_q, *rv = rows + n * n_q + i * n_q;
    for (int j = 0; j < n_q; ++j) { rq[j] = q[state_index(i, j, n_q, n, src_rows)]; rv[j] = qd[state_index(i, j, n_q, n, src_rows)]; }
    reinterpret_cast<uint8_t *>(rows + 2 * n * n_q)[i] = feas[i] ? 1 : 0;
}
__global__ void unpack_rows_kernel(const float *rows, float *planes, int n_q, long n, int dst_rows) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int j = 0; j < n_q; ++j) planes[state_index(i, j, n_q, n, dst_rows)] = rows[i * n_q + j];
}
__global__ void feas_from_u8_kernel(const uint8_t *f, uint32_t *o, long n) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) o[i] = (f == nullptr || f[i]) ? 1u : 0u;
}

// synthetic actions: env i, step t -> n_t uniforms in [-1, 1), row-major
__global__ void fill_actions_kernel(float *act, int n_t, long n, uint64_t seed, uint64_t env0, uint32_t step) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int b = 0; 4 * b < n_t; ++b) {
        const rb::Philox4 r = rb::philox_draw(seed, env0 + uint64_t(i), step, rb::STREAM_ACTIONS, uint32_t(b));
        for (int e = 0; e < 4 && 4 * b + e < n_t; ++e) act[i * n_t + 4 * b + e] = rb::usym(r.v[e]);
    }
}

// goal = lo + (hi - lo) * u, both operations rounded separately in fp32 so the
// numpy restatement reproduces it bit for bit
__global__ void sample_goals_kernel(float *goal, uint32_t *count, const uint8_t *mask, GoalBox box,
                                    int n_q, long n, uint64_t seed, uint64_t env0, int rows) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    const uint32_t draw = count[i];
    count[i] = draw + 1u;
    for (int b = 0; 4 * b < n_q; ++b) {
        const rb::Philox4 r = rb::philox_draw(seed, env0 + uint64_t(i), draw, rb::STREAM_GOALS, uint32_t(b));
        for (int e = 0; e < 4 && 4 * b + e < n_q; ++e) {
            const int j = 4 * b + e;
            const float g = goal_value(box.lo[j], box.hi[j], r.v[e]);
            if (rows) goal[i * n_q + j] = g; else goal[j * n + i] = g;
        }
    }
}


// rb_env_stats: reduce the per-env accumulators in fp64, ONE launch and nothing else (no memset, no copy:
// the statistics run at the end of every reporting interval of a rollout).  Every block leaves its 8 partial
// sums in `partials`, takes a ticket, and the block that arrives last adds the partials up - thread b owns
// block b's row, then a fixed shuffle / LDS tree - and writes the result to `out` and, if given, `out2`
// (the caller's device buffer).  The sum has a fixed order: bit-reproducible, unlike float atomics.
// Hand-off as MI355X_MICROARCH.md prescribes: stores -> agent-scope release -> vmcnt(0) -> ticket; the last
// block: ticket value -> agent-scope acquire -> barrier -> plain loads.
constexpr int STATS_BLOCKS = 256;
// ENV: the handle runs the fused env layer (all eight slots live); plain rollouts only count infeasible envs, so
// their reduction moves one value instead of eight through the shuffles (8 -> 4 us at 262 144 envs)
template <bool ENV>
__global__ void __launch_bounds__(256)
stats_reduce_kernel(const double *ep_sum, const uint32_t *ep_cnt, const float *ep_ret, const uint32_t *infeas_n,
                    const uint32_t *feas, double *partials, unsigned int *ticket, double *out, double *out2,
                    double env_steps, long n) {
    __shared__ double sh[4][8];
    __shared__ bool last;
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // [sum return, sum return^2, n_episodes, sum length, n_goal, n_infeasible, -, running returns]
    for (long i = long(blockIdx.x) * 256 + threadIdx.x; i < n; i += long(gridDim.x) * 256) {
        if (ENV) {
            v[0] += ep_sum[i]; v[1] += ep_sum[n + i];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[2 + k] += double(ep_cnt[k * n + i]);
            v[7] += double(ep_ret[i]);
            v[5] += double(infeas_n[i]);     // env layer: infeasible env-steps since the reset
        } else {
            v[5] += feas[i] ? 0.0 : 1.0;     // plain rollouts: envs flagged infeasible right now
        }
    }
    auto block_sum = [&]() {                 // -> sh[0][k] in threads 0..7 after the barrier
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (ENV || k == 5)
                for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < 8; ++k) sh[w][k] = v[k];
        __syncthreads();
    };
    block_sum();
    if (threadIdx.x < 8)
        partials[blockIdx.x * 8 + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (threadIdx.x == 0) last = false;
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = threadIdx.x < gridDim.x ? __hip_atomic_load(partials + threadIdx.x * 8 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    block_sum();
    if (threadIdx.x < 8) {
        double t = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        // out: [sum return, sum return^2, n_episodes, sum length, n_goal, n_infeasible, n_env_steps, sum reward]
        if (threadIdx.x == 6) t = env_steps;
        if (threadIdx.x == 7) t += sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];      // sum reward = finished + running returns
        out[threadIdx.x] = t;
        if (out2) out2[threadIdx.x] = t;
    }
    if (threadIdx.x == 0) *ticket = 0u;       // ready for the next launch (same stream: ordered behind this kernel)
}

// Episode-end codes (rb_env_done_kind_*): behind an env-step kernel of any form, over the envs [i0, i1) it stepped.
// An env that is done reached its goal iff its goal counter moved since its last episode end (`seen`); its done word becomes
// RB_DONE_TERMINATED or RB_DONE_TRUNCATED.  Lanes that are not done read nothing but their done word.
__global__ void __launch_bounds__(256)
done_kind_kernel(uint32_t *__restrict__ done, const uint32_t *__restrict__ goals, uint32_t *__restrict__ seen,
                 uint32_t *__restrict__ kind, long i0, long i1) {
    const long i = i0 + long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= i1) return;
    uint32_t d = done[i];
    if (d) {
        const uint32_t g = goals[i];
        d = g != seen[i] ? uint32_t(RB_DONE_TERMINATED) : uint32_t(RB_DONE_TRUNCATED);
        done[i] = d;
        seen[i] = g;
    }
    kind[i] = d;
}

__global__ void env_reset_kernel(const GoalBox box, float *q, float *qd, uint32_t *feas, float *goal,
                                 uint32_t *step_num, float *ep_ret, uint32_t *goal_count, float *obs,
                                 long n, uint64_t seed, uint64_t env0) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float g[3];
    const uint32_t draw = goal_count[i];
    draw_goal3(box, seed, env0 + uint64_t(i), draw, g);
    goal_count[i] = draw + 1u;
    for (int j = 0; j < 3; ++j) {
        q[j * n + i] = 0.0f; qd[j * n + i] = 0.0f; goal[j * n + i] = g[j];
        if (obs) { obs[i * 9 + j] = 0.0f; obs[i * 9 + 3 + j] = 0.0f; obs[i * 9 + 6 + j] = g[j]; }
    }
    feas[i] = 1u; step_num[i] = 1u; ep_ret[i] = 0.0f;
}

inline unsigned blocks_for(long n, int block) { return unsigned((n + block - 1) / block); }

// The options of the fused env layer (env_host.hpp; DESIGN.md §6 has the table): ONE record each, a member of the handle below - what
// the option owns, release() to free and null it, need*() for the entry points that are refused without it.  rb_destroy releases them all.
// Per-env physical parameters (env_params.hpp; rb_params_*): while on, the step and env-step entries launch the parameter kernels
// instead of the dispatch table's row.  Planes [n][n_envs], draw counters [n_envs], ranges lo[n] | hi[n] (device and host copies)
struct OptParams {
    bool on = false, resample = false; int n = 0;
    float *d_planes = nullptr, *d_ranges = nullptr; uint32_t *d_draws = nullptr;
    std::vector<float> ranges;
    void release() { (void)hipFree(d_planes); (void)hipFree(d_draws); (void)hipFree(d_ranges); *this = OptParams{}; }
    int need() const { return on ? RB_OK : fail(RB_EINVAL, "per-env parameters are not enabled (rb_params_enable)"); }
};
// Tendon channels in the env step's observation (env_obs.hpp; rb_env_obs_*): while the mask is set, the env-step entry launches
// the extended kernels - the nominal or the parameter form
struct OptChannels { int mask = 0; float scale[4] = {1.0f, 1.0f, 1.0f, 1.0f}; void release() { *this = OptChannels{}; } };
// Action latency and sensor noise of the env step (env_io.hpp; rb_env_io_*): while on, the env-step entry launches the io kernels -
// nominal or parameter form, with or without channels.  Planes [n_envs] each; the ring [slots][n_envs][n_t] exists with
// delay_hi > 0 or with action rows: slots above max(delay_hi, K - 1)
struct OptIo {
    bool on = false; rb_env_io_config cfg = {};
    uint32_t *d_delay = nullptr, *d_draws = nullptr, *d_rows = nullptr;
    float *d_ring = nullptr; int slots = 0;
    void release() { (void)hipFree(d_delay); (void)hipFree(d_draws); (void)hipFree(d_rows); (void)hipFree(d_ring); *this = OptIo{}; }
};
// The last K handed action rows as observation columns (env_hist.hpp; rb_env_action_obs_*): while rows > 0 the env-step entry
// launches the history kernels, with or without any of the above; the ring is the io record's
struct OptActionRows { int rows = 0; void release() { rows = 0; } };
// Episode-end codes (rb_env_done_kind_*): while on, every env-step launch is followed by done_kind_kernel over its range.
// Planes [n_envs] each: the goal counter d_ep_cnt[2n + i] as of env i's last episode end, and the last step's codes
struct OptDoneKind {
    bool on = false; uint32_t *d_seen = nullptr, *d_kind = nullptr;
    void release() { (void)hipFree(d_seen); (void)hipFree(d_kind); *this = OptDoneKind{}; }
    int need() const { return on ? RB_OK : fail(RB_EINVAL, "episode-end codes are not enabled (rb_env_done_kind_configure)"); }
};
// Privileged critic rows (env_critic.hpp; rb_env_critic_obs_*): while the mask is set, every env-step launch and every reset is
// followed by critic_rows_kernel over its range.  dim: the row width the mask had when it was configured; the plane [n_envs][dim]
struct OptCritic {
    int mask = 0, dim = 0; float *d_rows = nullptr;
    void release() { (void)hipFree(d_rows); *this = OptCritic{}; }
    int need() const { return mask ? RB_OK : fail(RB_EINVAL, "critic rows are not enabled (rb_env_critic_obs_configure)"); }
};
// Goal pool (env_goal.hpp; rb_env_goal_pool_*): while set, every env-step launch and every reset is followed by ONE goal kernel
// over its range, and rb_sample_goals(_dev) return pool rows.  Rows [m][n_q]; m is fixed by the first call, the pointer never moves.
// Curriculum over the pool's row order (rb_env_goal_curriculum_*): while L > 0 that kernel is goal_curriculum_kernel.  Planes
// [n_envs] each, one allocation starting at d_level: the env's level, the row it holds, and the goals-reached counter
// d_ep_cnt[2n + i] as of its last episode end (a copy of its own: episode-end codes may be off); d_hist: [L] counts behind them,
// rb_env_goal_level_hist's device buffer.  Outcome counts per pool row (rb_env_goal_row_stats_*): while d_row_stats is set the
// kernel is goal_curriculum_stats_kernel.  [2][m]: attempts, then reached
struct OptGoals {
    float *d_pool = nullptr; int64_t m = 0;
    uint32_t L = 0, up = 0, down = 0;
    uint32_t *d_level = nullptr, *d_index = nullptr, *d_seen = nullptr;
    uint64_t *d_hist = nullptr, *d_row_stats = nullptr;
    void release() { (void)hipFree(d_pool); (void)hipFree(d_level); (void)hipFree(d_row_stats); *this = OptGoals{}; }
    int need_pool() const { return d_pool ? RB_OK : fail(RB_EINVAL, "no goal pool is set (rb_env_goal_pool_set)"); }
    int need_curriculum() const { return L ? RB_OK : fail(RB_EINVAL, "no goal curriculum is configured (rb_env_goal_curriculum_configure)"); }
    int need_row_stats() const { return d_row_stats ? RB_OK : fail(RB_EINVAL, "goal row stats are not enabled (rb_env_goal_row_stats_enable)"); }
};
// Reward shaping (env_shaping.hpp; rb_env_shaping_*): while on, every env-step launch has shaping_cost in front of it and
// shaping_apply behind it, over its range.  Planes: the previous clamped action rows [n_envs][n_t], the last step's costs [n_envs],
// the running episode costs [n_envs] (fp64), sums [2][n_envs] (finished episodes' costs, all step costs; fp64) and counts [2][n_envs]
// (finished episodes, steps); d_red: the reduction's block partials [REDUCE_BLOCKS][4], then its result [4]
struct OptShaping {
    bool on = false; rb_env_shaping_config cfg = {};
    float *d_prev = nullptr, *d_cost = nullptr;
    double *d_run = nullptr, *d_sums = nullptr, *d_red = nullptr; uint32_t *d_cnt = nullptr;
    int tree_waves = 1;                  // joint trees: waves per workgroup of the cost kernel (its LDS holds the per-tendon terms too)
    bool tendons() const { return on && (cfg.tension != 0.0f || cfg.activation != 0.0f); }
    void release() {
        (void)hipFree(d_prev); (void)hipFree(d_cost); (void)hipFree(d_run); (void)hipFree(d_sums); (void)hipFree(d_red); (void)hipFree(d_cnt);
        *this = OptShaping{};
    }
    int need() const { return on ? RB_OK : fail(RB_EINVAL, "reward shaping is not configured (rb_env_shaping_configure)"); }
};
// Random velocity pushes (env_push.hpp; rb_env_push_*): while on, every env-step launch has env_push in front of it (and in front of
// shaping_cost), over its range.  Planes [n_envs] each: steps counted, the count at the env's last push, pushes; the last impulses
// [n_envs][n_q]; d_total: rb_env_push_count's device word
struct OptPush {
    bool on = false; rb_env_push_config cfg = {};
    uint32_t *d_count = nullptr, *d_last = nullptr, *d_n = nullptr;
    float *d_impulse = nullptr; unsigned long long *d_total = nullptr;
    void release() {
        (void)hipFree(d_count); (void)hipFree(d_last); (void)hipFree(d_n); (void)hipFree(d_impulse); (void)hipFree(d_total);
        *this = OptPush{};
    }
    int need() const { return on ? RB_OK : fail(RB_EINVAL, "random pushes are not configured (rb_env_push_configure)"); }
};
// Episode log (env_episode_log.hpp; rb_env_episode_log_*): while E > 0, every env-step launch is followed by episode_log_kernel over
// its range.  Planes [n_envs] each: the running return and age of the current episode, the goals-reached counter d_ep_cnt[2n + i] as of
// the env's last episode end (a copy of its own, like the curriculum's), records written; records [E][n_envs] each: return, length,
// outcome; d_full: the number of envs with E records; d_red: the summary's result [8], block partials [SUMMARY_BLOCKS][8], ticket
struct OptEpisodeLog {
    int E = 0;
    float *d_acc = nullptr, *d_ret = nullptr;
    uint32_t *d_age = nullptr, *d_seen = nullptr, *d_count = nullptr, *d_len = nullptr, *d_kind = nullptr, *d_full = nullptr;
    double *d_red = nullptr;
    void release() {
        (void)hipFree(d_acc); (void)hipFree(d_ret); (void)hipFree(d_age); (void)hipFree(d_seen); (void)hipFree(d_count); (void)hipFree(d_len);
        (void)hipFree(d_kind); (void)hipFree(d_full); (void)hipFree(d_red);
        *this = OptEpisodeLog{};
    }
    int need() const { return E ? RB_OK : fail(RB_EINVAL, "the episode log is not configured (rb_env_episode_log_configure)"); }
};
// Start poses (env_start.hpp; rb_env_start_poses_*): while d_pool is set, every reset kernel and - on a handle with auto_reset - every
// env-step launch is followed by env_start over its range.  Rows [m][n_q]; m and the pointer stay for the option's life
// (rb_env_start_poses_set writes the rows in place).  Planes [n_envs] each: starts counted, the row the running episode began at
struct OptStart {
    float *d_pool = nullptr; int64_t m = 0;
    uint32_t threshold = 0; double prob = 0.0;
    uint32_t *d_count = nullptr, *d_index = nullptr;
    void release() { (void)hipFree(d_pool); (void)hipFree(d_count); (void)hipFree(d_index); *this = OptStart{}; }
    int need() const { return d_pool ? RB_OK : fail(RB_EINVAL, "start poses are not configured (rb_env_start_poses_configure)"); }
};

}  // namespace

// --------------------------------------------------------------------- handle
struct rb_sim {
    int device = 0, n_cu = 256;
    long n = 0;
    int n_q = 0, n_t = 0;
    int integrator = 0, nsub = 1, kernel = RB_KERNEL_ENV_PER_LANE;
    double step_size = 0.1;
    uint64_t seed = 0;
    int64_t env0 = 0;
    Const8 c8;
    ConstX cx;               // ball-joint robots with n_t != 8 (ntx = true)
    bool ntx = false;
    bool baked = false;      // c8 equals MsjRobot's compile-time table (msj_baked.hpp): the BK kernel instances apply
    // any other 8-tendon ball-joint robot: the same instances compiled at run time on ITS constants (msj_jit.hpp),
    // built by the first large-batch call; 0 = not tried yet, 1 = in use, -1 = not available (kernarg instances run)
    int jit_state = 0;
    rbj::Module jit;
    std::string jit_why;
    rb::MsjTendon<float> *d_ten = nullptr;   // device copy of c8.ten for the tendon-per-lane form
    // two lanes per env (msj_kernels.hpp: mirror pairs): available when the robot has a mirror plane (find_mirror_pairs)
    bool pair_ok = false, pair_baked = false;   // pair_baked: the baked table's own tendons 0..3 are a mirror half (BK instances apply)
    int pair_mirror = 0;                        // 0: x-z plane, 1: y-z plane
    int pair_half[4] = {0, 1, 2, 3}, pair_image[4] = {7, 6, 5, 4};   // the even lane's tendons and their mirror images
    Const8 c8p;                                 // c8 with the even lane's tendons first (kernarg instances)
    int kernel_choice = RB_KERNEL_AUTO;
    // generic joint-tree robots (tree_aba.hpp): a few envs per wave, articulated-body algorithm
    bool tree = false;
    rbt::TreeHost tree_host;
    uint32_t *d_tree_words = nullptr;   // the robot tables, staged into LDS by every workgroup
    int tree_waves = 1;                 // waves per workgroup
    // the generated forms of the joint-tree kernels (tree_lane_gen.hpp), by rblg::FORM_*: one wave per 64 envs (tree_lane.hpp), and
    // the split forms (tree_lane_split.hpp: several waves per group of 64 envs, for small batches) - five waves, or the lean two-part
    // form (two workgroups per CU).  Ahead-of-time instances for the committed upper body, hiprtc-built kernels for any other robot
    rblj::TreeForm forms[rblg::N_FORMS];
    static int form_index(int kernel) {      // RB_KERNEL_ENV_PER_LANE, _SPLIT or _SPLIT2
        return kernel == RB_KERNEL_ENV_PER_LANE_SPLIT ? rblg::FORM_SPLIT : kernel == RB_KERNEL_ENV_PER_LANE_SPLIT2 ? rblg::FORM_SPLIT2 : rblg::FORM_LANE;
    }
    rblj::TreeForm &form(int kernel) { return forms[form_index(kernel)]; }
    const rblj::TreeForm &form(int kernel) const { return forms[form_index(kernel)]; }
    GoalBox box;
    hipStream_t own_stream = nullptr, stream = nullptr;
    static constexpr int MAX_CHAINS = 4;
    int chains_choice = 0;                                 // rb_set_rollout_chains: 0 = the library's choice, 1..MAX_CHAINS = that many
    hipStream_t chain_stream[MAX_CHAINS] = {};             // the further chains of rb_rollout_dev ([0] unused: the handle's stream; created on first use)
    hipEvent_t chain_fork = nullptr, chain_join[MAX_CHAINS] = {};
    // caller streams handed to rb_step_range_dev / rb_env_step_range_dev: the handle remembers each distinct one with an event
    // recorded behind its last range launch, so that drain() (rb_destroy, rb_select_kernel, rb_set_stream, graph eviction) waits
    // for that work too.  A small set (a closed-loop caller uses one stream per chain); beyond it the oldest entry is waited
    // for and reused.
    static constexpr int MAX_CALLER_STREAMS = 8;
    struct CallerStream { hipStream_t stream = nullptr; hipEvent_t done = nullptr; bool pending = false; uint64_t tick = 0; };
    CallerStream caller[MAX_CALLER_STREAMS];
    uint64_t caller_tick = 0;
    hipStream_t call_stream = nullptr;                     // the stream of the range call in progress (capturing() looks at it too)
    float *d_q = nullptr, *d_qd = nullptr;
    uint32_t *d_feas = nullptr, *d_goal_count = nullptr;
    // fused env layer (rb_env_*)
    bool env_ready = false;
    EnvParams env;
    float *d_goal = nullptr, *d_ep_ret = nullptr;
    double *d_ep_sum = nullptr;      // [2][n]: sum of episode returns, sum of squared returns
    uint32_t *d_ep_cnt = nullptr;    // [3][n]: episodes, summed episode length, goals reached
    uint32_t *d_step_num = nullptr, *d_infeas_n = nullptr;
    double *d_stats = nullptr;   // [8] result of the reduction, then [STATS_BLOCKS][8] block partials, then the ticket word
    double env_steps = 0.0;      // env steps issued since the statistics were reset
    // host I/O staging
    float *d_rows = nullptr;   // [n][max(n_q, n_t)]
    float *d_state_rows = nullptr, *h_state_rows = nullptr;   // read-back staging, device / pinned host
    uint8_t *d_u8 = nullptr;   // [n]
    // rollout graph cache
    struct GraphKey {
        const float *ring_ptr; int ring; int chunk; float scale; int kernel;
        bool operator<(const GraphKey &o) const {
            return std::memcmp(this, &o, sizeof(GraphKey)) < 0;
        }
    };
    struct ChainGraphs {                                   // one LINEAR graph per chain (a chain = a stream stepping its share of the envs)
        hipGraphExec_t exec[MAX_CHAINS] = {};
        int chains = 1;
        void destroy() { for (hipGraphExec_t &e : exec) { if (e) (void)hipGraphExecDestroy(e); e = nullptr; } }
    };
    std::map<GraphKey, ChainGraphs> graphs;
    // tendon-state readout (tendon_state.hpp): physical-unit constants of the ball-joint class, the same-link segment lengths of
    // a joint tree (device copy made by the first readout), and the host form's device outputs (4 x [n][n_t], first use)
    rbts::Units<rbk::NTX> ts_units;
    std::vector<float> ts_tree_lconst;
    float *d_ts_lconst = nullptr, *d_ts_out = nullptr;
    bool ts_attr_set = false;
    OptParams par; OptChannels chan; OptIo io; OptActionRows hist; OptDoneKind done; OptCritic critic; OptGoals goals;      // the env layer's options (above)
    OptShaping shaping;
    OptPush push;
    OptEpisodeLog elog;
    OptStart start;
    float qd_max[32] = {};               // the description's velocity bounds, as every step kernel holds them (fp32)
    int obs_dim() const { return 3 * n_q + rbo::n_channels(chan.mask) * n_t + hist.rows * n_t; }
    int critic_width() const { return rbc::row_dim(critic.mask, n_q, par.on ? par.n : 0, hist.rows * n_t); }
};

namespace {

// ---- the handle's state (rb_env_state_*, env_host.hpp) ----
// The ONE list of "what is state": everything a later step, reset, statistic or accessor reads that an earlier one wrote, as the handle
// is configured now, in blob order.  rb_env_state_segments / _bytes / _save_dev / _load_dev walk it and nothing else does.  Every
// device-pointer member of rb_sim and of the Opt* records above is EITHER named here OR on the list below (tests/test_env_state_cpu.py
// reads this text and fails for a member in neither or in both): a new option adds its planes here.
// not state - staging and scratch, written in full before they are read:
//   rb_sim.d_rows, rb_sim.d_state_rows, rb_sim.d_u8, rb_sim.d_stats, rb_sim.d_ts_out, OptGoals.d_hist, OptShaping.d_red,
//   OptEpisodeLog.d_red, OptPush.d_total
// not state - constants of the robot or the configuration:
//   rb_sim.d_ten, rb_sim.d_tree_words, rb_sim.d_ts_lconst, OptParams.d_ranges
struct StateSeg { const char *name; uint32_t dtype; int64_t rows, cols; void *ptr; };
inline size_t state_elem_bytes(uint32_t dtype) { return dtype == RB_STATE_F32 || dtype == RB_STATE_U32 ? 4 : 8; }
inline size_t state_seg_bytes(const StateSeg &g) { return state_elem_bytes(g.dtype) * size_t(g.rows) * size_t(g.cols); }
std::vector<StateSeg> state_segments(rb_sim *s) {
    std::vector<StateSeg> v;
    const int64_t n = s->n, nq = s->n_q, nt = s->n_t;
    auto seg = [&](const char *name, uint32_t dtype, int64_t rows, int64_t cols, void *p) {      // (an option that is off holds null planes)
        if (p && rows > 0 && cols > 0) v.push_back(StateSeg{name, dtype, rows, cols, p});
    };
    // joint planes: [n_q][n] for the ball-joint classes, [n][n_q] for joint trees
    const int64_t jr = s->tree ? n : nq, jc = s->tree ? nq : n;
    seg("core.q", RB_STATE_F32, jr, jc, s->d_q);
    seg("core.qd", RB_STATE_F32, jr, jc, s->d_qd);
    seg("core.feas", RB_STATE_U32, 1, n, s->d_feas);
    seg("core.goal_count", RB_STATE_U32, 1, n, s->d_goal_count);
    if (s->env_ready) {
        seg("env.goal", RB_STATE_F32, jr, jc, s->d_goal);
        seg("env.ep_ret", RB_STATE_F32, 1, n, s->d_ep_ret);
        seg("env.step_num", RB_STATE_U32, 1, n, s->d_step_num);
        seg("env.ep_sum", RB_STATE_F64, 2, n, s->d_ep_sum);
        seg("env.ep_cnt", RB_STATE_U32, 3, n, s->d_ep_cnt);
        seg("env.infeas_n", RB_STATE_U32, 1, n, s->d_infeas_n);      // (only env steps count into it)
    }
    if (s->par.on) {
        seg("par.planes", RB_STATE_F32, s->par.n, n, s->par.d_planes);
        seg("par.draws", RB_STATE_U32, 1, n, s->par.d_draws);
    }
    if (s->io.on) {
        seg("io.delay", RB_STATE_U32, 1, n, s->io.d_delay);
        seg("io.draws", RB_STATE_U32, 1, n, s->io.d_draws);
        seg("io.rows", RB_STATE_U32, 1, n, s->io.d_rows);
    }
    seg("io.ring", RB_STATE_F32, s->io.slots, n * nt, s->io.d_ring);      // (action rows keep a ring without an io configuration)
    if (s->done.on) {
        seg("done.seen", RB_STATE_U32, 1, n, s->done.d_seen);
        seg("done.kind", RB_STATE_U32, 1, n, s->done.d_kind);
    }
    seg("critic.rows", RB_STATE_F32, n, s->critic.dim, s->critic.d_rows);
    seg("goals.pool", RB_STATE_F32, s->goals.m, nq, s->goals.d_pool);
    if (s->goals.L) {
        seg("goals.level", RB_STATE_U32, 1, n, s->goals.d_level);
        seg("goals.index", RB_STATE_U32, 1, n, s->goals.d_index);
        seg("goals.seen", RB_STATE_U32, 1, n, s->goals.d_seen);
    }
    seg("goals.row_stats", RB_STATE_U64, 2, s->goals.m, s->goals.d_row_stats);
    if (s->shaping.on) {
        seg("shaping.prev", RB_STATE_F32, n, nt, s->shaping.d_prev);
        seg("shaping.cost", RB_STATE_F32, 1, n, s->shaping.d_cost);
        seg("shaping.run", RB_STATE_F64, 1, n, s->shaping.d_run);
        seg("shaping.sums", RB_STATE_F64, 2, n, s->shaping.d_sums);
        seg("shaping.cnt", RB_STATE_U32, 2, n, s->shaping.d_cnt);
    }
    if (s->push.on) {
        seg("push.count", RB_STATE_U32, 1, n, s->push.d_count);
        seg("push.last", RB_STATE_U32, 1, n, s->push.d_last);
        seg("push.n", RB_STATE_U32, 1, n, s->push.d_n);
        seg("push.impulse", RB_STATE_F32, n, nq, s->push.d_impulse);
    }
    if (s->elog.E) {
        seg("elog.acc", RB_STATE_F32, 1, n, s->elog.d_acc);
        seg("elog.ret", RB_STATE_F32, s->elog.E, n, s->elog.d_ret);
        seg("elog.age", RB_STATE_U32, 1, n, s->elog.d_age);
        seg("elog.seen", RB_STATE_U32, 1, n, s->elog.d_seen);
        seg("elog.count", RB_STATE_U32, 1, n, s->elog.d_count);
        seg("elog.len", RB_STATE_U32, s->elog.E, n, s->elog.d_len);
        seg("elog.kind", RB_STATE_U32, s->elog.E, n, s->elog.d_kind);
        seg("elog.full", RB_STATE_U32, 1, 1, s->elog.d_full);
    }
    if (s->start.m) {
        seg("start.pool", RB_STATE_F32, s->start.m, nq, s->start.d_pool);
        seg("start.count", RB_STATE_U32, 1, n, s->start.d_count);
        seg("start.index", RB_STATE_U32, 1, n, s->start.d_index);
    }
    return v;
}
// the segments' byte offsets in the blob (each 16-byte aligned) and the blob's size
inline int64_t state_layout(const std::vector<StateSeg> &segs, std::vector<int64_t> *offsets) {
    int64_t at = 0;
    for (const StateSeg &g : segs) {
        if (offsets) offsets->push_back(at);
        at += int64_t((state_seg_bytes(g) + 15) & ~size_t(15));
    }
    return at;
}

// Build the run-time specialised kernels of this robot once, outside any stream capture (hipModuleLoadData
// is not capturable): called by the entry points before they launch or capture.
// A stream that is being captured must not see the build: the attempt is left for a later call (the state stays
// "not tried") and this call launches the instances it already has.
bool stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return stream && hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
// the handle's stream, or the caller's stream of the range call in progress (rb_*_range_dev set call_stream around their work)
bool capturing(rb_sim *s) { return stream_capturing(s->stream) || (s->call_stream && stream_capturing(s->call_stream)); }
struct CallStreamScope {          // the stream a range entry point launches on, visible to the build guards for the call's duration
    rb_sim *s;
    CallStreamScope(rb_sim *sim, hipStream_t st) : s(sim) { s->call_stream = st; }
    ~CallStreamScope() { s->call_stream = nullptr; }
};

int jit_level() {      // ROBOY_SIM_JIT: 0 = never, 1 (default) = from the batch thresholds on, 2 = at any batch size
    const char *e = std::getenv("ROBOY_SIM_JIT");
    return e && e[0] >= '0' && e[0] <= '2' ? e[0] - '0' : 1;
}

// AUTO's own condition for the one-wave-per-64-envs form of the joint-tree kernels: instances at hand, or worth building
bool tree_wants_lane_auto(const rb_sim *s) {
    const rblj::TreeForm &f = s->form(RB_KERNEL_ENV_PER_LANE);
    if (!s->tree || !f.ok) return false;
    if (f.baked) return true;
    const int lvl = jit_level();
    return f.gen.max_live <= RB_TREE_LANE_MAX_LIVE && (lvl == 2 || (lvl == 1 && s->n >= RB_TREE_JIT_BATCH));
}
// may this handle run that form?  (an explicit choice, AUTO's condition, or as what the split forms degrade to)
bool tree_wants_lane(const rb_sim *s) {
    if (!s->tree || !s->form(RB_KERNEL_ENV_PER_LANE).ok || s->kernel_choice == RB_KERNEL_ENV_PER_WAVE) return false;
    return s->kernel_choice == RB_KERNEL_ENV_PER_LANE || tree_wants_lane_auto(s);
}

// Is generated form `kernel` (RB_KERNEL_ENV_PER_LANE, _SPLIT, _SPLIT2) at hand for `kind` (0 = step, 1 = env step)?  Its ahead-of-time
// instances, or its hiprtc-built kernel - which `build` = true builds if it has not been tried yet, never during a stream capture.
bool tree_form_ready(rb_sim *s, int kernel, int kind, bool build) {
    rblj::TreeForm &f = s->form(kernel);
    rblj::Kernel &k = f.kernel(kind);
    if (f.baked || k.state == 1) return true;
    if (build && f.ok && k.state == 0 && !capturing(s))
        return rblj::build(s->device, rb_sim::form_index(kernel), f.gen, s->integrator == RB_EULER ? 0 : 1, kind, k);
    return false;
}
void maybe_jit(rb_sim *s) {
    if (s->par.on) return;                        // the parameter kernels are ahead of time (and a later call builds after rb_params_disable)
    if (s->tree) { if (tree_wants_lane(s)) (void)tree_form_ready(s, RB_KERNEL_ENV_PER_LANE, 0, true); return; }
    if (s->jit_state != 0) return;
    if (s->ntx || s->baked || s->n <= RB_SMALL_BATCH || !rbj::enabled() || jit_level() == 0) { s->jit_state = -1; return; }
    if (capturing(s)) return;                     // try again outside the capture
    s->jit_state = -1;
    if (hipSetDevice(s->device) != hipSuccess) return;
    if (rbj::build(s->c8, s->jit, s->jit_why)) s->jit_state = 1;
}

// Chains: rb_rollout_dev steps large batches (ball joints; joint trees in the one-wave form) as TWO independent chains of
// half-batch launches on two streams (one linear graph per chain).  One launch per step leaves 1.8 us between launches and
// ~1.1 us of load / store phases that nothing overlaps (profiles/r3_a/headline_stamps.log: one generation of waves); with two
// chains one half's gaps lie under the other half's arithmetic, and two concurrent launches interleave their generations of
// waves.  Measured with bench.py's regions (profiles/r3_a/chain_thresholds.log, us per step, one launch -> two chains):
// MsjRobot RK4 98 304 envs 9.4 -> 9.0, 196 608 envs 12.8 -> 11.6, 262 144 envs 16.6 -> 13.0, 2 M envs 97 -> 92; Euler 131 072 envs
// 3.9 -> 4.1 (slower: a chain cannot step faster than ~3.6 us per launch), 262 144 envs 6.9 -> 5.6, 524 288 envs 11.0 -> 7.9,
// 2 M envs 33.7 -> 30.7; upper body (one wave per 64 envs) Euler 32 768 envs 15.8 -> 15.3, 65 536 envs 18.7 -> 16.8, 262 144 envs
// 70.3 -> 56.9; RK4 65 536 envs 55.6 -> 53.7, 131 072 envs 109.3 -> 102.1.  Three and four chains are no better anywhere
// (chain_count.log).  Envs are independent, so the results are those of one launch per step, bit for bit.
// ROBOY_SIM_CHAINS = 1 switches it off (2-4 force a count).
// Flags of the events that fork and join the chains.  Producer and consumer of such an event are kernels on the SAME device; the
// event's own system-scope release + acquire (for the host and other devices) is a fixed cost of ~3 us per event: without it a 20-step
// rollout of the headline batch takes 13.3-13.4 instead of 13.5-13.7 us per step (profiles/r5_a/event_flags_ab.log).  What the
// fence-free form rests on is read off the packets (profiles/r6_a/chain_fence_scopes.log: ROCclr's packet log of a two-chain rollout,
// HIP 7.2.26015 / ROCm 7.2.0): EVERY kernel dispatch packet of a chain - eager or replayed from a graph, 75 of 75 - carries header
// 0xb02 = barrier, acquire scope AGENT, release scope AGENT, with or without the flag; the event's marker is a barrier packet whose
// header goes from 0x1500 (acquire / release scope system) to 0x100 (completion only) with the flag; the waiting stream's barrier
// packet carries no fence in either mode.  So the join is: producer kernel (agent-scope release at its end) -> marker (completion
// signal) -> wait -> consumer kernel (agent-scope acquire at its start) - the XCD-private L2s are written back / invalidated at agent
// scope by the kernels' own packets, which is all a same-device consumer needs.  Host visibility is not these events' job: every
// host-facing entry point ends in hipStreamSynchronize (its barrier packet keeps system scope).  Guard tests with readers on other XCDs
// than the writers: tests/test_full_size_gpu.py::test_consumers_behind_the_join_see_the_other_chains_writes (graph chains; eager head +
// graphs + trailing whole-batch launches; the upper body's chains).  ROBOY_SIM_EVENT_SYSTEM_FENCE=1 restores the system-scope events at
// run time (another ROCm, a doubt, an A/B); a HIP without the flag builds the fenced form.
#ifndef RB_CHAIN_EVENT_FLAGS
#ifdef hipEventDisableSystemFence
#define RB_CHAIN_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
#else
#define RB_CHAIN_EVENT_FLAGS hipEventDisableTiming
#endif
#endif
inline unsigned chain_event_flags() {
    static const bool fenced = [] { const char *e = std::getenv("ROBOY_SIM_EVENT_SYSTEM_FENCE"); return e && e[0] == '1'; }();
    return fenced ? unsigned(hipEventDisableTiming) : unsigned(RB_CHAIN_EVENT_FLAGS);
}
#ifndef RB_CHAIN_BATCH_RK4
#define RB_CHAIN_BATCH_RK4 98304
#endif
#ifndef RB_CHAIN_BATCH_EULER
#define RB_CHAIN_BATCH_EULER 262144
#endif
#ifndef RB_CHAIN_BATCH_TREE_EULER
#define RB_CHAIN_BATCH_TREE_EULER 32768
#endif
#ifndef RB_CHAIN_BATCH_TREE_RK4
#define RB_CHAIN_BATCH_TREE_RK4 65536
#endif
#include "roboy_dispatch.hpp"

// does this handle run split form `kernel`: F_SPLIT (five waves per 64 envs) or F_SPLIT2 (the lean two-part form)?  An explicit choice
// (any robot with a split plan: rb_select_kernel has built the kernels of a robot without instances), or AUTO's rules: the five-wave
// form while its waves still find a SIMD each, the lean form from there up to a wave on every SIMD - both where ahead-of-time
// instances exist
bool tree_wants_split(const rb_sim *s, int kernel) {
    if (!s->tree || !s->form(kernel).ok) return false;
    if (s->kernel_choice == kernel) return true;
    return s->kernel_choice == RB_KERNEL_AUTO && auto_form(s, ENTRY_STEP) == kernel;
}

// kernel forms that step a sub-range of the batch (shifted pointers, own env count): what chains and the rb_*_range_dev entry points
// need.  A pure query: the row of what is at hand, no build (rb_rollout_dev / rb_step_range_dev / rb_range_capable build first).
bool range_capable(const rb_sim *s) {
    if (extension_serves(s, ENTRY_STEP)) return true;
    const Row *r = row_for(const_cast<rb_sim *>(s), ENTRY_STEP, /*build=*/false);
    return r && r->ranges;
}
bool chainable(const rb_sim *s) { return range_capable(s) && (s->tree || s->n > RB_SMALL_BATCH); }
int rollout_chains(const rb_sim *s) {
    static const int forced = [] { const char *e = getenv("ROBOY_SIM_CHAINS"); return e ? atoi(e) : 0; }();
    if (!chainable(s)) return 1;
    if (s->chains_choice >= 1) return s->chains_choice;
    if (forced >= 1 && forced <= rb_sim::MAX_CHAINS) return forced;
    if (s->tree) return s->n >= (s->integrator == RB_EULER ? RB_CHAIN_BATCH_TREE_EULER : RB_CHAIN_BATCH_TREE_RK4) ? 2 : 1;
    return s->n >= (s->integrator == RB_EULER ? RB_CHAIN_BATCH_EULER : RB_CHAIN_BATCH_RK4) ? 2 : 1;
}

// does rb_rollout_dev put one ring turn of plain launches in front of its graphs?  Where a step kernel outlasts the host's
// launches of a step (~3.5 us each, one per chain) with room to spare: ball joints, RK4, from 196 608 envs on (20-step rollouts
// of the headline batch 13.7 -> 13.4 us per step; at 131 072 envs and for the joint trees it is a wash: head_sweep.log);
// ROBOY_SIM_EAGER_HEAD=0 / 1 forces it off / on
#ifndef RB_EAGER_HEAD_BATCH_RK4
#define RB_EAGER_HEAD_BATCH_RK4 196608
#endif
bool rollout_eager_head(const rb_sim *s, int chains) {
    static const int forced = [] { const char *e = getenv("ROBOY_SIM_EAGER_HEAD"); return e ? atoi(e) : -1; }();
    if (forced >= 0) return forced != 0;
    if (s->tree) return false;
    return !s->ntx && s->integrator == RB_RK4 && s->n >= RB_EAGER_HEAD_BATCH_RK4;
}

// the physics step over envs [i0, i1) on `stream` (i1 < 0: the whole batch on the handle's stream): one row of the dispatch table
int launch_step(rb_sim *s, const float *d_act, float act_scale, long i0 = 0, long i1 = -1, hipStream_t stream = nullptr) {
    Launch L;
    if (i1 < 0) { L.i0 = 0; L.cnt = s->n; L.stream = s->stream; }
    else        { L.i0 = i0; L.cnt = i1 - i0; L.stream = stream; }
    L.act = d_act; L.act_scale = act_scale;
    return dispatch(s, ENTRY_STEP, L);
}

int check(const rb_sim *s) {
    if (!s) return fail(RB_EINVAL, "null simulation handle");
    return RB_OK;
}

int read_state_host(rb_sim *s, float *q, float *qd, uint8_t *feasible) {
    const long n = s->n;
    const size_t plane = sizeof(float) * size_t(n) * s->n_q;
    hipLaunchKernelGGL(pack_state_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s->stream,
                       s->d_q, s->d_qd, s->d_feas, s->d_state_rows, s->n_q, n, s->tree ? 1 : 0);
    RB_HIP(hipGetLastError());
    RB_HIP(hipMemcpyAsync(s->h_state_rows, s->d_state_rows, 2 * plane + size_t(n), hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    const char *h = reinterpret_cast<const char *>(s->h_state_rows);
    if (q) std::memcpy(q, h, plane);
    if (qd) std::memcpy(qd, h + plane, plane);
    if (feasible) std::memcpy(feasible, h + 2 * plane, size_t(n));
    return RB_OK;
}

// Every stream this handle may still have work on - the stream in use (the caller's after rb_set_stream), its own, and the
// chain streams of rb_rollout_dev / rb_env_step_dev - drained; then the cached graph executables may go.
int drain(rb_sim *s) {
    RB_HIP(hipSetDevice(s->device));
    RB_HIP(hipStreamSynchronize(s->stream));
    if (s->own_stream && s->own_stream != s->stream) RB_HIP(hipStreamSynchronize(s->own_stream));
    for (int c = 1; c < rb_sim::MAX_CHAINS; ++c)
        if (s->chain_stream[c]) RB_HIP(hipStreamSynchronize(s->chain_stream[c]));
    // range launches on caller streams: the event behind the last one on each (the stream itself may be gone by now - an
    // event outlives its stream - so the EVENT is waited for, never the stream)
    for (rb_sim::CallerStream &c : s->caller)
        if (c.pending) { RB_HIP(hipEventSynchronize(c.done)); c.pending = false; }
    return RB_OK;
}
// Remember that a range launch has just been enqueued on `st`, a stream that is not one of the handle's own: record the
// entry's event behind it.  Not while `st` is being captured (the launch is a graph node then, not work in flight: whoever
// replays that graph keeps the handle alive meanwhile - roboy_sim.h).
int note_caller_stream(rb_sim *s, hipStream_t st) {
    if (st == s->stream || st == s->own_stream) return RB_OK;
    for (int c = 1; c < rb_sim::MAX_CHAINS; ++c) if (st == s->chain_stream[c] && st) return RB_OK;
    if (stream_capturing(st)) return RB_OK;
    rb_sim::CallerStream *slot = nullptr;
    for (rb_sim::CallerStream &c : s->caller) if (c.done && c.stream == st) { slot = &c; break; }
    if (!slot) {
        for (rb_sim::CallerStream &c : s->caller) if (!c.done) { slot = &c; break; }
        if (!slot) {                                   // every entry taken: the least recently used one is waited for and reused
            slot = &s->caller[0];
            for (rb_sim::CallerStream &c : s->caller) if (c.tick < slot->tick) slot = &c;
            if (slot->pending) { RB_HIP(hipEventSynchronize(slot->done)); slot->pending = false; }
        } else {
            // (completion is all drain() needs from it - not host visibility of the launch's writes: no system-scope fence on the
            // caller's stream behind every range launch, ~3 us each)
            RB_HIP(hipEventCreateWithFlags(&slot->done, chain_event_flags()));
        }
        slot->stream = st;
    }
    RB_HIP(hipEventRecord(slot->done, st));
    slot->pending = true;
    slot->tick = ++s->caller_tick;
    return RB_OK;
}
int drop_graphs(rb_sim *s) {
    if (s->graphs.empty()) return RB_OK;
    int rc = drain(s);                 // none may be in flight when destroyed
    if (rc) return rc;
    for (auto &kv : s->graphs) kv.second.destroy();
    s->graphs.clear();
    return RB_OK;
}

// a sub-range on a stream of the caller's choice: envs are independent, so disjoint ranges may be stepped concurrently
int range_ok(const rb_sim *s, int64_t first, int64_t count) {
    if (first < 0 || count < 1 || first + count > s->n) return fail(RB_EINVAL, "range outside the batch");
    if (first % 256) return fail(RB_EINVAL, "a range starts at a multiple of 256 envs");
    return RB_OK;
}

}  // namespace

#include "env_host.hpp"       // the fused env layer and its options on the host: launch arguments, rb_env_*, rb_params_*, the statistics

// ----------------------------------------------------------------------- C ABI
extern "C" {

const char *rb_last_error(void) { return g_err.c_str(); }
int rb_abi_version(void) { return RB_ABI_VERSION; }

int rb_device_count(int *count) {
    if (!count) return fail(RB_EINVAL, "count is null");
    *count = 0;
    RB_HIP(hipGetDeviceCount(count));
    return RB_OK;
}

int rb_create(const rb_robot_desc *robot, int64_t n_envs, int integrator, double step_size,
              int n_substeps, int device, uint64_t seed, int64_t env_id_offset, rb_sim **out) {
    if (!robot || !out) return fail(RB_EINVAL, "robot/out is null");
    *out = nullptr;
    if (n_envs < 1) return fail(RB_EINVAL, "n_envs must be >= 1");
    if (integrator != RB_EULER && integrator != RB_RK4) return fail(RB_EINVAL, "unknown integrator");
    if (!(step_size > 0.0) || n_substeps < 1) return fail(RB_EINVAL, "step_size must be > 0 and n_substeps >= 1");
    if (robot->n_q < 1 || robot->n_q > 32 || robot->n_t < 1) return fail(RB_EINVAL, "n_q must be in [1, 32], n_t >= 1");
    if (n_envs > (int64_t(1) << 30)) return fail(RB_EINVAL, "n_envs too large");
    if (env_id_offset < 0) return fail(RB_EINVAL, "env_id_offset must be >= 0");

    rb_sim *s = new (std::nothrow) rb_sim();
    if (!s) return fail(RB_ENOMEM, "out of host memory");
    std::string why;
    int rc = rb::msj_build<float, NT8>(robot, step_size, n_substeps, &s->c8, why);
    if (rc == RB_OK) {
        // bit-for-bit equal to the baked table?  (field by field: the struct has alignment padding)
        const Const8 &a = s->c8, &b = rbk::BAKED_HOST;
        auto same = [](const float *x, const float *y, int n) { return std::memcmp(x, y, sizeof(float) * size_t(n)) == 0; };
        bool eq = same(a.IO, b.IO, 6) && same(a.mc, b.mc, 3) && same(a.g, b.g, 3) && same(a.arm, b.arm, 3) && same(a.damp, b.damp, 3) &&
                  same(a.qlo, b.qlo, 3) && same(a.qhi, b.qhi, 3) && same(a.qdmax, b.qdmax, 3) && same(&a.kps, &b.kps, 8) &&
                  a.nsub == b.nsub && a.simple == b.simple && a.nt == b.nt;
        for (int k = 0; k < NT8 && eq; ++k) eq = same(a.ten[k].A, b.ten[k].A, 16);
        s->baked = eq;
        s->pair_ok = rb::find_mirror_pairs(s->c8, s->pair_mirror, s->pair_half, s->pair_image);
        if (s->pair_ok) {
            s->c8p = s->c8;
            bool first_four = true;
            for (int k = 0; k < 4; ++k) { s->c8p.ten[k] = s->c8.ten[s->pair_half[k]]; first_four = first_four && s->pair_half[k] == k; }
            s->pair_baked = s->baked && first_four;      // the BK instances read BAKED.ten[0..3]
        }
    }
    if (rc == RB_EUNSUPPORTED && robot->n_t != NT8) {
        // a ball-joint robot with another tendon count: same closed form, run-time count
        std::string why_x;
        if (rb::msj_build<float, NTX>(robot, step_size, n_substeps, &s->cx, why_x, /*exact=*/false) == RB_OK) {
            s->ntx = true;
            rc = RB_OK;
        }
    }
    if (rc == RB_EUNSUPPORTED) {
        // not a ball-joint robot: the generic joint-tree kernel (one env per wave)
        std::string why_tree;
        rc = rbt::tree_build(robot, step_size, n_substeps, s->tree_host, why_tree);
        if (rc == RB_OK) {
            s->tree = true;
            // the generated forms (the lean two-part form only for robots the five-wave form serves) ...
            for (int f = 0; f < rblg::N_FORMS; ++f) {
                std::string why_gen;
                s->forms[f].ok = (f != rblg::FORM_SPLIT2 || s->forms[rblg::FORM_SPLIT].ok) &&
                                 rblg::generate_form(robot, f, s->forms[f].gen, why_gen) == RB_OK;
            }
            // ... and which of them the ahead-of-time instances serve: the text they were compiled from, in the layout the launch
            // asks LDS for (less LDS than the kernels lay out would be written past)
            rblj::TreeForm &lane = s->forms[rblg::FORM_LANE], &split = s->forms[rblg::FORM_SPLIT], &split2 = s->forms[rblg::FORM_SPLIT2];
            lane.baked = lane.ok && lane.gen.hash == RBL_TEXT_HASH && lane.gen.lds == size_t(rbl_baked::LDS_BYTES_PER_WAVE);
            split.baked = split.ok && split.gen.hash == RBL_SPLIT_TEXT_HASH && split.gen.n_parts == RBL_NPARTS &&
                          split.gen.n_helpers == RBL_NHELPERS && split.gen.lds == size_t(rbl_split_baked::SP_LDS_BYTES);
            // (the lean form's instances are the second translation unit's: its text and layout are asked for)
            split2.baked = split2.ok && robot->n_q == rbs2::n_q() && robot->n_t == rbs2::n_t() && split2.gen.hash == rbs2::text_hash() &&
                           split2.gen.n_parts == rbs2::n_parts() && split2.gen.lds == rbs2::lds_bytes();
        }
        else why = "not a ball-joint robot (" + why + ") and not a supported joint tree (" + why_tree + ")";
    }
    if (rc != RB_OK) {
        delete s;
        return fail(rc, "no HIP kernel for this robot structure: " + why);
    }
    if (s->tree) rbt::tree_tendon_lconst(robot, s->ts_tree_lconst);
    else rb::msj_tendon_units(robot, s->ts_units.u, NTX);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1) {
        delete s;
        return fail(RB_EHIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    }
    if (device < 0 || device >= count) { delete s; return fail(RB_EINVAL, "device index out of range"); }
    s->device = device; s->n = n_envs; s->n_q = robot->n_q; s->n_t = robot->n_t;
    s->integrator = integrator; s->nsub = n_substeps; s->step_size = step_size;
    s->seed = seed; s->env0 = env_id_offset;
    for (int j = 0; j < s->n_q; ++j) { s->box.lo[j] = float(robot->q_lo[j]); s->box.hi[j] = float(robot->q_hi[j]); s->qd_max[j] = float(robot->qd_max[j]); }

#define RB_TRY(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            std::string m_ = std::string(#call) + ": " + hipGetErrorString(e_);           \
            rb_destroy(s);                                                                \
            return fail(e_ == hipErrorOutOfMemory ? RB_ENOMEM : RB_EHIP, m_);             \
        }                                                                                 \
    } while (0)
    RB_TRY(hipSetDevice(device));
    {
        hipDeviceProp_t prop;
        RB_TRY(hipGetDeviceProperties(&prop, device));
        s->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    RB_TRY(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    s->stream = s->own_stream;
    const size_t plane = sizeof(float) * size_t(n_envs);
    RB_TRY(hipMalloc(&s->d_q, plane * s->n_q));
    RB_TRY(hipMalloc(&s->d_qd, plane * s->n_q));
    RB_TRY(hipMalloc(&s->d_feas, sizeof(uint32_t) * size_t(n_envs)));
    RB_TRY(hipMalloc(&s->d_goal_count, sizeof(uint32_t) * size_t(n_envs)));
    const int width = s->n_q > s->n_t ? s->n_q : s->n_t;
    RB_TRY(hipMalloc(&s->d_rows, plane * width));
    RB_TRY(hipMalloc(&s->d_u8, size_t(n_envs)));
    RB_TRY(hipMalloc(&s->d_state_rows, plane * (2 * s->n_q + 1)));   // q rows | qd rows | n bytes
    RB_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->h_state_rows), plane * (2 * s->n_q + 1), hipHostMallocDefault));
    if (!s->tree) {
        RB_TRY(hipMalloc(&s->d_ten, sizeof(s->c8.ten)));
        RB_TRY(hipMemcpyAsync(s->d_ten, s->c8.ten, sizeof(s->c8.ten), hipMemcpyHostToDevice, s->stream));
    } else {
        rbt::TreeHost &th = s->tree_host;
        RB_TRY(hipMalloc(&s->d_tree_words, sizeof(uint32_t) * th.words.size()));
        RB_TRY(hipMemcpy(s->d_tree_words, th.words.data(), sizeof(uint32_t) * th.words.size(), hipMemcpyHostToDevice));
        th.dev.g_words = reinterpret_cast<const float4 *>(s->d_tree_words);
        if (rbt::tree_lds_bytes(th, 1) > 160 * 1024) {
            rb_destroy(s);
            return fail(RB_EUNSUPPORTED, "robot working set exceeds the 160 KiB LDS of a CU");
        }
        s->tree_waves = rbt::tree_pick_waves(th);
        // more than 64 KiB of dynamic LDS per workgroup has to be granted per kernel
        const int lds_max = 160 * 1024;
#define RB_TREE_ATTR(K) RB_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max))
        RB_TREE_ATTR((rbt::tree_step_aba<0, rbt::TREE_E, true>)); RB_TREE_ATTR((rbt::tree_step_aba<1, rbt::TREE_E, true>));
        RB_TREE_ATTR((rbt::tree_step_aba<0, rbt::TREE_E, false>)); RB_TREE_ATTR((rbt::tree_step_aba<1, rbt::TREE_E, false>));
        RB_TREE_ATTR((rbt::tree_env_step_aba<0, rbt::TREE_E, true>)); RB_TREE_ATTR((rbt::tree_env_step_aba<1, rbt::TREE_E, true>));
        RB_TREE_ATTR((rbt::tree_env_step_aba<0, rbt::TREE_E, false>)); RB_TREE_ATTR((rbt::tree_env_step_aba<1, rbt::TREE_E, false>));
        RB_TREE_ATTR((rbt::tree_tendon_state<rbt::TREE_E, true>)); RB_TREE_ATTR((rbt::tree_tendon_state<rbt::TREE_E, false>));
        RB_TREE_ATTR((rbt::tree_shaping_cost<rbt::TREE_E, true>)); RB_TREE_ATTR((rbt::tree_shaping_cost<rbt::TREE_E, false>));
        RB_TRY(hipMalloc(&s->d_ts_lconst, sizeof(float) * s->ts_tree_lconst.size()));
        RB_TRY(hipMemcpy(s->d_ts_lconst, s->ts_tree_lconst.data(), sizeof(float) * s->ts_tree_lconst.size(), hipMemcpyHostToDevice));
        if (s->form(RB_KERNEL_ENV_PER_LANE_SPLIT).baked) {
            RB_TREE_ATTR(rbl_split_baked::tree_split_step<0>); RB_TREE_ATTR(rbl_split_baked::tree_split_step<1>);
            RB_TREE_ATTR(rbl_split_baked::tree_split_env_step<0>); RB_TREE_ATTR(rbl_split_baked::tree_split_env_step<1>);
        }
#undef RB_TREE_ATTR
    }
    RB_TRY(hipMemsetAsync(s->d_goal_count, 0, sizeof(uint32_t) * size_t(n_envs), s->stream));
    RB_TRY(hipMalloc(&s->d_infeas_n, sizeof(uint32_t) * size_t(n_envs)));
    RB_TRY(hipMemsetAsync(s->d_infeas_n, 0, sizeof(uint32_t) * size_t(n_envs), s->stream));
    RB_TRY(hipMalloc(&s->d_stats, sizeof(double) * 8 * (STATS_BLOCKS + 2)));
    RB_TRY(hipMemsetAsync(s->d_stats, 0, sizeof(double) * 8 * (STATS_BLOCKS + 2), s->stream));
#undef RB_TRY
    *out = s;
    (void)rb_select_kernel(s, RB_KERNEL_AUTO);
    rc = rb_reset(s, nullptr);
    if (rc != RB_OK) { std::string m = g_err; rb_destroy(s); *out = nullptr; return fail(rc, m); }
    return RB_OK;
}

void rb_destroy(rb_sim *s) {
    if (!s) return;
    // whichever stream is in use (a caller's after rb_set_stream - it must still exist), the handle's own and the chain
    // streams: nothing of this handle may be in flight when its graph executables, streams and buffers go
    (void)drain(s);
    for (auto &kv : s->graphs) kv.second.destroy();
    rbj::unload(s->jit);
    for (rblj::TreeForm &f : s->forms) rblj::unload(f);
    (void)hipFree(s->d_q); (void)hipFree(s->d_qd); (void)hipFree(s->d_feas);
    (void)hipFree(s->d_goal_count); (void)hipFree(s->d_rows); (void)hipFree(s->d_u8); (void)hipFree(s->d_ten);
    (void)hipFree(s->d_tree_words); (void)hipFree(s->d_ts_lconst); (void)hipFree(s->d_ts_out);
    (void)hipFree(s->d_state_rows); (void)hipHostFree(s->h_state_rows);
    (void)hipFree(s->d_goal); (void)hipFree(s->d_ep_ret); (void)hipFree(s->d_ep_sum); (void)hipFree(s->d_ep_cnt);
    (void)hipFree(s->d_step_num); (void)hipFree(s->d_infeas_n); (void)hipFree(s->d_stats);
    s->par.release(); s->chan.release(); s->io.release(); s->hist.release(); s->done.release(); s->critic.release(); s->goals.release(); s->shaping.release(); s->push.release(); s->elog.release(); s->start.release();
    for (rb_sim::CallerStream &c : s->caller) if (c.done) (void)hipEventDestroy(c.done);
    if (s->chain_fork) (void)hipEventDestroy(s->chain_fork);
    for (int c = 1; c < rb_sim::MAX_CHAINS; ++c) {
        if (s->chain_join[c]) (void)hipEventDestroy(s->chain_join[c]);
        if (s->chain_stream[c]) (void)hipStreamDestroy(s->chain_stream[c]);
    }
    if (s->own_stream) (void)hipStreamDestroy(s->own_stream);
    delete s;
}

int rb_info(const rb_sim *s, rb_sim_info *info) {
    if (check(s) || !info) return fail(RB_EINVAL, "null argument");
    info->n_envs = s->n; info->n_q = s->n_q; info->n_t = s->n_t;
    info->integrator = s->integrator; info->n_substeps = s->nsub; info->kernel = s->kernel;
    info->device = s->device; info->step_size = s->step_size;
    info->bytes_per_env_step = 4 * (4 * int64_t(s->n_q) + s->n_t + 1);
    info->env_id_offset = s->env0;
    return RB_OK;
}

#ifdef RB_TREE_DEBUG
// debug builds only: arm a dump of the LDS working set of the wave that owns `env` (joint-tree robots; filled by
// the next rb_step*), then fetch it.  Layout: TREE_E blocks of dev.ES floats (tree_build.hpp); *dev_out gets the
// table offsets.
int rb_debug_tree_arm(rb_sim *s, long env) {
    if (!s || !s->tree) return fail(RB_EINVAL, "not a joint-tree handle");
    RB_HIP(hipSetDevice(s->device));
    float *buf = nullptr;
    const size_t nf = size_t(rbt::TREE_E) * s->tree_host.dev.ES;
    RB_HIP(hipMalloc(&buf, nf * sizeof(float)));
    RB_HIP(hipMemset(buf, 0, nf * sizeof(float)));
    RB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rbt::rb_tree_dbg_out), &buf, sizeof(buf)));
    RB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rbt::rb_tree_dbg_env), &env, sizeof(env)));
    return RB_OK;
}
int rb_debug_tree_fetch(rb_sim *s, float *out, int n_floats, rbt::TreeDev *dev_out) {
    if (!s || !s->tree) return fail(RB_EINVAL, "not a joint-tree handle");
    RB_HIP(hipSetDevice(s->device));
    RB_HIP(hipStreamSynchronize(s->stream));
    float *buf = nullptr;
    RB_HIP(hipMemcpyFromSymbol(&buf, HIP_SYMBOL(rbt::rb_tree_dbg_out), sizeof(buf)));
    if (!buf) return fail(RB_EINVAL, "not armed");
    const int nf = rbt::TREE_E * s->tree_host.dev.ES;
    RB_HIP(hipMemcpy(out, buf, sizeof(float) * size_t(n_floats < nf ? n_floats : nf), hipMemcpyDeviceToHost));
    if (dev_out) *dev_out = s->tree_host.dev;
    float *none = nullptr;
    RB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rbt::rb_tree_dbg_out), &none, sizeof(none)));
    (void)hipFree(buf);
    return RB_OK;
}
#endif

#ifdef RB_SPLIT_STAMPS
// diagnostic builds only: the barrier stamps of the split kernels' workgroup 0 (tree_lane_defs.hpp), 8 waves x 128 entries
extern "C" int rb_debug_stamps(unsigned long long *out) {
    RB_HIP(hipDeviceSynchronize());
    RB_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rbl_stamp_buf), sizeof(unsigned long long) * 8 * 128));
    return RB_OK;
}
#endif

#ifdef RB_LANE_STAMPS
// diagnostic builds only: the phase stamps of the one-wave joint-tree kernels (tree_lane.hpp), RBL_STAMP_WAVES waves x 4 x (100 MHz clock, shader clock)
extern "C" int rb_debug_lane_stamps(unsigned long long *out, int n_words) {
    RB_HIP(hipDeviceSynchronize());
    const size_t all = sizeof(unsigned long long) * RBL_STAMP_WAVES * 8, want = sizeof(unsigned long long) * size_t(n_words);
    RB_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rbl_baked::rbl_lane_stamp_buf), want < all ? want : all));
    return RB_OK;
}
#endif

void rb_jit_cache_stats(int64_t *hits, int64_t *compiles, int64_t *stores) {
    rbj::CacheStats &c = rbj::cache_stats();
    if (hits) *hits = c.hits.load();
    if (compiles) *compiles = c.compiles.load();
    if (stores) *stores = c.stores.load();
}

int rb_specialization(rb_sim *s) {
    if (check(s)) return -1;
    if (s->tree) {
        const int form = tree_wants_split(s, F_SPLIT2) ? F_SPLIT2 : tree_wants_split(s, F_SPLIT) ? F_SPLIT : F_LANE;
        if (form == F_LANE && !tree_wants_lane(s)) {
            g_err = s->form(F_LANE).ok ? "the octet kernels are selected (batch below the build threshold, or by choice)" : "no generator for this robot";
            return RB_SPEC_NONE;
        }
        if (s->form(form).baked) return RB_SPEC_TABLE;
        if (tree_form_ready(s, form, 0, true)) return RB_SPEC_JIT;
        g_err = s->form(form).step.why;
        return RB_SPEC_NONE;
    }
    if (s->baked) return RB_SPEC_TABLE;
    if (s->jit_state == 0) maybe_jit(s);
    if (s->jit_state == 1) return RB_SPEC_JIT;
    if (!s->jit_why.empty()) g_err = s->jit_why;
    return RB_SPEC_NONE;
}

int rb_select_kernel(rb_sim *s, int kernel) {
    if (check(s)) return RB_EINVAL;
    // validate first: a refused request leaves the handle as it was (kernel_choice, rb_info, the graph cache)
    if (kernel < RB_KERNEL_AUTO || kernel > RB_KERNEL_ENV_PER_LANE_SPLIT2) return fail(RB_EINVAL, "unknown kernel variant");
    const bool generated = kernel == RB_KERNEL_ENV_PER_LANE || kernel == RB_KERNEL_ENV_PER_LANE_SPLIT || kernel == RB_KERNEL_ENV_PER_LANE_SPLIT2;
    if ((kernel == RB_KERNEL_ENV_PER_LANE_SPLIT || kernel == RB_KERNEL_ENV_PER_LANE_SPLIT2) && !(s->tree && s->form(kernel).ok))
        return fail(RB_EUNSUPPORTED, "no split form for this robot (a ball-joint robot, a serial chain, or branches tied together by tendons)");
    if (kernel == RB_KERNEL_LANE_PAIR && !(s->pair_ok && !s->tree && !s->ntx))
        return fail(RB_EUNSUPPORTED, "the two-lanes-per-env form needs an 8-tendon ball-joint robot with a mirror plane (tendons in mirror-image pairs, "
                                     "principal-axis inertia, symmetric joint limits)");
    if (s->tree) {
        if (kernel == RB_KERNEL_TENDON_PER_LANE) return fail(RB_EUNSUPPORTED, "joint-tree robots have no tendon-per-lane kernel");
        if (kernel == RB_KERNEL_ENV_PER_LANE && !s->form(kernel).ok) return fail(RB_EUNSUPPORTED, "no env-per-lane kernel can be generated for this robot");
        const int before = s->kernel_choice;
        s->kernel_choice = kernel;           // tree_wants_*() read it; restored on every failure below
        if (generated && !s->form(kernel).baked) {
            // an explicit choice of a generated form builds its step kernel now (and fails loudly if that is not possible)
            static const char *const NAME[rblg::N_FORMS] = {"env-per-lane kernel", "split-form kernel", "lean split-form kernel"};
            static const char *const CAPTURED[rblg::N_FORMS] = {"the env-per-lane kernels cannot be built during a stream capture",
                                                                "the split-form kernel cannot be built during a stream capture",
                                                                "the lean split-form kernel cannot be built during a stream capture"};
            const int f = rb_sim::form_index(kernel);
            if (capturing(s)) { s->kernel_choice = before; return fail(RB_EINVAL, CAPTURED[f]); }
            if (!tree_form_ready(s, kernel, 0, true)) {
                s->kernel_choice = before;
                return fail(RB_EUNSUPPORTED, std::string(NAME[f]) + " not available: " + s->form(kernel).step.why);
            }
        }
        int rc = drop_graphs(s);             // graphs captured with another variant must not be replayed
        if (rc) { s->kernel_choice = before; return rc; }
        { const int form = resolve_form(s, ENTRY_STEP, /*build=*/false, nullptr); s->kernel = form > 0 ? form : RB_KERNEL_ENV_PER_WAVE; }
        return RB_OK;
    }
    if (kernel == RB_KERNEL_ENV_PER_WAVE) return fail(RB_EUNSUPPORTED, "ball-joint robots have no env-per-wave kernel");
    if (s->ntx && kernel == RB_KERNEL_TENDON_PER_LANE)    // 8 lanes per env is the 8-tendon form
        return fail(RB_EUNSUPPORTED, "the tendon-per-lane kernel is built for 8 tendons");
    int rc = drop_graphs(s);
    if (rc) return rc;
    s->kernel_choice = kernel;
    if (s->ntx) { s->kernel = RB_KERNEL_ENV_PER_LANE; return RB_OK; }
    s->kernel = kernel != RB_KERNEL_AUTO ? kernel : auto_form(s, ENTRY_STEP);
    return RB_OK;
}

int rb_mirror_info(const rb_sim *s, int32_t *plane, int32_t *joint_sign, int32_t *tendon_image) {
    if (check(s) || !plane || !joint_sign || !tendon_image) return fail(RB_EINVAL, "null argument");
    // what rb_create found in the robot's constants (find_mirror_pairs), whatever kernel form steps the handle
    if (s->tree || s->ntx || !s->pair_ok)
        return fail(RB_EUNSUPPORTED, "this robot has no mirror plane (an 8-tendon ball-joint robot with its tendons in mirror-image pairs, "
                                     "principal-axis inertia and symmetric joint limits has one)");
    *plane = s->pair_mirror;
    // the two joints whose axes lie in the mirror plane change sign (find_mirror_pairs' f0, f1): x-z (-1, +1, -1), y-z (+1, -1, -1)
    for (int j = 0; j < 3; ++j) joint_sign[j] = (j == 2 || j == s->pair_mirror) ? -1 : 1;
    for (int k = 0; k < 4; ++k) {
        tendon_image[s->pair_half[k]] = s->pair_image[k];
        tendon_image[s->pair_image[k]] = s->pair_half[k];
    }
    return RB_OK;
}

int rb_set_stream(rb_sim *s, void *hip_stream) {
    if (check(s)) return RB_EINVAL;
    { int rc = drain(s); if (rc) return rc; }                            // the previous stream and the chain streams
    if (hip_stream == RB_STREAM_DEVICE_DEFAULT) s->stream = nullptr;     // the null stream
    else s->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->own_stream;
    return RB_OK;
}

int rb_synchronize(rb_sim *s) {
    if (check(s)) return RB_EINVAL;
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

int rb_reset(rb_sim *s, const uint8_t *mask) {
    if (check(s)) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    const uint8_t *d_mask = nullptr;
    if (mask) {
        RB_HIP(hipMemcpyAsync(s->d_u8, mask, size_t(s->n), hipMemcpyHostToDevice, s->stream));
        d_mask = s->d_u8;
    }
    hipLaunchKernelGGL(reset_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                       s->d_q, s->d_qd, s->d_feas, d_mask, s->n_q, s->n, s->tree ? 1 : 0);
    RB_HIP(hipGetLastError());
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

int rb_set_state(rb_sim *s, const float *q, const float *qd, const uint8_t *feasible) {
    if (check(s) || !q || !qd) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    const long n = s->n;
    const unsigned g = blocks_for(n, 256);
    RB_HIP(hipMemcpyAsync(s->d_rows, q, sizeof(float) * n * s->n_q, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(g), dim3(256), 0, s->stream, s->d_rows, s->d_q, s->n_q, n, s->tree ? 1 : 0);
    RB_HIP(hipStreamSynchronize(s->stream));
    RB_HIP(hipMemcpyAsync(s->d_rows, qd, sizeof(float) * n * s->n_q, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(g), dim3(256), 0, s->stream, s->d_rows, s->d_qd, s->n_q, n, s->tree ? 1 : 0);
    const uint8_t *d_f = nullptr;
    if (feasible) {
        RB_HIP(hipMemcpyAsync(s->d_u8, feasible, size_t(n), hipMemcpyHostToDevice, s->stream));
        d_f = s->d_u8;
    }
    hipLaunchKernelGGL(feas_from_u8_kernel, dim3(g), dim3(256), 0, s->stream, d_f, s->d_feas, n);
    RB_HIP(hipGetLastError());
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

int rb_read_state(rb_sim *s, float *q, float *qd, uint8_t *feasible) {
    if (check(s)) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    return read_state_host(s, q, qd, feasible);
}

int rb_step(rb_sim *s, const float *act, float act_scale, float *q, float *qd, uint8_t *feasible) {
    if (check(s) || !act) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    maybe_jit(s);
    RB_HIP(hipMemcpyAsync(s->d_rows, act, sizeof(float) * s->n * s->n_t, hipMemcpyHostToDevice, s->stream));
    int rc = launch_step(s, s->d_rows, act_scale);
    if (rc) return rc;
    s->env_steps += double(s->n);
    return read_state_host(s, q, qd, feasible);
}

int rb_sample_goals(rb_sim *s, const uint8_t *mask, float *goal_q) {
    if (check(s) || !goal_q) return fail(RB_EINVAL, "null argument");
    if (s->goals.L) return curriculum_refuse_sample(s);
    RB_HIP(hipSetDevice(s->device));
    const uint8_t *d_mask = nullptr;
    if (mask) {
        RB_HIP(hipMemcpyAsync(s->d_u8, mask, size_t(s->n), hipMemcpyHostToDevice, s->stream));
        d_mask = s->d_u8;
    }
    if (mask) RB_HIP(hipMemsetAsync(s->d_rows, 0, sizeof(float) * s->n * s->n_q, s->stream));
    if (s->goals.d_pool)
        hipLaunchKernelGGL(rbg::goal_pool_sample_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->goals.d_pool,
                           uint32_t(s->goals.m), s->d_rows, s->d_goal_count, d_mask, s->n_q, s->n, s->seed, uint64_t(s->env0), 1);
    else
        hipLaunchKernelGGL(sample_goals_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                           s->d_rows, s->d_goal_count, d_mask, s->box, s->n_q, s->n, s->seed, uint64_t(s->env0), 1);
    RB_HIP(hipGetLastError());
    RB_HIP(hipMemcpyAsync(goal_q, s->d_rows, sizeof(float) * s->n * s->n_q, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

int rb_state_ptrs(rb_sim *s, float **d_q, float **d_qd, uint32_t **d_feasible) {
    if (check(s)) return RB_EINVAL;
    if (d_q) *d_q = s->d_q;
    if (d_qd) *d_qd = s->d_qd;
    if (d_feasible) *d_feasible = s->d_feas;
    return RB_OK;
}

int rb_step_dev(rb_sim *s, const float *d_act, float act_scale) {
    if (check(s) || !d_act) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (reinterpret_cast<uintptr_t>(d_act) % 16) return fail(RB_EINVAL, "action slab must be 16-byte aligned");
    maybe_jit(s);
    s->env_steps += double(s->n);
    return launch_step(s, d_act, act_scale);
}

int rb_rollout_dev(rb_sim *s, const float *d_ring, int ring, int n_steps, float act_scale, int use_graph) {
    if (check(s) || !d_ring) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (ring < 1 || n_steps < 0) return fail(RB_EINVAL, "ring must be >= 1 and n_steps >= 0");
    if (reinterpret_cast<uintptr_t>(d_ring) % 16) return fail(RB_EINVAL, "action ring must be 16-byte aligned");
    maybe_jit(s);                    // before any capture below
    const size_t slab = size_t(s->n) * s->n_t;
    const int chains = use_graph ? rollout_chains(s) : 1;
    if (use_graph && n_steps >= 8 && !s->stream) return fail(RB_EINVAL, "hipGraph capture needs a non-default stream (rb_set_stream)");
    // chain c steps envs [lo_c, lo_{c+1}) (cuts at multiples of 256) on its own stream (chain 0: the handle's)
    long lo[rb_sim::MAX_CHAINS + 1];
    for (int c = 0; c <= chains; ++c) lo[c] = c == chains ? s->n : (chains == 1 ? 0 : ((s->n * c / chains + 255) / 256) * 256);
    auto chain_stream = [&](int c) { return c ? s->chain_stream[c] : s->stream; };
    bool forked = false;
    auto fork = [&]() -> int {       // the further chains start behind everything the handle's stream holds so far
        if (chains == 1 || forked) return RB_OK;
        if (!s->chain_fork) RB_HIP(hipEventCreateWithFlags(&s->chain_fork, chain_event_flags()));
        for (int c = 1; c < chains; ++c)
            if (!s->chain_stream[c]) {
                RB_HIP(hipStreamCreateWithFlags(&s->chain_stream[c], hipStreamNonBlocking));
                RB_HIP(hipEventCreateWithFlags(&s->chain_join[c], chain_event_flags()));
            }
        // (a stream that reports everything done has nothing for the chains to wait for: saves the two calls' ~5 us of host time in
        // front of the first launch of a short rollout)
        if (capturing(s) || hipStreamQuery(s->stream) != hipSuccess) {
            RB_HIP(hipEventRecord(s->chain_fork, s->stream));
            for (int c = 1; c < chains; ++c) if (lo[c + 1] > lo[c]) RB_HIP(hipStreamWaitEvent(s->chain_stream[c], s->chain_fork, 0));
        }
        (void)hipGetLastError();         // hipErrorNotReady from the query is not an error
        forked = true;
        return RB_OK;
    };
    auto join = [&]() -> int {       // ... and the handle's stream continues behind all of them
        if (!forked) return RB_OK;
        for (int c = 1; c < chains; ++c)
            if (lo[c + 1] > lo[c]) {
                RB_HIP(hipEventRecord(s->chain_join[c], s->chain_stream[c]));
                RB_HIP(hipStreamWaitEvent(s->stream, s->chain_join[c], 0));
            }
        forked = false;
        return RB_OK;
    };
    int t = 0;
    // An eager head in front of the graphs (large batches whose step kernel outlasts a host-side launch): replaying a graph
    // costs ~10 us between the call and its first kernel, and the second chain's graph is launched after the first one's - a
    // 20-step rollout of the headline batch lost 38 us to that (13.9 instead of 12.0 us per step, profiles/r4_a).  One ring
    // turn of plain launches, the chains taking turns, has the device busy after ~4 us; the graphs are enqueued behind them
    // while they run.  The same kernels on the same streams: nothing changes in the results.
    if (use_graph && rollout_eager_head(s, chains) && n_steps >= ring + 8 && ring <= 8) {
        int rc = fork();
        for (int k = 0; k < ring && rc == RB_OK; ++k)
            for (int c = chains - 1; c >= 0 && rc == RB_OK; --c)      // the further chains first (below)
                if (lo[c + 1] > lo[c])
                    rc = chains == 1 ? launch_step(s, d_ring + size_t(k) * slab, act_scale)
                                     : launch_step(s, d_ring + size_t(k) * slab, act_scale, lo[c], lo[c + 1], chain_stream(c));
        if (rc) return rc;
        t = ring;
    }
    // graphs of up to 128 per-step kernel nodes, each a whole number of ring turns (so every
    // graph starts at ring slot 0); what is left over (< 8 steps or a partial turn) is launched eagerly
    while (use_graph) {
        const int left = n_steps - t;
        const int chunk = ((left < 128 ? left : 128) / ring) * ring;
        if (chunk < 8) break;
        rb_sim::GraphKey key;
        std::memset(&key, 0, sizeof(key));
        key.ring_ptr = d_ring; key.ring = ring; key.chunk = chunk; key.scale = act_scale; { const Row *row = row_for(s, ENTRY_STEP, true); key.kernel = (row ? int(row - TABLE) : 0xffff) | (chains << 16); }
        auto it = s->graphs.find(key);
        if (it == s->graphs.end()) {
            { int rc = fork(); if (rc) return rc; }     // creates the chain streams
            // one LINEAR graph of `chunk` launches per chain, captured on the chain's own stream.  (One graph with parallel
            // branches is replayed badly - its second branch starts late: 16.2 us per step in a 20-step region against 13.9 for two
            // linear graphs on two streams.)
            rb_sim::ChainGraphs cg;
            cg.chains = chains;
            for (int c = 0; c < chains; ++c) {
                if (lo[c + 1] <= lo[c]) continue;
                hipStream_t st = chain_stream(c);
                hipGraph_t graph = nullptr;
                hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
                if (e != hipSuccess) { cg.destroy(); return fail(RB_EHIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e)); }
                int rc = RB_OK;
                for (int k = 0; k < chunk && rc == RB_OK; ++k) {
                    const float *slab_k = d_ring + size_t(k % ring) * slab;
                    rc = chains == 1 ? launch_step(s, slab_k, act_scale) : launch_step(s, slab_k, act_scale, lo[c], lo[c + 1], st);
                }
                e = hipStreamEndCapture(st, &graph);
                if (rc != RB_OK) { if (graph) (void)hipGraphDestroy(graph); cg.destroy(); return rc; }
                if (e != hipSuccess) { cg.destroy(); return fail(RB_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e)); }
                e = hipGraphInstantiate(&cg.exec[c], graph, nullptr, nullptr, 0);
                (void)hipGraphDestroy(graph);
                if (e != hipSuccess) { cg.destroy(); return fail(RB_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
            }
            if (s->graphs.size() >= 16) {   // bound the cache: callers that keep changing slabs get re-captures, not a leak
                int rc = drop_graphs(s);                   // a cached exec may still be in flight (launched by an earlier chunk, on any chain)
                if (rc) { cg.destroy(); return rc; }
                forked = false;                            // (drained: fork again below)
            }
            it = s->graphs.emplace(key, cg).first;
        }
        // all the chunks of this size: the chains replay their graphs back to back; they are joined once, at the end
        const rb_sim::ChainGraphs &cg = it->second;
        { int rc = fork(); if (rc) return rc; }
        // The further chains' graphs are launched FIRST: with the handle's stream first its chain ran ahead and the other one
        // finished 13 us behind it - a 20-step rollout of the headline batch took 308 us against 272 us in this order, where the
        // two chains end within 6 us of each other (tools/proto/region_timeline_probe.hip, profiles/r4_a/region_timeline.log)
        for (; t + chunk <= n_steps; t += chunk)
            for (int c = cg.chains - 1; c >= 0; --c)
                if (cg.exec[c]) RB_HIP(hipGraphLaunch(cg.exec[c], chain_stream(c)));
    }
    { int rc = join(); if (rc) return rc; }
    for (; t < n_steps; ++t) {
        int rc = launch_step(s, d_ring + size_t(t % ring) * slab, act_scale);
        if (rc) return rc;
    }
    s->env_steps += double(s->n) * n_steps;
    return RB_OK;
}

int rb_rollout_chains(rb_sim *s) {
    if (check(s)) return -1;
    maybe_jit(s);                    // (what rb_rollout_dev would build first)
    return rollout_chains(s);
}

int rb_set_rollout_chains(rb_sim *s, int chains) {
    if (check(s)) return RB_EINVAL;
    if (chains < 0 || chains > rb_sim::MAX_CHAINS) return fail(RB_EINVAL, "chains must be 0 (the library's choice) or 1..4");
    s->chains_choice = chains;      // (graphs are cached per chain count: nothing to drop)
    return RB_OK;
}

int rb_rollout_fused_dev(rb_sim *s, const float *d_ring, int ring, int n_steps, float act_scale) {
    if (check(s) || !d_ring) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (ring < 1 || n_steps < 0) return fail(RB_EINVAL, "ring must be >= 1 and n_steps >= 0");
    if (reinterpret_cast<uintptr_t>(d_ring) % 16) return fail(RB_EINVAL, "action ring must be 16-byte aligned");
    if (s->tree || s->ntx) return fail(RB_EUNSUPPORTED, "fused rollout is built for 8-tendon ball-joint robots");
    if (s->par.on) return params_refuse(s, "the fused rollout (rb_rollout_fused_dev)");
    if (s->shaping.on)
        return fail(RB_EUNSUPPORTED, "the fused rollout (rb_rollout_fused_dev) forms its rewards inside one kernel and cannot apply reward shaping "
                                     "(rb_env_shaping_configure(sim, NULL) first)");
    if (s->push.on)
        return fail(RB_EUNSUPPORTED, "the fused rollout (rb_rollout_fused_dev) steps inside one kernel and cannot apply random pushes "
                                     "(rb_env_push_configure(sim, NULL) first)");
    if (s->elog.E)
        return fail(RB_EUNSUPPORTED, "the fused rollout (rb_rollout_fused_dev) ends episodes inside one kernel and cannot record them in the episode log "
                                     "(rb_env_episode_log_configure(sim, 0) first)");
    if (s->goals.d_pool)
        return fail(RB_EUNSUPPORTED, "the fused rollout (rb_rollout_fused_dev) redraws goals inside one kernel and cannot draw them from a goal pool");
    if (s->start.d_pool)
        return fail(RB_EUNSUPPORTED, "the fused rollout (rb_rollout_fused_dev) resets episodes inside one kernel and cannot start them at poses from a pool "
                                     "(rb_env_start_poses_configure(sim, NULL, 0, 0) first)");
    if (n_steps == 0) return RB_OK;
    const long n = s->n;
    maybe_jit(s);
    Launch L;
    L.i0 = 0; L.cnt = n; L.stream = s->stream; L.act = d_ring; L.act_scale = act_scale; L.ring = ring; L.n_steps = n_steps;
    { int rc = dispatch(s, ENTRY_FUSED, L); if (rc) return rc; }
    s->env_steps += double(n) * n_steps;
    return RB_OK;
}

int rb_fill_actions_dev(rb_sim *s, float *d_act, uint32_t step) {
    if (check(s) || !d_act) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    hipLaunchKernelGGL(fill_actions_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                       d_act, s->n_t, s->n, s->seed, uint64_t(s->env0), step);
    RB_HIP(hipGetLastError());
    return RB_OK;
}

int rb_sample_goals_dev(rb_sim *s, const uint8_t *d_mask, float *d_goal_q) {
    if (check(s) || !d_goal_q) return fail(RB_EINVAL, "null argument");
    if (s->goals.L) return curriculum_refuse_sample(s);
    RB_HIP(hipSetDevice(s->device));
    if (s->goals.d_pool)
        hipLaunchKernelGGL(rbg::goal_pool_sample_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->goals.d_pool,
                           uint32_t(s->goals.m), d_goal_q, s->d_goal_count, d_mask, s->n_q, s->n, s->seed, uint64_t(s->env0), 0);
    else
        hipLaunchKernelGGL(sample_goals_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                           d_goal_q, s->d_goal_count, d_mask, s->box, s->n_q, s->n, s->seed, uint64_t(s->env0), 0);
    RB_HIP(hipGetLastError());
    return RB_OK;
}

int rb_step_range_dev(rb_sim *s, int64_t first_env, int64_t n_envs, void *hip_stream, const float *d_act, float act_scale) {
    if (check(s) || !d_act) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (reinterpret_cast<uintptr_t>(d_act) % 16) return fail(RB_EINVAL, "action slab must be 16-byte aligned");
    if (range_ok(s, first_env, n_envs)) return RB_EINVAL;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    CallStreamScope scope(s, st);          // a first call captured on the caller's stream defers the run-time builds (capturing())
    maybe_jit(s);
    // (a whole batch is taken by every form, on the caller's stream too; sub-ranges by the forms of rb_range_capable - dispatch() refuses others)
    int rc = launch_step(s, d_act, act_scale, long(first_env), long(first_env + n_envs), st);
    if (rc == RB_OK) { s->env_steps += double(n_envs); rc = note_caller_stream(s, st); }
    return rc;
}
int rb_range_capable(rb_sim *s) {
    if (check(s)) return -1;
    // builds what a launch would build (outside captures), then asks the table - or the extension kernels, which take sub-ranges:
    // bit 0 = the step, bit 1 = the env step
    maybe_jit(s);
    auto ranges = [s](int entry, bool build) {
        if (extension_serves(s, entry)) return true;
        const Row *r = row_for(s, entry, build);
        return r && r->ranges;
    };
    return (ranges(ENTRY_STEP, true) ? 1 : 0) | (ranges(ENTRY_ENV, s->env_ready) ? 2 : 0);
}

// ---- tendon state readout (tendon_state.hpp): one kernel per robot class, not a row of the dispatch table ----
namespace {
int tendon_state_check(rb_sim *s, const float *act, int mode, float act_scale) {
    if (check(s)) return RB_EINVAL;
    if (s->par.on) return params_refuse(s, "the tendon-state readout (rb_tendon_state_dev)");
    if (mode != RB_SP_SCALED && mode != RB_SP_ENV) return fail(RB_EINVAL, "unknown set-point mode (RB_SP_SCALED or RB_SP_ENV)");
    if (mode == RB_SP_ENV && !s->env_ready) return fail(RB_EINVAL, "RB_SP_ENV needs the env layer's action box: call rb_env_configure first");
    if (mode == RB_SP_SCALED && act && !(act_scale > 0.0f)) return fail(RB_EINVAL, "act_scale must be > 0 under RB_SP_SCALED");
    return RB_OK;
}

int tendon_state_launch(rb_sim *s, const float *d_act, int mode, float act_scale, const rbts::Outputs &out) {
    const rbts::SetPoints sp{d_act, mode, act_scale, mode == RB_SP_ENV ? s->env.slope : 0.0f, mode == RB_SP_ENV ? s->env.act_hi : 0.0f};
    const long n = s->n;
    constexpr int BLOCK = 256;
    if (s->tree) {
        const int wv = s->tree_waves;
        const size_t lds = rbt::tree_lds_bytes(s->tree_host, wv);
        const long per_block = long(wv) * rbt::TREE_E;
        const unsigned blocks = unsigned((n + per_block - 1) / per_block);
        if (s->tree_host.dev.single_pass)
            hipLaunchKernelGGL((rbt::tree_tendon_state<rbt::TREE_E, true>), dim3(blocks), dim3(64 * wv), lds, s->stream, s->tree_host.dev,
                               s->d_ts_lconst, s->d_q, s->d_qd, sp, out, n);
        else
            hipLaunchKernelGGL((rbt::tree_tendon_state<rbt::TREE_E, false>), dim3(blocks), dim3(64 * wv), lds, s->stream, s->tree_host.dev,
                               s->d_ts_lconst, s->d_q, s->d_qd, sp, out, n);
    } else if (s->ntx) {
        hipLaunchKernelGGL(rbts::msj_tendon_state_nt<BLOCK>, dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, s->stream, s->cx, s->ts_units,
                           s->d_q, s->d_qd, sp, out, n);
    } else {
        rbts::Units<NT8> u8;
        for (int k = 0; k < NT8; ++k) u8.u[k] = s->ts_units.u[k];
        hipLaunchKernelGGL(rbts::msj_tendon_state8<BLOCK>, dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, s->stream, s->c8, u8,
                           s->d_q, s->d_qd, sp, out, n);
    }
    RB_HIP(hipGetLastError());
    return RB_OK;
}
}  // namespace

int rb_tendon_state_dev(rb_sim *s, const float *d_act, int sp_mode, float act_scale,
                        float *d_length, float *d_rate, float *d_activation, float *d_force) {
    int rc = tendon_state_check(s, d_act, sp_mode, act_scale);
    if (rc) return rc;
    for (const void *p : {static_cast<const void *>(d_act), static_cast<const void *>(d_length), static_cast<const void *>(d_rate),
                          static_cast<const void *>(d_activation), static_cast<const void *>(d_force)})
        if (reinterpret_cast<uintptr_t>(p) % 16) return fail(RB_EINVAL, "tendon state: device arrays must be 16-byte aligned");
    RB_HIP(hipSetDevice(s->device));
    return tendon_state_launch(s, d_act, sp_mode, act_scale, rbts::Outputs{d_length, d_rate, d_activation, d_force});
}

int rb_tendon_state(rb_sim *s, const float *act, int sp_mode, float act_scale,
                    float *length, float *rate, float *activation, float *force) {
    int rc = tendon_state_check(s, act, sp_mode, act_scale);
    if (rc) return rc;
    RB_HIP(hipSetDevice(s->device));
    const size_t cnt = size_t(s->n) * size_t(s->n_t), slab = sizeof(float) * cnt;
    if (!s->d_ts_out) RB_HIP(hipMalloc(&s->d_ts_out, 4 * slab));
    const float *d_act = nullptr;
    if (act) {
        RB_HIP(hipMemcpyAsync(s->d_rows, act, slab, hipMemcpyHostToDevice, s->stream));
        d_act = s->d_rows;
    }
    float *h[4] = {length, rate, activation, force}, *d[4];
    for (int r = 0; r < 4; ++r) d[r] = h[r] ? s->d_ts_out + r * cnt : nullptr;
    rc = tendon_state_launch(s, d_act, sp_mode, act_scale, rbts::Outputs{d[0], d[1], d[2], d[3]});
    if (rc) return rc;
    for (int r = 0; r < 4; ++r)
        if (h[r]) RB_HIP(hipMemcpyAsync(h[r], d[r], slab, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

static rb_dispatch_row g_rows[N_ROWS];
static rb_dispatch_row public_row(const Row &r) {
    return rb_dispatch_row{r.key.cls, r.key.entry, r.key.form, r.key.integ, r.key.block, r.key.src, r.key.variant, r.ranges ? 1 : 0};
}
int rb_dispatch_rows(const rb_dispatch_row **rows) {
    static const bool filled = [] { for (int i = 0; i < N_ROWS; ++i) g_rows[i] = public_row(TABLE[i]); return true; }();
    (void)filled;
    if (rows) *rows = g_rows;
    return N_ROWS;
}
int rb_auto_rules(const rb_auto_rule **rules) {
    if (rules) *rules = AUTO_RULES;
    return N_AUTO_RULES;
}
int rb_get_launch_thresholds(rb_launch_thresholds *out) {
    if (!out) return fail(RB_EINVAL, "null argument");
    *out = rb_launch_thresholds{RB_SMALL_BATCH, RB_PAIR_SMALL_BATCH, RB_CHAIN_BATCH_RK4, RB_CHAIN_BATCH_EULER, RB_CHAIN_BATCH_TREE_RK4,
                                RB_CHAIN_BATCH_TREE_EULER, RB_EAGER_HEAD_BATCH_RK4, RB_TREE_JIT_BATCH};
    return RB_OK;
}
int rb_dispatch_current(rb_sim *s, int entry, rb_dispatch_row *out) {
    if (check(s) || !out) return fail(RB_EINVAL, "null argument");
    if (entry < ENTRY_STEP || entry > ENTRY_FUSED) return fail(RB_EINVAL, "unknown entry kind");
    if (entry == ENTRY_FUSED && (s->tree || s->ntx)) return fail(RB_EUNSUPPORTED, "fused rollout is built for 8-tendon ball-joint robots");
    if (extension_serves(s, entry))
        return fail(RB_EUNSUPPORTED,
                    s->hist.rows && entry == ENTRY_ENV
                        ? "action rows are set (rb_env_action_obs_configure): the history env-step kernels (env_hist.hpp) are not rows of the dispatch table"
                    : s->par.on ? "per-env parameters are enabled: the parameter kernels (env_params.hpp) are not rows of the dispatch table"
                    : s->io.on ? "an io configuration is set (rb_env_io_configure): the io env-step kernels (env_io.hpp) are not rows of the dispatch table"
                              : "tendon channels are set (rb_env_obs_configure): the extended env-step kernels (env_obs.hpp) are not rows of the dispatch table");
    RB_HIP(hipSetDevice(s->device));
    if (entry != ENTRY_ENV || s->env_ready) maybe_jit(s);
    std::string why;
    const Row *r = row_for(s, entry, /*build=*/entry != ENTRY_ENV || s->env_ready, &why);
    if (!r) return fail(RB_EUNSUPPORTED, why);
    *out = public_row(*r);
    return RB_OK;
}

int rb_malloc(rb_sim *s, int64_t bytes, void **d_ptr) {
    if (check(s) || !d_ptr || bytes < 0) return fail(RB_EINVAL, "bad argument");
    RB_HIP(hipSetDevice(s->device));
    RB_HIP(hipMalloc(d_ptr, size_t(bytes)));
    return RB_OK;
}
int rb_free(rb_sim *s, void *d_ptr) {
    if (check(s)) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    RB_HIP(hipFree(d_ptr));
    return RB_OK;
}
int rb_memcpy_h2d(rb_sim *s, void *d_dst, const void *h_src, int64_t bytes) {
    if (check(s) || !d_dst || !h_src) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    RB_HIP(hipMemcpyAsync(d_dst, h_src, size_t(bytes), hipMemcpyHostToDevice, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}
int rb_memcpy_d2h(rb_sim *s, void *h_dst, const void *d_src, int64_t bytes) {
    if (check(s) || !h_dst || !d_src) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    RB_HIP(hipMemcpyAsync(h_dst, d_src, size_t(bytes), hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

}  // extern "C"
