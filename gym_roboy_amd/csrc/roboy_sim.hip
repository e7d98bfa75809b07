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
// handle with per-env parameters, tendon channels or an io configuration, whose kernels (env_params.hpp, env_obs.hpp, env_io.hpp) one
// launch path below chooses (extension_launch).  This file holds the kernels that are not in a header of their own, the handle, the
// availability predicates and the C ABI.
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
    // per-env physical parameters (env_params.hpp; rb_params_*): while enabled, the step and env-step entries launch the parameter
    // kernels instead of the dispatch table's row.  Planes [P][n], draw counters [n], ranges lo[P] | hi[P] (device and host copies)
    bool params = false;
    int n_params = 0;
    float *d_params = nullptr, *d_param_ranges = nullptr;
    uint32_t *d_param_draws = nullptr;
    std::vector<float> param_ranges;
    bool param_resample = false;
    // tendon channels in the env step's observation (env_obs.hpp; rb_env_obs_*): while the mask is set, the env-step entry launches
    // the extended kernels - the nominal or the parameter form - instead of the dispatch table's row / the parameter kernel
    int obs_mask = 0;
    float obs_scale[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    int obs_dim() const { return 3 * n_q + rbo::n_channels(obs_mask) * n_t + hist_rows * n_t; }
    // action latency and sensor noise of the env step (env_io.hpp; rb_env_io_*): while configured, the env-step entry launches the io
    // kernels - nominal or parameter form, with or without channels.  Planes [n] each; the ring [io_slots][n][n_t] only with delay_hi > 0
    bool io = false;
    rb_env_io_config io_cfg = {};
    uint32_t *d_io_delay = nullptr, *d_io_draws = nullptr, *d_io_rows = nullptr;
    float *d_io_hist = nullptr;
    int io_slots = 0;
    // the last K handed action rows as observation columns (env_hist.hpp; rb_env_action_obs_*): while K > 0 the env-step entry launches
    // the history kernels, with or without any of the above, and the ring exists whatever delay_hi is (io_slots above max(delay_hi, K - 1))
    int hist_rows = 0;
    // episode-end codes (rb_env_done_kind_*): while enabled, every env-step launch is followed by done_kind_kernel over its range.
    // Planes [n] each: the goal counter d_ep_cnt[2n + i] as of env i's last episode end, and the last step's codes
    bool done_kind = false;
    uint32_t *d_done_seen = nullptr, *d_done_kind = nullptr;
    // privileged critic rows (env_critic.hpp; rb_env_critic_obs_*): while the mask is set, every env-step launch and every reset is
    // followed by critic_rows_kernel over its range.  critic_dim: the row width the mask had when it was configured; the plane [n][Dc]
    int critic_mask = 0, critic_dim = 0;
    float *d_critic = nullptr;
    int critic_width() const {
        return rbc::row_dim(critic_mask, n_q, params ? n_params : 0, hist_rows * n_t);
    }
    // goal pool (env_goal.hpp; rb_env_goal_pool_*): while set, every env-step launch and every reset is followed by goal_pool_kernel
    // over its range, and rb_sample_goals(_dev) return pool rows.  Rows [m][n_q]; m is fixed by the first call, the pointer never moves
    float *d_goal_pool = nullptr;
    int64_t goal_pool_m = 0;
    // goal curriculum over the pool's row order (env_goal.hpp; rb_env_goal_curriculum_*): while curr_L > 0, goal_pool_launch enqueues
    // goal_curriculum_kernel in place of goal_pool_kernel.  Planes [n] each: the env's level, the row it holds, and the goals-reached
    // counter d_ep_cnt[2n + i] as of its last episode end (a copy of its own: episode-end codes may be off)
    uint32_t curr_L = 0, curr_up = 0, curr_down = 0;
    uint32_t *d_goal_level = nullptr, *d_goal_index = nullptr, *d_goal_seen = nullptr;      // one allocation, d_goal_level its start
    uint64_t *d_goal_hist = nullptr;          // [L] counts behind the planes: rb_env_goal_level_hist's device buffer
    // outcome counts per pool row (env_goal.hpp; rb_env_goal_row_stats_*): while non-null, goal_pool_launch enqueues
    // goal_curriculum_stats_kernel in place of goal_curriculum_kernel.  [2][m]: attempts, then reached
    uint64_t *d_goal_row_stats = nullptr;
};

namespace {

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
    if (s->params) return;                        // the parameter kernels are ahead of time (and a later call builds after rb_params_disable)
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

// ---- tendon channels in the observation (env_obs.hpp): the arguments of a launch while a mask is set ----
// dynamic LDS of an extended env-step launch: the rows of its workgroup's envs, where they fit beside the instance's own columns (0: per-lane stores)
size_t obs_stage_bytes(const rb_sim *s, int block = 256) {
    const size_t columns = (s->baked ? 0 : s->ntx ? 4 * block * NTX : 4 * block * NT8) * (s->params ? 2 : 1);
    const size_t rows = size_t(4) * block * s->obs_dim();
    return columns + rows <= 65536 ? rows : 0;
}
template <int NT>
rbo::ObsArgs<NT> obs_args(const rb_sim *s, bool staged = false) {
    rbo::ObsArgs<NT> oa;
    oa.mask = s->obs_mask; oa.obs_dim = s->obs_dim(); oa.staged = staged ? 1 : 0; oa.pad_ = 0;
    for (int c = 0; c < 4; ++c) oa.scale[c] = s->obs_scale[c];
    for (int k = 0; k < NT; ++k) oa.units[k] = s->ts_units.u[k];
    return oa;
}
// ---- action latency and sensor noise (env_io.hpp): the argument of a launch while rb_env_io_configure holds ----
// first: the launch's first env (the planes and the ring inside each slot are shifted by it)
rbio::IoArgs io_args(const rb_sim *s, long first) {
    rbio::IoArgs io;
    std::memset(&io, 0, sizeof(io));
    const rb_env_io_config cfg = s->io ? s->io_cfg : rb_env_io_config{};      // (no io configuration, K > 0: zeros and the ring)
    if (s->io) { io.delay = s->d_io_delay + first; io.delay_draws = s->d_io_draws + first; io.rows = s->d_io_rows + first; }
    io.hist = s->d_io_hist ? s->d_io_hist + first * s->n_t : nullptr;
    io.slot_stride = long(s->n) * s->n_t;
    io.slot_mask = s->io_slots ? s->io_slots - 1 : 0;
    io.delay_lo = cfg.delay_lo; io.delay_hi = cfg.delay_hi; io.resample = cfg.resample_on_reset ? 1 : 0;
    // row positions: q, qd, (goal: never), then the selected channels in row order, each sigma in the units the column reports (x scale)
    const int nq = s->n_q;
    for (int j = 0; j < nq; ++j) { io.colsig[j] = cfg.sigma_q; io.colsig[nq + j] = cfg.sigma_qd; }
    int col = 3 * nq;
    for (int ch = 0; ch < 4; ++ch)
        if (s->obs_mask >> ch & 1)
            for (int k = 0; k < s->n_t; ++k) io.colsig[col++] = cfg.sigma_tendon[ch] * s->obs_scale[ch];
    for (int c = 0; c < col; ++c)
        if (io.colsig[c] != 0.0f) io.noise_blocks |= 1u << (c >> 2);
    return io;
}
void io_free(rb_sim *s) {
    (void)hipFree(s->d_io_delay); (void)hipFree(s->d_io_draws); (void)hipFree(s->d_io_rows); (void)hipFree(s->d_io_hist);
    s->d_io_delay = nullptr; s->d_io_draws = nullptr; s->d_io_rows = nullptr; s->d_io_hist = nullptr;
    s->io = false; s->io_slots = 0;
}
// the ring both options share: S slots, the smallest power of two above max(delay_hi, K - 1); none without a delay range and K = 0
int ring_slots_wanted(int delay_hi, int hist_rows) {
    if (delay_hi <= 0 && hist_rows <= 0) return 0;
    const int reach = delay_hi > hist_rows - 1 ? delay_hi : hist_rows - 1;
    int slots = 1;
    while (slots <= reach) slots *= 2;
    return slots;
}
// ... rebuilt (zeroed) for the handle as configured
int ring_rebuild(rb_sim *s) {
    (void)hipFree(s->d_io_hist);
    s->d_io_hist = nullptr;
    s->io_slots = ring_slots_wanted(s->io ? s->io_cfg.delay_hi : 0, s->hist_rows);
    if (!s->io_slots) return RB_OK;
    const size_t bytes = sizeof(float) * size_t(s->io_slots) * size_t(s->n) * size_t(s->n_t);
    const hipError_t e = hipMalloc(&s->d_io_hist, bytes);
    if (e != hipSuccess) {                   // no ring: neither a delay range nor action rows (their kernels index it unasked)
        s->d_io_hist = nullptr; s->io_slots = 0; s->hist_rows = 0;
        if (s->io) s->io_cfg.delay_lo = s->io_cfg.delay_hi = 0;
        return fail(RB_EHIP, std::string("the action history ring: ") + hipGetErrorString(e));
    }
    RB_HIP(hipMemsetAsync(s->d_io_hist, 0, bytes, s->stream));
    return RB_OK;
}
// rb_env_reset_dev's observation rows on such a handle: the state the reset kernel has just written, every set-point 0
void obs_rows_launch(rb_sim *s, float *d_obs) {
    const dim3 grid(blocks_for(s->n, 256)), block(256);
    const float *par = s->params ? s->d_params : nullptr;
    if (s->ntx)
        hipLaunchKernelGGL((rbo::msj_obs_rows<256, ConstX>), grid, block, 0, s->stream, s->cx, obs_args<NTX>(s), s->d_q, s->d_qd, s->d_goal, par, d_obs, s->n);
    else
        hipLaunchKernelGGL((rbo::msj_obs_rows<256, Const8>), grid, block, 0, s->stream, s->c8, obs_args<NT8>(s), s->d_q, s->d_qd, s->d_goal, par, d_obs, s->n);
}

// ---- what dispatch() launches where extension_serves() (roboy_dispatch.hpp): the kernels of env_params.hpp, env_obs.hpp, env_io.hpp ----
// The constants an instance is compiled for, chosen here and nowhere else: f(the constants object, BK as a type) with BK = the
// constants are MsjRobot's literals (msj_baked.hpp), the object then only fills the argument's place
template <typename F>
int with_consts(const rb_sim *s, F &&f) {
    if (s->ntx) return f(s->cx, std::false_type{});
    if (s->baked) return f(s->c8, std::true_type{});
    return f(s->c8, std::false_type{});
}
rbp::ParamArgs param_args(const rb_sim *s, const Launch &L) {
    return rbp::ParamArgs{s->d_params + L.i0, s->d_param_draws + L.i0, s->d_param_ranges, s->n, s->n_params, s->param_resample ? 1 : 0};
}
// the plain step under parameters: three argument lists of their own
template <int INTEG>
int params_step_launch(rb_sim *s, const Launch &L) {
    constexpr int B = 256;
    const dim3 grid(blocks_for(L.cnt, B)), block(B);
    float *q = s->d_q + L.i0, *qd = s->d_qd + L.i0, *par = s->d_params + L.i0;
    uint32_t *feas = s->d_feas + L.i0;
    const float *act = L.act + size_t(L.i0) * s->n_t;
    return with_consts(s, [&](const auto &c, auto bk) {
        if constexpr (std::is_same<std::decay_t<decltype(c)>, ConstX>::value)
            hipLaunchKernelGGL((rbp::msj_params_step_nt<INTEG, B>), grid, block, 0, L.stream, c, q, qd, feas, act, L.act_scale, par, s->n, L.cnt);
        else
            hipLaunchKernelGGL((rbp::msj_params_step<INTEG, B, decltype(bk)::value>), grid, block, 0, L.stream, c, q, qd, feas, act, scale8(s, L.act_scale), par, s->n, L.cnt);
        return RB_OK;
    });
}
// The env step of a handle with any combination of parameters, channels and io: the env-step body with the extension of the last
// header that applies (io over channels over none), in its parameter form where parameters are enabled.
template <int INTEG>
int ext_env_launch(rb_sim *s, const Launch &L) {
    MsjEnvArgs a = msj_env_args(s, L);
    a.obs = L.obs + L.i0 * s->obs_dim();                 // the row stride is the handle's obs_dim (9 without channels)
    const int K = s->hist_rows;                           // > 0: the history kernels (env_hist.hpp), an io argument of zeros without io
    const bool par = s->params, io = s->io || K > 0, rows = io || s->obs_mask;       // rows: TendonObs writes them (env_obs.hpp)
    return with_consts(s, [&](const auto &c, auto bk) {
        using CONST = std::decay_t<decltype(c)>;
        constexpr bool BK = decltype(bk)::value;
        constexpr int NT = rbo::NtOf<CONST>::N;
        // the unroll factors of the large-batch env-per-lane rows (0: run-time tendon count)
        constexpr int U = NT == NTX ? 0 : BK ? (INTEG == 0 ? UBE : UBR) : (INTEG == 0 ? UKE : UKR);
        // An io kernel is the text of the kernel it stands in for.  Without parameters and channels that is the table's env-per-lane
        // row, which for MsjRobot's baked constants at small batches is the 64-thread instance with tendons AND integrator stages written
        // out - another summation order of the RK4 stages than the large-batch text (rolled stages): a configuration of zeros steps like
        // no configuration there too.  (Kernarg constants: the large-batch text's rolled tendon loop adds the same terms in the same order
        // as the written-out 64-thread row, and that row has no scalar register to spare - with the io arguments it would spill.)
        const bool small = BK && io && !par && !s->obs_mask && s->n <= RB_SMALL_BATCH;
        const int B = small ? 64 : 256;
        const size_t lds = rows ? obs_stage_bytes(s, B) : 0;
        const rbo::ObsArgs<NT> oa = obs_args<NT>(s, lds != 0);
        auto go = [&](auto kernel, const auto &...behind) {      // every instance takes (constants, MsjEnvArgs, ...)
            hipLaunchKernelGGL(kernel, dim3(blocks_for(L.cnt, B)), dim3(B), lds, L.stream, c, a, behind...);
            return RB_OK;
        };
        auto io_step = [&](auto block, auto unroll) {
            return go(rbio::msj_io_env_step<INTEG, decltype(block)::value, decltype(unroll)::value, CONST, BK>, oa, io_args(s, L.i0));
        };
        if (K > 0) {
            const rbh::HistIoArgs hio{io_args(s, L.i0), {K, s->obs_dim() - K * s->n_t}};
            if (par) return go(rbh::msj_hist_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L), oa, hio);
            if constexpr (BK) if (small) return go(rbh::msj_hist_env_step<INTEG, 64, 8, CONST, BK>, oa, hio);
            return go(rbh::msj_hist_env_step<INTEG, 256, U, CONST, BK>, oa, hio);
        }
        if (par && io) return go(rbio::msj_io_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L), oa, io_args(s, L.i0));
        if (io) {
            if constexpr (BK) if (small) return io_step(std::integral_constant<int, 64>{}, std::integral_constant<int, 8>{});
            return io_step(std::integral_constant<int, 256>{}, std::integral_constant<int, U>{});
        }
        if (par && rows) return go(rbo::msj_obs_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L), oa);
        if (rows) return go(rbo::msj_obs_env_step<INTEG, 256, U, CONST, BK>, oa);
        return go(rbp::msj_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L));
    });
}
int extension_launch(rb_sim *s, int entry, const Launch &L) {
    if (L.cnt <= 0) return RB_OK;
    const bool euler = s->integrator == RB_EULER;
    if (entry == ENTRY_STEP) return euler ? params_step_launch<0>(s, L) : params_step_launch<1>(s, L);
    if (entry == ENTRY_ENV) return euler ? ext_env_launch<0>(s, L) : ext_env_launch<1>(s, L);
    return fail(RB_EUNSUPPORTED, "per-env parameters have no fused-rollout kernel (rb_params_disable first)");
}
// ---- privileged critic rows (env_critic.hpp): one launch behind an env step or a reset, over the envs [i0, i0 + cnt) ----
// the options the mask was configured against are still there, and the row is as wide as the plane's
int critic_check(rb_sim *s) {
    const int m = s->critic_mask;
    if ((m & rbc::PARAMS && !s->params) || (m & rbc::DELAY && !s->io) || (m & rbc::ACTIONS && !s->hist_rows) || s->critic_width() != s->critic_dim)
        return fail(RB_EINVAL, "an option the critic rows depend on changed after rb_env_critic_obs_configure: configure the rows again");
    return RB_OK;
}
// d_obs: the observation rows the step has just written (null: no rows, zero action blocks); out: rows [n][Dc] of the whole batch
int critic_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const float *d_obs, float *out) {
    if (cnt <= 0) return RB_OK;
    rbc::CriticArgs a;
    a.q = s->d_q; a.qd = s->d_qd; a.goal = s->d_goal; a.step_num = s->d_step_num;
    a.par = s->params ? s->d_params : nullptr;
    a.delay = s->io ? s->d_io_delay : nullptr;
    a.obs = d_obs; a.out = out;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    a.max_len = float(s->env.max_len);
    a.nq = s->n_q; a.np = s->params ? s->n_params : 0; a.mask = s->critic_mask; a.dc = s->critic_dim;
    a.od = s->obs_dim(); a.act_cols = s->hist_rows * s->n_t; a.lead = a.od - a.act_cols;
    a.flat = reinterpret_cast<uintptr_t>(out) % 16 == 0 ? 1 : 0;
    hipLaunchKernelGGL(rbc::critic_rows_kernel, dim3(blocks_for(cnt, 256)), dim3(256), sizeof(float) * 256 * size_t(a.dc), stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
// ---- goal pool (env_goal.hpp): one launch behind an env step (d_done: its done words) or a reset (null: every env), over [i0, i0 + cnt) ----
int goal_pool_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const uint32_t *d_done, float *d_obs) {
    rbg::GoalPoolArgs a;
    a.pool = s->d_goal_pool; a.done = d_done; a.goal_count = s->d_goal_count; a.goal = s->d_goal; a.obs = d_obs;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    a.seed = s->seed; a.env0 = uint64_t(s->env0);
    a.m = uint32_t(s->goal_pool_m);
    a.nq = s->n_q; a.od = s->obs_dim(); a.rows = s->tree ? 1 : 0;
    if (s->curr_L) {                          // a curriculum: the same launch, the row drawn inside the env's window
        rbg::GoalCurriculumArgs c;
        c.p = a;
        c.level = s->d_goal_level; c.index = s->d_goal_index; c.seen = s->d_goal_seen;
        c.reached = s->d_ep_cnt + 2 * size_t(s->n);
        c.L = s->curr_L; c.up = s->curr_up; c.down = s->curr_down;
        if (s->d_goal_row_stats) {            // outcome counts per row: the same launch again, two adds per episode end more
            rbg::GoalCurriculumStatsArgs t;
            t.c = c; t.counts = reinterpret_cast<unsigned long long *>(s->d_goal_row_stats);
            hipLaunchKernelGGL(rbg::goal_curriculum_stats_kernel, dim3(blocks_for(cnt, RBG_STATS_BLOCK)), dim3(RBG_STATS_BLOCK), 0, stream, t);
        } else
            hipLaunchKernelGGL(rbg::goal_curriculum_kernel, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, c);
    } else
        hipLaunchKernelGGL(rbg::goal_pool_kernel, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
void params_free(rb_sim *s) {
    (void)hipFree(s->d_params); (void)hipFree(s->d_param_draws); (void)hipFree(s->d_param_ranges);
    s->d_params = nullptr; s->d_param_draws = nullptr; s->d_param_ranges = nullptr;
    s->params = false; s->n_params = 0; s->param_resample = false; s->param_ranges.clear();
}
// refusal of the entry points that have no parameter form
int params_refuse(rb_sim *s, const char *what) {
    return fail(RB_EUNSUPPORTED, std::string(what) + " has no per-env-parameter form: the handle has parameters enabled (rb_params_disable first)");
}
// rb_sample_goals(_dev) on a handle with a goal curriculum: without an env step there is no episode outcome to move a level
int curriculum_refuse_sample(rb_sim *) {
    return fail(RB_EUNSUPPORTED, "rb_sample_goals: the handle has a goal curriculum, whose levels move with the env layer's episode ends");
}

}  // namespace

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
    for (int j = 0; j < s->n_q; ++j) { s->box.lo[j] = float(robot->q_lo[j]); s->box.hi[j] = float(robot->q_hi[j]); }

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
    params_free(s);
    io_free(s);
    (void)hipFree(s->d_done_seen); (void)hipFree(s->d_done_kind);
    (void)hipFree(s->d_critic);
    (void)hipFree(s->d_goal_pool);
    (void)hipFree(s->d_goal_level);          // (with it the index plane, the seen plane and the histogram counts)
    (void)hipFree(s->d_goal_row_stats);
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
    if (s->curr_L) return curriculum_refuse_sample(s);
    RB_HIP(hipSetDevice(s->device));
    const uint8_t *d_mask = nullptr;
    if (mask) {
        RB_HIP(hipMemcpyAsync(s->d_u8, mask, size_t(s->n), hipMemcpyHostToDevice, s->stream));
        d_mask = s->d_u8;
    }
    if (mask) RB_HIP(hipMemsetAsync(s->d_rows, 0, sizeof(float) * s->n * s->n_q, s->stream));
    if (s->d_goal_pool)
        hipLaunchKernelGGL(rbg::goal_pool_sample_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->d_goal_pool,
                           uint32_t(s->goal_pool_m), s->d_rows, s->d_goal_count, d_mask, s->n_q, s->n, s->seed, uint64_t(s->env0), 1);
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
    if (s->params) return params_refuse(s, "the fused rollout (rb_rollout_fused_dev)");
    if (s->d_goal_pool)
        return fail(RB_EUNSUPPORTED, "the fused rollout (rb_rollout_fused_dev) redraws goals inside one kernel and cannot draw them from a goal pool");
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
    if (s->curr_L) return curriculum_refuse_sample(s);
    RB_HIP(hipSetDevice(s->device));
    if (s->d_goal_pool)
        hipLaunchKernelGGL(rbg::goal_pool_sample_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->d_goal_pool,
                           uint32_t(s->goal_pool_m), d_goal_q, s->d_goal_count, d_mask, s->n_q, s->n, s->seed, uint64_t(s->env0), 0);
    else
        hipLaunchKernelGGL(sample_goals_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                           d_goal_q, s->d_goal_count, d_mask, s->box, s->n_q, s->n, s->seed, uint64_t(s->env0), 0);
    RB_HIP(hipGetLastError());
    return RB_OK;
}

int rb_env_configure(rb_sim *s, const rb_env_config *cfg) {
    if (check(s) || !cfg) return fail(RB_EINVAL, "null argument");
    if (!s->tree && s->n_q != 3) return fail(RB_EUNSUPPORTED, "fused env layer: unsupported robot");
    if (cfg->max_episode_length < 1) return fail(RB_EINVAL, "max_episode_length must be >= 1");
    if (!(cfg->angle_hi > cfg->angle_lo) || !(cfg->vel_hi > cfg->vel_lo) || !(cfg->action_hi > cfg->action_lo))
        return fail(RB_EINVAL, "empty box in env config");
    RB_HIP(hipSetDevice(s->device));
    EnvParams &e = s->env;
    e.vel_penalty = cfg->joint_vel_penalty != 0; e.bonus = cfg->goal_bonus != 0;
    e.max_len = cfg->max_episode_length; e.auto_reset = cfg->auto_reset != 0;
    e.penalty = cfg->penalty_boundary; e.bonus_val = cfg->bonus_goal;
    e.a_lo = cfg->angle_lo; e.a_hi = cfg->angle_hi; e.v_lo = cfg->vel_lo; e.v_hi = cfg->vel_hi;
    e.act_hi = cfg->action_hi;
    // (out.high - out.low) / (in.high - in.low) evaluated in fp32 like the reference's float32 Boxes
    e.slope = (cfg->action_hi - cfg->action_lo) / (1.0f - (-1.0f));
    e.tol_a2 = cfg->goal_angle_tol * cfg->goal_angle_tol; e.tol_v2 = cfg->goal_vel_tol * cfg->goal_vel_tol;
    e.a_scale = 2.0f / (cfg->angle_hi - cfg->angle_lo); e.v_scale = 2.0f / (cfg->vel_hi - cfg->vel_lo);
    if (!s->d_goal) {
        const size_t plane = sizeof(float) * size_t(s->n);
        RB_HIP(hipMalloc(&s->d_goal, plane * s->n_q));
        RB_HIP(hipMalloc(&s->d_ep_ret, plane));
        RB_HIP(hipMalloc(&s->d_step_num, sizeof(uint32_t) * size_t(s->n)));
        RB_HIP(hipMalloc(&s->d_ep_sum, sizeof(double) * size_t(s->n) * 2));
        RB_HIP(hipMalloc(&s->d_ep_cnt, sizeof(uint32_t) * size_t(s->n) * 3));
    }
    RB_HIP(hipMemsetAsync(s->d_ep_sum, 0, sizeof(double) * size_t(s->n) * 2, s->stream));
    RB_HIP(hipMemsetAsync(s->d_ep_cnt, 0, sizeof(uint32_t) * size_t(s->n) * 3, s->stream));
    if (s->done_kind) RB_HIP(hipMemsetAsync(s->d_done_seen, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    if (s->curr_L) RB_HIP(hipMemsetAsync(s->d_goal_seen, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    RB_HIP(hipMemsetAsync(s->d_infeas_n, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    s->env_steps = 0.0;
    s->env_ready = true;
    // the run-time specialised kernels are built here, outside any capture a caller may wrap around its first step
    maybe_jit(s);
    if (s->tree) (void)resolve_form(s, ENTRY_ENV, /*build=*/true, nullptr);      // (the env step's kernel of the generated form it runs)
    return rb_env_reset_dev(s, nullptr);
}

int rb_env_reset_dev(rb_sim *s, float *d_obs) {
    if (check(s)) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (s->tree)
        hipLaunchKernelGGL(rbt::tree_env_reset_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                           s->box, s->d_q, s->d_qd, s->d_feas, s->d_goal, s->d_step_num, s->d_ep_ret,
                           s->d_goal_count, d_obs, s->n_q, s->n, s->seed, uint64_t(s->env0));
    else
        hipLaunchKernelGGL(env_reset_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                           s->box, s->d_q, s->d_qd, s->d_feas, s->d_goal, s->d_step_num, s->d_ep_ret,
                           s->d_goal_count, s->obs_mask || s->hist_rows ? nullptr : d_obs, s->n, s->seed, uint64_t(s->env0));
    RB_HIP(hipGetLastError());
    if ((s->obs_mask || s->hist_rows) && d_obs) {      // rows of obs_dim floats: the tendon columns at the zero pose, every set-point 0
        obs_rows_launch(s, d_obs);
        RB_HIP(hipGetLastError());
    }
    if (s->done_kind) {                       // a reset is no episode end: the next one is judged against the counters as they stand, and nothing is reported
        RB_HIP(hipMemcpyAsync(s->d_done_seen, s->d_ep_cnt + 2 * size_t(s->n), sizeof(uint32_t) * size_t(s->n), hipMemcpyDeviceToDevice, s->stream));
        RB_HIP(hipMemsetAsync(s->d_done_kind, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    }
    if (s->io && d_obs) {                     // sensor readings too: the rows' noise, in place (the episode restarts, the history needs nothing)
        const rbio::IoArgs io = io_args(s, 0);
        if (io.noise_blocks) {
            const int od = s->obs_dim();
            if (s->hist_rows)                 // (the noise stops in front of the action blocks: row stride and noised width apart)
                hipLaunchKernelGGL(rbh::hist_noise_rows, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, d_obs, od, od - s->hist_rows * s->n_t, io,
                                   long(s->n), s->seed, uint64_t(s->env0));
            else
                hipLaunchKernelGGL(rbio::io_noise_rows, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, d_obs, od, io, s->n, s->seed, uint64_t(s->env0));
            RB_HIP(hipGetLastError());
        }
    }
    if (s->hist_rows && d_obs) {              // nothing has been handed yet: K zero blocks
        const int od = s->obs_dim();
        hipLaunchKernelGGL(rbh::hist_zero_rows, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, d_obs, od, od - s->hist_rows * s->n_t, long(s->n));
        RB_HIP(hipGetLastError());
    }
    if (s->d_goal_pool) {                     // every env's goal becomes the pool row of the draw the reset kernel made (a curriculum:
        // inside the env's window, levels as they stand, and its `seen` plane re-based to the counters like d_done_seen above)
        const int rc = goal_pool_launch(s, 0, s->n, s->stream, nullptr, d_obs);
        if (rc) return rc;
    }
    if (s->critic_mask) {                     // the privileged rows of the reset state, behind every kernel that wrote the rows above
        int rc = critic_check(s);
        if (rc == RB_OK) rc = critic_launch(s, 0, s->n, s->stream, d_obs, s->d_critic);
        if (rc) return rc;
    }
    return RB_OK;
}

// ---- tendon channels in the fused env step's observation (env_obs.hpp) ----
int32_t rb_env_obs_count(int32_t n_q, int32_t n_t, uint32_t channel_mask) {
    if (n_q < 0 || n_t < 0 || (channel_mask & ~uint32_t(RB_OBS_ALL))) return -1;
    return 3 * n_q + rbo::n_channels(int(channel_mask)) * n_t;
}
int rb_env_obs_configure(rb_sim *s, uint32_t channel_mask, const float *scale) {
    if (check(s)) return RB_EINVAL;
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (channel_mask & ~uint32_t(RB_OBS_ALL)) return fail(RB_EINVAL, "unknown bits in the channel mask (RB_OBS_LENGTH | RB_OBS_RATE | RB_OBS_ACTIVATION | RB_OBS_FORCE)");
    if (scale)
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(scale[c])) return fail(RB_EINVAL, "channel scales must be finite");
    if (s->tree && channel_mask)
        return fail(RB_EUNSUPPORTED, "tendon channels in the observation are built for ball-joint robots (1-16 tendons); a joint tree's readout is "
                                     "rb_tendon_state_dev");
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still write rows of the old width
    if (rc) return rc;
    rc = drop_graphs(s);
    if (rc) return rc;
    s->obs_mask = int(channel_mask);
    for (int c = 0; c < 4; ++c) s->obs_scale[c] = scale ? scale[c] : 1.0f;
    return RB_OK;
}
// ---- per-env action latency and sensor noise in the fused env step (env_io.hpp) ----
int rb_env_io_configure(rb_sim *s, const rb_env_io_config *cfg) {
    if (check(s)) return RB_EINVAL;
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (cfg) {
        const float sig[6] = {cfg->sigma_q, cfg->sigma_qd, cfg->sigma_tendon[0], cfg->sigma_tendon[1], cfg->sigma_tendon[2], cfg->sigma_tendon[3]};
        for (float v : sig)
            if (!std::isfinite(v) || v < 0.0f) return fail(RB_EINVAL, "sensor-noise standard deviations must be finite and >= 0");
        if (cfg->delay_lo < 0 || cfg->delay_lo > cfg->delay_hi || cfg->delay_hi > RB_IO_MAX_DELAY)
            return fail(RB_EINVAL, "action delay: 0 <= delay_lo <= delay_hi <= RB_IO_MAX_DELAY");
        if (s->tree)
            return fail(RB_EUNSUPPORTED, "action latency and sensor noise are built for ball-joint robots (1-16 tendons); joint trees have none");
    }
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still use the planes or the ring
    if (rc) return rc;
    rc = drop_graphs(s);
    if (rc) return rc;
    io_free(s);
    if (!cfg) return ring_rebuild(s);        // (the ring stays for the action columns, rb_env_action_obs_configure)
    const size_t n = size_t(s->n);
    auto planes = [&]() -> int {
        RB_HIP(hipMalloc(&s->d_io_delay, sizeof(uint32_t) * n));
        RB_HIP(hipMalloc(&s->d_io_draws, sizeof(uint32_t) * n));
        RB_HIP(hipMalloc(&s->d_io_rows, sizeof(uint32_t) * n));
        RB_HIP(hipMemsetAsync(s->d_io_draws, 0, sizeof(uint32_t) * n, s->stream));
        RB_HIP(hipMemsetAsync(s->d_io_rows, 0, sizeof(uint32_t) * n, s->stream));
        return RB_OK;
    };
    rc = planes();
    if (rc) {                                // no io configuration; action rows keep a ring of their own (or are switched off with it)
        io_free(s);
        (void)ring_rebuild(s);               // (clears the action rows itself where it fails too)
        return rc;
    }
    s->io_cfg = *cfg;
    s->io = true;
    rc = ring_rebuild(s);
    if (rc) return rc;
    return rb_env_io_sample_delay_dev(s, nullptr);      // draw 0 of every env
}
// ---- the last K commanded actions as observation columns (env_hist.hpp) ----
int32_t rb_env_action_obs_count(int32_t n_q, int32_t n_t, uint32_t channel_mask, int32_t rows) {
    if (rows < 0 || rows > RB_ACTION_OBS_MAX) return -1;
    const int32_t lead = rb_env_obs_count(n_q, n_t, channel_mask);
    return lead < 0 ? -1 : lead + rows * n_t;
}
int rb_env_action_obs_configure(rb_sim *s, int32_t rows) {
    if (check(s)) return RB_EINVAL;
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (rows < 0 || rows > RB_ACTION_OBS_MAX) return fail(RB_EINVAL, "action rows in the observation: 0 <= rows <= RB_ACTION_OBS_MAX");
    if (s->tree && rows)
        return fail(RB_EUNSUPPORTED, "action columns in the observation are built for ball-joint robots (1-16 tendons); joint trees have none");
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still write rows of the old width or use the ring
    if (rc) return rc;
    rc = drop_graphs(s);
    if (rc) return rc;
    const int delay_hi = s->io ? s->io_cfg.delay_hi : 0;
    const bool resize = ring_slots_wanted(delay_hi, rows) != s->io_slots;
    s->hist_rows = rows;
    if (!resize) return RB_OK;
    if (s->io) {                             // another S: planes, counters and ring as a fresh io configuration leaves them
        const rb_env_io_config cfg = s->io_cfg;
        return rb_env_io_configure(s, &cfg);
    }
    return ring_rebuild(s);
}
int rb_env_action_obs_rows(rb_sim *s, int32_t *rows) {
    if (check(s) || !rows) return fail(RB_EINVAL, "null argument");
    *rows = s->hist_rows;
    return RB_OK;
}
int rb_env_io_ptr(rb_sim *s, uint32_t **d_delay, uint32_t **d_delay_draws, uint32_t **d_rows, float **d_history, int32_t *slots) {
    if (check(s)) return RB_EINVAL;
    if (!s->io && !s->hist_rows) return fail(RB_EINVAL, "no io configuration (rb_env_io_configure)");
    if (d_delay) *d_delay = s->d_io_delay;
    if (d_delay_draws) *d_delay_draws = s->d_io_draws;
    if (d_rows) *d_rows = s->d_io_rows;
    if (d_history) *d_history = s->d_io_hist;
    if (slots) *slots = s->io_slots;
    return RB_OK;
}
int rb_env_io_sample_delay_dev(rb_sim *s, const uint8_t *d_mask) {
    if (check(s)) return RB_EINVAL;
    if (!s->io) return fail(RB_EINVAL, "no io configuration (rb_env_io_configure)");
    RB_HIP(hipSetDevice(s->device));
    hipLaunchKernelGGL(rbio::io_sample_delay, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->d_io_delay, s->d_io_draws, d_mask,
                       s->io_cfg.delay_lo, s->io_cfg.delay_hi, long(s->n), s->seed, uint64_t(s->env0));
    RB_HIP(hipGetLastError());
    return RB_OK;
}

// ---- episode-end codes of the fused env step (done_kind_kernel) ----
int rb_env_done_kind_configure(rb_sim *s, int enable) {
    if (check(s)) return RB_EINVAL;
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still write the planes
    if (rc) return rc;
    rc = drop_graphs(s);
    if (rc) return rc;
    s->done_kind = false;
    (void)hipFree(s->d_done_seen); (void)hipFree(s->d_done_kind);
    s->d_done_seen = nullptr; s->d_done_kind = nullptr;
    if (!enable) return RB_OK;
    const size_t plane = sizeof(uint32_t) * size_t(s->n);
    RB_HIP(hipMalloc(&s->d_done_seen, plane));
    RB_HIP(hipMalloc(&s->d_done_kind, plane));
    RB_HIP(hipMemcpyAsync(s->d_done_seen, s->d_ep_cnt + 2 * size_t(s->n), plane, hipMemcpyDeviceToDevice, s->stream));
    RB_HIP(hipMemsetAsync(s->d_done_kind, 0, plane, s->stream));
    s->done_kind = true;
    return RB_OK;
}
int rb_env_done_kind_ptr(rb_sim *s, uint32_t **d_kind) {
    if (check(s) || !d_kind) return fail(RB_EINVAL, "null argument");
    if (!s->done_kind) return fail(RB_EINVAL, "episode-end codes are not enabled (rb_env_done_kind_configure)");
    *d_kind = s->d_done_kind;
    return RB_OK;
}

// ---- privileged critic rows behind the fused env step (env_critic.hpp) ----
int32_t rb_env_critic_obs_count(int32_t n_q, int32_t n_t, uint32_t mask, int32_t n_params, int32_t action_rows) {
    if (n_q < 0 || n_t < 0 || n_params < 0 || action_rows < 0 || (mask & ~uint32_t(RB_CRITIC_ALL))) return -1;
    return mask ? rbc::row_dim(int(mask | RB_CRITIC_STATE), n_q, n_params, action_rows * n_t) : 0;
}
int rb_env_critic_obs_configure(rb_sim *s, uint32_t mask) {
    if (check(s)) return RB_EINVAL;
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (mask & ~uint32_t(RB_CRITIC_ALL))
        return fail(RB_EINVAL, "unknown bits in the critic-row mask (RB_CRITIC_STATE | _AGE | _PARAMS | _DELAY | _ACTIONS)");
    if (s->tree && mask)
        return fail(RB_EUNSUPPORTED, "critic rows are built for ball-joint robots (1-16 tendons); joint trees have none");
    if (mask) mask |= RB_CRITIC_STATE;       // (always selected)
    if (mask & RB_CRITIC_PARAMS && !s->params) return fail(RB_EINVAL, "critic rows: RB_CRITIC_PARAMS needs per-env parameters (rb_params_enable first)");
    if (mask & RB_CRITIC_DELAY && !s->io) return fail(RB_EINVAL, "critic rows: RB_CRITIC_DELAY needs an io configuration (rb_env_io_configure first)");
    if (mask & RB_CRITIC_ACTIONS && !s->hist_rows)
        return fail(RB_EINVAL, "critic rows: RB_CRITIC_ACTIONS needs action rows in the observation (rb_env_action_obs_configure first)");
    const int dim = rbc::row_dim(int(mask), s->n_q, s->params ? s->n_params : 0, s->hist_rows * s->n_t);
    if (dim > RB_CRITIC_OBS_MAX_DIM)
        return fail(RB_EINVAL, "critic rows: " + std::to_string(dim) + " columns, at most RB_CRITIC_OBS_MAX_DIM = 63 (the PPO gradient kernels' input limit)");
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still write rows of the old width
    if (rc) return rc;
    rc = drop_graphs(s);
    if (rc) return rc;
    (void)hipFree(s->d_critic);
    s->d_critic = nullptr; s->critic_mask = 0; s->critic_dim = 0;
    if (!mask) return RB_OK;
    const size_t bytes = sizeof(float) * size_t(s->n) * size_t(dim);
    RB_HIP(hipMalloc(&s->d_critic, bytes));
    s->critic_mask = int(mask); s->critic_dim = dim;
    // the rows of the envs as they stand (no observation rows at hand: zero action blocks, as behind a reset)
    return critic_launch(s, 0, s->n, s->stream, nullptr, s->d_critic);
}
int rb_env_critic_obs_dim(rb_sim *s, int32_t *dim) {
    if (check(s) || !dim) return fail(RB_EINVAL, "null argument");
    *dim = s->critic_dim;
    return RB_OK;
}
int rb_env_critic_obs_ptr(rb_sim *s, float **d_rows) {
    if (check(s) || !d_rows) return fail(RB_EINVAL, "null argument");
    if (!s->critic_mask) return fail(RB_EINVAL, "critic rows are not enabled (rb_env_critic_obs_configure)");
    *d_rows = s->d_critic;
    return RB_OK;
}

// ---- goal pool: env goals drawn from a set of poses instead of the box (env_goal.hpp) ----
int rb_env_goal_pool_set(rb_sim *s, const float *goal_q, int64_t m) {
    if (check(s) || !goal_q) return fail(RB_EINVAL, "null argument");
    if (m < 1 || m > int64_t(UINT32_MAX)) return fail(RB_EINVAL, "goal pool: m must be >= 1 (and below 2^32)");
    if (s->d_goal_pool && m != s->goal_pool_m)
        return fail(RB_EINVAL, "goal pool: the handle's pool has " + std::to_string(s->goal_pool_m) + " rows, fixed by the first call; got " + std::to_string(m));
    // the angle box of rb_env_configure, or the robot's own box (what rb_sample_goals draws from) without an env layer
    for (int64_t r = 0; r < m; ++r)
        for (int j = 0; j < s->n_q; ++j) {
            const float v = goal_q[r * s->n_q + j];
            const float lo = s->env_ready ? s->env.a_lo : s->box.lo[j], hi = s->env_ready ? s->env.a_hi : s->box.hi[j];
            if (!std::isfinite(v) || v < lo || v > hi)
                return fail(RB_EINVAL, "goal pool: row " + std::to_string(r) + ", joint " + std::to_string(j) + " is not finite or outside the angle box");
        }
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still read the rows
    if (rc) return rc;
    const size_t bytes = sizeof(float) * size_t(m) * size_t(s->n_q);
    if (!s->d_goal_pool) {
        float *d = nullptr;
        hipError_t e = hipMalloc(&d, bytes);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RB_ENOMEM : RB_EHIP, std::string("hipMalloc (goal pool): ") + hipGetErrorString(e));
        e = hipMemcpy(d, goal_q, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); return fail(RB_EHIP, std::string("hipMemcpy (goal pool): ") + hipGetErrorString(e)); }
        s->d_goal_pool = d; s->goal_pool_m = m;      // (from here on the env step and the reset launch goal_pool_kernel)
        // an env layer already drew every env's goal from the box (rb_env_configure resets): that draw's pool row takes its place,
        // counters untouched, so from here on every goal of the handle is a row of the pool
        return s->env_ready ? goal_pool_launch(s, 0, s->n, s->stream, nullptr, nullptr) : RB_OK;
    }
    RB_HIP(hipMemcpy(s->d_goal_pool, goal_q, bytes, hipMemcpyHostToDevice));      // in place: a captured graph reads the new rows on its next replay
    return RB_OK;
}
int rb_env_goal_pool_ptr(rb_sim *s, float **d_pool, int64_t *m) {
    if (check(s) || !d_pool || !m) return fail(RB_EINVAL, "null argument");
    if (!s->d_goal_pool) return fail(RB_EINVAL, "no goal pool is set (rb_env_goal_pool_set)");
    *d_pool = s->d_goal_pool; *m = s->goal_pool_m;
    return RB_OK;
}

// ---- goal curriculum: a level per env over the pool's row order (env_goal.hpp) ----
int rb_env_goal_curriculum_configure(rb_sim *s, int32_t levels, int32_t up, int32_t down, int32_t level0) {
    if (check(s)) return RB_EINVAL;
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (!s->d_goal_pool) return fail(RB_EINVAL, "goal curriculum: no goal pool is set (rb_env_goal_pool_set first)");
    if (s->curr_L) return fail(RB_EINVAL, "goal curriculum: already configured (once per handle: a captured graph holds the arguments by value)");
    const int64_t most = s->goal_pool_m < RB_GOAL_LEVELS_MAX ? s->goal_pool_m : int64_t(RB_GOAL_LEVELS_MAX);
    if (levels < 1 || levels > most)
        return fail(RB_EINVAL, "goal curriculum: levels must be in 1.." + std::to_string(most) + " (at most the pool's rows and RB_GOAL_LEVELS_MAX = 256), got " +
                                   std::to_string(levels));
    if (up < 0 || down < 0) return fail(RB_EINVAL, "goal curriculum: up and down must be >= 0");
    if (level0 < 0 || level0 >= levels) return fail(RB_EINVAL, "goal curriculum: level0 must be in 0..levels - 1");
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still launch the pool's own kernel
    if (rc) return rc;
    rc = drop_graphs(s);
    if (rc) return rc;
    const size_t plane = sizeof(uint32_t) * size_t(s->n);
    if (!s->d_goal_level) {                  // (one block: the three planes, then the host histogram's L counts)
        uint32_t *d = nullptr;
        const hipError_t e = hipMalloc(&d, 3 * plane + sizeof(uint64_t) * RB_GOAL_LEVELS_MAX + 8);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? RB_ENOMEM : RB_EHIP, std::string("hipMalloc (goal curriculum): ") + hipGetErrorString(e));
        s->d_goal_level = d; s->d_goal_index = d + s->n; s->d_goal_seen = d + 2 * s->n;
        s->d_goal_hist = reinterpret_cast<uint64_t *>((reinterpret_cast<uintptr_t>(d + 3 * s->n) + 7) & ~uintptr_t(7));
    }
    {
        std::vector<uint32_t> l0(size_t(s->n), uint32_t(level0));
        RB_HIP(hipMemcpy(s->d_goal_level, l0.data(), plane, hipMemcpyHostToDevice));
    }
    s->curr_L = uint32_t(levels); s->curr_up = uint32_t(up); s->curr_down = uint32_t(down);      // (from here on goal_pool_launch enqueues goal_curriculum_kernel)
    // every env's current goal, a row of the whole pool, becomes the row of that same draw inside its window (counters untouched);
    // the launch also sets `seen` to the counters as they stand and fills the index plane
    return goal_pool_launch(s, 0, s->n, s->stream, nullptr, nullptr);
}
static int curriculum_check(rb_sim *s) {
    if (check(s)) return RB_EINVAL;
    if (!s->curr_L) return fail(RB_EINVAL, "no goal curriculum is configured (rb_env_goal_curriculum_configure)");
    return RB_OK;
}
int rb_env_goal_level_ptr(rb_sim *s, uint32_t **d_level) {
    if (curriculum_check(s)) return RB_EINVAL;
    if (!d_level) return fail(RB_EINVAL, "null argument");
    *d_level = s->d_goal_level;
    return RB_OK;
}
int rb_env_goal_index_ptr(rb_sim *s, uint32_t **d_index) {
    if (curriculum_check(s)) return RB_EINVAL;
    if (!d_index) return fail(RB_EINVAL, "null argument");
    *d_index = s->d_goal_index;
    return RB_OK;
}
int rb_env_goal_levels_set(rb_sim *s, const uint32_t *levels) {
    if (curriculum_check(s)) return RB_EINVAL;
    if (!levels) return fail(RB_EINVAL, "null argument");
    for (long i = 0; i < s->n; ++i)
        if (levels[i] >= s->curr_L)
            return fail(RB_EINVAL, "goal levels: env " + std::to_string(i) + " has level " + std::to_string(levels[i]) + ", the curriculum has " +
                                       std::to_string(s->curr_L) + " levels");
    RB_HIP(hipSetDevice(s->device));
    const int rc = drain(s);                 // nothing in flight may still move a level
    if (rc) return rc;
    RB_HIP(hipMemcpy(s->d_goal_level, levels, sizeof(uint32_t) * size_t(s->n), hipMemcpyHostToDevice));
    return RB_OK;
}
int rb_env_goal_level_hist_dev(rb_sim *s, uint64_t *d_out, void *hip_stream) {
    if (curriculum_check(s)) return RB_EINVAL;
    if (!d_out) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    RB_HIP(hipMemsetAsync(d_out, 0, sizeof(uint64_t) * s->curr_L, st));
    unsigned g = blocks_for(s->n, 256);
    if (g > 1024u) g = 1024u;                // (grid-stride beyond: at most 1024 x L atomics into the output)
    hipLaunchKernelGGL(rbg::goal_level_hist_kernel, dim3(g), dim3(256), 0, st, s->d_goal_level, long(s->n), s->curr_L,
                       reinterpret_cast<unsigned long long *>(d_out));
    RB_HIP(hipGetLastError());
    return RB_OK;
}
int rb_env_goal_level_hist(rb_sim *s, uint64_t *out) {
    if (curriculum_check(s)) return RB_EINVAL;
    if (!out) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    const int rc = rb_env_goal_level_hist_dev(s, s->d_goal_hist, nullptr);
    if (rc) return rc;
    RB_HIP(hipMemcpyAsync(out, s->d_goal_hist, sizeof(uint64_t) * s->curr_L, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

// ---- outcome counts per pool row, and re-ordering a live pool (env_goal.hpp) ----
int rb_env_goal_row_stats_enable(rb_sim *s) {
    if (curriculum_check(s)) return RB_EINVAL;
    if (s->d_goal_row_stats) return fail(RB_EINVAL, "goal row stats: already enabled (once per handle: a captured graph holds the kernel it was captured with)");
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may still launch the curriculum's own kernel
    if (rc) return rc;
    rc = drop_graphs(s);
    if (rc) return rc;
    const size_t bytes = sizeof(uint64_t) * 2 * size_t(s->goal_pool_m);
    uint64_t *d = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RB_ENOMEM : RB_EHIP, std::string("hipMalloc (goal row stats): ") + hipGetErrorString(e));
    e = hipMemset(d, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(d); return fail(RB_EHIP, std::string("hipMemset (goal row stats): ") + hipGetErrorString(e)); }
    s->d_goal_row_stats = d;                 // (from here on goal_pool_launch enqueues goal_curriculum_stats_kernel)
    return RB_OK;
}
static int row_stats_check(rb_sim *s) {
    if (check(s)) return RB_EINVAL;
    if (!s->d_goal_row_stats) return fail(RB_EINVAL, "goal row stats are not enabled (rb_env_goal_row_stats_enable)");
    return RB_OK;
}
int rb_env_goal_row_stats_ptr(rb_sim *s, uint64_t **d_counts, int64_t *m) {
    if (row_stats_check(s)) return RB_EINVAL;
    if (!d_counts || !m) return fail(RB_EINVAL, "null argument");
    *d_counts = s->d_goal_row_stats; *m = s->goal_pool_m;
    return RB_OK;
}
int rb_env_goal_row_stats_read(rb_sim *s, uint64_t *host, int clear) {
    if (row_stats_check(s)) return RB_EINVAL;
    if (!host) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    const int rc = drain(s);                 // every count enqueued so far is in
    if (rc) return rc;
    const size_t bytes = sizeof(uint64_t) * 2 * size_t(s->goal_pool_m);
    RB_HIP(hipMemcpy(host, s->d_goal_row_stats, bytes, hipMemcpyDeviceToHost));
    if (clear) {
        RB_HIP(hipMemset(s->d_goal_row_stats, 0, bytes));
        RB_HIP(hipDeviceSynchronize());
    }
    return RB_OK;
}
int rb_env_goal_row_stats_set(rb_sim *s, const uint64_t *host) {
    if (row_stats_check(s)) return RB_EINVAL;
    if (!host) return fail(RB_EINVAL, "null argument");
    const int64_t m = s->goal_pool_m;
    for (int64_t k = 0; k < m; ++k)
        if (host[m + k] > host[k])
            return fail(RB_EINVAL, "goal row stats: row " + std::to_string(k) + " has reached " + std::to_string(host[m + k]) + " > attempts " +
                                       std::to_string(host[k]));
    RB_HIP(hipSetDevice(s->device));
    const int rc = drain(s);                 // nothing in flight may still add to the planes
    if (rc) return rc;
    RB_HIP(hipMemcpy(s->d_goal_row_stats, host, sizeof(uint64_t) * 2 * size_t(m), hipMemcpyHostToDevice));
    return RB_OK;
}
int rb_env_goal_pool_permute(rb_sim *s, const uint32_t *order) {
    if (check(s) || !order) return fail(RB_EINVAL, "null argument");
    if (!s->d_goal_pool) return fail(RB_EINVAL, "no goal pool is set (rb_env_goal_pool_set)");
    const size_t m = size_t(s->goal_pool_m), nq = size_t(s->n_q);
    std::vector<uint32_t> inv(m, UINT32_MAX);        // inv[old row] = new row
    for (size_t j = 0; j < m; ++j) {
        if (order[j] >= m) return fail(RB_EINVAL, "goal pool permute: entry " + std::to_string(j) + " is " + std::to_string(order[j]) + ", the pool has " + std::to_string(m) + " rows");
        if (inv[order[j]] != UINT32_MAX) return fail(RB_EINVAL, "goal pool permute: row " + std::to_string(order[j]) + " occurs twice (not a permutation)");
        inv[order[j]] = uint32_t(j);
    }
    RB_HIP(hipSetDevice(s->device));
    const int rc = drain(s);                 // nothing in flight may still read the rows, the indices or the counts
    if (rc) return rc;
    uint32_t *d_inv = nullptr;
    if (s->curr_L) {                         // (everything that can fail for want of memory: before anything changes)
        const hipError_t e = hipMalloc(&d_inv, sizeof(uint32_t) * m);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RB_ENOMEM : RB_EHIP, std::string("hipMalloc (goal pool permute): ") + hipGetErrorString(e));
    }
    auto done = [&](hipError_t e, const char *what) {
        (void)hipFree(d_inv);
        return e == hipSuccess ? RB_OK : fail(RB_EHIP, std::string(what) + " (goal pool permute): " + hipGetErrorString(e));
    };
    // the rows through the host, back IN PLACE: the pointer never moves, so a graph captured earlier reads the new order
    std::vector<float> rows(m * nq), out(m * nq);
    hipError_t e = hipMemcpy(rows.data(), s->d_goal_pool, sizeof(float) * m * nq, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(e, "hipMemcpy");
    for (size_t j = 0; j < m; ++j) std::memcpy(&out[j * nq], &rows[size_t(order[j]) * nq], sizeof(float) * nq);
    e = hipMemcpy(s->d_goal_pool, out.data(), sizeof(float) * m * nq, hipMemcpyHostToDevice);
    if (e != hipSuccess) return done(e, "hipMemcpy");
    if (s->d_goal_row_stats) {               // both count planes travel with their rows
        std::vector<uint64_t> cnt(2 * m), cout2(2 * m);
        e = hipMemcpy(cnt.data(), s->d_goal_row_stats, sizeof(uint64_t) * 2 * m, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return done(e, "hipMemcpy");
        for (size_t j = 0; j < m; ++j) { cout2[j] = cnt[order[j]]; cout2[m + j] = cnt[m + order[j]]; }
        e = hipMemcpy(s->d_goal_row_stats, cout2.data(), sizeof(uint64_t) * 2 * m, hipMemcpyHostToDevice);
        if (e != hipSuccess) return done(e, "hipMemcpy");
    }
    if (s->curr_L) {                         // every env keeps the pose it holds: its index becomes that row's new number
        e = hipMemcpy(d_inv, inv.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice);
        if (e != hipSuccess) return done(e, "hipMemcpy");
        unsigned g = blocks_for(s->n, 256);
        if (g > 1024u) g = 1024u;            // (grid-stride beyond)
        hipLaunchKernelGGL(rbg::goal_index_permute_kernel, dim3(g), dim3(256), 0, s->stream, s->d_goal_index, d_inv, long(s->n), uint32_t(m));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) return done(e, "index kernel");
    }
    return done(hipSuccess, "");
}

int rb_env_obs_dim(rb_sim *s, int32_t *obs_dim) {
    if (check(s) || !obs_dim) return fail(RB_EINVAL, "null argument");
    *obs_dim = s->obs_dim();
    return RB_OK;
}

int rb_env_set_goal(rb_sim *s, const float *goal_q, const uint32_t *step_num) {
    if (check(s) || !goal_q) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    const long n = s->n;
    RB_HIP(hipMemcpyAsync(s->d_rows, goal_q, sizeof(float) * n * s->n_q, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s->stream, s->d_rows, s->d_goal, s->n_q, n, s->tree ? 1 : 0);
    RB_HIP(hipGetLastError());
    if (step_num)
        RB_HIP(hipMemcpyAsync(s->d_step_num, step_num, sizeof(uint32_t) * n, hipMemcpyHostToDevice, s->stream));
    if (s->curr_L)                            // these goals are no row of the pool: RB_GOAL_INDEX_NONE, every byte 0xFF
        RB_HIP(hipMemsetAsync(s->d_goal_index, 0xFF, sizeof(uint32_t) * n, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

// RoboyEnv.step for envs [i0, i0 + cnt) on `stream`; the array arguments are those of the whole batch (the launchers apply the
// offsets).  Sub-ranges: every ball-joint form and the joint trees' one-wave-per-64-envs form (Row::ranges).
// d_cobs: where the range's critic rows go while rb_env_critic_obs_configure holds (null: the handle's plane)
static int env_step_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done,
                           float *d_cobs = nullptr) {
    if (s->critic_mask) { const int rc = critic_check(s); if (rc) return rc; }       // (before anything is enqueued)
    Launch L;
    L.i0 = i0; L.cnt = cnt; L.stream = stream; L.act = d_act; L.obs = d_obs; L.reward = d_reward; L.done = d_done;
    const int rc = dispatch(s, ENTRY_ENV, L);
    if (rc != RB_OK) return rc;
    if (s->d_goal_pool) {                     // the done envs' new goal becomes a pool row, in front of everything that reads the goal (same stream)
        const int rc1 = goal_pool_launch(s, i0, cnt, stream, d_done, d_obs);
        if (rc1) return rc1;
    }
    if (s->critic_mask) {                     // the privileged rows of the range, from the planes as the step left them (same stream)
        const int rc2 = critic_launch(s, i0, cnt, stream, d_obs, d_cobs ? d_cobs : s->d_critic);
        if (rc2) return rc2;
    }
    if (!s->done_kind) return RB_OK;
    // the episode-end codes of the range, behind whichever kernel stepped it (same stream)
    hipLaunchKernelGGL(done_kind_kernel, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, d_done, s->d_ep_cnt + 2 * size_t(s->n),
                       s->d_done_seen, s->d_done_kind, i0, i0 + cnt);
    RB_HIP(hipGetLastError());
    return RB_OK;
}

int rb_env_step_dev(rb_sim *s, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done) {
    if (check(s) || !d_act || !d_obs || !d_reward || !d_done) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (!s->tree && reinterpret_cast<uintptr_t>(d_act) % 16) return fail(RB_EINVAL, "action slab must be 16-byte aligned");
    int rc = env_step_launch(s, 0, s->n, s->stream, d_act, d_obs, d_reward, d_done);
    if (rc == RB_OK) s->env_steps += double(s->n);
    return rc;
}

int rb_env_step_critic_dev(rb_sim *s, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done, float *d_cobs) {
    if (check(s) || !d_act || !d_obs || !d_reward || !d_done || !d_cobs) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (!s->critic_mask) return fail(RB_EINVAL, "critic rows are not enabled (rb_env_critic_obs_configure)");
    if (reinterpret_cast<uintptr_t>(d_act) % 16) return fail(RB_EINVAL, "action slab must be 16-byte aligned");
    int rc = env_step_launch(s, 0, s->n, s->stream, d_act, d_obs, d_reward, d_done, d_cobs);
    if (rc == RB_OK) s->env_steps += double(s->n);
    return rc;
}

// a sub-range on a stream of the caller's choice: envs are independent, so disjoint ranges may be stepped concurrently
static int range_ok(const rb_sim *s, int64_t first, int64_t count) {
    if (first < 0 || count < 1 || first + count > s->n) return fail(RB_EINVAL, "range outside the batch");
    if (first % 256) return fail(RB_EINVAL, "a range starts at a multiple of 256 envs");
    return RB_OK;
}
int rb_env_step_range_dev(rb_sim *s, int64_t first_env, int64_t n_envs, void *hip_stream, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done) {
    if (check(s) || !d_act || !d_obs || !d_reward || !d_done) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (!s->tree && reinterpret_cast<uintptr_t>(d_act) % 16) return fail(RB_EINVAL, "action slab must be 16-byte aligned");
    if (range_ok(s, first_env, n_envs)) return RB_EINVAL;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    CallStreamScope scope(s, st);          // a first call captured on the caller's stream defers the run-time builds (capturing())
    int rc = env_step_launch(s, long(first_env), long(n_envs), st, d_act, d_obs, d_reward, d_done);
    if (rc == RB_OK) { s->env_steps += double(n_envs); rc = note_caller_stream(s, st); }
    return rc;
}
int rb_env_step_range_critic_dev(rb_sim *s, int64_t first_env, int64_t n_envs, void *hip_stream, const float *d_act, float *d_obs, float *d_reward,
                                 uint32_t *d_done, float *d_cobs) {
    if (check(s) || !d_act || !d_obs || !d_reward || !d_done || !d_cobs) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (!s->critic_mask) return fail(RB_EINVAL, "critic rows are not enabled (rb_env_critic_obs_configure)");
    if (reinterpret_cast<uintptr_t>(d_act) % 16) return fail(RB_EINVAL, "action slab must be 16-byte aligned");
    if (range_ok(s, first_env, n_envs)) return RB_EINVAL;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    CallStreamScope scope(s, st);          // a first call captured on the caller's stream defers the run-time builds (capturing())
    int rc = env_step_launch(s, long(first_env), long(n_envs), st, d_act, d_obs, d_reward, d_done, d_cobs);
    if (rc == RB_OK) { s->env_steps += double(n_envs); rc = note_caller_stream(s, st); }
    return rc;
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

static int stats_launch(rb_sim *s, double *d_out2) {
    unsigned g = blocks_for(s->n, 256);
    if (g > unsigned(STATS_BLOCKS)) g = STATS_BLOCKS;
    double *partials = s->d_stats + 8;
    unsigned int *ticket = reinterpret_cast<unsigned int *>(s->d_stats + 8 * (STATS_BLOCKS + 1));
    if (s->env_ready)
        hipLaunchKernelGGL(stats_reduce_kernel<true>, dim3(g), dim3(256), 0, s->stream, s->d_ep_sum, s->d_ep_cnt, s->d_ep_ret,
                           s->d_infeas_n, s->d_feas, partials, ticket, s->d_stats, d_out2, s->env_steps, s->n);
    else
        hipLaunchKernelGGL(stats_reduce_kernel<false>, dim3(g), dim3(256), 0, s->stream, nullptr, s->d_ep_cnt, s->d_ep_ret,
                           s->d_infeas_n, s->d_feas, partials, ticket, s->d_stats, d_out2, s->env_steps, s->n);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
static int stats_reset(rb_sim *s) {
    if (s->env_ready) {
        RB_HIP(hipMemsetAsync(s->d_ep_sum, 0, sizeof(double) * size_t(s->n) * 2, s->stream));
        RB_HIP(hipMemsetAsync(s->d_ep_cnt, 0, sizeof(uint32_t) * size_t(s->n) * 3, s->stream));
        if (s->done_kind) RB_HIP(hipMemsetAsync(s->d_done_seen, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
        if (s->curr_L) RB_HIP(hipMemsetAsync(s->d_goal_seen, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    }
    RB_HIP(hipMemsetAsync(s->d_infeas_n, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    s->env_steps = 0.0;
    return RB_OK;
}

int rb_env_stats_dev(rb_sim *s, double *d_stats8, int reset) {
    if (check(s) || !d_stats8) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    int rc = stats_launch(s, d_stats8);
    if (rc) return rc;
    return reset ? stats_reset(s) : RB_OK;
}

int rb_env_stats(rb_sim *s, double *stats8, int reset) {
    if (check(s) || !stats8) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    int rc = stats_launch(s, nullptr);
    if (rc) return rc;
    RB_HIP(hipMemcpyAsync(stats8, s->d_stats, sizeof(double) * 8, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return reset ? stats_reset(s) : RB_OK;
}

// ---- tendon state readout (tendon_state.hpp): one kernel per robot class, not a row of the dispatch table ----
namespace {
int tendon_state_check(rb_sim *s, const float *act, int mode, float act_scale) {
    if (check(s)) return RB_EINVAL;
    if (s->params) return params_refuse(s, "the tendon-state readout (rb_tendon_state_dev)");
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
                    s->hist_rows && entry == ENTRY_ENV
                        ? "action rows are set (rb_env_action_obs_configure): the history env-step kernels (env_hist.hpp) are not rows of the dispatch table"
                    : s->params ? "per-env parameters are enabled: the parameter kernels (env_params.hpp) are not rows of the dispatch table"
                    : s->io   ? "an io configuration is set (rb_env_io_configure): the io env-step kernels (env_io.hpp) are not rows of the dispatch table"
                              : "tendon channels are set (rb_env_obs_configure): the extended env-step kernels (env_obs.hpp) are not rows of the dispatch table");
    RB_HIP(hipSetDevice(s->device));
    if (entry != ENTRY_ENV || s->env_ready) maybe_jit(s);
    std::string why;
    const Row *r = row_for(s, entry, /*build=*/entry != ENTRY_ENV || s->env_ready, &why);
    if (!r) return fail(RB_EUNSUPPORTED, why);
    *out = public_row(*r);
    return RB_OK;
}

// ---- per-env physical parameters (env_params.hpp) ----
int rb_params_enable(rb_sim *s, int32_t *n_params) {
    if (check(s)) return RB_EINVAL;
    if (s->tree) return fail(RB_EUNSUPPORTED, "per-env parameters are built for ball-joint robots (the closed-form kernels); joint trees have none");
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // nothing in flight may read the planes while they are reset
    if (rc) return rc;
    rc = drop_graphs(s);                     // captured graphs hold the nominal kernels' nodes
    if (rc) return rc;
    const int nt = s->n_t, P = rbp::n_params(nt);
    const size_t n = size_t(s->n);
    if (!s->d_params) {
        hipError_t e = hipMalloc(&s->d_params, sizeof(float) * size_t(P) * n);
        if (e == hipSuccess) e = hipMalloc(&s->d_param_draws, sizeof(uint32_t) * n);
        if (e == hipSuccess) e = hipMalloc(&s->d_param_ranges, sizeof(float) * 2 * size_t(P));
        if (e != hipSuccess) {
            params_free(s);
            return fail(e == hipErrorOutOfMemory ? RB_ENOMEM : RB_EHIP, std::string("parameter planes: ") + hipGetErrorString(e));
        }
    }
    // nominal values: force scales 1, offsets 0, mass scale 1, damping scales 1; counters 0; ranges lo = hi = nominal, no redraw
    uint32_t one, zero = 0u;
    const float onef = 1.0f;
    std::memcpy(&one, &onef, 4);
    RB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->d_params), int(one), size_t(nt) * n, s->stream));
    RB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->d_params + size_t(nt) * n), int(zero), size_t(nt) * n, s->stream));
    RB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->d_params + size_t(2 * nt) * n), int(one), 4 * n, s->stream));
    RB_HIP(hipMemsetAsync(s->d_param_draws, 0, sizeof(uint32_t) * n, s->stream));
    s->param_ranges.assign(2 * size_t(P), 1.0f);
    for (int k = 0; k < nt; ++k) s->param_ranges[nt + k] = s->param_ranges[P + nt + k] = 0.0f;
    RB_HIP(hipMemcpyAsync(s->d_param_ranges, s->param_ranges.data(), sizeof(float) * 2 * size_t(P), hipMemcpyHostToDevice, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    s->n_params = P;
    s->param_resample = false;
    s->params = true;
    if (n_params) *n_params = P;
    return RB_OK;
}
int rb_params_disable(rb_sim *s) {
    if (check(s)) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);
    if (rc) return rc;
    rc = drop_graphs(s);                     // captured graphs hold the parameter kernels' nodes
    if (rc) return rc;
    params_free(s);
    return RB_OK;
}
int rb_params_ptr(rb_sim *s, float **d_params, uint32_t **d_draws) {
    if (check(s)) return RB_EINVAL;
    if (!s->params) return fail(RB_EINVAL, "per-env parameters are not enabled (rb_params_enable)");
    if (d_params) *d_params = s->d_params;
    if (d_draws) *d_draws = s->d_param_draws;
    return RB_OK;
}
int rb_params_set_ranges(rb_sim *s, const float *lo, const float *hi, int resample_on_reset) {
    if (check(s) || !lo || !hi) return fail(RB_EINVAL, "null argument");
    if (!s->params) return fail(RB_EINVAL, "per-env parameters are not enabled (rb_params_enable)");
    const int nt = s->n_t, P = s->n_params;
    for (int p = 0; p < P; ++p) {
        const std::string at = "parameter " + std::to_string(p) + ": ";
        if (!std::isfinite(lo[p]) || !std::isfinite(hi[p])) return fail(RB_EINVAL, at + "range bounds must be finite");
        if (lo[p] > hi[p]) return fail(RB_EINVAL, at + "lo > hi");
        if (p == 2 * nt && !(lo[p] > 0.0f)) return fail(RB_EINVAL, at + "mass_scale must stay > 0");
        if ((p < nt || p > 2 * nt) && lo[p] < 0.0f) return fail(RB_EINVAL, at + "force_scale and damping_scale must stay >= 0");
    }
    RB_HIP(hipSetDevice(s->device));
    int rc = drain(s);                       // (a kernel in flight may be reading the ranges)
    if (rc) return rc;
    s->param_ranges.assign(lo, lo + P);
    s->param_ranges.insert(s->param_ranges.end(), hi, hi + P);
    RB_HIP(hipMemcpyAsync(s->d_param_ranges, s->param_ranges.data(), sizeof(float) * 2 * size_t(P), hipMemcpyHostToDevice, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    s->param_resample = resample_on_reset != 0;
    return RB_OK;
}
int rb_params_sample_dev(rb_sim *s, const uint8_t *d_mask) {
    if (check(s)) return RB_EINVAL;
    if (!s->params) return fail(RB_EINVAL, "per-env parameters are not enabled (rb_params_enable)");
    RB_HIP(hipSetDevice(s->device));
    hipLaunchKernelGGL(rbp::params_sample, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->d_params, s->d_param_draws, s->d_param_ranges,
                       d_mask, s->n_params, s->n, s->seed, uint64_t(s->env0));
    RB_HIP(hipGetLastError());
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
