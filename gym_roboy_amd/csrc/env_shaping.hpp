// env_shaping.hpp - regularising reward terms around the fused env step (rb_env_shaping_*): an action-rate term and two
// effort terms, for both robot classes and every kernel form, because no env-step kernel changes.  With the option on, the reward an
// env step returns is
//     reward[i] = fl32( r_step[i] - cost[i] )                                     (one rounding)
//     cost[i]   = w_r c_rate + w_f c_tension + w_a c_activation                    (combine(): three fp32 roundings, fixed order)
// evaluated at the state s_t the env is in BEFORE the step and the action row a_t handed to this step - the cost of (s_t, a_t), which
// an auto-reset inside the step does not disturb:
//     c_rate       = mean_k (â_k - p_k)^2     â = rbe::clip_action(a_t), p = the clamped row of the same episode's previous step;
//                                             0 on an episode's first step (entered with step_num == 1: env_io.hpp's rule for its ring)
//     c_tension    = mean_k (F_k / F_max,k)^2 F, act: the tendon-state readout (tendon_state.hpp) at s_t under the env layer's
//     c_activation = mean_k act_k^2           set-points for a_t (RB_SP_ENV through rbts::offset_of): what rb_tendon_state_dev reports
// THE ORDER OF THE SUMS.  Each env's three means are summed over k ascending, one after the other, in fp32 (s = fmaf(x, x, s) from
// s = 0, then one division by n_t), by ONE lane.  So a cost does not depend on the batch size, on the launch range, or on the kernel
// form the step runs in: the tests rely on this (bit-equal costs across forms and across whole-batch / sub-range steps).
// Not rows of the dispatch table.  Two kernels around the env-step kernel, on its stream, over its envs [i0, i1):
//   shaping_cost   IN FRONT.  One instance per robot class, following tendon_state.hpp's kernels: ball joints - one env per lane,
//                  256-thread groups, 8 tendons written out (rows as two float4) or 1..16 rolled, Model::tendon_state per tendon;
//                  joint trees - tables staged to LDS, sweep_p1, one lane per (env, tendon) calling p2_tendon_state, the per-tendon
//                  terms to the wave's LDS region (behind the working sets), then one lane per env adds them up in order.
//                  No [n][n_t] array of readings is ever written to memory: per env the kernel reads q, qd, the action row and the
//                  previous row, and writes the previous row and 4 bytes of cost.  With w_f == w_a == 0 (uniform) the tendon
//                  evaluation is skipped, and so is the joint trees' table staging; with w_r == 0 the previous rows are not touched.
//   shaping_apply  BEHIND, first in behind_step(): reward -= cost; the cost is added to the env's running episode cost and to its
//                  all-steps sum (fp64: every addend is an exact fp32 value), a step is counted; on a done word - read as a flag,
//                  before done_kind_kernel turns it into a code - the episode cost goes to the env's finished-episodes sum and
//                  count (rbe::stat_add) and the running value restarts at 0.  Every slot is touched by its own env's lane only.
//   shaping_reduce / shaping_reduce_final   the statistics, in a fixed order (two launches: block partials, then one block).
// None of the kernels uses scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "env_common.hpp"
#include "tendon_state.hpp"

namespace rbs {

// planes of the whole batch; the kernels index them with the env's number in the batch
struct CostArgs {
    const float *q, *qd;             // ball joints: planes [3][n]; joint trees: rows [n][n_q]
    const float *act;                // [n][n_t], the rows handed to this step
    const uint32_t *step_num;        // [n], as the step will find it: 1 = the episode's first step
    float *prev;                     // [n][n_t]: the clamped row of the env's previous step (this option's own plane)
    float *cost;                     // [n]
    float w_rate, w_tension, w_act;
    float slope, act_hi;             // the env layer's action box (RB_SP_ENV)
    long n, i0, i1;
};

__device__ __forceinline__ float combine(const CostArgs &a, float c_rate, float c_tension, float c_act) {
    return fmaf(a.w_act, c_act, fmaf(a.w_tension, c_tension, a.w_rate * c_rate));
}
__device__ __forceinline__ rbts::SetPoints env_setpoints(const CostArgs &a) {
    return rbts::SetPoints{a.act, RB_SP_ENV, 0.0f, a.slope, a.act_hi};
}

// ---- ball joints, 8 tendons written out ----
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
msj_shaping_cost8(const rbk::Const8 c, const rbts::Units<8> pu, const CostArgs a) {
    using Model = rb::MsjModel<float, 8>;
    const long i = a.i0 + long(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= a.i1) return;
    const float4 a0 = reinterpret_cast<const float4 *>(a.act)[2 * i];
    const float4 a1 = reinterpret_cast<const float4 *>(a.act)[2 * i + 1];
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    float c_rate = 0.0f, c_tension = 0.0f, c_act = 0.0f;
    if (a.w_rate != 0.0f) {
        float ah[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) ah[k] = rbe::clip_action(av[k]);
        float4 *pp = reinterpret_cast<float4 *>(a.prev) + 2 * i;
        if (a.step_num[i] != 1u) {
            const float4 p0 = pp[0], p1 = pp[1];
            const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float d = ah[k] - pv[k]; c_rate = fmaf(d, d, c_rate); }
            c_rate = c_rate / 8.0f;
        }
        pp[0] = make_float4(ah[0], ah[1], ah[2], ah[3]);
        pp[1] = make_float4(ah[4], ah[5], ah[6], ah[7]);
    }
    if (a.w_tension != 0.0f || a.w_act != 0.0f) {
        const long n = a.n;
        float qq[3], vv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { qq[j] = a.q[j * n + i]; vv[j] = a.qd[j * n + i]; }
        const rbts::SetPoints sp = env_setpoints(a);
        const Model::Frame f = Model::frame(qq, vv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const rb::TendonReading<float> r = Model::tendon_state(c, f, c.ten[k], pu.u[k], rbts::offset_of(sp, av[k], c.ten[k].ksg));
            const float x = r.force / pu.u[k].fmax;
            c_tension = fmaf(x, x, c_tension);
            c_act = fmaf(r.activation, r.activation, c_act);
        }
        c_tension = c_tension / 8.0f;
        c_act = c_act / 8.0f;
    }
    a.cost[i] = combine(a, c_rate, c_tension, c_act);
}

// ---- ball joints, 1..16 tendons: the tendon loop rolled, its trip count c.nt read at run time ----
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
msj_shaping_cost_nt(const rbk::ConstX c, const rbts::Units<rbk::NTX> pu, const CostArgs a) {
    using Model = rb::MsjModel<float, rbk::NTX>;
    const long i = a.i0 + long(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= a.i1) return;
    const int nt = c.nt;
    const long row = i * nt;
    const float fnt = float(nt);
    float c_rate = 0.0f, c_tension = 0.0f, c_act = 0.0f;
    if (a.w_rate != 0.0f) {
        const bool first = a.step_num[i] == 1u;
#pragma unroll 1
        for (int k = 0; k < nt; ++k) {
            const float ah = rbe::clip_action(a.act[row + k]);
            if (!first) { const float d = ah - a.prev[row + k]; c_rate = fmaf(d, d, c_rate); }
            a.prev[row + k] = ah;
        }
        c_rate = c_rate / fnt;
    }
    if (a.w_tension != 0.0f || a.w_act != 0.0f) {
        const long n = a.n;
        float qq[3], vv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { qq[j] = a.q[j * n + i]; vv[j] = a.qd[j * n + i]; }
        const rbts::SetPoints sp = env_setpoints(a);
        const Model::Frame f = Model::frame(qq, vv);
#pragma unroll 1
        for (int k = 0; k < nt; ++k) {
            const rb::TendonReading<float> r = Model::tendon_state(c, f, c.ten[k], pu.u[k], rbts::offset_of(sp, a.act[row + k], c.ten[k].ksg));
            const float x = r.force / pu.u[k].fmax;
            c_tension = fmaf(x, x, c_tension);
            c_act = fmaf(r.activation, r.activation, c_act);
        }
        c_tension = c_tension / fnt;
        c_act = c_act / fnt;
    }
    a.cost[i] = combine(a, c_rate, c_tension, c_act);
}

// ---- behind the env step: reward, running episode cost, statistics ----
struct ApplyArgs {
    float *reward;                   // [n]: what the env step wrote
    const float *cost;               // [n]
    const uint32_t *done;            // [n]: read as a flag
    double *run;                     // [n]: the running episode's cost
    double *sums;                    // [2][n]: finished episodes' costs, all step costs
    uint32_t *cnt;                   // [2][n]: finished episodes, steps
    long n, i0, i1;
};
__global__ void __launch_bounds__(256) shaping_apply(const ApplyArgs a) {
    const long i = a.i0 + long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.i1) return;
    const float c = a.cost[i];
    a.reward[i] = a.reward[i] - c;
    double run = a.run[i] + double(c);
    rbe::stat_add(&a.sums[a.n + i], double(c));
    rbe::stat_add(&a.cnt[a.n + i], 1u);
    if (a.done[i]) {
        rbe::stat_add(&a.sums[i], run);
        rbe::stat_add(&a.cnt[i], 1u);
        run = 0.0;
    }
    a.run[i] = run;
}

// ---- the statistics: {sum of finished episodes' costs, finished episodes, sum of all step costs, steps}, a fixed order of additions.
//      Block b adds up the envs b * 256 + t, + gridDim * 256, ... per thread, then the threads by a fixed shuffle / LDS tree, and leaves
//      its four sums in partials[b]; the second launch (one block, thread b owns block b's row) adds those the same way. ----
constexpr int REDUCE_BLOCKS = 256;
__device__ __forceinline__ void block_sum4(double v[4], double (*sh)[4]) {      // -> every thread's v = the block's sums
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) sh[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
}
__global__ void __launch_bounds__(256) shaping_reduce(const double *sums, const uint32_t *cnt, double *partials, long n) {
    __shared__ double sh[4][4];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (long i = long(blockIdx.x) * 256 + threadIdx.x; i < n; i += long(gridDim.x) * 256) {
        v[0] += sums[i]; v[1] += double(cnt[i]); v[2] += sums[n + i]; v[3] += double(cnt[n + i]);
    }
    block_sum4(v, sh);
    if (threadIdx.x < 4) partials[blockIdx.x * 4 + threadIdx.x] = v[threadIdx.x];
}
__global__ void __launch_bounds__(256) shaping_reduce_final(const double *partials, int blocks, double *out) {
    __shared__ double sh[4][4];
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = int(threadIdx.x) < blocks ? partials[threadIdx.x * 4 + k] : 0.0;
    block_sum4(v, sh);
    if (threadIdx.x < 4) out[threadIdx.x] = v[threadIdx.x];
}

}  // namespace rbs

namespace rbt {

// ---- joint trees: tree_tendon_state's launch configuration (tree_waves waves per workgroup) with 3 E n_t floats of LDS per wave
//      behind the working sets: the per-tendon terms [E][3][n_t] (rate, tension, activation).  Envs [a.i0, a.i1) of rows q[n][n_q]. ----
template <int E, bool SP>
__global__ void __launch_bounds__(512, RB_TREE_MIN_WAVES)
tree_shaping_cost(const TreeDev tg, const float *__restrict__ lconst, const rbs::CostArgs a) {
    constexpr int NP = Passes<E>::N;
    extern __shared__ float4 lds_raw4[];
    float *lds = reinterpret_cast<float *>(lds_raw4);
    const bool tendons = a.w_tension != 0.0f || a.w_act != 0.0f;      // (uniform)
    if (tendons) stage_tables(tg, lds, threadIdx.x, blockDim.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long env0 = a.i0 + (long(blockIdx.x) * nw + wave) * E;
    if (env0 >= a.i1) return;                                   // whole wave idle (no barrier follows)
    const int nt = tg.n_t;
    const Ctx c{tg, lds, lds + 4 * tg.n_vec4 + wave * (E * tg.ES), lane};
    float *terms = lds + 4 * tg.n_vec4 + nw * (E * tg.ES) + wave * (3 * E * nt);
    if (tendons) {
        // as tree_tendon_state: a slot past the end of the range shadows its last env and stores nothing
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            int e, j;
            if (joint_slot<E>(tg, lane, p, e, j)) {
                const long env = env0 + e < a.i1 ? env0 + e : a.i1 - 1;
                const float *jr = c.tab + tg.o_joint + __mul24(j, JOINT_REC);
                const Rot r = rodrigues({jr[4], jr[5], jr[6]}, a.q[env * tg.n_q + j]);
                float *dst = c.env(e) + tg.o_W + tg.n_q + __mul24(j, ROT);
                st3(dst, r.c0); st3(dst + 3, r.c1); st3(dst + 6, r.c2);
                (c.env(e) + tg.o_SQD)[j] = a.qd[env * tg.n_q + j];
            }
        }
        wave_sync();
        sweep_p1<E, SP>(c);
    }
    const rbts::SetPoints sp = rbs::env_setpoints(a);
    for (int it = lane; it < E * nt; it += 64) {
        int e, k;
        split<E>(it, nt, e, k);
        const long env = env0 + e;
        if (env >= a.i1) continue;
        const long o = env * nt + k;
        const float act = a.act[o];
        float t_rate = 0.0f, t_tension = 0.0f, t_act = 0.0f;
        if (a.w_rate != 0.0f) {
            const float ah = rbe::clip_action(act);
            if (a.step_num[env] != 1u) { const float d = ah - a.prev[o]; t_rate = d; }
            a.prev[o] = ah;
        }
        if (tendons) {
            const float u = rbts::offset_of(sp, act, c.tf(tg.o_tendon + k * TENDON_REC + 2));
            const rb::TendonReading<float> r = p2_tendon_state(c, e, k, u, lconst[k]);
            t_tension = r.force / c.tf(tg.o_tendon + k * TENDON_REC + 3);
            t_act = r.activation;
        }
        float *te = terms + e * (3 * nt);
        te[k] = t_rate; te[nt + k] = t_tension; te[2 * nt + k] = t_act;
    }
    wave_sync();
    if (lane < E && env0 + lane < a.i1) {
        const float *te = terms + lane * (3 * nt);
        float s[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            float acc = 0.0f;
            for (int k = 0; k < nt; ++k) { const float x = te[m * nt + k]; acc = fmaf(x, x, acc); }
            s[m] = acc / float(nt);
        }
        a.cost[env0 + lane] = rbs::combine(a, s[0], s[1], s[2]);
    }
}

}  // namespace rbt
