// tendon_state.hpp - the tendon-state readout (rb_tendon_state_dev): length, length rate, activation and force of every
// tendon of every env at the handle's current state, under given set-points, without modifying the state.  DESIGN.md §11.
//
// Not rows of the dispatch table (roboy_dispatch.hpp keys the three step entry kinds): one kernel per robot class.
//   * ball joints (msj_math.hpp's closed form): one env per lane, 256-thread workgroups, robot constants through the kernarg
//     (SGPRs) as in the RB_SPEC_NONE step instances, plus one TendonUnits record per tendon for the physical units.  Two
//     instances: 8 tendons written out (rows of 32 bytes: two dwordx4 loads per lane, two dwordx4 stores per output), and
//     1..16 tendons in a rolled loop with the count read at run time (c.nt).  Per tendon: MsjModel::tendon_state, the
//     readout twin of the step's tendon() / tendon_force().
//   * joint trees (tree_aba.hpp's tables, whichever step form the handle uses): E envs per wave, tables staged to LDS, the
//     step's own P1 sweep (sweep_p1) for world frames and velocities, then one lane per (env, tendon) evaluates
//     p2_tendon_state, the readout twin of p2_tendon, and stores.  The constant length of the same-link segments - which
//     the step folds into its strain constant - comes from a small buffer of its own (tree_build.hpp: tree_tendon_lconst).
// Activation offsets are formed with the step's own products (rb_step_dev: act * (act_scale * ksg); rb_env_step_dev: the
// env layer's rescale, then * ksg), so activation and force are what the next step's first acceleration evaluation uses.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/roboy_sim.h"
#include "env_common.hpp"
#include "msj_kernels.hpp"
#include "msj_math.hpp"
#include "tree_aba.hpp"

namespace rbts {

// how a lane turns its action row into activation offsets
struct SetPoints {
    const float *act;      // [n][n_t], or nullptr: every set-point 0
    int mode;              // RB_SP_SCALED / RB_SP_ENV
    float scale;           // RB_SP_SCALED: set-point = scale * act
    float slope, act_hi;   // RB_SP_ENV: set-point = slope * (clamp(act, -1, 1) - 1) + act_hi, two roundings (roboy_env.py:157-158)
};
// [n][n_t] outputs; a null pointer is not written
struct Outputs { float *length, *rate, *activation, *force; };

template <int NT> struct Units { rb::TendonUnits<float> u[NT]; };

// activation offset of one tendon from its action (ksg: the tendon's set-point -> activation factor), rounded here as in the step
__device__ __forceinline__ float offset_of(const SetPoints &sp, float a, float ksg) {
    const float u = sp.mode == RB_SP_ENV ? rbe::action_setpoint(sp.slope, a, sp.act_hi) * ksg
                                         : a * (sp.scale * ksg);
    return rbe::rounded_here(u);
}

// ---- ball joints, 8 tendons written out.  Loads: q, qd planes (dword per lane) and the 32-byte action row; stores: four
//      32-byte rows.  184 algorithmic bytes per env. ----
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
msj_tendon_state8(const rbk::Const8 c, const Units<8> pu, const float *__restrict__ q, const float *__restrict__ qd,
                  const SetPoints sp, const Outputs out, long n) {
    using Model = rb::MsjModel<float, 8>;
    const long i = long(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    float qq[3], vv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + i]; vv[j] = qd[j * n + i]; }
    float u[8];
    if (sp.act) {
        const float4 a0 = reinterpret_cast<const float4 *>(sp.act)[2 * i];
        const float4 a1 = reinterpret_cast<const float4 *>(sp.act)[2 * i + 1];
        const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) u[k] = offset_of(sp, a[k], c.ten[k].ksg);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) u[k] = 0.0f;
    }
    const Model::Frame f = Model::frame(qq, vv);
    float L[8], R[8], A[8], F[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const rb::TendonReading<float> r = Model::tendon_state(c, f, c.ten[k], pu.u[k], u[k]);
        L[k] = r.length; R[k] = r.rate; A[k] = r.activation; F[k] = r.force;
    }
    auto store = [&](float *dst, const float *v) {
        if (!dst) return;
        float4 *p = reinterpret_cast<float4 *>(dst) + 2 * i;
        p[0] = make_float4(v[0], v[1], v[2], v[3]);
        p[1] = make_float4(v[4], v[5], v[6], v[7]);
    };
    store(out.length, L); store(out.rate, R); store(out.activation, A); store(out.force, F);
}

// ---- ball joints, 1..16 tendons: the tendon loop rolled, its trip count c.nt read at run time (one scalar load of the
//      tendon's records per trip) ----
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
msj_tendon_state_nt(const rbk::ConstX c, const Units<rbk::NTX> pu, const float *__restrict__ q, const float *__restrict__ qd,
                    const SetPoints sp, const Outputs out, long n) {
    using Model = rb::MsjModel<float, rbk::NTX>;
    const long i = long(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    float qq[3], vv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + i]; vv[j] = qd[j * n + i]; }
    const Model::Frame f = Model::frame(qq, vv);
    const int nt = c.nt;
    const long row = i * nt;
#pragma unroll 1
    for (int k = 0; k < nt; ++k) {
        const float u = sp.act ? offset_of(sp, sp.act[row + k], c.ten[k].ksg) : 0.0f;
        const rb::TendonReading<float> r = Model::tendon_state(c, f, c.ten[k], pu.u[k], u);
        if (out.length) out.length[row + k] = r.length;
        if (out.rate) out.rate[row + k] = r.rate;
        if (out.activation) out.activation[row + k] = r.activation;
        if (out.force) out.force[row + k] = r.force;
    }
}

}  // namespace rbts

namespace rbt {

// The readout twin of p2_tendon (tree_aba.hpp): the same crossings, length, rate and Hill force - change the two together -
// but the tendon's state in physical units instead of the wrenches.  u: activation offset; lconst: the same-link segments.
__device__ __forceinline__ rb::TendonReading<float> p2_tendon_state(const Ctx &c, int e, int k, float u, float lconst) {
    const TreeDev &t = c.t;
    const int c0 = c.ti(t.o_t_cr_start + k), c1 = c.ti(t.o_t_cr_start + k + 1);
    float len = 0.0f, ldot = 0.0f;
    for (int cr = c0; cr < c1; ++cr) {
        const float *rec = c.tab + t.o_cross + cr * CROSS_REC;
        const int la = __float_as_int(rec[0]), lb = __float_as_int(rec[1]);
        V3 xa, va, xb, vb;
        point_on_link(c, e, la, ld3(rec + 2), xa, va);
        point_on_link(c, e, lb, ld3(rec + 5), xb, vb);
        const V3 d = xb - xa;
        const float d2 = dot(d, d), inv = __builtin_amdgcn_rsqf(d2);
        len += d2 * inv;
        ldot += dot(d * inv, vb - va);
    }
    const float *tr = c.tab + t.o_tendon + k * TENDON_REC;
    const float es = len * tr[0] + tr[1];
    const float act = __builtin_amdgcn_fmed3f(t.kps * es - u, 0.0f, 1.0f);
    const float fl = __builtin_amdgcn_exp2f(-(es * es));
    const float v = ldot * tr[4];
    const float vp = fmaxf(v, 0.0f), p = __builtin_amdgcn_fmed3f(v + 1.0f, 0.0f, 1.0f);
    const float num = t.fv_c1l * vp + p, den = t.fv_c2l * vp + (t.fv_c2s * p + t.fv_k);
    const float fpe = fmaxf(__builtin_amdgcn_exp2f(t.pe_k2s * es) * t.inv_pe_den - t.inv_pe_den, 0.0f);
    rb::TendonReading<float> r;
    r.length = len + lconst;
    r.rate = ldot;
    r.activation = act;
    r.force = tr[3] * ((act * fl) * num * __builtin_amdgcn_rcpf(den) + fpe);
    return r;
}

// E envs per wave, the launch configuration of tree_step_aba (tree_waves waves per workgroup, tree_lds_bytes of LDS).
// State rows q[n][n_q], qd[n][n_q]; outputs [n][n_t].
template <int E, bool SP>
__global__ void __launch_bounds__(512, RB_TREE_MIN_WAVES)
tree_tendon_state(const TreeDev tg, const float *__restrict__ lconst, const float *__restrict__ q, const float *__restrict__ qd,
                  const rbts::SetPoints sp, const rbts::Outputs out, long n) {
    constexpr int NP = Passes<E>::N;
    extern __shared__ float4 lds_raw4[];
    float *lds = reinterpret_cast<float *>(lds_raw4);
    stage_tables(tg, lds, threadIdx.x, blockDim.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long env0 = (long(blockIdx.x) * nw + wave) * E;
    if (env0 >= n) return;                                      // whole wave idle (no barrier follows)
    const Ctx c{tg, lds, lds + 4 * tg.n_vec4 + wave * (E * tg.ES), lane};
    // the joints' rotations and velocities where sweep_p1 looks for them (as tree_accel stages them); a slot past the end
    // of the batch shadows the last env and stores nothing
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        int e, j;
        if (joint_slot<E>(tg, lane, p, e, j)) {
            const long env = env0 + e < n ? env0 + e : n - 1;
            const float *jr = c.tab + tg.o_joint + __mul24(j, JOINT_REC);
            const Rot r = rodrigues({jr[4], jr[5], jr[6]}, q[env * tg.n_q + j]);
            float *dst = c.env(e) + tg.o_W + tg.n_q + __mul24(j, ROT);
            st3(dst, r.c0); st3(dst + 3, r.c1); st3(dst + 6, r.c2);
            (c.env(e) + tg.o_SQD)[j] = qd[env * tg.n_q + j];
        }
    }
    wave_sync();
    sweep_p1<E, SP>(c);
    for (int it = lane; it < E * tg.n_t; it += 64) {
        int e, k;
        split<E>(it, tg.n_t, e, k);
        const long env = env0 + e;
        if (env >= n) continue;
        const long o = env * tg.n_t + k;
        const float u = sp.act ? rbts::offset_of(sp, sp.act[o], c.tf(tg.o_tendon + k * TENDON_REC + 2)) : 0.0f;
        const rb::TendonReading<float> r = p2_tendon_state(c, e, k, u, lconst[k]);
        if (out.length) out.length[o] = r.length;
        if (out.rate) out.rate[o] = r.rate;
        if (out.activation) out.activation[o] = r.activation;
        if (out.force) out.force[o] = r.force;
    }
}

}  // namespace rbt
