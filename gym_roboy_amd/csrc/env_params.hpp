// env_params.hpp - per-env physical parameters of the ball-joint class and their on-device redraw (rb_params_*).  DESIGN.md §12.
//
// Included by roboy_sim.hip only: hiprtc (msj_kernels.hpp, msj_jit.hpp) compiles none of these kernels.  Not rows of the dispatch
// table: while a handle has parameters enabled, dispatch() launches these kernels for the step and env-step entries instead of the
// handle's row.  Planes, fp32, struct-of-arrays [P][n_envs] with P = 2 n_t + 4 (rb_params_count):
//     0 .. n_t-1        force_scale[k]      multiplies tendon k's tension (F_max, passive term included)
//     n_t .. 2n_t-1     setpoint_offset[k]  m, added to tendon k's set-point after the step's own rescale
//     2n_t              mass_scale          multiplies I_O and m c (not the armature)
//     2n_t+1 .. 2n_t+3  damping_scale[j]    multiplies joint j's viscous damping
// The offset folds into the activation offset u; the other three enter MsjModel additively (scaled_tendon: the force
// scale; rigid_body's body policy: mass and damping), whose identity defaults leave every other kernel as it was.
//
// One env per lane at every batch size: mirror pairs and tendon-per-lane rely on every env being the same robot.  Per env step the
// lane reads its P values once (dword per lane, 256 B contiguous per wave and plane), besides what the nominal step reads.
#pragma once
#include <hip/hip_runtime.h>

#include "env_common.hpp"
#include "msj_kernels.hpp"
#include "msj_math.hpp"
#include "philox.hpp"

namespace rbp {

using rbk::Const8;
using rbk::ConstX;
using rbk::MsjEnvArgs;
using rbk::NT8;
using rbk::NTX;
using rbk::Scale8;

__host__ __device__ constexpr int n_params(int nt) { return 2 * nt + 4; }

// rigid_body()'s body policy of one env (msj_math.hpp: NominalBody is the identity)
struct BodyScale {
    float ms, ds[3];
    __device__ __forceinline__ float mass(float x) const { return ms * x; }
    __device__ __forceinline__ float damping(int j, float x) const { return ds[j] * x; }
};

// NT tendons written out, each behind a scheduling barrier (MsjModel::AccelPinned with the env's scales)
template <int NT>
struct AccelScaled {
    const rb::MsjConst<float, NT> &c;
    const float *u, *fs;                 // activation offsets, force scales
    const BodyScale &bs;
    __device__ __forceinline__ void operator()(const float q[3], const float qd[3], float qdd[3]) const {
        using M = rb::MsjModel<float, NT>;
        const typename M::Frame f = M::frame(q, qd);
        float tx = 0.0f, ty = 0.0f, tz = 0.0f;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            M::tendon(c, f, M::scaled_tendon(c.ten[k], fs[k]), u[k], tx, ty, tz);
            __builtin_amdgcn_sched_barrier(0);
        }
        M::rigid_body(c, f, qd, tx, ty, tz, qdd, &bs);
    }
};

// A rolled tendon loop (robot constants through the kernarg: one scalar load of the tendon's record per trip, as in the nominal
// kernarg instances - written out, all NT records would be held in scalar registers across the integrator; or RUNTIME_NT: c.nt
// trips).  Activation offset and force scale of tendon k come from the lane's LDS column, col[k * stride] and col[(NT + k) * stride]:
// a rolled loop cannot index registers.
template <int NT, bool RUNTIME_NT>
struct AccelScaledLds {
    const rb::MsjConst<float, NT> &c;
    const float *col;
    int stride;
    const BodyScale &bs;
    __device__ __forceinline__ void operator()(const float q[3], const float qd[3], float qdd[3]) const {
        using M = rb::MsjModel<float, NT>;
        const typename M::Frame f = M::frame(q, qd);
        float tx = 0.0f, ty = 0.0f, tz = 0.0f;
        if constexpr (RUNTIME_NT) {
#pragma unroll 1
            for (int k = 0; k < c.nt; ++k) M::tendon(c, f, M::scaled_tendon(c.ten[k], col[(NT + k) * stride]), col[k * stride], tx, ty, tz);
        } else {
#pragma unroll 2
            for (int k = 0; k < NT; ++k) M::tendon(c, f, M::scaled_tendon(c.ten[k], col[(NT + k) * stride]), col[k * stride], tx, ty, tz);
        }
        M::rigid_body(c, f, qd, tx, ty, tz, qdd, &bs);
    }
};

// Draw number draws[i] of env i (global id gid) into its planes; draws[i] advances by one.  Block b of the draw is
// philox_draw(seed, gid, d, STREAM_PARAMS, b); parameter p takes word p mod 4 of block p / 4 and becomes
// lo_p + (hi_p - lo_p) u01(word) with two roundings (goal_value).  ranges: lo[np] then hi[np].
__device__ __forceinline__ void draw_params(float *__restrict__ par, uint32_t *__restrict__ draws, const float *__restrict__ ranges,
                                            int np, long n, long i, uint64_t seed, uint64_t gid) {
    const uint32_t d = draws[i];
#pragma unroll 1
    for (int b = 0; 4 * b < np; ++b) {
        const rb::Philox4 r = rb::philox_draw(seed, gid, d, rb::STREAM_PARAMS, uint32_t(b));
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int p = 4 * b + w;
            if (p < np) par[p * n + i] = rbe::goal_value(ranges[p], ranges[np + p], r.v[w]);
        }
    }
    draws[i] = d + 1u;
}

// rb_params_sample_dev: envs with mask[i] != 0 (mask NULL: all) draw new parameters
__global__ void __launch_bounds__(256)
params_sample(float *__restrict__ par, uint32_t *__restrict__ draws, const float *__restrict__ ranges, const uint8_t *__restrict__ mask,
              int np, long n, uint64_t seed, uint64_t env0) {
    const long i = long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    draw_params(par, draws, ranges, np, n, i, seed, env0 + uint64_t(i));
}

// ---- the physics step.  Sub-ranges arrive on shifted pointers (q, qd, feas, act, par): the planes keep their stride n. ----

// 8 tendons (MsjRobot's baked table, BK; any other 8-tendon robot on kernarg constants): the shape of msj_step_env_per_lane_rs -
// integrator stages rolled (integrate_acc; Euler is integrate<0>), tendons written out (BK; kernarg constants: the rolled loop of
// AccelScaledLds), loads and stores through workgroup buffer resources.  Loads: q, qd, the 32-byte action record and the env's 20 parameters; 164 algorithmic bytes per env step.
template <int INTEG, int BLOCK, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_params_step(const Const8 c_arg, float *__restrict__ q, float *__restrict__ qd, uint32_t *__restrict__ feas,
                const float *__restrict__ act, const Scale8 us, const float *__restrict__ par, long n, long cnt) {
    const Const8 &c = rbk::robot_consts<BK>(c_arg);
    const long env0 = long(blockIdx.x) * BLOCK;
    const long left = cnt - env0;
    const int live = int(left < BLOCK ? left : BLOCK);
    const int le = int(threadIdx.x);
    if (le >= live) return;
    const int off = le * 4;
    auto plane = [&](const float *base, long p) {     // dword of this lane in plane p of a [.][n] array
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rbk::wg_rsrc(base + p * n + env0, live * 4), off, 0, 0));
    };
    const __amdgpu_buffer_rsrc_t ra = rbk::wg_rsrc(act + env0 * NT8, live * NT8 * 4);
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 a0 = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ra, off * NT8, 0, 0));
    const f4 a1 = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ra, off * NT8 + 16, 0, 0));
    float qq[3], vv[3], u[NT8], fs[NT8];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = plane(q, j); vv[j] = plane(qd, j); }
    const float a[NT8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int k = 0; k < NT8; ++k) {
        fs[k] = plane(par, k);
        u[k] = a[k] * us.v[k] + plane(par, NT8 + k) * c.ten[k].ksg;       // (set-point + offset) -> activation offset
    }
    BodyScale bs;
    bs.ms = plane(par, 2 * NT8);
#pragma unroll
    for (int j = 0; j < 3; ++j) bs.ds[j] = plane(par, 2 * NT8 + 1 + j);
    bool ok;
    if constexpr (BK) {
        ok = rb::MsjModel<float, NT8>::template integrate_acc<INTEG>(c, qq, vv, AccelScaled<NT8>{c, u, fs, bs});
    } else {
        __shared__ float lds[2 * NT8][BLOCK];
#pragma unroll
        for (int k = 0; k < NT8; ++k) { lds[k][threadIdx.x] = u[k]; lds[NT8 + k][threadIdx.x] = fs[k]; }
        ok = rb::MsjModel<float, NT8>::template integrate_acc<INTEG>(c, qq, vv, AccelScaledLds<NT8, false>{c, &lds[0][threadIdx.x], BLOCK, bs});
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(qq[j]), rbk::wg_rsrc(q + j * n + env0, live * 4), off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vv[j]), rbk::wg_rsrc(qd + j * n + env0, live * 4), off, 0, 0);
    }
    __builtin_amdgcn_raw_buffer_store_b32(ok ? 1u : 0u, rbk::wg_rsrc(feas + env0, live * 4), off, 0, 0);
}

// 1..16 tendons (ConstX, c.nt at run time): action rows of c.nt floats; offsets and force scales staged as the lane's LDS column
template <int INTEG, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
msj_params_step_nt(const ConstX c, float *__restrict__ q, float *__restrict__ qd, uint32_t *__restrict__ feas,
                   const float *__restrict__ act, float act_scale, const float *__restrict__ par, long n, long cnt) {
    const long i = long(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= cnt) return;
    __shared__ float lds[2 * NTX][BLOCK];
    const int nt = c.nt;
    const float *row = act + i * nt;
    for (int k = 0; k < nt; ++k) {
        lds[k][threadIdx.x] = row[k] * (act_scale * c.ten[k].ksg) + par[(nt + k) * n + i] * c.ten[k].ksg;
        lds[NTX + k][threadIdx.x] = par[k * n + i];
    }
    BodyScale bs;
    bs.ms = par[2 * nt * n + i];
#pragma unroll
    for (int j = 0; j < 3; ++j) bs.ds[j] = par[(2 * nt + 1 + j) * n + i];
    float qq[3], vv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + i]; vv[j] = qd[j * n + i]; }
    // each lane reads back only what it wrote: no barrier
    const bool ok = rb::MsjModel<float, NTX>::template integrate_acc<INTEG>(c, qq, vv, AccelScaledLds<NTX, true>{c, &lds[0][threadIdx.x], BLOCK, bs});
#pragma unroll
    for (int j = 0; j < 3; ++j) { q[j * n + i] = qq[j]; qd[j * n + i] = vv[j]; }
    feas[i] = ok ? 1u : 0u;
}

// ---- the fused env step ----
// What the parameter form of the env step takes besides MsjEnvArgs: the planes (read in front of the step), and behind it - read
// late, like MsjEnvArgs - the draw counters and ranges of the redraw on episode end.  Pointers shifted for a sub-range.
struct ParamArgs {
    float *par;
    uint32_t *draws;
    const float *ranges;             // lo[np], hi[np]
    long n;                          // stride of the planes (the handle's envs)
    int np;
    int resample;                    // redraw on done with auto_reset
};
// byte offset of the ParamArgs argument behind (constants, MsjEnvArgs)
__host__ __device__ constexpr int param_args_offset(int lead) {
    return (rbk::msj_env_args_offset(lead) + int(sizeof(MsjEnvArgs)) + int(alignof(ParamArgs)) - 1) / int(alignof(ParamArgs)) * int(alignof(ParamArgs));
}
typedef const __attribute__((address_space(4))) ParamArgs *param_kernarg_ptr;

// env_account's episode-end hook: the env's parameters are redrawn where its goal is (auto_reset, ranges set with resample)
template <typename PA>
struct RedrawParams {
    PA pa;
    __device__ __forceinline__ void operator()(long i, uint64_t gid, uint64_t seed, int auto_reset) const {
        if (!auto_reset || !pa->resample) return;
        draw_params(pa->par, pa->draws, pa->ranges, pa->np, pa->n, i, seed, gid);
    }
};

// The body as text, for the reason and with the conventions of RB_MSJ_ENV_STEP_BODY (msj_kernels.hpp): env_obs.hpp's parameter kernels
// expand it with their extension for OX; by-value arguments c_arg, a, pa; template parameters INTEG, BLOCK, CONST, BK by name.
#define RB_MSJ_PARAMS_ENV_STEP_BODY(OX) \
    constexpr bool X = std::is_same<CONST, ConstX>::value;                                                                          \
    const float *__restrict__ q = a.q, *__restrict__ qd = a.qd, *__restrict__ goal = a.goal, *__restrict__ act = a.act;             \
    const float *par = pa.par;        /* (not restrict: the redraw behind the step writes the planes) */                            \
    const long n = a.n, cnt = a.cnt;                                                                                                \
    const float slope = a.e.slope, act_hi = a.e.act_hi;                                                                             \
    const CONST &c = rbk::robot_consts<BK>(c_arg);                                                                                  \
    const long i = long(blockIdx.x) * BLOCK + threadIdx.x;                                                                          \
    if (i >= cnt) return;                                                                                                           \
    float qq[3], vv[3], gg[3];                                                                                                      \
    _Pragma("unroll")                                                                                                               \
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + i]; vv[j] = qd[j * n + i]; gg[j] = goal[j * n + i]; }                           \
    /* action -> set-point (rbe::action_setpoint) or the rest command, + the env's offset; times ksg: the activation offset         */ \
    decltype((OX).applied(a.step_num, act, i, 0)) ap{};        /* the row the lane steps with: named where each branch reads it */ \
    auto setpoint = [&](float x, float o) { return (ap.rest ? 0.0f : rbe::action_setpoint(slope, x, act_hi)) + o; };                            \
    BodyScale bs;                                                                                                                   \
    bool ok;                                                                                                                        \
    rbk::HeldOffsets held{nullptr, nullptr, 1};                                                                                     \
    constexpr bool IN_LDS = !BK;                                                                                                    \
    float u[NT8], fs[NT8];                                                                                                          \
    if constexpr (X) {                                                                                                              \
        __shared__ float lds[2 * NTX][BLOCK];                                                                                       \
        const int nt = c.nt;                                                                                                        \
        ap = (OX).applied(a.step_num, act, i, nt);                                                                                  \
        const float *row = ap.row;                                                                                                  \
        for (int k = 0; k < nt; ++k) {                                                                                              \
            lds[k][threadIdx.x] = setpoint(row[k], par[(nt + k) * n + i]) * c.ten[k].ksg;                                           \
            lds[NTX + k][threadIdx.x] = par[k * n + i];                                                                             \
        }                                                                                                                           \
        bs.ms = par[2 * nt * n + i];                                                                                                \
    _Pragma("unroll")                                                                                                               \
        for (int j = 0; j < 3; ++j) bs.ds[j] = par[(2 * nt + 1 + j) * n + i];                                                       \
        ok = rb::MsjModel<float, NTX>::template integrate_acc<INTEG>(c, qq, vv, AccelScaledLds<NTX, true>{c, &lds[0][threadIdx.x], BLOCK, bs}); \
        held = rbk::HeldOffsets{&lds[0][threadIdx.x], &lds[NTX][threadIdx.x], BLOCK};                                               \
    } else {                                                                                                                        \
        ap = (OX).applied(a.step_num, act, i, NT8);                                                                                 \
        const float4 a0 = reinterpret_cast<const float4 *>(ap.row)[0];                                                              \
        const float4 a1 = reinterpret_cast<const float4 *>(ap.row)[1];                                                              \
        const float av[NT8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};                                                     \
    _Pragma("unroll")                                                                                                               \
        for (int k = 0; k < NT8; ++k) {                                                                                             \
            fs[k] = par[k * n + i];                                                                                                 \
            u[k] = setpoint(av[k], par[(NT8 + k) * n + i]) * c.ten[k].ksg;                                                          \
        }                                                                                                                           \
        bs.ms = par[2 * NT8 * n + i];                                                                                               \
    _Pragma("unroll")                                                                                                               \
        for (int j = 0; j < 3; ++j) bs.ds[j] = par[(2 * NT8 + 1 + j) * n + i];                                                      \
        if constexpr (BK) {                                                                                                         \
            ok = rb::MsjModel<float, NT8>::template integrate_acc<INTEG>(c, qq, vv, AccelScaled<NT8>{c, u, fs, bs});                \
            held = rbk::HeldOffsets{u, fs, 1};                                                                                      \
        } else {                                                                                                                    \
            __shared__ float lds[2 * NT8][BLOCK];                                                                                   \
    _Pragma("unroll")                                                                                                               \
            for (int k = 0; k < NT8; ++k) { lds[k][threadIdx.x] = u[k]; lds[NT8 + k][threadIdx.x] = fs[k]; }                        \
            ok = rb::MsjModel<float, NT8>::template integrate_acc<INTEG>(c, qq, vv, AccelScaledLds<NT8, false>{c, &lds[0][threadIdx.x], BLOCK, bs}); \
            held = rbk::HeldOffsets{&lds[0][threadIdx.x], &lds[NT8][threadIdx.x], BLOCK};                                           \
        }                                                                                                                           \
    }                                                                                                                               \
    if constexpr (BK) {                                                                                                             \
        rbk::env_account(&a, i, qq, vv, gg, ok, (OX).done_hook(&a, RedrawParams<const ParamArgs *>{&pa}), (OX).template policy<IN_LDS>(&a, &pa, ap, c, held, i)); \
    } else {                                                                                                                        \
        const rbk::msj_env_kernarg_ptr la = rbk::late_env_args(rbk::msj_env_args_offset(int(sizeof(CONST))));                       \
        const param_kernarg_ptr lp = (param_kernarg_ptr)((const __attribute__((address_space(4))) char *)la - rbk::msj_env_args_offset(int(sizeof(CONST))) + \
                                                         param_args_offset(int(sizeof(CONST))));                                    \
        rbk::env_account(la, i, qq, vv, gg, ok, (OX).done_hook(la, RedrawParams<param_kernarg_ptr>{lp}), (OX).template policy<IN_LDS>(la, lp, ap, c, held, i)); \
    }
template <int INTEG, int BLOCK, typename CONST, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_params_env_step(const CONST c_arg, const MsjEnvArgs a, const ParamArgs pa) {
    RB_MSJ_PARAMS_ENV_STEP_BODY(rbk::NoObsExt{})
}

}  // namespace rbp
