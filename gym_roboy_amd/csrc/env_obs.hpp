// env_obs.hpp - optional tendon channels in the fused env step's observation (rb_env_obs_configure).  DESIGN.md §13.
//
// Included by roboy_sim.hip only: hiprtc (msj_kernels.hpp, msj_jit.hpp) compiles none of these kernels.  Not rows of the dispatch
// table: while a handle has a channel mask set, dispatch() launches these kernels for the env-step entry instead of the handle's row
// (or instead of env_params.hpp's kernel, on a handle with parameters enabled).  The kernels ARE the env-step bodies of
// msj_kernels.hpp / env_params.hpp - RB_MSJ_ENV_STEP_BODY, RB_MSJ_PARAMS_ENV_STEP_BODY - expanded with an observation policy for
// env_account: one env per lane, 256-thread groups at every batch size (the policy itself takes any group size: env_io.hpp has a
// 64-thread instance).
//
// Row: [q (3), qd (3), goal (3), then per selected channel in the order length, rate, activation, force: n_t values], obs_dim =
// 9 + C n_t floats, rows dword-aligned only.  The tendon columns are MsjModel::tendon_state at the state the row reports, under the
// activation offsets the lane stepped with (the set-points just applied, held) and - parameter form - under the env's force scales;
// an env that was auto-reset reports the zero pose under the same actions, and in the parameter form under the parameters the
// episode-end hook has just redrawn (the lane reads its planes again).  Each channel times its scale, one rounded multiply.
//
// Stores: the lanes of a wave write their rows into the wave's region of dynamic LDS and the wave copies the 64 rows out as one
// contiguous run, 16 bytes per lane and instruction; where the rows do not fit beside the step's own LDS columns (ObsArgs::staged =
// 0: wide rows of a ConstX robot) each lane stores its own row, as env_account's record - dword-aligned 16-byte stores.
#pragma once
#include <hip/hip_runtime.h>

#include "env_common.hpp"
#include "env_params.hpp"
#include "msj_kernels.hpp"
#include "msj_math.hpp"

namespace rbo {

using rbk::Const8;
using rbk::ConstX;
using rbk::HeldOffsets;
using rbk::MsjEnvArgs;
using rbk::NT8;
using rbk::NTX;

// channel bits (= RB_OBS_* of roboy_sim.h), in row order
constexpr int CH_LENGTH = 1, CH_RATE = 2, CH_ACTIVATION = 4, CH_FORCE = 8, CH_ALL = 15;
__host__ __device__ constexpr int n_channels(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1); }

// The kernels' LAST argument, behind MsjEnvArgs (and ParamArgs): read behind the step, late like those where the robot's constants
// occupy the scalar registers (kernarg instances)
template <int NT>
struct alignas(8) ObsArgs {
    int mask, obs_dim;                     // obs_dim = 9 + n_channels(mask) n_t: the row stride
    int staged, pad_;                      // staged: the launch has 4 BLOCK obs_dim bytes of dynamic LDS for the waves' rows
    float scale[4];                        // per channel
    rb::TendonUnits<float> units[NT];
};
__host__ __device__ constexpr int obs_args_offset(int prev_end) { return (prev_end + 7) / 8 * 8; }

typedef const __attribute__((address_space(4))) char *kernarg_bytes;
template <typename CONST> struct NtOf { static constexpr int N = std::is_same<CONST, ConstX>::value ? NTX : NT8; };

// What the parameter form's policy needs to hold an auto-reset env's columns under its redrawn parameters: the action row and the
// planes again.  Nominal form: nothing (the offsets do not depend on the episode).
// (NOISY: the type also has noise(row, obs_dim, i), called with the lane's finished row where it has just been written - its LDS row
// or its row of the observation array - before the row leaves; MAYBE_EMPTY: the mask may be 0, nine columns and no tendon evaluated.
// Both are env_io.hpp's.)
struct NoRefresh {
    static constexpr bool NOISY = false, MAYBE_EMPTY = false;
    template <bool WRITTEN_OUT, typename CONST>
    __device__ __forceinline__ void run(const CONST &, const HeldOffsets &, int, long) const {}
};
// The refresh itself: env i's held offsets and force scales again from the planes par[.][n], under `row` (or the rest command) - the
// step's own products (RB_MSJ_PARAMS_ENV_STEP_BODY: setpoint)
template <bool WRITTEN_OUT, typename CONST>
__device__ __forceinline__ void refresh_held(const CONST &c, const HeldOffsets &h, int nt, long i, float slope, float act_hi, const float *row, bool rest,
                                             const float *par, long n) {
    const int trips = WRITTEN_OUT ? NT8 : nt;
#pragma unroll WRITTEN_OUT ? NT8 : 1        // (written out, the offsets are in registers: every index a constant)
    for (int k = 0; k < trips; ++k) {
        const float sp = (rest ? 0.0f : rbe::action_setpoint(slope, row[k], act_hi)) + par[(nt + k) * n + i];
        h.u[k * h.stride] = sp * c.ten[k].ksg;
        h.fs[k * h.stride] = par[k * n + i];
    }
}
template <typename ARGS, typename PA>
struct ParamRefresh {
    static constexpr bool NOISY = false, MAYBE_EMPTY = false;
    ARGS a;
    PA pa;
    template <bool WRITTEN_OUT, typename CONST>
    __device__ __forceinline__ void run(const CONST &c, const HeldOffsets &h, int nt, long i) const {
        refresh_held<WRITTEN_OUT>(c, h, nt, i, a->e.slope, a->e.act_hi, a->act + i * nt, false, pa->par, pa->n);
    }
};

// env_account's observation policy.  OX: the ObsArgs - a pointer to the argument itself, or its late view in the kernel-argument
// segment.  WRITTEN_OUT: 8 tendons, constants as literals, offsets in registers; otherwise the rolled loop over an LDS column.
template <typename CONST, typename OX, bool WRITTEN_OUT, bool PARAMS, typename REFRESH>
struct TendonObs {
    const CONST &c;
    OX ox;
    HeldOffsets held;
    REFRESH refresh;
    long cnt_left;                         // envs of this launch from the wave's first lane on: >= 64 = every lane of the wave holds one
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    // up to four values of one channel: a dword-aligned 16-byte store into the global row, dwords into the LDS row (whose stride
    // obs_dim is odd)
    template <bool STAGED>
    static __device__ __forceinline__ void put(float *p, const float (&v)[4], int left) {
        if (!STAGED && left >= 4) { *reinterpret_cast<f4u *>(p) = f4u{v[0], v[1], v[2], v[3]}; return; }
        p[0] = v[0];
        if (left > 1) p[1] = v[1];
        if (left > 2) p[2] = v[2];
        if (left > 3) p[3] = v[3];
    }
    // the lane's row into `row`: its own row of the observation array, or its row of the wave's LDS region
    template <bool STAGED>
    __device__ __forceinline__ void write_row(float *row, const float (&o)[9], const float (&qq)[3], const float (&vv)[3], int nt) const {
        using M = rb::MsjModel<float, NtOf<CONST>::N>;
        const int mask = ox->mask;
        if constexpr (STAGED) {
#pragma unroll
            for (int j = 0; j < 9; ++j) row[j] = o[j];
        } else {
            rbk::PlainObs::store9(row, o);
        }
        if constexpr (REFRESH::MAYBE_EMPTY) { if (!mask) return; }
        const float s_len = ox->scale[0], s_rate = ox->scale[1], s_act = ox->scale[2], s_force = ox->scale[3];
        const bool want_force = (mask & CH_FORCE) != 0;
        const typename M::Frame f = M::frame(qq, vv);
        auto four = [&](int h, auto index) {      // tendons h .. h + 3 (index(j): which tendon slot j evaluates)
            float L[4], R[4], A[4], F[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = index(j);
                rb::TendonUnits<float> pu;
                pu.lc = ox->units[k].lc; pu.vl0 = ox->units[k].vl0; pu.fmax = ox->units[k].fmax; pu.pad = 0.0f;
                if constexpr (PARAMS) pu.fmax = pu.fmax * held.fs[k * held.stride];
                const rb::TendonReading<float> r = M::tendon_state_sel(c, f, c.ten[k], pu, held.u[k * held.stride], want_force);
                L[j] = r.length * s_len; R[j] = r.rate * s_rate; A[j] = r.activation * s_act; F[j] = r.force * s_force;
            }
            const int left = nt - h;              // wave-uniform
            float *p = row + 9 + h;
            if (mask & CH_LENGTH) { put<STAGED>(p, L, left); p += nt; }
            if (mask & CH_RATE) { put<STAGED>(p, R, left); p += nt; }
            if (mask & CH_ACTIVATION) { put<STAGED>(p, A, left); p += nt; }
            if (mask & CH_FORCE) { put<STAGED>(p, F, left); }
        };
        if constexpr (WRITTEN_OUT) {              // eight tendons written out, four at a time: 16 values in flight
#pragma unroll
            for (int h = 0; h < NT8; h += 4) four(h, [&](int j) { return h + j; });
        } else {
            // a rolled loop of four tendons per trip (one scalar load of each tendon's records per trip); a last trip of fewer than
            // four (c.nt at run time) evaluates its last tendon again and stores what is left
#pragma unroll 1
            for (int h = 0; h < nt; h += 4) four(h, [&](int j) { return h + j < nt ? h + j : nt - 1; });
        }
    }
    __device__ __forceinline__ void operator()(float *obs, long i, const float (&o)[9], const float (&qq)[3], const float (&vv)[3], bool reset) const {
        constexpr bool X = std::is_same<CONST, ConstX>::value;
        const int nt = X ? c.nt : NT8;
        const int od = ox->obs_dim;
        if (PARAMS && reset) refresh.template run<WRITTEN_OUT>(c, held, nt, i);
        if (!ox->staged) {                        // (wave-uniform: the rows do not fit into LDS beside the step's columns)
            write_row<false>(obs + i * od, o, qq, vv, nt);
            if constexpr (REFRESH::NOISY) refresh.noise(obs + i * od, od, i);
            return;
        }
        // The wave's 64 rows are one contiguous run of 256 obs_dim bytes, 16-byte aligned (a launch starts at a multiple of 256
        // envs), but one lane's row is only dword-aligned and 4 obs_dim bytes from the next: stored per lane, every store
        // instruction touches 64 cache lines.  So the lanes write their rows into the wave's LDS region and the wave copies the
        // run out, 1 KiB per store instruction (140 -> 79 us at 2 097 152 envs with 25 columns).
        extern __shared__ float obs_stage[];
        const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
        float *wrow = obs_stage + wave * 64 * od;
        write_row<true>(wrow + lane * od, o, qq, vv, nt);
        if constexpr (REFRESH::NOISY) refresh.noise(wrow + lane * od, od, i);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (one wave: LDS instructions execute in issue order)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float *gbase = obs + (i - lane) * od;
        if (cnt_left >= 64) {
            const int total = 64 * od;                              // (a multiple of 4)
            for (int e = lane * 4; e < total; e += 256)
                *reinterpret_cast<float4 *>(gbase + e) = *reinterpret_cast<const float4 *>(wrow + e);
        } else {                                                    // the launch's last wave, lanes missing: every lane its own row
            for (int e = 0; e < od; ++e) gbase[lane * od + e] = wrow[lane * od + e];
        }
    }
};

// The extension the env-step bodies take in NoObsExt's place (action row and episode-end hook as NoObsExt's).  BK: the robot's constants are literals, the ObsArgs argument is read
// directly; otherwise through the late pointer, OFF bytes behind the launch's MsjEnvArgs.
template <int NT, bool BK, int OFF>
struct ObsExt {
    const ObsArgs<NT> *direct;
    template <typename ARGS>
    __device__ __forceinline__ auto view(ARGS la) const {
        if constexpr (BK) return direct;
        else return (const __attribute__((address_space(4))) ObsArgs<NT> *)((kernarg_bytes)la + OFF);
    }
    __device__ __forceinline__ rbk::HandedRow applied(const uint32_t *, const float *act, long i, int nt) const { return rbk::HandedRow{act + i * nt}; }
    template <typename ARGS, typename HOOK>
    __device__ __forceinline__ HOOK done_hook(ARGS, const HOOK &h) const { return h; }
    template <bool IN_LDS, typename ARGS, typename AP, typename CONST>
    __device__ __forceinline__ auto policy(ARGS la, const AP &, const CONST &c, const HeldOffsets &held, long i) const {
        return TendonObs<CONST, decltype(view(la)), BK && !IN_LDS, false, NoRefresh>{c, view(la), held, NoRefresh{}, la->cnt - (i - (long(threadIdx.x) & 63))};
    }
    template <bool IN_LDS, typename ARGS, typename PA, typename AP, typename CONST>
    __device__ __forceinline__ auto policy(ARGS la, PA pa, const AP &, const CONST &c, const HeldOffsets &held, long i) const {
        return TendonObs<CONST, decltype(view(la)), BK && !IN_LDS, true, ParamRefresh<ARGS, PA>>{c, view(la), held, ParamRefresh<ARGS, PA>{la, pa}, la->cnt - (i - (long(threadIdx.x) & 63))};
    }
};
// byte distance from the MsjEnvArgs argument to the ObsArgs argument: nominal form (behind MsjEnvArgs), parameter form (behind ParamArgs)
template <typename CONST>
constexpr int obs_off() {
    return obs_args_offset(rbk::msj_env_args_offset(int(sizeof(CONST))) + int(sizeof(MsjEnvArgs))) - rbk::msj_env_args_offset(int(sizeof(CONST)));
}
template <typename CONST>
constexpr int obs_off_params() {
    return obs_args_offset(rbp::param_args_offset(int(sizeof(CONST))) + int(sizeof(rbp::ParamArgs))) - rbk::msj_env_args_offset(int(sizeof(CONST)));
}
// ---- the kernels: the env step's body (as text: RB_MSJ_ENV_STEP_BODY), the tendon columns behind it ----
template <int INTEG, int BLOCK, int UNROLL, typename CONST, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_obs_env_step(const CONST c_arg, const MsjEnvArgs a, const ObsArgs<NtOf<CONST>::N> oa) {
    using namespace rbk;
    const ObsExt<NtOf<CONST>::N, BK, obs_off<CONST>()> ox{&oa};
    RB_MSJ_ENV_STEP_BODY(ox)
}
template <int INTEG, int BLOCK, typename CONST, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_obs_params_env_step(const CONST c_arg, const MsjEnvArgs a, const rbp::ParamArgs pa, const ObsArgs<NtOf<CONST>::N> oa) {
    using namespace rbp;
    const ObsExt<NtOf<CONST>::N, BK, obs_off_params<CONST>()> ox{&oa};
    RB_MSJ_PARAMS_ENV_STEP_BODY(ox)
}

// rb_env_reset_dev on a handle with channels: the whole row at the state the reset has just written (the zero pose), every
// set-point 0 - the parameter form adds the env's set-point offset and scales the force.  par: the planes [2 n_t + 4][n], or null.
template <int BLOCK, typename CONST>
__global__ void __launch_bounds__(BLOCK)
msj_obs_rows(const CONST c, const ObsArgs<NtOf<CONST>::N> oa, const float *__restrict__ q, const float *__restrict__ qd, const float *__restrict__ goal,
             const float *__restrict__ par, float *__restrict__ obs, long n) {
    using M = rb::MsjModel<float, NtOf<CONST>::N>;
    const long i = long(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    float qq[3], vv[3], o[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) { qq[j] = q[j * n + i]; vv[j] = qd[j * n + i]; o[j] = qq[j]; o[3 + j] = vv[j]; o[6 + j] = goal[j * n + i]; }
    const int nt = std::is_same<CONST, ConstX>::value ? c.nt : NT8, mask = oa.mask;
    float *orow = obs + i * oa.obs_dim;
    rbk::PlainObs::store9(orow, o);
    const bool want_force = (mask & CH_FORCE) != 0;
    const typename M::Frame f = M::frame(qq, vv);
#pragma unroll 1
    for (int k = 0; k < nt; ++k) {
        rb::TendonUnits<float> pu = oa.units[k];
        float u = 0.0f;
        if (par) { pu.fmax = pu.fmax * par[k * n + i]; u = par[(nt + k) * n + i] * c.ten[k].ksg; }
        const rb::TendonReading<float> r = M::tendon_state_sel(c, f, c.ten[k], pu, u, want_force);
        float *p = orow + 9 + k;
        if (mask & CH_LENGTH) { *p = r.length * oa.scale[0]; p += nt; }
        if (mask & CH_RATE) { *p = r.rate * oa.scale[1]; p += nt; }
        if (mask & CH_ACTIVATION) { *p = r.activation * oa.scale[2]; p += nt; }
        if (mask & CH_FORCE) { *p = r.force * oa.scale[3]; }
    }
}

}  // namespace rbo
