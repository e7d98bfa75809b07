// env_io.hpp - per-env action latency and sensor noise in the fused env step (rb_env_io_configure).  DESIGN.md §14.
//
// Included by roboy_sim.hip only: hiprtc (msj_kernels.hpp, msj_jit.hpp) compiles none of these kernels.  Not rows of the dispatch
// table: while a handle has an io configuration, dispatch() launches these kernels for the env-step entry instead of the handle's row,
// env_params.hpp's kernel or env_obs.hpp's.  The kernels ARE the env-step bodies - RB_MSJ_ENV_STEP_BODY, RB_MSJ_PARAMS_ENV_STEP_BODY -
// expanded with an extension that varies the two places the bodies leave open: the action row a lane steps with (applied()) and
// env_account's observation policy (and, for the delay's redraw, the episode-end hook).  One env per lane, 256-thread groups - but
// for MsjRobot's baked constants without parameters and channels up to RB_SMALL_BATCH envs: 64-thread groups, as the row it stands in for.
//
// Latency: env i steps episode step k with the row its caller handed in at step k - d_i of the same episode, d_i = delay[i] in
// [0, MAX_DELAY]; k = step_num[i] on entry, which a reset and an auto-reset leave at 1 (env_account's sn is k + 1: the counter
// counts the steps behind it).  While k - d_i < 1 with the rest command (every set-point 0 m; the parameter form adds the env's
// offset).  History: a ring hist[S][n_envs][n_t] of raw rows, S the smallest power of two above delay_hi.  Every lane stores the row
// it was handed into slot k mod S; a lane with 0 < d_i < k reads slot (k - d_i) mod S: both rows are the lane's own, so nothing is
// ordered across lanes, and an auto-reset clears nothing (k restarts at 1, the k - d_i >= 1 rule shields the old episode's slots).
// Without a ring (delay_hi = 0) the delay plane is not read.  The ring is indexed by the counter: a caller that rewrites step_num
// (rb_env_set_goal) steps with whatever those slots hold.
//
// Noise: behind the step, on the finished row.  Row number r = rows[i] of the env with global id g takes for the column at row
// position c component c & 3 of block c >> 2 of philox_draw(seed, g, r, STREAM_SENSOR, block), Box-Muller as mlp_policy.hip's
// sampling noise (pairs (0,1), (2,3); u1 = ((w >> 8) + 1) / 2^24, u2 = (w >> 8) / 2^24; cosine to the even, sine to the odd
// component); the column reports value + colsig[c] z with colsig[c] = sigma x the channel's scale, one fused multiply-add on the
// scaled value.  Blocks without a noised column are skipped (IoArgs::noise_blocks, wave-uniform); the goal columns and everything
// else the step writes see the true state.  rows[i] advances by one per row written while any sigma is set.
#pragma once
#include <hip/hip_runtime.h>

#include "env_common.hpp"
#include "env_obs.hpp"
#include "env_params.hpp"
#include "msj_kernels.hpp"
#include "philox.hpp"

namespace rbio {

using rbk::Const8;
using rbk::ConstX;
using rbk::HeldOffsets;
using rbk::MsjEnvArgs;
using rbk::NT8;
using rbk::NTX;
using rbo::NtOf;
using rbo::ObsArgs;

constexpr int MAX_DELAY = 7;                  // = RB_IO_MAX_DELAY
constexpr int STREAM_SENSOR = 4, STREAM_DELAY = 5;
constexpr int MAX_COLS = 9 + 4 * NTX, COLS_PAD = (MAX_COLS + 3) / 4 * 4;

// The kernels' LAST argument, behind ObsArgs.  applied() reads its four ring fields in front of the step from the argument itself
// (a handful of scalars, dead once the row is fetched); everything behind the step goes through the kernel-argument segment in every
// instance: colsig is indexed at run time, which a by-value argument only allows after a copy into private memory.
struct alignas(8) IoArgs {
    uint32_t *delay, *delay_draws, *rows;     // planes [n_envs], shifted for a sub-range
    float *hist;                              // the ring, shifted by first_env n_t; null: delay_hi = 0, no delay traffic at all
    long slot_stride;                         // n_envs n_t floats
    int slot_mask;                            // S - 1
    int delay_lo, delay_hi, resample;
    uint32_t noise_blocks;                    // bit b: Philox block b of a row holds a noised column (0: noise off, rows not counted)
    int pad_;
    float colsig[COLS_PAD];                   // per row position: sigma x channel scale, 0 where the column is not noised
};
__host__ __device__ constexpr int io_args_offset(int prev_end) { return (prev_end + 7) / 8 * 8; }
typedef const __attribute__((address_space(4))) IoArgs *io_kernarg_ptr;

// d = lo + floor(u24 (hi - lo + 1) / 2^24) for draw m of global env gid: integers only
__device__ __forceinline__ uint32_t draw_delay(uint64_t seed, uint64_t gid, uint32_t m, int lo, int hi) {
    const uint32_t w = rb::philox_draw(seed, gid, m, STREAM_DELAY, 0u).v[0];
    return uint32_t(lo) + (((w >> 8) * uint32_t(hi - lo + 1)) >> 24);
}

// rb_env_io_sample_delay_dev, and configure's first fill: envs with mask[i] != 0 (mask NULL: all) draw a new delay
__global__ void __launch_bounds__(256)
io_sample_delay(uint32_t *__restrict__ delay, uint32_t *__restrict__ draws, const uint8_t *__restrict__ mask, int lo, int hi, long n,
                uint64_t seed, uint64_t env0) {
    const long i = long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    const uint32_t m = draws[i];
    delay[i] = draw_delay(seed, env0 + uint64_t(i), m, lo, hi);
    draws[i] = m + 1u;
}

// the row's noise, in place: `row` is the lane's finished row, in LDS or in the observation array
template <typename IOV>
__device__ __forceinline__ void add_noise(float *row, int od, IOV io, uint64_t seed, uint64_t gid, uint32_t r) {
    const uint32_t blocks = io->noise_blocks;
#pragma unroll 1
    for (int b = 0; 4 * b < od; ++b) {
        if (!((blocks >> b) & 1u)) continue;                       // (wave-uniform)
        const rb::Philox4 w = rb::philox_draw(seed, gid, r, STREAM_SENSOR, uint32_t(b));
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const float u1 = float((w.v[2 * pr] >> 8) + 1u) * (1.0f / 16777216.0f);
            const float u2 = rb::u01(w.v[2 * pr + 1]);
            const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(u1));
            float sn, cs;
            __sincosf(6.2831853071795865f * u2, &sn, &cs);
            const int c0 = 4 * b + 2 * pr;
            const float s0 = io->colsig[c0], s1 = io->colsig[c0 + 1];   // (padded to whole blocks, zeros behind the row)
            if (s0 != 0.0f && c0 < od) row[c0] = row[c0] + s0 * (rad * cs);
            if (s1 != 0.0f && c0 + 1 < od) row[c0 + 1] = row[c0 + 1] + s1 * (rad * sn);
        }
    }
}

// What applied() hands the body and the body hands back to the policy: the row the lane steps with, or the rest command
struct AppliedRow { const float *row; bool rest; };

// env_account's episode-end hook: the body's own (nothing, or the parameters' redraw), then the delay's redraw
template <typename HOOK, typename IOV>
struct DoneHook {
    HOOK inner;
    IOV io;
    __device__ __forceinline__ void operator()(long i, uint64_t gid, uint64_t seed, int auto_reset) const {
        inner(i, gid, seed, auto_reset);
        if (!auto_reset || !io->resample) return;
        const uint32_t m = io->delay_draws[i];
        io->delay[i] = draw_delay(seed, gid, m, io->delay_lo, io->delay_hi);
        io->delay_draws[i] = m + 1u;
    }
};

// TendonObs's row policy (env_obs.hpp: NoRefresh, ParamRefresh) of the io kernels: the env's row number (counted only while a sigma
// is set) and the noise on the finished row; run(): nothing in the nominal form
template <typename ARGS>
struct RowNoise {
    static constexpr bool NOISY = true, MAYBE_EMPTY = true;
    io_kernarg_ptr io;
    ARGS a;
    template <bool WRITTEN_OUT, typename CONST>
    __device__ __forceinline__ void run(const CONST &, const HeldOffsets &, int, long) const {}
    __device__ __forceinline__ void noise(float *row, int od, long i) const {
        if (io->noise_blocks == 0u) return;       // (uniform)
        const uint32_t r = io->rows[i];
        io->rows[i] = r + 1u;
        add_noise(row, od, io, a->seed, a->env0 + uint64_t(i), r);
    }
};
// ... and of the parameter form: the done-lane refresh (ParamRefresh) under the row that was APPLIED
template <typename ARGS, typename PA>
struct AppliedRefresh : RowNoise<ARGS> {
    PA pa;
    AppliedRow ap;
    template <bool WRITTEN_OUT, typename CONST>
    __device__ __forceinline__ void run(const CONST &c, const HeldOffsets &h, int nt, long i) const {
        rbo::refresh_held<WRITTEN_OUT>(c, h, nt, i, this->a->e.slope, this->a->e.act_hi, ap.row, ap.rest, pa->par, pa->n);
    }
};

// The extension the env-step bodies take.  OFF_OBS / OFF_IO: byte distances from the launch's MsjEnvArgs to its ObsArgs and IoArgs.
template <int NT, bool BK, int OFF_OBS, int OFF_IO>
struct IoExt {
    const IoArgs *io_direct;
    // ObsArgs and IoArgs behind the step: through the kernel-argument segment in EVERY instance (the baked parameter kernel, with
    // MsjEnvArgs, ParamArgs and ObsArgs read directly, ran out of scalar registers: 36 bytes of private segment).  BK: la is the
    // MsjEnvArgs argument's own address, the segment pointer is taken here, behind the step.
    template <typename ARGS>
    __device__ __forceinline__ rbo::kernarg_bytes env_args_bytes(ARGS la) const {
        if constexpr (BK) return (rbo::kernarg_bytes)rbk::late_env_args(rbk::msj_env_args_offset(int(sizeof(rb::MsjConst<float, NT>))));
        else return (rbo::kernarg_bytes)la;
    }
    template <typename ARGS>
    __device__ __forceinline__ auto obs_view(ARGS la) const {
        return (const __attribute__((address_space(4))) ObsArgs<NT> *)(env_args_bytes(la) + OFF_OBS);
    }
    template <typename ARGS>
    __device__ __forceinline__ io_kernarg_ptr io_view(ARGS la) const { return (io_kernarg_ptr)(env_args_bytes(la) + OFF_IO); }
    // In front of the step: store the handed row into the env's slot of this step, name the row of d steps ago
    __device__ __forceinline__ AppliedRow applied(const uint32_t *step_num, const float *act, long i, int nt) const {
        const float *handed = act + i * nt;
        float *hist = io_direct->hist;
        if (!hist) return AppliedRow{handed, false};               // (uniform: no ring)
        const long stride = io_direct->slot_stride;
        const uint32_t sm = uint32_t(io_direct->slot_mask);
        const uint32_t k = step_num[i], d = io_direct->delay[i];      // (1 for an episode's first step)
        float *mine = hist + long(k & sm) * stride + i * nt;
        if constexpr (NT == NT8) {
            reinterpret_cast<float4 *>(mine)[0] = reinterpret_cast<const float4 *>(handed)[0];
            reinterpret_cast<float4 *>(mine)[1] = reinterpret_cast<const float4 *>(handed)[1];
        } else {
            for (int j = 0; j < nt; ++j) mine[j] = handed[j];
        }
        if (d == 0u) return AppliedRow{handed, false};
        if (k <= d) return AppliedRow{handed, true};               // k - d < 1: the rest command (the row is read, not used)
        return AppliedRow{hist + long((k - d) & sm) * stride + i * nt, false};
    }
    template <typename ARGS, typename HOOK>
    __device__ __forceinline__ auto done_hook(ARGS la, const HOOK &h) const { return DoneHook<HOOK, io_kernarg_ptr>{h, io_view(la)}; }
    template <bool IN_LDS, typename ARGS, typename CONST>
    __device__ __forceinline__ auto policy(ARGS la, const AppliedRow &, const CONST &c, const HeldOffsets &held, long i) const {
        using R = RowNoise<ARGS>;
        return rbo::TendonObs<CONST, decltype(obs_view(la)), BK && !IN_LDS, false, R>{c, obs_view(la), held, R{io_view(la), la},
                                                                                      la->cnt - (i - (long(threadIdx.x) & 63))};
    }
    template <bool IN_LDS, typename ARGS, typename PA, typename CONST>
    __device__ __forceinline__ auto policy(ARGS la, PA pa, const AppliedRow &ap, const CONST &c, const HeldOffsets &held, long i) const {
        using R = AppliedRefresh<ARGS, PA>;
        return rbo::TendonObs<CONST, decltype(obs_view(la)), BK && !IN_LDS, true, R>{c, obs_view(la), held, R{{io_view(la), la}, pa, ap},
                                                                                     la->cnt - (i - (long(threadIdx.x) & 63))};
    }
};
template <typename CONST>
constexpr int io_off() { return io_args_offset(rbo::obs_off<CONST>() + int(sizeof(ObsArgs<NtOf<CONST>::N>))); }
template <typename CONST>
constexpr int io_off_params() { return io_args_offset(rbo::obs_off_params<CONST>() + int(sizeof(ObsArgs<NtOf<CONST>::N>))); }

// ---- the kernels: the env step's body (as text), the delayed row in front of it, tendon columns and noise behind it ----
template <int INTEG, int BLOCK, int UNROLL, typename CONST, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_io_env_step(const CONST c_arg, const MsjEnvArgs a, const ObsArgs<NtOf<CONST>::N> oa, const IoArgs io) {
    using namespace rbk;
    const IoExt<NtOf<CONST>::N, BK, rbo::obs_off<CONST>(), io_off<CONST>()> ox{&io};
    RB_MSJ_ENV_STEP_BODY(ox)
}
template <int INTEG, int BLOCK, typename CONST, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_io_params_env_step(const CONST c_arg, const MsjEnvArgs a, const rbp::ParamArgs pa, const ObsArgs<NtOf<CONST>::N> oa, const IoArgs io) {
    using namespace rbp;
    const IoExt<NtOf<CONST>::N, BK, rbo::obs_off_params<CONST>(), io_off_params<CONST>()> ox{&io};
    RB_MSJ_PARAMS_ENV_STEP_BODY(ox)
}

// rb_env_reset_dev on a handle with noise: the rows the reset has just written are sensor readings too.  One lane per env, the
// row in place in the observation array.
__global__ void __launch_bounds__(256)
io_noise_rows(float *__restrict__ obs, int od, const IoArgs io, long n, uint64_t seed, uint64_t env0) {
    const long i = long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    // (the argument through the kernel-argument segment: colsig is indexed at run time)
    const io_kernarg_ptr iov = (io_kernarg_ptr)((rbo::kernarg_bytes)__builtin_amdgcn_kernarg_segment_ptr() + 16);
    const uint32_t r = io.rows[i];
    io.rows[i] = r + 1u;
    add_noise(obs + i * od, od, iov, seed, env0 + uint64_t(i), r);
}

}  // namespace rbio
