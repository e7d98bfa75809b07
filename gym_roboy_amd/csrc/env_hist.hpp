// env_hist.hpp - the last K commanded actions as observation columns of the fused env step (rb_env_action_obs_configure).  DESIGN.md §18.
//
// Included by roboy_sim.hip only: hiprtc (msj_kernels.hpp, msj_jit.hpp) compiles none of these kernels.  Not rows of the dispatch
// table: while a handle has K > 0, dispatch() launches these kernels for the env-step entry instead of whatever it launched before
// (its row, env_params.hpp's kernel, env_obs.hpp's or env_io.hpp's).  The kernels ARE the env-step bodies - RB_MSJ_ENV_STEP_BODY,
// RB_MSJ_PARAMS_ENV_STEP_BODY - expanded with env_io.hpp's extension plus the readout below: launched with an io argument of zeros
// where the handle has no io configuration.  One env per lane, 256-thread groups - but for MsjRobot's baked constants without
// parameters and channels up to RB_SMALL_BATCH envs: 64-thread groups, as the io kernel and the row they stand in for.
//
// Row: [q, qd, goal | tendon channels | K blocks of n_t action columns], newest block first; lead = 3 n_q + C n_t columns in front,
// written and noised as without the option (the noise stops at `lead`: its Philox blocks are numbered by row position, so the leading
// columns take the same draws).  With s the env's step counter as the step leaves it, block j holds clip_action of the row the env
// was HANDED at episode step s - 1 - j of the same episode - not the row a delay applied - and 0.0f where s - 1 - j < 1: an env that
// was auto-reset reports K zero blocks.  Never noised, never scaled.
//
// Ring: env_io.hpp's, hist[S][n_envs][n_t] of raw rows indexed by the step counter k on entry, S the smallest power of two above
// max(delay_hi, K - 1).  Every lane stores the row it was handed into slot k mod S in front of the step (as IoExt does) and reads,
// behind the step, block 0 from the handed row itself and block j from slot (k - j) mod S while k - j >= 1: slots it wrote itself in
// this episode, nothing is ordered across lanes and an auto-reset clears nothing.  A caller that rewrites step_num reads whatever
// the slots hold.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "env_common.hpp"
#include "env_io.hpp"
#include "env_obs.hpp"
#include "env_params.hpp"
#include "msj_kernels.hpp"

namespace rbh {

using rbio::IoArgs;
using rbk::Const8;
using rbk::ConstX;
using rbk::HeldOffsets;
using rbk::MsjEnvArgs;
using rbk::NT8;
using rbk::NTX;
using rbo::NtOf;
using rbo::ObsArgs;

constexpr int MAX_ROWS = 8;                   // = RB_ACTION_OBS_MAX

// The kernels' LAST argument, in the io kernels' IoArgs' place: that argument (zeros and the ring on a handle without an io
// configuration) and, read behind the step only through the kernel-argument segment, the option's two numbers
struct alignas(8) HistArgs {
    int rows, lead;                           // K; the columns in front of the blocks: obs_dim - K n_t, the noised width
};
struct alignas(8) HistIoArgs {
    IoArgs io;
    HistArgs h;
};
typedef const __attribute__((address_space(4))) HistArgs *hist_kernarg_ptr;

// What applied() hands the body: env_io.hpp's AppliedRow and the step counter on entry (the accounting overwrites the plane)
struct HistRow { const float *row; bool rest; uint32_t k; };

// env_account's observation policy: TendonObs's row over the leading columns, its noise, then the K blocks - in the lane's LDS row
// before the wave copies its rows out, or in its row of the observation array
template <typename CONST, typename OX, bool WRITTEN_OUT, bool PARAMS, typename REFRESH, typename ARGS>
struct HistObs : rbo::TendonObs<CONST, OX, WRITTEN_OUT, PARAMS, REFRESH> {
    using Base = rbo::TendonObs<CONST, OX, WRITTEN_OUT, PARAMS, REFRESH>;
    rbio::io_kernarg_ptr io;
    hist_kernarg_ptr ha;
    ARGS a;
    uint32_t k;
    // block j of the lane's row: dst[j nt ..]; `live` lanes read a row of their own (the handed row, or a slot of this episode)
    template <bool STAGED>
    __device__ __forceinline__ void blocks(float *dst, long i, int nt, int rows, bool reset) const {
        const float *handed = a->act + i * nt;
        const float *hist = io->hist;
        const long stride = io->slot_stride;
        const uint32_t sm = uint32_t(io->slot_mask);
#pragma unroll 1
        for (int j = 0; j < rows; ++j) {
            const bool live = !reset && k > uint32_t(j);             // episode step k - j >= 1
            const float *src = j == 0 ? handed : hist + long((k - uint32_t(j)) & sm) * stride + i * nt;
            float *p = dst + j * nt;
            if constexpr (!std::is_same<CONST, ConstX>::value) {
                float4 x0 = float4{0.0f, 0.0f, 0.0f, 0.0f}, x1 = x0;
                if (live) { x0 = reinterpret_cast<const float4 *>(src)[0]; x1 = reinterpret_cast<const float4 *>(src)[1]; }
                const float v0[4] = {live ? rbe::clip_action(x0.x) : 0.0f, live ? rbe::clip_action(x0.y) : 0.0f,
                                     live ? rbe::clip_action(x0.z) : 0.0f, live ? rbe::clip_action(x0.w) : 0.0f};
                const float v1[4] = {live ? rbe::clip_action(x1.x) : 0.0f, live ? rbe::clip_action(x1.y) : 0.0f,
                                     live ? rbe::clip_action(x1.z) : 0.0f, live ? rbe::clip_action(x1.w) : 0.0f};
                Base::template put<STAGED>(p, v0, 4);
                Base::template put<STAGED>(p + 4, v1, 4);
            } else {
                for (int e = 0; e < nt; ++e) p[e] = live ? rbe::clip_action(src[e]) : 0.0f;
            }
        }
    }
    __device__ __forceinline__ void operator()(float *obs, long i, const float (&o)[9], const float (&qq)[3], const float (&vv)[3], bool reset) const {
        constexpr bool X = std::is_same<CONST, ConstX>::value;
        const int nt = X ? this->c.nt : NT8;
        const int od = this->ox->obs_dim;
        const int rows = ha->rows, lead = ha->lead;
        if (PARAMS && reset) this->refresh.template run<WRITTEN_OUT>(this->c, this->held, nt, i);
        if (!this->ox->staged) {                  // (wave-uniform: the rows do not fit into LDS beside the step's columns)
            float *row = obs + i * od;
            this->template write_row<false>(row, o, qq, vv, nt);
            this->refresh.noise(row, lead, i);
            blocks<false>(row + lead, i, nt, rows, reset);
            return;
        }
        // (TendonObs's staged path: the wave's 64 rows through its LDS region, copied out as one contiguous run)
        extern __shared__ float obs_stage[];
        const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
        float *wrow = obs_stage + wave * 64 * od;
        this->template write_row<true>(wrow + lane * od, o, qq, vv, nt);
        this->refresh.noise(wrow + lane * od, lead, i);
        blocks<true>(wrow + lane * od + lead, i, nt, rows, reset);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float *gbase = obs + (i - lane) * od;
        if (this->cnt_left >= 64) {
            const int total = 64 * od;                              // (a multiple of 4)
            for (int e = lane * 4; e < total; e += 256)
                *reinterpret_cast<float4 *>(gbase + e) = *reinterpret_cast<const float4 *>(wrow + e);
        } else {                                                    // the launch's last wave, lanes missing: every lane its own row
            for (int e = 0; e < od; ++e) gbase[lane * od + e] = wrow[lane * od + e];
        }
    }
};

// The extension the env-step bodies take: IoExt's late views and episode-end hook, its ring store with the counter kept, and the
// policy above.  OFF_HIST: byte distance from the launch's MsjEnvArgs to its HistArgs.
template <int NT, bool BK, int OFF_OBS, int OFF_IO, int OFF_HIST>
struct HistExt : rbio::IoExt<NT, BK, OFF_OBS, OFF_IO> {
    template <typename ARGS>
    __device__ __forceinline__ hist_kernarg_ptr hist_view(ARGS la) const { return (hist_kernarg_ptr)(this->env_args_bytes(la) + OFF_HIST); }
    // In front of the step: the handed row into the env's slot of this step (the ring always exists here), the row of d steps ago.
    // Without a delay range the delay plane is not read (a handle without an io configuration has none).
    __device__ __forceinline__ HistRow applied(const uint32_t *step_num, const float *act, long i, int nt) const {
        const float *handed = act + i * nt;
        const IoArgs *io = this->io_direct;
        float *hist = io->hist;
        const long stride = io->slot_stride;
        const uint32_t sm = uint32_t(io->slot_mask);
        const uint32_t k = step_num[i];                              // (1 for an episode's first step)
        float *mine = hist + long(k & sm) * stride + i * nt;
        if constexpr (NT == NT8) {
            reinterpret_cast<float4 *>(mine)[0] = reinterpret_cast<const float4 *>(handed)[0];
            reinterpret_cast<float4 *>(mine)[1] = reinterpret_cast<const float4 *>(handed)[1];
        } else {
            for (int j = 0; j < nt; ++j) mine[j] = handed[j];
        }
        if (io->delay_hi == 0) return HistRow{handed, false, k};     // (uniform)
        const uint32_t d = io->delay[i];
        if (d == 0u) return HistRow{handed, false, k};
        if (k <= d) return HistRow{handed, true, k};                 // k - d < 1: the rest command (the row is read, not used)
        return HistRow{hist + long((k - d) & sm) * stride + i * nt, false, k};
    }
    template <bool IN_LDS, typename ARGS, typename CONST>
    __device__ __forceinline__ auto policy(ARGS la, const HistRow &ap, const CONST &c, const HeldOffsets &held, long i) const {
        using R = rbio::RowNoise<ARGS>;
        using OX = decltype(this->obs_view(la));
        using P = HistObs<CONST, OX, BK && !IN_LDS, false, R, ARGS>;
        return P{typename P::Base{c, this->obs_view(la), held, R{this->io_view(la), la}, la->cnt - (i - (long(threadIdx.x) & 63))},
                 this->io_view(la), hist_view(la), la, ap.k};
    }
    template <bool IN_LDS, typename ARGS, typename PA, typename CONST>
    __device__ __forceinline__ auto policy(ARGS la, PA pa, const HistRow &ap, const CONST &c, const HeldOffsets &held, long i) const {
        using R = rbio::AppliedRefresh<ARGS, PA>;
        using OX = decltype(this->obs_view(la));
        using P = HistObs<CONST, OX, BK && !IN_LDS, true, R, ARGS>;
        return P{typename P::Base{c, this->obs_view(la), held, R{{this->io_view(la), la}, pa, rbio::AppliedRow{ap.row, ap.rest}},
                                  la->cnt - (i - (long(threadIdx.x) & 63))},
                 this->io_view(la), hist_view(la), la, ap.k};
    }
};
template <typename CONST>
constexpr int hist_off() { return rbio::io_off<CONST>() + int(offsetof(HistIoArgs, h)); }
template <typename CONST>
constexpr int hist_off_params() { return rbio::io_off_params<CONST>() + int(offsetof(HistIoArgs, h)); }

// ---- the kernels: the env step's body (as text), the io extension's row in front of it, the row and its K blocks behind it ----
template <int INTEG, int BLOCK, int UNROLL, typename CONST, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_hist_env_step(const CONST c_arg, const MsjEnvArgs a, const ObsArgs<NtOf<CONST>::N> oa, const HistIoArgs hio) {
    using namespace rbk;
    const HistExt<NtOf<CONST>::N, BK, rbo::obs_off<CONST>(), rbio::io_off<CONST>(), hist_off<CONST>()> ox{{&hio.io}};
    RB_MSJ_ENV_STEP_BODY(ox)
}
template <int INTEG, int BLOCK, typename CONST, bool BK>
__global__ void __launch_bounds__(BLOCK)
msj_hist_params_env_step(const CONST c_arg, const MsjEnvArgs a, const rbp::ParamArgs pa, const ObsArgs<NtOf<CONST>::N> oa, const HistIoArgs hio) {
    using namespace rbp;
    const HistExt<NtOf<CONST>::N, BK, rbo::obs_off_params<CONST>(), rbio::io_off_params<CONST>(), hist_off_params<CONST>()> ox{{&hio.io}};
    RB_MSJ_PARAMS_ENV_STEP_BODY(ox)
}

// rb_env_reset_dev on a handle with K > 0 and noise: io_noise_rows (env_io.hpp) with the row stride and the noised width apart - the
// noise stops at `lead` (colsig and noise_blocks cover the leading columns only).  One lane per env, the row in place.
__global__ void __launch_bounds__(256)
hist_noise_rows(float *__restrict__ obs, int od, int lead, const IoArgs io, long n, uint64_t seed, uint64_t env0) {
    const long i = long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    // (the argument through the kernel-argument segment: colsig is indexed at run time)
    const rbio::io_kernarg_ptr iov = (rbio::io_kernarg_ptr)((rbo::kernarg_bytes)__builtin_amdgcn_kernarg_segment_ptr() + 16);
    const uint32_t r = io.rows[i];
    io.rows[i] = r + 1u;
    rbio::add_noise(obs + i * od, lead, iov, seed, env0 + uint64_t(i), r);
}

// ... a reset env has been handed nothing yet - K zero blocks behind the rows the reset has
// just written.  One lane per env.
__global__ void __launch_bounds__(256)
hist_zero_rows(float *__restrict__ obs, int od, int lead, long n) {
    const long i = long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    float *row = obs + i * od;
    for (int e = lead; e < od; ++e) row[e] = 0.0f;
}

}  // namespace rbh
