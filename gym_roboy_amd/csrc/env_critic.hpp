// env_critic.hpp - privileged critic rows of the fused env step (rb_env_critic_obs_*).  DESIGN.md §20.
//
// Included by roboy_sim.hip only: hiprtc (msj_kernels.hpp, msj_jit.hpp) compiles none of this.  Not a row of the dispatch table and no
// env-step kernel: while a handle has the option on, env_step_launch enqueues critic_rows_kernel behind whichever kernel stepped the
// range (same stream, same envs), and rb_env_reset_dev behind the reset and its row kernels - as done_kind_kernel (§17) trails a step.
//
// One env per lane.  The lane reads the planes as the step LEFT them - after any auto-reset and redraw - so a row describes the state,
// goal, parameters and delay that the returned observation row belongs to.  Row, blocks in this order, each only if selected:
//     state    3 n_q   q, qd, goal from the planes (the obs row's first 3 n_q columns without noise)
//     age      1       __fdiv_rn(float(step_num), float(max_episode_length))      (1 / max_len behind a reset)
//     params   np      the parameter planes in plane order, unscaled              (needs rb_params_enable)
//     delay    1       float(delay)                                               (needs rb_env_io_configure)
//     actions  K n_t   columns [lead, lead + K n_t) of the obs row just written, bit for bit (needs rb_env_action_obs_configure;
//                      zeros where no row was written: rb_env_reset_dev(sim, NULL))
// Tendon channels are not offered: their exact values are in no plane and the obs row's copies may be noised.
//
// Rows leave as env_obs.hpp's do: each lane writes its row into the wave's LDS region (64 x Dc floats), a wave-level release / acquire
// fence and barrier, then the wave copies its 64 rows out as ONE contiguous run of float4 (64 Dc floats: a multiple of four; the run
// starts at a multiple of 64 rows, so it is 16-byte aligned whenever the array is).  The launch's last, partial wave - and every wave
// of an array that is not 16-byte aligned (a slice [t] of a [T, n, Dc] tensor with n Dc odd) - writes one row per lane.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rbc {

enum : int { STATE = 1, AGE = 2, PARAMS = 4, DELAY = 8, ACTIONS = 16, ALL = 31 };      // = RB_CRITIC_* (roboy_sim.h)
constexpr int MAX_DIM = 63;                   // = RB_CRITIC_OBS_MAX_DIM: the PPO gradient kernels' input limit

// row width of `mask` on a robot with n_q joints, np parameter planes, K action rows of n_t columns
inline int row_dim(int mask, int nq, int np, int act_cols) {
    return (mask & STATE ? 3 * nq : 0) + (mask & AGE ? 1 : 0) + (mask & PARAMS ? np : 0) + (mask & DELAY ? 1 : 0) + (mask & ACTIONS ? act_cols : 0);
}

struct CriticArgs {
    const float *q, *qd, *goal;               // planes [n_q][n] of the whole batch
    const uint32_t *step_num;                 // [n]
    const float *par;                         // planes [np][n], or null
    const uint32_t *delay;                    // [n], or null
    const float *obs;                         // the step's observation rows [n][od] (whole batch), or null: zero action blocks
    float *out;                               // rows [n][dc] of the whole batch
    long n, i0, i1;                           // plane stride; the launch's envs [i0, i1), i0 a multiple of 64
    float max_len;
    int nq, np, mask, dc;
    int od, lead, act_cols;                   // the obs row's stride, the columns in front of its action blocks, K n_t
    int flat;                                 // the array is 16-byte aligned: full waves copy their rows out as one run
};

__global__ void __launch_bounds__(256)
critic_rows_kernel(const CriticArgs a) {
    extern __shared__ float critic_stage[];
    const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
    const long i = a.i0 + long(blockIdx.x) * 256 + threadIdx.x;
    const long wave0 = i - lane;
    if (wave0 >= a.i1) return;                // (the whole wave: no lane of it has an env)
    const int dc = a.dc;
    float *wrow = critic_stage + wave * 64 * dc;
    if (i < a.i1) {
        float *row = wrow + lane * dc;
        int c = 0;
        if (a.mask & STATE) {
            const int nq = a.nq;
            for (int j = 0; j < nq; ++j) {
                row[c + j] = a.q[j * a.n + i];
                row[c + nq + j] = a.qd[j * a.n + i];
                row[c + 2 * nq + j] = a.goal[j * a.n + i];
            }
            c += 3 * nq;
        }
        if (a.mask & AGE) row[c++] = __fdiv_rn(float(a.step_num[i]), a.max_len);
        if (a.mask & PARAMS) {
            const int np = a.np;
            for (int p = 0; p < np; ++p) row[c + p] = a.par[p * a.n + i];
            c += np;
        }
        if (a.mask & DELAY) row[c++] = float(a.delay[i]);
        if (a.mask & ACTIONS) {
            const int m = a.act_cols;
            if (a.obs) {
                const float *src = a.obs + i * a.od + a.lead;
                for (int e = 0; e < m; ++e) row[c + e] = src[e];
            } else {
                for (int e = 0; e < m; ++e) row[c + e] = 0.0f;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float *gbase = a.out + wave0 * dc;
    if (a.flat && wave0 + 64 <= a.i1) {       // (wave-uniform)
        const int total = 64 * dc;
        for (int e = lane * 4; e < total; e += 256)
            *reinterpret_cast<float4 *>(gbase + e) = *reinterpret_cast<const float4 *>(wrow + e);
    } else if (i < a.i1) {                    // lanes missing, or an array off the float4 grid: every lane its own row
        for (int e = 0; e < dc; ++e) gbase[lane * dc + e] = wrow[lane * dc + e];
    }
}

}  // namespace rbc
