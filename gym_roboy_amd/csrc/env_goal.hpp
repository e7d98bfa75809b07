// env_goal.hpp - goals drawn from a pool of poses instead of the observation box (rb_env_goal_pool_*).  DESIGN.md §22.
//
// Included by roboy_sim.hip only: hiprtc (msj_kernels.hpp, msj_jit.hpp) compiles none of this.  Not a row of the dispatch table and no
// env-step kernel: while a handle holds a pool, env_step_launch enqueues goal_pool_kernel directly behind whichever kernel stepped the
// range (same stream, same envs) - in front of critic_rows_kernel and done_kind_kernel, which then see the pool goal - and
// rb_env_reset_dev behind the reset and its row kernels.  The step kernels still draw their box goal; this kernel replaces it.
//
// Goal number `draw` of the env with global id `gid` is row k of the pool [m][n_q]:
//     w = philox_draw(seed, gid, draw, STREAM_GOAL_POOL, 0).v[0]
//     k = (uint64(w) * uint64(m)) >> 32
// One multiply-shift, no rejection loop: a row's probability differs from 1 / m by at most 2^-32, i.e. a relative bias of at most
// m / 2^32 (4e-6 at the default 16 384 rows).  `draw` is the env's goal counter as the step kernels advance it (+1 at a reset, +1 or
// +2 at an episode end): the row evaluated is the one for goal_count - 1 AFTER the step, the draw whose box goal the step kernel wrote.
//
// One env per lane.  A lane whose done word is 0 reads nothing else (a reset passes done = null: every lane draws).  A drawing lane
// writes n_q values into the goal plane and into columns [2 n_q, 3 n_q) of its observation row (stride: the handle's obs_dim).  Sensor
// noise never touches those columns, so they are the pool's bits.  The pool is small and read by the few lanes that are done: plain
// loads, no LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "philox.hpp"

namespace rbg {

__host__ __device__ __forceinline__ uint32_t pool_row(uint64_t seed, uint64_t gid, uint32_t draw, uint32_t m) {
    const uint32_t w = rb::philox_draw(seed, gid, draw, rb::STREAM_GOAL_POOL, 0u).v[0];
    return uint32_t((uint64_t(w) * uint64_t(m)) >> 32);
}

// (roboy_sim.hip's layout rule: SoA planes [n_q][n] for ball joints, env-major rows [n][n_q] for joint trees)
__device__ __forceinline__ long state_index(long i, int j, int n_q, long n, int rows) { return rows ? i * n_q + j : long(j) * n + i; }

struct GoalPoolArgs {
    const float *pool;                        // [m][n_q]
    const uint32_t *done;                     // the step's done words [n] (whole batch), or null: every lane draws (reset)
    const uint32_t *goal_count;               // [n]
    float *goal;                              // planes [n_q][n] or rows [n][n_q] of the whole batch
    float *obs;                               // rows [n][od] of the whole batch, or null
    long n, i0, i1;                           // plane stride; the launch's envs [i0, i1)
    uint64_t seed, env0;
    uint32_t m;
    int nq, od, rows;
};

__global__ void __launch_bounds__(256)
goal_pool_kernel(const GoalPoolArgs a) {
    const long i = a.i0 + long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.i1) return;
    if (a.done && !a.done[i]) return;
    const uint32_t k = pool_row(a.seed, a.env0 + uint64_t(i), a.goal_count[i] - 1u, a.m);
    const float *row = a.pool + size_t(k) * a.nq;
    const int nq = a.nq;
    for (int j = 0; j < nq; ++j) {
        const float g = row[j];
        a.goal[state_index(i, j, nq, a.n, a.rows)] = g;
        if (a.obs) a.obs[i * a.od + 2 * nq + j] = g;
    }
}

// rb_sample_goals / rb_sample_goals_dev while a pool is set: sample_goals_kernel's contract (mask, counter + 1, rows or planes out)
__global__ void __launch_bounds__(256)
goal_pool_sample_kernel(const float *__restrict__ pool, uint32_t m, float *__restrict__ goal, uint32_t *__restrict__ count,
                        const uint8_t *__restrict__ mask, int n_q, long n, uint64_t seed, uint64_t env0, int rows) {
    const long i = long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    const uint32_t draw = count[i];
    count[i] = draw + 1u;
    const float *row = pool + size_t(pool_row(seed, env0 + uint64_t(i), draw, m)) * n_q;
    for (int j = 0; j < n_q; ++j) goal[state_index(i, j, n_q, n, rows)] = row[j];
}

}  // namespace rbg
