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
//
// Goal curriculum (rb_env_goal_curriculum_*): the caller has ordered the pool's rows from easiest to hardest, every env
// carries a level l in [0, L), and an env at level l draws from the rows [0, hi(l)) with hi(l) = uint32((uint64(l + 1) * m) / L) - the
// same Philox word, scaled by hi(l) instead of m, so the top level draws exactly pool_row's row.  At an episode end the level moves
// first: up by `up` (at most to L - 1) if the env's goals-reached counter moved since its last episode end (done_kind_kernel's rule,
// on a `seen` plane of the curriculum's own), down by `down` (at most to 0) otherwise; the draw is made at the new level.  While a
// curriculum is configured goal_curriculum_kernel is launched IN PLACE of goal_pool_kernel: the launches per step are a pool handle's.
// The window, the row and the level rule are plain functions a host compiler takes too (tests/hostmath/goal_curriculum_host.cpp):
// without hipcc this header declares them and no kernel.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBG_HD __host__ __device__ __forceinline__
#else
#define RBG_HD inline
#endif

#include <cstdint>

#include "philox.hpp"

namespace rbg {

RBG_HD uint32_t pool_row(uint64_t seed, uint64_t gid, uint32_t draw, uint32_t m) {
    const uint32_t w = rb::philox_draw(seed, gid, draw, rb::STREAM_GOAL_POOL, 0u).v[0];
    return uint32_t((uint64_t(w) * uint64_t(m)) >> 32);
}

// ---- curriculum: window, row, level rule (l < L <= min(m, 256), so hi(l) is in [1, m]) ----
RBG_HD uint32_t curriculum_hi(uint32_t l, uint32_t m, uint32_t L) { return uint32_t((uint64_t(l + 1u) * uint64_t(m)) / uint64_t(L)); }
RBG_HD uint32_t curriculum_row(uint64_t seed, uint64_t gid, uint32_t draw, uint32_t l, uint32_t m, uint32_t L) {
    return pool_row(seed, gid, draw, curriculum_hi(l, m, L));
}
RBG_HD uint32_t curriculum_next_level(uint32_t l, bool reached, uint32_t up, uint32_t down, uint32_t L) {
    if (reached) { const uint32_t room = L - 1u - l; return l + (up < room ? up : room); }
    return l - (down < l ? down : l);
}

#if defined(__HIPCC__)
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

// ---- goal curriculum: goal_pool_kernel's contract plus a level per env ----
struct GoalCurriculumArgs {
    GoalPoolArgs p;
    uint32_t *level, *index, *seen;           // [n] each (whole batch): the env's level, the row it holds, its reached counter as of its last episode end
    const uint32_t *reached;                  // [n]: the goals-reached counters (the statistics' third counter plane)
    uint32_t L, up, down;
};

__global__ void __launch_bounds__(256)
goal_curriculum_kernel(const GoalCurriculumArgs c) {
    const GoalPoolArgs &a = c.p;
    const long i = a.i0 + long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.i1) return;
    if (a.done && !a.done[i]) return;
    uint32_t l = c.level[i];
    if (l >= c.L) l = c.L - 1u;               // (the plane is the caller's to write through rb_env_goal_level_ptr: never index past the pool)
    const uint32_t r = c.reached[i];
    if (a.done) {                             // an episode end moves the level; a reset (done = null) does not
        l = curriculum_next_level(l, r != c.seen[i], c.up, c.down, c.L);
        c.level[i] = l;
    }
    c.seen[i] = r;
    const uint32_t k = curriculum_row(a.seed, a.env0 + uint64_t(i), a.goal_count[i] - 1u, l, a.m, c.L);
    c.index[i] = k;
    const float *row = a.pool + size_t(k) * a.nq;
    const int nq = a.nq;
    for (int j = 0; j < nq; ++j) {
        const float g = row[j];
        a.goal[state_index(i, j, nq, a.n, a.rows)] = g;
        if (a.obs) a.obs[i * a.od + 2 * nq + j] = g;
    }
}

// how many envs sit at each level: one histogram of L <= 256 bins per workgroup in LDS, then one atomic add per non-empty bin and
// workgroup into out[L], which the caller has zeroed on the same stream.  Grid-stride: any number of workgroups covers [0, n)
__global__ void __launch_bounds__(256)
goal_level_hist_kernel(const uint32_t *__restrict__ level, long n, uint32_t L, unsigned long long *__restrict__ out) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    for (long i = long(blockIdx.x) * 256 + threadIdx.x; i < n; i += long(gridDim.x) * 256) {
        const uint32_t l = level[i];
        if (l < L) atomicAdd(&bins[l], 1u);
    }
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (threadIdx.x < L && c) atomicAdd(&out[threadIdx.x], (unsigned long long)c);
}
#endif  // __HIPCC__

}  // namespace rbg
