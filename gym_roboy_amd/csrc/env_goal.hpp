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
//
// Outcome counts per pool row (rb_env_goal_row_stats_*): while a handle has them enabled, goal_curriculum_stats_kernel
// is launched IN PLACE of goal_curriculum_kernel - the same lane text plus, for a lane whose episode ended in an env step, one add
// into attempts[row it was aimed at] and, if it reached it, one into reached[row].  rb_env_goal_pool_permute re-orders a live pool:
// rows and counts on the host, the index plane by goal_index_permute_kernel.
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

// One lane of the curriculum, as TEXT: goal_curriculum_kernel is this body and nothing else, and goal_curriculum_stats_kernel holds
// it between its own loads and its adds, so neither calls through a function that could change the other's instruction stream.
// `c`: the GoalCurriculumArgs; BLOCK: the lanes per workgroup of the kernel it stands in; EXIT: how a lane with nothing to do leaves
// the text (`return`, or `break` where the text stands in a do { } while (0) and the kernel goes on behind it).
#define RBG_CURRICULUM_LANE(c, BLOCK, EXIT)                                                                                             \
    const GoalPoolArgs &a = c.p;                                                                                                        \
    const long i = a.i0 + long(blockIdx.x) * BLOCK + threadIdx.x;                                                                       \
    if (i >= a.i1) EXIT;                                                                                                                \
    if (a.done && !a.done[i]) EXIT;                                                                                                     \
    uint32_t l = c.level[i];                                                                                                            \
    if (l >= c.L) l = c.L - 1u; /* (the plane is the caller's to write through rb_env_goal_level_ptr: never index past the pool) */    \
    const uint32_t r = c.reached[i];                                                                                                    \
    if (a.done) { /* an episode end moves the level; a reset (done = null) does not */                                                  \
        l = curriculum_next_level(l, r != c.seen[i], c.up, c.down, c.L);                                                               \
        c.level[i] = l;                                                                                                                 \
    }                                                                                                                                   \
    c.seen[i] = r;                                                                                                                      \
    const uint32_t k = curriculum_row(a.seed, a.env0 + uint64_t(i), a.goal_count[i] - 1u, l, a.m, c.L);                                 \
    c.index[i] = k;                                                                                                                     \
    const float *row = a.pool + size_t(k) * a.nq;                                                                                       \
    const int nq = a.nq;                                                                                                                \
    for (int j = 0; j < nq; ++j) {                                                                                                      \
        const float g = row[j];                                                                                                         \
        a.goal[state_index(i, j, nq, a.n, a.rows)] = g;                                                                                 \
        if (a.obs) a.obs[i * a.od + 2 * nq + j] = g;                                                                                    \
    }

__global__ void __launch_bounds__(256)
goal_curriculum_kernel(const GoalCurriculumArgs c) {
    RBG_CURRICULUM_LANE(c, 256, return)
}

// ---- outcome counts per pool row (rb_env_goal_row_stats_*): the curriculum's lane between the counting's loads and its adds ----
// counts: uint64 [2][m], attempts[m] then reached[m].  A lane whose episode ended in an env step, aimed at row k0 = index[i] < m
// (RB_GOAL_INDEX_NONE, behind rb_env_set_goal, is no row), adds 1 to attempts[k0] and, if its reached counter moved since its last
// episode end - the outcome the level rule is about to use - 1 to reached[k0].  A reset launch (done = null) counts nothing.
// Integer adds through global atomics whose result is unused: exact in any order, so ranges of one handle stepped on two streams
// add into the same planes safely.
//
// One env per lane, 1024 lanes per workgroup.  Every lane reads its row and its outcome BEFORE the lane text writes the level, the
// `seen` word or the index, and adds BEHIND it: the loads travel with the lane text's own, and the workgroup's barrier delays no
// goal.  How the adds are made depends on how many of the workgroup's episodes ended (DESIGN.md §24 has the timings):
//   - fewer than RBG_STATS_DENSE (training's ordinary step: a few per cent): each such lane adds into its row directly.  Lanes that
//     share no row cost one memory-side request each, which is cheap while they are few;
//   - otherwise (the envs time out together, or every step ends an episode): a histogram in LDS over the rows [0, RBG_STATS_BINS) -
//     the first levels' windows, where the envs crowd - one word per row with attempts in the low half and reached in the high half
//     (a workgroup adds at most 1024 to either).  It is flushed with one add per non-empty half, lane t taking the bins t, t + 1024,
//     ...: neighbouring lanes add into neighbouring words, which the memory side takes as a few wide requests where the direct form
//     sends one per lane.  A row beyond the bins is added to directly.
struct GoalCurriculumStatsArgs {
    GoalCurriculumArgs c;
    unsigned long long *counts;               // [2][m]
};

#define RBG_STATS_BLOCK 1024
#define RBG_STATS_BINS 4096u
#define RBG_STATS_DENSE 512

__global__ void __launch_bounds__(RBG_STATS_BLOCK)
goal_curriculum_stats_kernel(const GoalCurriculumStatsArgs s) {
    __shared__ uint32_t bins[RBG_STATS_BINS];
    const GoalPoolArgs &p = s.c.p;
    const long e = p.i0 + long(blockIdx.x) * RBG_STATS_BLOCK + threadIdx.x;
    const bool ended = p.done && e < p.i1 && p.done[e];
    uint32_t k0 = 0xFFFFFFFFu, hit = 0u;       // (no row)
    if (ended) {                              // read here, in front of the lane text that overwrites them; used behind it
        k0 = s.c.index[e];
        hit = s.c.reached[e] != s.c.seen[e] ? 1u : 0u;
    }
    do {
        RBG_CURRICULUM_LANE(s.c, RBG_STATS_BLOCK, break)
    } while (0);
    if (p.done) {                             // (uniform: a reset launch counts nothing)
        if (__syncthreads_count(ended) >= RBG_STATS_DENSE) {
            const uint32_t top = p.m < RBG_STATS_BINS ? p.m : RBG_STATS_BINS;
            for (uint32_t b = threadIdx.x; b < top; b += RBG_STATS_BLOCK) bins[b] = 0u;
            __syncthreads();
            if (k0 < top) atomicAdd(&bins[k0], 1u | (hit << 16));
            else if (k0 < p.m) {
                atomicAdd(s.counts + k0, 1ull);
                if (hit) atomicAdd(s.counts + p.m + k0, 1ull);
            }
            __syncthreads();
            for (uint32_t b = threadIdx.x; b < top; b += RBG_STATS_BLOCK) {
                const uint32_t w = bins[b];
                if (w & 0xFFFFu) atomicAdd(s.counts + b, (unsigned long long)(w & 0xFFFFu));
                if (w >> 16) atomicAdd(s.counts + p.m + b, (unsigned long long)(w >> 16));
            }
        } else if (k0 < p.m) {
            atomicAdd(s.counts + k0, 1ull);
            if (hit) atomicAdd(s.counts + p.m + k0, 1ull);
        }
    }
}


// rb_env_goal_pool_permute on a handle with a curriculum: index[i] <- inv[index[i]] (inv[old row] = new row), one env per lane,
// grid-stride.  RB_GOAL_INDEX_NONE is no row (>= m) and stays as it is
__global__ void __launch_bounds__(256)
goal_index_permute_kernel(uint32_t *__restrict__ index, const uint32_t *__restrict__ inv, long n, uint32_t m) {
    for (long i = long(blockIdx.x) * 256 + threadIdx.x; i < n; i += long(gridDim.x) * 256) {
        const uint32_t k = index[i];
        if (k < m) index[i] = inv[k];
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
