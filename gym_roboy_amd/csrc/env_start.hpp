// env_start.hpp - episodes that begin at a pose from a pool instead of the zero pose (rb_env_start_poses_*): random or
// reference state initialisation, for both robot classes, every kernel form and every other option, because no env-step kernel
// changes.  With the option on, ONE kernel runs behind every reset kernel (in front of everything else a reset enqueues) and behind
// every env-step launch of a handle with auto_reset (directly behind the goal kernel, in front of critic_rows_kernel), on its stream,
// over its envs [i0, i1).  The step and reset kernels still write the zero pose; this kernel replaces it.
//
// Start number d of the env with global id g = env0 + i (start_draw below, shared with tests/hostmath/start_pose_host.cpp):
//     w         = philox_draw(seed, g, d, STREAM_START, 0)
//     from_pool = (w.v[1] >> 8) < threshold                  threshold = round(start_prob 2^24): 2^24 always, 0 never (integers only)
//     k         = (uint64(w.v[0]) m) >> 32                   the pool's row, goal_pool's multiply-shift
//     count[i]  = d + 1                                      (uint32, wraps; only rb_env_start_poses_configure zeroes it; a start that
//                                                             stays at the rest pose counts too; independent of the goal counter)
//     index[i]  = from_pool ? k : INDEX_REST                 the row the env's running episode began at
// A lane whose done word is 0 reads nothing else (a reset passes done = null: every lane draws).  A drawing lane from the pool writes
// q = pool[k], qd = 0 into the state (SoA planes [n_q][n] for ball joints, env-major rows [n][n_q] for joint trees), feas = 1 and
// columns [0, 2 n_q) of its observation row (stride: the handle's obs_dim); a lane that stays at the rest pose writes count and index only.
//
// Sensor noise (env_io.hpp): behind a STEP the row already carries the noise of row number rows[i] - 1 on the zero pose.
// The kernel evaluates the same Philox blocks with add_noise's expression - RESTATED below, not shared, as env_push.hpp does - and
// writes value + colsig[c] z into the columns it replaces: the row is what the step kernel would have written had it reset to the
// pose.  Blocks without a noised column in [0, 2 n_q) are skipped.  Behind a RESET the noise kernels run behind this one.
// Not a row of the dispatch table.  One env per lane, 256-lane groups.  colsig is indexed by a run-time column number: it is read
// through the kernel-argument segment (wave-uniform index: scalar loads), so the kernel has no private segment.
// The decision, the row and the counter are one function a host compiler takes too: without hipcc this header declares it and no kernel.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBST_HD __host__ __device__ __forceinline__
#else
#define RBST_HD inline
#endif

#include <cstdint>

#include "philox.hpp"

namespace rbstart {

constexpr int STREAM_START = 7;
constexpr uint32_t INDEX_REST = 0xFFFFFFFFu;     // = RB_START_INDEX_REST
constexpr int MAX_Q = 32;                        // = the description's joint limit (GoalBox)

// start number d of env gid: the index plane's new word (a row of the pool [m], or INDEX_REST) and the counter's
struct Start { uint32_t index, count; };
RBST_HD Start start_draw(uint64_t seed, uint64_t gid, uint32_t d, uint32_t threshold, uint32_t m) {
    const rb::Philox4 w = rb::philox_draw(seed, gid, d, uint32_t(STREAM_START), 0u);
    const bool from_pool = (w.v[1] >> 8) < threshold;
    const uint32_t k = uint32_t((uint64_t(w.v[0]) * uint64_t(m)) >> 32);
    return Start{from_pool ? k : INDEX_REST, d + 1u};
}

#if defined(__HIPCC__)
constexpr int STREAM_SENSOR = 4;                 // = rbio::STREAM_SENSOR

// the kernel's ONLY argument (the kernel-argument segment starts with it)
struct alignas(8) StartArgs {
    const float *pool;                        // [m][n_q]
    const uint32_t *done;                     // the step's done words [n] (whole batch), or null: every lane draws (reset)
    float *q, *qd;                            // the whole batch: planes [n_q][n] (rows == 0) or rows [n][n_q]
    uint32_t *feas, *count, *index;           // [n]
    float *obs;                               // rows [n][od] of the whole batch, or null
    const uint32_t *noise_rows;               // the sensor noise's row counters [n], or null: no noise on the replaced columns
    long n, i0, i1;                           // the batch's env count (plane stride), the launch's envs [i0, i1)
    uint64_t seed, env0;
    uint32_t m, threshold;                    // 0 .. 2^24
    int nq, od, rows;
    uint32_t noise_blocks;                    // bit b: Philox block b of a row holds a noised column in [0, 2 n_q)
    float colsig[2 * MAX_Q];                  // per row position: the sigma, 0 where the column is not noised (whole blocks)
};
typedef const __attribute__((address_space(4))) StartArgs *start_kernarg_ptr;

__global__ void __launch_bounds__(256) env_start(const StartArgs a) {
    const long i = a.i0 + long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.i1) return;
    if (a.done && !a.done[i]) return;
    const uint64_t gid = a.env0 + uint64_t(i);
    const Start st = start_draw(a.seed, gid, a.count[i], a.threshold, a.m);
    a.count[i] = st.count;
    a.index[i] = st.index;
    if (st.index == INDEX_REST) return;
    const int nq = a.nq;
    const long n = a.n;
    const bool rows = a.rows != 0;
    const float *pose = a.pool + size_t(st.index) * nq;
    float *orow = a.obs ? a.obs + i * a.od : nullptr;
    for (int j = 0; j < nq; ++j) {
        const float v = pose[j];
        const long at = rows ? i * nq + j : long(j) * n + i;
        a.q[at] = v;
        a.qd[at] = 0.0f;
        if (orow) { orow[j] = v; orow[nq + j] = 0.0f; }
    }
    a.feas[i] = 1u;
    if (!orow || !a.noise_rows || !a.noise_blocks) return;       // (uniform but for orow's lanes: all of a launch or none)
    // the noise the step kernel put on the zero pose, on the pose: row number rows[i] - 1 (the step counted its row already)
    const start_kernarg_ptr tab = (start_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const uint32_t r = a.noise_rows[i] - 1u;
    const uint32_t blocks = a.noise_blocks;
    const int cols = 2 * nq;
#pragma unroll 1
    for (int b = 0; 4 * b < cols; ++b) {
        if (!((blocks >> b) & 1u)) continue;                       // (wave-uniform)
        const rb::Philox4 w = rb::philox_draw(a.seed, gid, r, uint32_t(STREAM_SENSOR), uint32_t(b));
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const float u1 = float((w.v[2 * pr] >> 8) + 1u) * (1.0f / 16777216.0f);
            const float u2 = rb::u01(w.v[2 * pr + 1]);
            const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(u1));
            float sn, cs;
            __sincosf(6.2831853071795865f * u2, &sn, &cs);
            const int c0 = 4 * b + 2 * pr;
            const float s0 = tab->colsig[c0], s1 = tab->colsig[c0 + 1];
            if (s0 != 0.0f && c0 < cols) orow[c0] = __builtin_fmaf(s0, rad * cs, c0 < nq ? pose[c0] : 0.0f);
            if (s1 != 0.0f && c0 + 1 < cols) orow[c0 + 1] = __builtin_fmaf(s1, rad * sn, c0 + 1 < nq ? pose[c0 + 1] : 0.0f);
        }
    }
}
#endif  // __HIPCC__

}  // namespace rbstart
