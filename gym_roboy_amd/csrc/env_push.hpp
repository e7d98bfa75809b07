// env_push.hpp - random velocity pushes in front of the fused env step (rb_env_push_*): an external disturbance, for
// both robot classes, every kernel form and every other option, because no env-step kernel changes.  With the option on, ONE kernel
// runs in front of every env-step launch (and in front of shaping_cost: the cost is that of the state the step really starts from),
// on its stream, over its envs [i0, i1).  For env i of the batch, global id g = env0 + i:
//     m = count[i];  count[i] = m + 1                       (uint32, wraps; only rb_env_push_configure zeroes it)
//     w = philox_draw(seed, g, m, STREAM_PUSH, 0).v[0];     the env is PUSHED iff (w >> 8) < threshold      (integers only)
//     pushed, for every joint j < n_q:
//         z_j          = component j & 3 of block 1 + (j >> 2) of the same draw, Box-Muller as env_io.hpp's add_noise - the expression
//                        is RESTATED below, not shared: pairs (0,1), (2,3); u1 = ((w >> 8) + 1) / 2^24, u2 = (w >> 8) / 2^24; cosine to
//                        the even, sine to the odd component
//         impulse[i][j] = fl32(sigma_j z_j)
//         qd_j          = clamp(fl32(qd_j + impulse[i][j]), -qd_max_j, +qd_max_j)      product and sum: two roundings, no fma
//       then last[i] = m + 1 and n_pushes[i] += 1
//     not pushed: nothing but count[i] is touched (the impulse row keeps its old content).
// After a step, "env i was pushed in this step" reads last[i] == count[i].  q is never touched; the velocity is stored in the handle's
// own layout (ball joints: planes [n_q][n]; joint trees: rows [n][n_q]); the impulse plane is env-major [n][n_q] for both.
// Not a row of the dispatch table.  One env per lane, 256-lane groups; a lane that is not pushed leaves after one Philox block.
// sigma and qd_max (32 floats each) are indexed by a run-time joint number: they are read through the kernel-argument segment, as
// io_noise_rows reads colsig - the index is wave-uniform, so each is one scalar load, and the kernel has no private segment.
#pragma once
#include <hip/hip_runtime.h>

#include "env_common.hpp"
#include "philox.hpp"

namespace rbpush {

constexpr int STREAM_PUSH = 6;
constexpr int MAX_Q = 32;                     // = the description's joint limit (GoalBox)

// the kernel's ONLY argument (the kernel-argument segment starts with it)
struct alignas(8) PushArgs {
    float *qd;                                // the whole batch: planes [n_q][n] (rows == 0) or rows [n][n_q]
    uint32_t *count, *last, *n_pushes;        // [n]
    float *impulse;                           // [n][n_q]
    long n, i0, i1;                           // the batch's env count (plane stride), the launch's envs [i0, i1)
    uint64_t seed, env0;
    uint32_t threshold;                       // 0 .. 2^24
    int nq, rows, pad_;
    float sigma[MAX_Q], qd_max[MAX_Q];
};
typedef const __attribute__((address_space(4))) PushArgs *push_kernarg_ptr;

__global__ void __launch_bounds__(256) env_push(const PushArgs a) {
    const long i = a.i0 + long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.i1) return;
    const uint32_t m = a.count[i];
    a.count[i] = m + 1u;
    const uint64_t gid = a.env0 + uint64_t(i);
    const uint32_t w0 = rb::philox_draw(a.seed, gid, m, STREAM_PUSH, 0u).v[0];
    if ((w0 >> 8) >= a.threshold) return;
    // (the tables through the kernel-argument segment: indexed at run time)
    const push_kernarg_ptr tab = (push_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const int nq = a.nq;
    const long n = a.n;
    const bool rows = a.rows != 0;
    float *imp_row = a.impulse + i * nq;
    // joint j takes deviate z: two roundings between the velocity and its new value, and the stored impulse is what was added
    auto push = [&](int j, float z) {
#pragma clang fp contract(off)
        const float imp = tab->sigma[j] * z;
        const float vmax = tab->qd_max[j];
        float *v = a.qd + (rows ? i * nq + j : j * n + i);
        const float moved = *v + imp;
        imp_row[j] = imp;
        *v = fminf(fmaxf(moved, -vmax), vmax);
    };
#pragma unroll 1
    for (int b = 0; 4 * b < nq; ++b) {
        const rb::Philox4 w = rb::philox_draw(a.seed, gid, m, STREAM_PUSH, uint32_t(1 + b));
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const float u1 = float((w.v[2 * pr] >> 8) + 1u) * (1.0f / 16777216.0f);
            const float u2 = rb::u01(w.v[2 * pr + 1]);
            const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(u1));
            float sn, cs;
            __sincosf(6.2831853071795865f * u2, &sn, &cs);
            const int j0 = 4 * b + 2 * pr;
            if (j0 < nq) push(j0, rad * cs);
            if (j0 + 1 < nq) push(j0 + 1, rad * sn);
        }
    }
    a.last[i] = m + 1u;
    a.n_pushes[i] = a.n_pushes[i] + 1u;
}

// rb_env_push_count: the sum of n_pushes into *out (zeroed in front of the launch); integers, so the order of the adds is free
__global__ void __launch_bounds__(256) push_count_sum(const uint32_t *__restrict__ n_pushes, long n, unsigned long long *out) {
    unsigned long long v = 0;
    for (long i = long(blockIdx.x) * 256 + threadIdx.x; i < n; i += long(gridDim.x) * 256) v += n_pushes[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

}  // namespace rbpush
