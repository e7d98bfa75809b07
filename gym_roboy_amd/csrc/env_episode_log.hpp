// env_episode_log.hpp - a per-env record of finished episodes behind the fused env step (rb_env_episode_log_*): each
// env's first E episodes with their return, length and outcome, for both robot classes, every kernel form and every other option,
// because no env-step kernel changes.  With the option on, ONE kernel runs behind every env-step launch - behind the shaping apply
// (the reward is the one the caller receives) and the goal pool, in front of done_kind_kernel, which turns the done words into codes
// (here they are read as flags) - on its stream, over its envs [i0, i1).  For env i of the batch (planes are indexed by the batch's
// env index, never by the position in the launch):
//     r = reward[i];  a = fl32(acc[i] + r);  t = age[i] + 1
//     done[i] == 0:  acc[i] = a; age[i] = t
//     done[i] != 0:  g = reached[i]                         the goals-reached counter d_ep_cnt[2n + i]
//                    k = (g != seen[i]) ? RB_DONE_TERMINATED : RB_DONE_TRUNCATED      (done_kind_kernel's rule, a `seen` plane of its own)
//                    seen[i] = g;  c = count[i]
//                    c < E: ret[c][i] = a; len[c][i] = t; kind[c][i] = k; count[i] = c + 1
//                           c + 1 == E: one relaxed agent-scope add of 1 into `full`
//                    acc[i] = 0; age[i] = 0
// The rule is ONE plain function (lane_step) a host compiler takes too (tests/hostmath/episode_log_host.cpp): without hipcc this
// header declares it and no kernel.  Not a row of the dispatch table.  One env per lane, 256-lane groups; a lane whose env is not
// done reads and writes two words.
// The summary (episode_log_summary) is stats_reduce_kernel's two-stage reduction: every block leaves its 8 partial sums, takes a
// ticket, and the block that arrives last adds the partials in block order - the same planes give the same bits.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBEL_HD __host__ __device__ __forceinline__
#else
#define RBEL_HD inline
#endif

#include <cstdint>

#include "../../include/roboy_sim.h"

namespace rbel {

constexpr int MAX_CAPACITY = RB_EPISODE_LOG_MAX;
constexpr int SUMMARY_BLOCKS = 256;

// an env's running words, and what a step leaves to be written: slot < E is the record to write (ret, len, kind), else none
struct Lane { float acc; uint32_t age, seen, count; };
struct Record { uint32_t slot; float ret; uint32_t len, kind; bool filled; };      // filled: this record was the env's E-th
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

RBEL_HD Record lane_step(Lane &s, float reward, uint32_t done, uint32_t reached, uint32_t E) {
    Record rec{NO_SLOT, 0.0f, 0u, 0u, false};
    const float a = s.acc + reward;
    const uint32_t t = s.age + 1u;
    if (!done) { s.acc = a; s.age = t; return rec; }
    const uint32_t k = reached != s.seen ? uint32_t(RB_DONE_TERMINATED) : uint32_t(RB_DONE_TRUNCATED);
    s.seen = reached;
    const uint32_t c = s.count;
    if (c < E) {
        rec.slot = c; rec.ret = a; rec.len = t; rec.kind = k;
        s.count = c + 1u;
        rec.filled = c + 1u == E;
    }
    s.acc = 0.0f; s.age = 0u;
    return rec;
}

#if defined(__HIPCC__)
// the kernel's ONLY argument
struct LogArgs {
    const float *reward;                      // the whole batch's arrays [n]
    const uint32_t *done, *reached;
    float *acc; uint32_t *age, *seen, *count; // [n]
    float *ret; uint32_t *len, *kind;         // [E][n], plane-major
    uint32_t *full;                           // one word
    long n, i0, i1;                           // the batch's env count (plane stride), the launch's envs [i0, i1)
    uint32_t E, pad_;
};

__global__ void __launch_bounds__(256) episode_log_kernel(const LogArgs a) {
    const long i = a.i0 + long(blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.i1) return;
    const uint32_t d = a.done[i];
    Lane s{a.acc[i], a.age[i], 0u, 0u};
    if (!d) {                                 // (seen, count and the counter are read by done lanes only)
        (void)lane_step(s, a.reward[i], 0u, 0u, a.E);
        a.acc[i] = s.acc; a.age[i] = s.age;
        return;
    }
    s.seen = a.seen[i]; s.count = a.count[i];
    const Record rec = lane_step(s, a.reward[i], d, a.reached[i], a.E);
    a.seen[i] = s.seen;
    if (rec.slot != NO_SLOT) {                // slot < E <= 64 and i < i1 <= n: inside the [E][n] planes
        const size_t at = size_t(rec.slot) * size_t(a.n) + size_t(i);
        a.ret[at] = rec.ret; a.len[at] = rec.len; a.kind[at] = rec.kind;
        a.count[i] = s.count;
        if (rec.filled) (void)__hip_atomic_fetch_add(a.full, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a.acc[i] = 0.0f; a.age[i] = 0u;
}

// rb_env_episode_log_summary(_dev): over the records k < min(count[i], first_k) of every env
//   out: [records, sum return, sum return^2, sum length, terminated, truncated, envs with at least first_k records, 0]
__global__ void __launch_bounds__(256)
episode_log_summary(const uint32_t *__restrict__ count, const float *__restrict__ ret, const uint32_t *__restrict__ len,
                    const uint32_t *__restrict__ kind, uint32_t first_k, double *partials, unsigned int *ticket, double *out, double *out2, long n) {
    __shared__ double sh[4][8];
    __shared__ bool last;
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long i = long(blockIdx.x) * 256 + threadIdx.x; i < n; i += long(gridDim.x) * 256) {
        const uint32_t c = count[i], m = c < first_k ? c : first_k;
        for (uint32_t k = 0; k < m; ++k) {
            const size_t at = size_t(k) * size_t(n) + size_t(i);
            const double r = double(ret[at]);
            v[1] += r; v[2] += r * r; v[3] += double(len[at]);
            if (kind[at] == uint32_t(RB_DONE_TERMINATED)) v[4] += 1.0; else v[5] += 1.0;
        }
        v[0] += double(m);
        if (c >= first_k) v[6] += 1.0;
    }
    auto block_sum = [&]() {                 // -> sh[0..3][k] after the barrier
#pragma unroll
        for (int k = 0; k < 8; ++k)
            for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < 8; ++k) sh[w][k] = v[k];
        __syncthreads();
    };
    block_sum();
    if (threadIdx.x < 8)
        partials[blockIdx.x * 8 + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (threadIdx.x == 0) last = false;
    __syncthreads();
    if (threadIdx.x == 0) {                  // the hand-off of stats_reduce_kernel: stores -> release -> vmcnt(0) -> ticket
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = threadIdx.x < gridDim.x ? __hip_atomic_load(partials + threadIdx.x * 8 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    block_sum();
    if (threadIdx.x < 8) {
        const double t = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        out[threadIdx.x] = t;
        if (out2) out2[threadIdx.x] = t;
    }
    if (threadIdx.x == 0) *ticket = 0u;       // ready for the next launch (same stream: ordered behind this kernel)
}
#endif  // __HIPCC__

}  // namespace rbel
