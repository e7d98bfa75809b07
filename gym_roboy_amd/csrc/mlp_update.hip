// mlp_update.hip - what surrounds the minibatch gradient in a PPO update (gym_roboy_amd/ppo.py: update), as kernels of
// their own instead of ~10 torch launches per minibatch (include/roboy_policy.h):
//   rp_perm_dev        the epoch's sample order: a keyed bijection of [0, n) evaluated per element (a cycle-walking
//                      Feistel network on the next even power of two), instead of torch.randperm's sort of n keys
//   rp_adv_stats_dev   mean and 1 / (std + 1e-8) of the minibatch's advantages (gathered through the index), which
//                      rp_ppo_grad_dev then applies per sample: no gathered / normalised copy is materialised
//   rp_obs_moments_dev, rp_obs_norm_merge_dev   the running observation statistics (ppo.py: ObsNorm): shifted fp64 column sums of a
//                      rollout in one pass, and Chan's merge of them into (mean, var, count) + the float form the kernels read
//   rp_rollout_tail_dev   the rollout's tail under running return normalisation of the reward (ppo.py: RewardNorm): reward scaling,
//                      the discounted-return scan with its fp64 moments, the done conversion and GAE as one launch
//   rp_clip_adam_dev   clip_grad_norm_ + Adam.step over the flat gradient vector of rp_ppo_grad_dev and a parameter
//                      buffer of the same layout: one workgroup, two passes over ~10^4 floats
// The reference's consumer is stable_baselines' PPO2 (train_parallel.py:28-31); torch's optimiser is the statement these
// kernels are tested against (tests/test_policy_gpu.py); tests/test_policy_scale_gpu.py holds them against the float64 statements of
// oracle/policy_ref.py where the small cases do not reach: rp_adv_stats_dev with all STAT_BLOCKS blocks (more than 522 240 samples: the
// last block sums 256 partials), constant and far-from-zero advantages, repeated calls on one scratch; rp_clip_adam_dev's grad_scale
// (applied BEFORE the entropy bonus: the mean over ranks of gradients that each carry it), the slots it must neither read nor write,
// a zero gradient, norms on both sides of the bound, step numbers up to 100 000.  The exploration noise those tests restate bit for
// bit (csrc/mlp_policy.hip): Philox4x32-10, key = seed, counter = (sample id low, high, step + step base, 2 << 8 | block), action j =
// component j & 3 of block j >> 2, Box-Muller on words (0, 1) and (2, 3) with u1 = ((w >> 8) + 1) / 2^24, u2 = (w >> 8) / 2^24.
#include <hip/hip_runtime.h>


#include "../../include/roboy_policy.h"
#include "mlp_common.hpp"

namespace {
using namespace rpd;

// ---- keyed permutation of [0, n) ----
__host__ __device__ inline uint32_t mix32(uint32_t v) {
    v *= 0x9E3779B1u; v ^= v >> 15; v *= 0x85EBCA77u; v ^= v >> 13; v *= 0xC2B2AE3Du; v ^= v >> 16;
    return v;
}
struct PermKey { uint32_t k[4]; int half; uint32_t mask; };
__host__ __device__ inline PermKey perm_key(uint64_t key, long long n) {
    PermKey p;
    int bits = 2;
    while ((1ll << bits) < n) bits += 2;                  // an even number of bits: two equal halves
    p.half = bits / 2;
    p.mask = (1u << p.half) - 1u;
    const uint32_t lo = uint32_t(key), hi = uint32_t(key >> 32);
    for (int r = 0; r < 4; ++r) p.k[r] = mix32(lo + 0x9E3779B9u * uint32_t(r + 1)) ^ mix32(hi + 0x7F4A7C15u * uint32_t(r + 1));
    return p;
}
__host__ __device__ inline long long perm_at(const PermKey &p, long long n, long long i) {
    unsigned long long x = (unsigned long long)i;
    do {                                                   // cycle walking: the network permutes [0, 4^half) and i < n
        uint32_t L = uint32_t(x >> p.half), R = uint32_t(x) & p.mask;
        for (int r = 0; r < 4; ++r) {
            const uint32_t F = mix32(R ^ p.k[r]) & p.mask;
            const uint32_t t = L ^ F;
            L = R; R = t;
        }
        x = ((unsigned long long)L << p.half) | R;
    } while ((long long)x >= n);
    return (long long)x;
}
__global__ void perm_kernel(uint64_t key, long long n, long long first, long long count, long long *out) {
    const PermKey p = perm_key(key, n);
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (long long)gridDim.x * blockDim.x)
        out[j] = perm_at(p, n, first + j);
}

// ---- advantage statistics of a minibatch ----
constexpr int STAT_BLOCKS = 256;
__global__ void __launch_bounds__(256)
adv_stats_kernel(const float *__restrict__ adv, const long long *__restrict__ index, long long B, double *scratch, float *stats) {
    __shared__ double sh[2][4];
    __shared__ bool last;
    double s = 0.0, ss = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < B; i += (long long)gridDim.x * 256) {
        const double a = double(adv[index ? index[i] : i]);
        s += a; ss += a * a;
    }
    auto block_sum = [&]() {
        for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off, 64); ss += __shfl_xor(ss, off, 64); }
        if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = ss; }
        __syncthreads();
    };
    block_sum();
    unsigned int *ticket = reinterpret_cast<unsigned int *>(scratch + 2 * STAT_BLOCKS);
    if (threadIdx.x == 0) {
        scratch[2 * blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        scratch[2 * blockIdx.x + 1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
        // hand-off as MI355X_MICROARCH.md prescribes: stores -> agent-scope release -> vmcnt(0) -> ticket; the last block acquires
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
    s = threadIdx.x < gridDim.x ? __hip_atomic_load(scratch + 2 * threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    ss = threadIdx.x < gridDim.x ? __hip_atomic_load(scratch + 2 * threadIdx.x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    block_sum();
    if (threadIdx.x == 0) {
        const double sum = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3], sq = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
        const double mean = sum / double(B);
        // torch.Tensor.std(): the unbiased estimate
        const double var = B > 1 ? (sq - sum * mean) / double(B - 1) : 0.0;
        stats[0] = float(mean);
        stats[1] = float(1.0 / (sqrt(var > 0.0 ? var : 0.0) + 1e-8));
        *ticket = 0u;                                      // ready for the next launch (same stream: ordered behind this one)
    }
}

// ---- running observation statistics ----
// Column sums of obs [rows][obs_dim] around a shift, in fp64.  A workgroup takes RPB = 256 / obs_dim whole rows per pass: thread t <
// RPB * obs_dim reads element t of that contiguous span (coalesced) and owns column t % obs_dim for the whole launch; the grid strides
// over the spans, four loads in flight per thread.  Then per workgroup: the RPB partial sums of a column in row order; the last
// workgroup (ticket, as adv_stats_kernel) adds the workgroups' partials in block order.  Every sum has one fixed order.
constexpr int MOM_BLOCKS = 1024, MOM_ROWS_PER_THREAD = 8;
__global__ void __launch_bounds__(256)
obs_moments_kernel(const float *__restrict__ obs, long long rows, int obs_dim, const double *__restrict__ shift, double *scratch,
                   double *__restrict__ sums) {
    __shared__ double sh[2][256];
    __shared__ bool last;
    const int rpb = 256 / obs_dim, t = threadIdx.x;
    const bool active = t < rpb * obs_dim;
    const int c = t % obs_dim, r = t / obs_dim;
    const double sft = active && shift ? shift[c] : 0.0;
    double s = 0.0, ss = 0.0;
    if (active) {
        const long long step = (long long)gridDim.x * rpb;
        long long row = (long long)blockIdx.x * rpb + r;
        for (; row + 3 * step < rows; row += 4 * step) {
            const float x0 = obs[row * obs_dim + c], x1 = obs[(row + step) * obs_dim + c];
            const float x2 = obs[(row + 2 * step) * obs_dim + c], x3 = obs[(row + 3 * step) * obs_dim + c];
            const double d0 = double(x0) - sft, d1 = double(x1) - sft, d2 = double(x2) - sft, d3 = double(x3) - sft;
            s += d0; ss += d0 * d0; s += d1; ss += d1 * d1; s += d2; ss += d2 * d2; s += d3; ss += d3 * d3;
        }
        for (; row < rows; row += step) {
            const double d = double(obs[row * obs_dim + c]) - sft;
            s += d; ss += d * d;
        }
    }
    sh[0][t] = s; sh[1][t] = ss;
    __syncthreads();
    const int nq = 2 * obs_dim;                             // outputs: q < obs_dim the sum of column q, then the squares
    double *mine = scratch + (long long)blockIdx.x * nq;
    if (t < nq) {
        const int w = t >= obs_dim, cc = t - w * obs_dim;
        double v = 0.0;
        for (int rr = 0; rr < rpb; ++rr) v += sh[w][rr * obs_dim + cc];
        mine[t] = v;
    }
    unsigned int *ticket = reinterpret_cast<unsigned int *>(scratch + (long long)MOM_BLOCKS * 2 * RP_MAX_OBS);
    // hand-off as in adv_stats_kernel - stores -> agent-scope release -> vmcnt(0) -> ticket; the last block acquires - but the partials
    // are stored by several waves here, so every wave releases its own stores before the barrier in front of the ticket
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (t < nq) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
        int b = 0;
        for (; b + 3 < int(gridDim.x); b += 4) {
            v0 += __hip_atomic_load(scratch + (long long)b * nq + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v1 += __hip_atomic_load(scratch + (long long)(b + 1) * nq + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v2 += __hip_atomic_load(scratch + (long long)(b + 2) * nq + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v3 += __hip_atomic_load(scratch + (long long)(b + 3) * nq + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (; b < int(gridDim.x); ++b) v0 += __hip_atomic_load(scratch + (long long)b * nq + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sums[1 + t] = (v0 + v1) + (v2 + v3);
    }
    if (t == 0) {
        sums[0] = double(rows);
        *ticket = 0u;                                      // ready for the next launch (same stream: ordered behind this one)
    }
}

// Chan's merge of the shifted sums (shift = the state's mean, so the batch mean's offset from it IS sum / n) into the state; one
// workgroup, a thread per column
__global__ void __launch_bounds__(128)
obs_norm_merge_kernel(double *state, const double *__restrict__ sums, int obs_dim, double eps, float *__restrict__ norm) {
    const int c = threadIdx.x;
    const double n = sums[0], count = state[2 * obs_dim];
    if (!(n > 0.0)) return;                                 // (uniform: every thread reads the same two values)
    const double tot = count + n;
    if (c < obs_dim) {
        const double S = sums[1 + c], SS = sums[1 + obs_dim + c];
        const double delta = S / n;                         // batch mean - running mean
        double m2b = SS - S * delta;                        // the batch's sum of squares around its own mean
        m2b = m2b > 0.0 ? m2b : 0.0;
        const double mean = state[c] + delta * (n / tot);
        const double var = (state[obs_dim + c] * count + m2b + delta * delta * (count * n / tot)) / tot;
        state[c] = mean;
        state[obs_dim + c] = var;
        norm[c] = float(mean);
        norm[obs_dim + c] = float(1.0 / sqrt(var + eps));
    }
    __syncthreads();                                        // every thread has read the count
    if (c == 0) state[2 * obs_dim] = tot;
}

// ---- the rollout's tail with running return normalisation of the reward (ppo.py: RewardNorm) ----
// One env per lane, [T][N] arrays indexed t * N + i (coalesced over i), two scans per lane:
//   forward   r_s = fl32(rew_raw * scale);  R = gamma R + r_s in fp64;  d = R - shift joins S, SS;  R = 0 where done  (R: ret_carry)
//   backward  gae_kernel's recurrence over r~ = med3(fl32(r_s * rstd), -clip, clip); writes rew, done (as float), adv, ret
// TAIL_UNROLL steps' loads are issued before the first of them is used: a lane's scan is a serial chain, and the bytes in flight per
// wave are what the loads of independent steps put there.  Then the fp64 sums as obs_moments_kernel hands them on: per wave by
// shuffles, per workgroup in wave order to scratch, every wave releasing its own stores before the barrier in front of the ticket;
// the last workgroup adds the workgroups' partials - thread k those of workgroups k, k + 256, ... in that order, then the same
// shuffle / wave-order tree - so every sum has one fixed order.  A grid of at most TAIL_BLOCKS workgroups strides over the envs.
constexpr int TAIL_BLOCKS = 4096, TAIL_UNROLL = 8;
#define TAIL_ADDRESSING \
    typedef __attribute__((address_space(1))) char *gchar; \
    typedef __attribute__((address_space(1))) float *gfloat; \
    typedef __attribute__((address_space(1))) int *gint; \
    auto uni = [](const void *row) { \
        const unsigned long long a = reinterpret_cast<unsigned long long>(row); \
        const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(a)), hi = __builtin_amdgcn_readfirstlane(unsigned(a >> 32)); \
        return reinterpret_cast<gchar>((unsigned long long)hi << 32 | lo); \
    }; \
    auto ldf = [&](const float *row, unsigned off) { return *reinterpret_cast<gfloat>(uni(row) + off); }; \
    auto ldi = [&](const int *row, unsigned off) { return *reinterpret_cast<gint>(uni(row) + off); }; \
    auto st = [&](float *row, unsigned off, float x) { *reinterpret_cast<gfloat>(uni(row) + off) = x; };
// The fp64 sums of a workgroup of BS lanes, handed on as obs_moments_kernel does (see above); called once, by every lane.
template <int BS>
__device__ __forceinline__ void tail_reduce(double s, double ss, double *scratch, double *__restrict__ sums3, int T, long long n) {
    __shared__ double sh[2][BS / 64];
    __shared__ bool last;
    const int tid = threadIdx.x;
    auto wave_sum = [&](int q) { double v = sh[q][0]; for (int w = 1; w < BS / 64; ++w) v += sh[q][w]; return v; };
    auto block_sum = [&]() {
        for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off, 64); ss += __shfl_xor(ss, off, 64); }
        if ((tid & 63) == 0) { sh[0][tid >> 6] = s; sh[1][tid >> 6] = ss; }
        __syncthreads();
    };
    block_sum();
    unsigned int *ticket = reinterpret_cast<unsigned int *>(scratch + 2 * TAIL_BLOCKS);
    if (tid == 0) {
        scratch[2 * blockIdx.x] = wave_sum(0);
        scratch[2 * blockIdx.x + 1] = wave_sum(1);
    }
    // hand-off as in obs_moments_kernel: every wave releases its own stores (the partials above, and nothing of the arrays needs it)
    // before the barrier in front of the ticket; the last workgroup acquires
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    s = 0.0; ss = 0.0;
    for (int b = tid; b < int(gridDim.x); b += BS) {
        s += __hip_atomic_load(scratch + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ss += __hip_atomic_load(scratch + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();                                        // (thread 0 has read sh for its partial)
    block_sum();
    if (tid == 0) {
        sums3[0] = double(T) * double(n);
        sums3[1] = wave_sum(0);
        sums3[2] = wave_sum(1);
        *ticket = 0u;                                      // ready for the next launch (same stream: ordered behind this one)
    }
}

// the kernel's text, once per instance: rollout_tail_kernel, and rollout_tail_boot_kernel whose done words are episode-end codes and
// whose backward scan bootstraps the truncated steps
#define RP_BOOT 0
#include "rollout_tail_kernel.inc"
#define RP_BOOT 1
#include "rollout_tail_kernel.inc"

// ---- gradient clipping by global norm + Adam, one workgroup ----
struct AdamArgs {
    float *p, *m, *v;
    const float *g;
    int n;
    float lr, beta1, beta2, eps, bc1, bc2, max_norm, gscale;
    int ls_off, ls_len;          // the log-std range: its entropy bonus -ent_coef is added to the gradient here
    float ent_coef;
    int pi_end, vf_begin, vf_end; // the parameters' slots: [0, pi_end) and [vf_begin, vf_end); the rest of the vector (loss terms,
                                 // the value net's unused log-std slot, padding) is neither counted in the norm nor updated
};
// the learning-rate rule of clip_adam_kl_kernel (rsl_rl's "adaptive" schedule), in fp32: kl = the action net's
// approx_kl slot of the gradient vector times gscale (the mean over the ranks after an all-reduce)
struct KlArgs {
    float *lr;                   // one float on the device: read by every thread, rewritten by one
    int kl_slot;
    float desired, factor, lr_min, lr_max;
};
__device__ __forceinline__ float adapt_lr(float lr, float kl, const KlArgs &k) {
    if (kl > 2.0f * k.desired) return fmaxf(k.lr_min, lr / k.factor);
    if (kl < 0.5f * k.desired && kl > 0.0f) return fminf(k.lr_max, lr * k.factor);
    return lr;                                              // (every comparison is false on a NaN)
}
// the kernel's text, once per instance: clip_adam_kernel (the learning rate a host float: the instruction stream it has always had) and
// clip_adam_kl_kernel, which takes the learning rate from the device and moves it by the rule in front of the step
#define RP_KL 0
#include "clip_adam_kernel.inc"
#define RP_KL 1
#include "clip_adam_kernel.inc"

// the two instances of rollout_tail_kernel.inc share their argument list, their checks and their grid
int rollout_tail_launch(decltype(&rollout_tail_kernel) kernel, const char *name, const float *d_rew_raw, const int32_t *d_done_i, const float *d_val, const float *d_last_val,
                        float reward_scale, const float *d_norm2, float clip, const double *d_shift, double gamma, double lam,
                        double *d_ret_carry, float *d_rew, float *d_done, float *d_adv, float *d_ret, double *d_sums3, double *d_scratch,
                        int n_steps, int64_t n_envs, void *stream) {
    if (!d_rew_raw || !d_done_i || !d_val || !d_last_val || !d_ret_carry || !d_rew || !d_done || !d_adv || !d_ret || !d_sums3 || !d_scratch)
        return fail(RP_EINVAL, "null argument");
    const int64_t blocks = rp_rollout_tail_blocks(n_steps, n_envs);
    if (blocks < 0) return int(blocks);
    if (!(clip > 0.0f)) return fail(RP_EINVAL, "clip must be > 0");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(RP_EINVAL, "gamma must lie in [0, 1]");
    DeviceScope scope(d_rew_raw); if (scope.rc) return scope.rc;
    const int *di = reinterpret_cast<const int *>(d_done_i);
    hipLaunchKernelGGL(kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), d_rew_raw, di,
                       d_val, d_last_val, reward_scale, d_norm2, clip, d_shift, gamma, float(lam), d_ret_carry, d_rew, d_done, d_adv,
                       d_ret, d_sums3, d_scratch, n_steps, (long long)n_envs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string(name) + ": " + hipGetErrorString(e));
    return RP_OK;
}

// rp_clip_adam_dev (d_lr == NULL: the learning rate is the host float) and rp_clip_adam_kl_dev share their checks and their arguments;
// so do their asymmetric forms, whose value net's block is laid out for cobs_dim input columns (the symmetric ones: cobs_dim = obs_dim)
int clip_adam_launch(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int cobs_dim, int act_dim, float lr, float *d_lr,
                     float desired_kl, float lr_factor, float lr_min, float lr_max, float beta1, float beta2, float eps, int64_t step,
                     float max_grad_norm, float grad_scale, float ent_coef, void *stream) {
    if (!d_params || !d_grad || !d_m || !d_v) return fail(RP_EINVAL, "null argument");
    if (step < 1) return fail(RP_EINVAL, "step counts from 1");
    const int64_t n = rp_grad_asym_floats(obs_dim, cobs_dim, act_dim);
    if (n < 0) return RP_EUNSUPPORTED;
    DeviceScope scope(d_params); if (scope.rc) return scope.rc;
    AdamArgs a;
    a.p = d_params; a.g = d_grad; a.m = d_m; a.v = d_v; a.n = int(n);
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.bc1 = float(1.0 - pow(double(beta1), double(step))); a.bc2 = float(1.0 - pow(double(beta2), double(step)));
    a.max_norm = max_grad_norm; a.gscale = grad_scale; a.ent_coef = ent_coef;
    // layout of the gradient vector (mlp_common.hpp: goff_of): per net w1, b1, w2, b2, w3, b3, log_std, loss (4)
    const GOff pi = goff_of(obs_dim, act_dim), vf = goff_of(cobs_dim, 1);
    const int gs = gstride_of(obs_dim, act_dim);
    a.ls_off = pi.ls; a.ls_len = act_dim;
    a.pi_end = pi.loss; a.vf_begin = gs; a.vf_end = gs + vf.ls;
    if (d_lr) {
        KlArgs k;
        k.lr = d_lr; k.kl_slot = pi.loss + 1; k.desired = desired_kl; k.factor = lr_factor; k.lr_min = lr_min; k.lr_max = lr_max;
        hipLaunchKernelGGL(clip_adam_kl_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a, k);
    } else
        hipLaunchKernelGGL(clip_adam_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("clip_adam_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

}  // namespace

extern "C" {

int rp_perm_host(uint64_t key, int64_t n, int64_t first, int64_t count, int64_t *out) {
    if (!out || n < 1 || first < 0 || count < 0 || first + count > n) return fail(RP_EINVAL, "need 0 <= first, first + count <= n");
    const PermKey p = perm_key(key, n);
    for (int64_t j = 0; j < count; ++j) out[j] = perm_at(p, n, first + j);
    return RP_OK;
}

int rp_perm_dev(uint64_t key, int64_t n, int64_t first, int64_t count, int64_t *d_out, void *stream) {
    if (!d_out || n < 1 || first < 0 || count < 0 || first + count > n) return fail(RP_EINVAL, "need 0 <= first, first + count <= n");
    int dev = 0;
    DeviceScope scope(d_out); if (scope.rc) return scope.rc; dev = scope.dev;
    if (count == 0) return RP_OK;
    long blocks = (count + 255) / 256;
    const long cap = 8l * cu_count(dev);
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(perm_kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), key, (long long)n,
                       (long long)first, (long long)count, reinterpret_cast<long long *>(d_out));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("perm_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

int64_t rp_adv_stats_scratch_doubles(void) { return 2 * STAT_BLOCKS + 1; }

int rp_adv_stats_dev(const float *d_adv, const int64_t *d_index, int64_t batch, float *d_stats2, double *d_scratch, void *stream) {
    if (!d_adv || !d_stats2 || !d_scratch) return fail(RP_EINVAL, "null argument");
    if (batch < 1) return fail(RP_EINVAL, "batch must be >= 1");
    DeviceScope scope(d_adv); if (scope.rc) return scope.rc;
    long blocks = (batch + 2047) / 2048;                   // at least eight samples per thread
    if (blocks > STAT_BLOCKS) blocks = STAT_BLOCKS;
    hipLaunchKernelGGL(adv_stats_kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), d_adv,
                       reinterpret_cast<const long long *>(d_index), (long long)batch, d_scratch, d_stats2);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("adv_stats_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

int64_t rp_obs_moments_scratch_doubles(void) { return int64_t(MOM_BLOCKS) * 2 * RP_MAX_OBS + 1; }

int64_t rp_obs_moments_blocks(int64_t rows, int obs_dim) {
    if (rows < 1 || obs_dim < 1 || obs_dim > RP_MAX_OBS) return fail(RP_EINVAL, "need rows >= 1 and 1 <= obs_dim <= 95");
    const int64_t per_block = int64_t(256 / obs_dim) * MOM_ROWS_PER_THREAD;       // at least eight rows per thread
    const int64_t blocks = (rows + per_block - 1) / per_block;
    return blocks < MOM_BLOCKS ? blocks : MOM_BLOCKS;
}

int rp_obs_moments_dev(const float *d_obs, int64_t rows, int obs_dim, const double *d_shift, double *d_sums, double *d_scratch,
                       void *stream) {
    if (!d_obs || !d_sums || !d_scratch) return fail(RP_EINVAL, "null argument");
    const int64_t blocks = rp_obs_moments_blocks(rows, obs_dim);
    if (blocks < 0) return int(blocks);
    DeviceScope scope(d_obs); if (scope.rc) return scope.rc;
    hipLaunchKernelGGL(obs_moments_kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), d_obs,
                       (long long)rows, obs_dim, d_shift, d_scratch, d_sums);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("obs_moments_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

int rp_obs_norm_merge_dev(double *d_state, const double *d_sums, int obs_dim, double eps, float *d_norm, void *stream) {
    if (!d_state || !d_sums || !d_norm) return fail(RP_EINVAL, "null argument");
    if (obs_dim < 1 || obs_dim > RP_MAX_OBS) return fail(RP_EINVAL, "need 1 <= obs_dim <= 95");
    if (!(eps >= 0.0)) return fail(RP_EINVAL, "eps must be >= 0");
    DeviceScope scope(d_state); if (scope.rc) return scope.rc;
    hipLaunchKernelGGL(obs_norm_merge_kernel, dim3(1), dim3(128), 0, static_cast<hipStream_t>(stream), d_state, d_sums, obs_dim, eps, d_norm);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("obs_norm_merge_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

int64_t rp_rollout_tail_scratch_doubles(void) { return 2 * int64_t(TAIL_BLOCKS) + 1; }

int64_t rp_rollout_tail_blocks(int n_steps, int64_t n_envs) {
    if (n_steps < 1 || n_envs < 1) return fail(RP_EINVAL, "n_steps and n_envs must be >= 1");
    if (n_envs >= (int64_t(1) << 26)) return fail(RP_EUNSUPPORTED, "the rollout tail supports fewer than 2^26 envs");
    const int64_t blocks = (n_envs + 255) / 256;
    return blocks < TAIL_BLOCKS ? blocks : TAIL_BLOCKS;
}

int rp_rollout_tail_dev(const float *d_rew_raw, const int32_t *d_done_i, const float *d_val, const float *d_last_val, float reward_scale,
                        const float *d_norm2, float clip, const double *d_shift, double gamma, double lam, double *d_ret_carry,
                        float *d_rew, float *d_done, float *d_adv, float *d_ret, double *d_sums3, double *d_scratch, int n_steps,
                        int64_t n_envs, void *stream) {
    return rollout_tail_launch(rollout_tail_kernel, "rollout_tail_kernel", d_rew_raw, d_done_i, d_val, d_last_val, reward_scale, d_norm2, clip,
                               d_shift, gamma, lam, d_ret_carry, d_rew, d_done, d_adv, d_ret, d_sums3, d_scratch, n_steps, n_envs, stream);
}

int rp_rollout_tail_boot_dev(const float *d_rew_raw, const int32_t *d_done_i, const float *d_val, const float *d_last_val, float reward_scale,
                             const float *d_norm2, float clip, const double *d_shift, double gamma, double lam, double *d_ret_carry,
                             float *d_rew, float *d_done, float *d_adv, float *d_ret, double *d_sums3, double *d_scratch, int n_steps,
                             int64_t n_envs, void *stream) {
    return rollout_tail_launch(rollout_tail_boot_kernel, "rollout_tail_boot_kernel", d_rew_raw, d_done_i, d_val, d_last_val, reward_scale, d_norm2,
                               clip, d_shift, gamma, lam, d_ret_carry, d_rew, d_done, d_adv, d_ret, d_sums3, d_scratch, n_steps, n_envs, stream);
}

int rp_clip_adam_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int act_dim, float lr,
                     float beta1, float beta2, float eps, int64_t step, float max_grad_norm, float grad_scale, float ent_coef,
                     void *stream) {
    return clip_adam_launch(d_params, d_grad, d_m, d_v, obs_dim, obs_dim, act_dim, lr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, beta1, beta2, eps, step,
                            max_grad_norm, grad_scale, ent_coef, stream);
}

int rp_clip_adam_asym_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int cobs_dim, int act_dim, float lr,
                          float beta1, float beta2, float eps, int64_t step, float max_grad_norm, float grad_scale, float ent_coef,
                          void *stream) {
    return clip_adam_launch(d_params, d_grad, d_m, d_v, obs_dim, cobs_dim, act_dim, lr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, beta1, beta2, eps, step,
                            max_grad_norm, grad_scale, ent_coef, stream);
}

int rp_clip_adam_kl_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int act_dim, float *d_lr,
                        float desired_kl, float lr_factor, float lr_min, float lr_max, float beta1, float beta2, float eps, int64_t step,
                        float max_grad_norm, float grad_scale, float ent_coef, void *stream) {
    return rp_clip_adam_kl_asym_dev(d_params, d_grad, d_m, d_v, obs_dim, obs_dim, act_dim, d_lr, desired_kl, lr_factor, lr_min, lr_max, beta1,
                                    beta2, eps, step, max_grad_norm, grad_scale, ent_coef, stream);
}

int rp_clip_adam_kl_asym_dev(float *d_params, const float *d_grad, float *d_m, float *d_v, int obs_dim, int cobs_dim, int act_dim, float *d_lr,
                             float desired_kl, float lr_factor, float lr_min, float lr_max, float beta1, float beta2, float eps, int64_t step,
                             float max_grad_norm, float grad_scale, float ent_coef, void *stream) {
    if (!d_lr) return fail(RP_EINVAL, "null argument");
    if (!(desired_kl > 0.0f)) return fail(RP_EINVAL, "desired_kl must be > 0");
    if (!(lr_factor > 1.0f)) return fail(RP_EINVAL, "lr_factor must be > 1");
    if (!(lr_min > 0.0f) || !(lr_min <= lr_max)) return fail(RP_EINVAL, "need 0 < lr_min <= lr_max");
    return clip_adam_launch(d_params, d_grad, d_m, d_v, obs_dim, cobs_dim, act_dim, 0.0f, d_lr, desired_kl, lr_factor, lr_min, lr_max, beta1, beta2,
                            eps, step, max_grad_norm, grad_scale, ent_coef, stream);
}

}  // extern "C"
