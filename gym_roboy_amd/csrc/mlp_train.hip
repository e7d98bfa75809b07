// mlp_train.hip - the PPO minibatch gradient of MlpPolicy as one kernel per network on the matrix cores
// (include/roboy_policy.h: rp_ppo_grad_dev; gym_roboy_amd/ppo.py: _minibatch_loss is the torch statement of it).
//
// For a minibatch (obs, act, normalised advantage, old log-probability, old value, return), one launch per net
// (NET 0: action mean + log-std, the clipped surrogate; NET 1: value, the clipped value loss) runs, per 64-sample
// tile of a wave:  forward (as mlp_policy.hip; the activations stay in registers)  ->  per-sample loss derivative
// delta3 (one sample per lane)  ->  delta2 = (W3^T delta3) (1 - h2^2),  delta1 = (W2^T delta2) (1 - h1^2)  with
// the same "a layer's result registers are the next layer's B operands" chaining (the transposed weights are
// packed as A operands by rp_pack_train)  ->  the weight gradients  dW3 += delta3 h2^T, dW2 += delta2 h1^T,
// dW1 += delta1 [obs | 1]^T.  Those contract over SAMPLES, which sit on the lanes of every activation register,
// so both factors go through a 32x32 transpose in LDS (33-float rows: conflict-free both ways) into the layout
// "units on the lanes, samples in the registers"; there register r of the two factors is directly an A / B operand
// pair whose K pair is the samples (U(r), U(r) + 4) of the column tile.  The gradient accumulators (64 + 32 + 32
// registers of 32x32 tiles) live across all tiles of a wave; bias and log-std gradients are per-lane sums reduced
// once at the end.  Each wave writes its partial gradient (torch parameter order); a second kernel sums the waves.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "../../include/roboy_policy.h"
#include "mlp_common.hpp"

namespace {
using namespace rpd;

__device__ __forceinline__ void wave_fence() {         // orders this wave's LDS traffic (in-order per wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 32x32 transpose of an accumulator tile through the wave's LDS scratch T (32 rows of 33 floats):
// in: lane (column n = l & 31, half h), register r <-> row U(r) + 4 h;  out: the same with rows and columns exchanged
__device__ __forceinline__ f32x16 transpose_tile(const f32x16 &d, float *T, int col, int half) {
#pragma unroll
    for (int r = 0; r < 16; ++r) T[(unit_of(r) + 4 * half) * 33 + col] = d[r];
    wave_fence();
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = T[col * 33 + unit_of(r) + 4 * half];
    wave_fence();
    return o;
}

// One dword per lane from this lane's global address straight into LDS at (wave-uniform byte address) + 4 * lane: no
// register destination, so a tile's inputs can be in flight under the previous tile's arithmetic in a kernel that has no
// registers to spare.  hipcc does not count it: the consumer waits with wait_dma() (vmcnt covers loads in issue order).
__device__ __forceinline__ void dma_dword(const float *gsrc, const float *lds_dst) {
    const unsigned at = __builtin_amdgcn_readfirstlane(unsigned(reinterpret_cast<uintptr_t>(lds_dst)));   // LDS aperture: low 32 bits
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(at) : "memory");
}
__device__ __forceinline__ void wait_dma() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// A value read from a clamped address and then selected (`in range ? value : constant`) is what keeps an MFMA stage free of
// branches - but hipcc sinks such a read back under the condition: an EXEC-masked block per element (s_and_saveexec, address
// arithmetic, ds_read, s_or, s_waitcnt lgkmcnt(0)), i.e. one exposed LDS latency per MFMA pair and no scheduling across them.
// Passing the value through an empty asm statement pins the read where it is written.
__device__ __forceinline__ float pinned(float v) { asm volatile("" : "+v"(v)); return v; }
constexpr int PFS = 65;                                   // row stride of the prefetched inputs: [row][sample], conflict-free both ways

struct TrainArgs {
    const float *packed;                                  // rp_pack_train blob
    const float *obs, *act, *adv, *logp_old, *val_old, *ret;
    const long long *index;                               // row of sample i in obs / act / logp_old / val_old / ret (NULL: i); adv is direct ...
    const float *adv_stats;                               // ... unless this is given: {mean, 1 / (std + 1e-8)} of the minibatch's advantages
                                                          // (rp_adv_stats_dev); adv is then indexed like the rest and normalised here
    float *partials;                                      // [waves][gstride]
    long B;
    int obs_dim, act_dim, gstride;
    float cliprange, vf_coef, inv_B;
};

// KX: 32-column tiles of [obs | 1] (obs_dim + 1 <= 32 KX);  NJ: compile-time bound of the outputs (n_out <= NJ,
// a multiple of 8): the per-sample arrays of the loss derivative are NJ registers each
// PF (KX == 1 only): the tile's rows (observation, action, advantage, old log-probability | old value, return) arrive by
// LDS-DMA one tile ahead, double-buffered per wave; without it they are loaded when the tile starts (the indexed minibatch
// of 8 388 608 samples: 4.4 ms against 3.5 contiguous, 29 % of the wave cycles waiting)
// the instances of one kernel text (KX: 32-column tiles of [obs | 1]; NJ: bound of the outputs; PF: inputs by LDS-DMA - see the text):
// without normalisation and with it; and the action net's diagnostics instances of both (RP_DIAG 1: approx_kl and clip_frac)
// the mirror-symmetry loss: what the RP_SYM 1 instances take beside TrainArgs - a struct of its own, so that the
// kernel arguments of the instances above are what they were
struct SymArgs {
    const float *obs_image;                               // [rows][obs_dim]: row r is the mirror image M obs[r]
    float c2, lscale;                                     // 2 coef / (B A): the factor of d3;  coef / (B A): of the loss term
    int act_src[64];                                      // P: image action j is action act_src[j] (an involution; entries >= act_dim: 0)
};
constexpr int RP_SYM_LOSS_SLOT = 3;                       // L_sym's slot behind the action net's loss slot (roboy_policy.h: rp_sym_grad_dev)
#define RP_NORM 0
#define RP_DIAG 0
#define RP_SYM 0
#include "mlp_grad_kernel.inc"
#define RP_NORM 1
#define RP_DIAG 0
#define RP_SYM 0
#include "mlp_grad_kernel.inc"
#define RP_NORM 0
#define RP_DIAG 1
#define RP_SYM 0
#include "mlp_grad_kernel.inc"
#define RP_NORM 1
#define RP_DIAG 1
#define RP_SYM 0
#include "mlp_grad_kernel.inc"

// the symmetry-loss instances of the same text (RP_SYM 1)
#define RP_NORM 0
#define RP_DIAG 0
#define RP_SYM 1
#include "mlp_grad_kernel.inc"
#define RP_NORM 1
#define RP_DIAG 0
#define RP_SYM 1
#include "mlp_grad_kernel.inc"

// out[k] = sum over the partials (one per workgroup, `gstride` apart)
__global__ void reduce_partials_kernel(const float *__restrict__ partials, int n_waves, int gstride, int n, float *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int w = 0;
    for (; w + 3 < n_waves; w += 4) {
        s0 += partials[long(w) * gstride + k]; s1 += partials[long(w + 1) * gstride + k];
        s2 += partials[long(w + 2) * gstride + k]; s3 += partials[long(w + 3) * gstride + k];
    }
    for (; w < n_waves; ++w) s0 += partials[long(w) * gstride + k];
    out[k] = (s0 + s1) + (s2 + s3);
}

// reduce_partials_kernel's sums in its order for the symmetry loss's block: the parameter entries [0, n_params) and the one slot
// `slot` (L_sym) - the slots between them (pg loss, approx_kl, clip_frac) are neither read nor written.  The sum over the partials is
// formed first and added to what is there last (accumulate), so that accumulate = 1 onto g0 is exactly g0 + (accumulate = 0).
__global__ void reduce_sym_kernel(const float *__restrict__ partials, int n_waves, int gstride, int n_params, int slot, int accumulate,
                                  float *__restrict__ out) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_params) return;
    if (k == n_params) k = slot;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int w = 0;
    for (; w + 3 < n_waves; w += 4) {
        s0 += partials[long(w) * gstride + k]; s1 += partials[long(w + 1) * gstride + k];
        s2 += partials[long(w + 2) * gstride + k]; s3 += partials[long(w + 3) * gstride + k];
    }
    for (; w < n_waves; ++w) s0 += partials[long(w) * gstride + k];
    const float sum = (s0 + s1) + (s2 + s3);
    out[k] = accumulate ? out[k] + sum : sum;
}

// generalised advantage estimation over a [T][N] rollout, one env per thread, backwards in time (ppo.py: gae())
__global__ void gae_kernel(const float *__restrict__ rew, const float *__restrict__ val, const float *__restrict__ done,
                           const float *__restrict__ last_val, float gamma, float lam, float *__restrict__ adv,
                           float *__restrict__ ret, int T, long n) {
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float next_value = last_val[i], last = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const float nonterminal = 1.0f - done[t * n + i], v = val[t * n + i];
        const float delta = rew[t * n + i] + gamma * next_value * nonterminal - v;
        last = delta + gamma * lam * nonterminal * last;
        adv[t * n + i] = last;
        ret[t * n + i] = last + v;
        next_value = v;
    }
}

constexpr int WAVES_PER_BLOCK = 4;
// (every MI355X of a node has the same CU count, so the workspace size a caller asks for before it names a device -
// rp_ppo_workspace_floats - and the grid of the launch agree; the count is the current device's)
long grad_blocks(long B) {
    const long tiles = (B + 63) / 64;
    long blocks = (tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const long cap = cu_count(dev);
    return blocks < cap ? blocks : cap;
}

// dynamic LDS of one gradient-kernel instance: the staged operand blocks of one net + per-wave scratch
// (pf_rows > 0: the prefetching form's two input buffers per wave instead of the observation staging)
size_t grad_lds_bytes(const Layout &L, int net, int nj, int kx_inst, int pf_rows = 0) {
    const int ot = net == 0 ? L.ot_pi : 1;
    const size_t w = size_t(HT) * L.k1s * 64 + 2 * size_t(HT * HT * 16 * 64) + HT * 64 + size_t(ot) * (HT * 16 * 64 + 64) + 64 +
                     size_t(HT) * L.k3s[net] * 64;
    const size_t xs = pf_rows > 0 ? size_t(2) * pf_rows * PFS : (kx_inst == 1 ? 64 * 33 : 0);
    return sizeof(float) * (w + WAVES_PER_BLOCK * (32 * 33 + 64 * (nj + 1) + xs));
}
// the instance pair rp_ppo_grad_dev picks: the reference's robot class (obs <= 31, up to 8 actions) or the general
// one (obs <= 63, up to 64 actions); false if the general instance of the action net does not fit the 160 KB of LDS
bool grad_fits(int obs_dim, int act_dim) {
    const Layout L = layout_of(obs_dim, act_dim);
    const bool small = obs_dim + 1 <= 32 && act_dim <= 8;
    return grad_lds_bytes(L, 0, small ? 8 : 64, small ? 1 : 2) <= 160 * 1024;
}

template <int NET, int KX, int NJ, bool PF = false, bool DIAG = false>
int launch_grad(const TrainArgs &a, const float *norm, float clip, long blocks, size_t lds, int dev, hipStream_t stream) {
    // the opt-in above 64 KB of dynamic LDS is per kernel AND per device (mlp_common.hpp: grant_lds)
    constexpr int kernel_id = 1 + NET * 2 + (KX - 1) + (PF ? 4 : 0);
    if constexpr (DIAG) {                                  // the diagnostics instances (the action net's): kernels and grants of their own
        static_assert(NET == 0, "the diagnostics are the action net's");
        if (norm) {
            if (int rc = grant_lds(reinterpret_cast<const void *>(&mlp_grad_norm_diag_kernel<NET, KX, NJ, PF>), kernel_id + 27, dev, lds)) return rc;
            hipLaunchKernelGGL((mlp_grad_norm_diag_kernel<NET, KX, NJ, PF>), dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, stream, a, norm, clip);
        } else {
            if (int rc = grant_lds(reinterpret_cast<const void *>(&mlp_grad_diag_kernel<NET, KX, NJ, PF>), kernel_id + 18, dev, lds)) return rc;
            hipLaunchKernelGGL((mlp_grad_diag_kernel<NET, KX, NJ, PF>), dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, stream, a);
        }
    } else if (norm) {                                            // the normalising instance: a kernel of its own, a grant of its own
        if (int rc = grant_lds(reinterpret_cast<const void *>(&mlp_grad_norm_kernel<NET, KX, NJ, PF>), kernel_id + 9, dev, lds)) return rc;
        hipLaunchKernelGGL((mlp_grad_norm_kernel<NET, KX, NJ, PF>), dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, stream, a, norm, clip);
    } else {
        if (int rc = grant_lds(reinterpret_cast<const void *>(&mlp_grad_kernel<NET, KX, NJ, PF>), kernel_id, dev, lds)) return rc;
        hipLaunchKernelGGL((mlp_grad_kernel<NET, KX, NJ, PF>), dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, stream, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("mlp_grad_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

// the symmetry-loss instances: FORM 2 = small + prefetch, 1 = small (staged), 0 = general; kernels and LDS grants of their own
template <int KX, int NJ, bool PF>
int launch_sym(const TrainArgs &a, const SymArgs &sym, const float *norm, float clip, long blocks, size_t lds, int dev, hipStream_t stream) {
    constexpr int kernel_id = 36 + (KX - 1) + (PF ? 2 : 0);
    if (norm) {
        if (int rc = grant_lds(reinterpret_cast<const void *>(&mlp_sym_norm_kernel<0, KX, NJ, PF>), kernel_id + 3, dev, lds)) return rc;
        hipLaunchKernelGGL((mlp_sym_norm_kernel<0, KX, NJ, PF>), dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, stream, a, norm, clip, sym);
    } else {
        if (int rc = grant_lds(reinterpret_cast<const void *>(&mlp_sym_kernel<0, KX, NJ, PF>), kernel_id, dev, lds)) return rc;
        hipLaunchKernelGGL((mlp_sym_kernel<0, KX, NJ, PF>), dim3(unsigned(blocks)), dim3(64 * WAVES_PER_BLOCK), lds, stream, a, sym);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("mlp_sym_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

}  // namespace

extern "C" {

int64_t rp_train_packed_floats(int obs_dim, int act_dim) {
    if (rp_packed_floats(obs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    if (obs_dim + 1 > 64) return fail(RP_EUNSUPPORTED, "the gradient kernel supports obs_dim <= 63");
    if (!grad_fits(obs_dim, act_dim))
        return fail(RP_EUNSUPPORTED, "policy too large for the LDS-resident gradient kernel (operands + scratch > 160 KB)");
    return layout_of(obs_dim, act_dim).total_train;
}

int rp_pack_train(const rp_mlp_params *p, int obs_dim, int act_dim, float *out) {
    if (rp_train_packed_floats(obs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    const int rc = rp_pack(p, obs_dim, act_dim, out);
    if (rc) return rc;
    const Layout L = layout_of(obs_dim, act_dim);
    std::memset(out + L.total, 0, sizeof(float) * size_t(L.total_train - L.total));
    const float *w2[2] = {p->pi_w2, p->vf_w2}, *w3[2] = {p->pi_w3, p->vf_w3};
    for (int net = 0; net < 2; ++net) {
        const int n_out = net == 0 ? act_dim : 1;
        for (int m = 0; m < HT; ++m)
            for (int s = 0; s < L.k3s[net]; ++s)
                for (int l = 0; l < 64; ++l) {
                    const int unit = 32 * m + (l & 31), j = 2 * s + (l >> 5);
                    out[L.o_l3t[net] + (m * L.k3s[net] + s) * 64 + l] = j < n_out ? w3[net][j * H + unit] : 0.0f;
                }
        for (int ip = 0; ip < HT; ++ip)
            for (int o = 0; o < HT; ++o)
                for (int r = 0; r < 16; ++r)
                    for (int l = 0; l < 64; ++l) {
                        const int in = 32 * ip + (l & 31), outu = 32 * o + unit_of(r) + 4 * (l >> 5);
                        out[L.o_l2t[net] + ((ip * HT + o) * 16 + r) * 64 + l] = w2[net][outu * H + in];
                    }
    }
    return RP_OK;
}

int rp_gae_dev(const float *d_rew, const float *d_val, const float *d_done, const float *d_last_val, float gamma, float lam,
               float *d_adv, float *d_ret, int n_steps, int64_t n_envs, void *stream) {
    if (!d_rew || !d_val || !d_done || !d_last_val || !d_adv || !d_ret) return fail(RP_EINVAL, "null argument");
    if (n_steps < 1 || n_envs < 1) return fail(RP_EINVAL, "n_steps and n_envs must be >= 1");
    DeviceScope scope(d_rew); if (scope.rc) return scope.rc;
    hipLaunchKernelGGL(gae_kernel, dim3(unsigned((n_envs + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_rew,
                       d_val, d_done, d_last_val, gamma, lam, d_adv, d_ret, n_steps, long(n_envs));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("gae_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

// instances: the reference's robot class (obs <= 31, up to 8 actions; its inputs prefetched by LDS-DMA when the two
// buffers per wave fit beside the operands - ROBOY_POLICY_PREFETCH=0 keeps the loads at the start of each tile) and the
// general one (obs <= 63, 64 actions)
int rp_grad_form(int obs_dim, int act_dim) {
    if (rp_train_packed_floats(obs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    const Layout L = layout_of(obs_dim, act_dim);
    if (!((obs_dim + 1 + 31) / 32 == 1 && act_dim <= 8)) return 0;
    static const bool prefetch_off = [] { const char *e = getenv("ROBOY_POLICY_PREFETCH"); return e && e[0] == '0'; }();
    const bool fits = grad_lds_bytes(L, 0, 8, 1, obs_dim + act_dim + 4) <= 160 * 1024 && grad_lds_bytes(L, 1, 8, 1, obs_dim + 4) <= 160 * 1024;
    return !prefetch_off && fits ? 2 : 1;
}

int64_t rp_grad_floats(int obs_dim, int act_dim) {
    if (rp_train_packed_floats(obs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    return 2 * int64_t(gstride_of(obs_dim, act_dim));
}

int64_t rp_ppo_workspace_floats(int obs_dim, int act_dim, int64_t batch) {
    if (rp_train_packed_floats(obs_dim, act_dim) < 0 || batch < 1) return RP_EUNSUPPORTED;
    return 2 * grad_blocks(batch) * WAVES_PER_BLOCK * int64_t(gstride_of(obs_dim, act_dim));
}

int rp_ppo_grad_dev(const float *d_packed_train, const float *d_obs, const float *d_act, const float *d_adv,
                    const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                    const int64_t *d_index, int64_t batch, int obs_dim, int act_dim, float cliprange, float vf_coef,
                    float *d_grad, float *d_workspace, void *stream) {
    return rp_ppo_grad_norm_dev(d_packed_train, d_obs, d_act, d_adv, d_adv_stats, d_logp_old, d_val_old, d_ret, d_index, batch, obs_dim,
                                act_dim, cliprange, vf_coef, nullptr, 0.0f, d_grad, d_workspace, stream);
}

}  // extern "C"

namespace {
// One net's launch: the instance its OWN input width asks for (rp_grad_form: small + prefetch, small, general), with the arguments
// `a` as they stand (a.packed, a.obs, a.obs_dim, a.gstride and a.partials are that net's).  diag: the action net's diagnostics instance.
template <int NET>
int grad_net_launch(bool diag, const TrainArgs &a, const float *d_norm, float clip, long blocks, int dev, hipStream_t st) {
    const int obs_dim = a.obs_dim, act_dim = a.act_dim;
    const Layout L = layout_of(obs_dim, act_dim);
    auto lds_of = [&](int nj, int kx_inst, int pf_rows = 0) { return grad_lds_bytes(L, NET, nj, kx_inst, pf_rows); };
    const int form = rp_grad_form(obs_dim, act_dim);                     // 2: small + prefetch, 1: small, 0: general
    const bool small = form >= 1, pf = form == 2;
    const int pf_rows = obs_dim + (NET == 0 ? act_dim : 0) + 4;         // rows of one input buffer (mlp_grad_kernel: pf_rows)
    if constexpr (NET == 0) {
        if (diag) {
            if (pf) return launch_grad<0, 1, 8, true, true>(a, d_norm, clip, blocks, lds_of(8, 1, pf_rows), dev, st);
            if (small) return launch_grad<0, 1, 8, false, true>(a, d_norm, clip, blocks, lds_of(8, 1), dev, st);
            return launch_grad<0, 2, 64, false, true>(a, d_norm, clip, blocks, lds_of(64, 2), dev, st);
        }
        if (pf) return launch_grad<0, 1, 8, true>(a, d_norm, clip, blocks, lds_of(8, 1, pf_rows), dev, st);
        if (small) return launch_grad<0, 1, 8>(a, d_norm, clip, blocks, lds_of(8, 1), dev, st);
        return launch_grad<0, 2, 64>(a, d_norm, clip, blocks, lds_of(64, 2), dev, st);
    } else {
        if (pf) return launch_grad<1, 1, 8, true>(a, d_norm, clip, blocks, lds_of(8, 1, pf_rows), dev, st);
        if (small) return launch_grad<1, 1, 8>(a, d_norm, clip, blocks, lds_of(8, 1), dev, st);
        return launch_grad<1, 2, 8>(a, d_norm, clip, blocks, lds_of(8, 2), dev, st);
    }
}

// Every gradient entry point: its checks and its launches.  The symmetric ones hand both nets the same blob, rows, width and
// statistics; rp_ppo_grad_asym_dev gives the value net (NET 1) its own - the kernels are the same instances either way.  The gradient
// vector: the action net's block at stride gstride_of(obs_dim, act_dim), then the value net's at gstride_of(cobs_dim, act_dim); the
// workspace: the action net's partials, then the value net's.  diag: the action net's launch is its diagnostics instance.
int ppo_grad_launch(bool diag, const float *d_packed_pi, const float *d_packed_vf, const float *d_obs, const float *d_cobs, const float *d_act,
                    const float *d_adv, const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                    const int64_t *d_index, int64_t batch, int obs_dim, int cobs_dim, int act_dim, float cliprange, float vf_coef,
                    const float *d_norm_pi, float clip_pi, const float *d_norm_vf, float clip_vf, float *d_grad, float *d_workspace, void *stream) {
    if ((d_norm_pi && !(clip_pi > 0.0f)) || (d_norm_vf && !(clip_vf > 0.0f))) return fail(RP_EINVAL, "clip must be > 0");
    if (!d_packed_pi || !d_packed_vf || !d_obs || !d_cobs || !d_act || !d_adv || !d_logp_old || !d_val_old || !d_ret || !d_grad || !d_workspace)
        return fail(RP_EINVAL, "null argument");
    if (batch < 1) return fail(RP_EINVAL, "batch must be >= 1");
    if (rp_train_packed_floats(obs_dim, act_dim) < 0 || rp_train_packed_floats(cobs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    int dev = 0;
    DeviceScope scope(d_packed_pi); if (scope.rc) return scope.rc; dev = scope.dev;         // the blob's device is the device of the call
    const int gs_pi = gstride_of(obs_dim, act_dim), gs_vf = gstride_of(cobs_dim, act_dim);
    const long blocks = grad_blocks(batch), waves = blocks * WAVES_PER_BLOCK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainArgs a;
    a.packed = d_packed_pi; a.obs = d_obs; a.act = d_act; a.adv = d_adv; a.adv_stats = d_adv_stats; a.logp_old = d_logp_old; a.val_old = d_val_old;
    a.ret = d_ret; a.index = reinterpret_cast<const long long *>(d_index); a.B = batch; a.obs_dim = obs_dim; a.act_dim = act_dim; a.gstride = gs_pi; a.cliprange = cliprange;
    a.vf_coef = vf_coef; a.inv_B = 1.0f / float(batch);
    a.partials = d_workspace;
    int rc = grad_net_launch<0>(diag, a, d_norm_pi, clip_pi, blocks, dev, st);
    if (rc) return rc;
    a.packed = d_packed_vf; a.obs = d_cobs; a.obs_dim = cobs_dim; a.gstride = gs_vf;
    a.partials = d_workspace + waves * gs_pi;
    rc = grad_net_launch<1>(false, a, d_norm_vf, clip_vf, blocks, dev, st);
    if (rc) return rc;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((gs_pi + 255) / 256), dim3(256), 0, st, d_workspace, int(blocks), WAVES_PER_BLOCK * gs_pi, gs_pi,
                       d_grad);                                                             // one folded partial per workgroup
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((gs_vf + 255) / 256), dim3(256), 0, st, d_workspace + waves * gs_pi, int(blocks),
                       WAVES_PER_BLOCK * gs_vf, gs_vf, d_grad + gs_pi);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("reduce_partials_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}
}  // namespace

extern "C" {

int rp_ppo_grad_norm_dev(const float *d_packed_train, const float *d_obs, const float *d_act, const float *d_adv,
                         const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                         const int64_t *d_index, int64_t batch, int obs_dim, int act_dim, float cliprange, float vf_coef,
                         const float *d_norm, float clip, float *d_grad, float *d_workspace, void *stream) {
    return ppo_grad_launch(false, d_packed_train, d_packed_train, d_obs, d_obs, d_act, d_adv, d_adv_stats, d_logp_old, d_val_old, d_ret, d_index, batch,
                           obs_dim, obs_dim, act_dim, cliprange, vf_coef, d_norm, clip, d_norm, clip, d_grad, d_workspace, stream);
}

int rp_ppo_grad_diag_dev(const float *d_packed_train, const float *d_obs, const float *d_act, const float *d_adv,
                         const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                         const int64_t *d_index, int64_t batch, int obs_dim, int act_dim, float cliprange, float vf_coef,
                         const float *d_norm, float clip, float *d_grad, float *d_workspace, void *stream) {
    return ppo_grad_launch(true, d_packed_train, d_packed_train, d_obs, d_obs, d_act, d_adv, d_adv_stats, d_logp_old, d_val_old, d_ret, d_index, batch,
                           obs_dim, obs_dim, act_dim, cliprange, vf_coef, d_norm, clip, d_norm, clip, d_grad, d_workspace, stream);
}

// ---- the mirror-symmetry loss: one launch of an RP_SYM instance over ceil(batch / 32) pair tiles + its reduction ----
// the small instance's two variants: the prefetching one wherever its two input buffers per wave (obs_dim + 2 rows each: fewer than
// the PPO kernel's, which also carry the actions, the advantage and the old log-probability) fit beside the operands - that is every
// small policy - unless ROBOY_POLICY_PREFETCH=0
int rp_sym_grad_form(int obs_dim, int act_dim) {
    if (rp_train_packed_floats(obs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    const Layout L = layout_of(obs_dim, act_dim);
    if (!((obs_dim + 1 + 31) / 32 == 1 && act_dim <= 8)) return 0;
    static const bool prefetch_off = [] { const char *e = getenv("ROBOY_POLICY_PREFETCH"); return e && e[0] == '0'; }();
    return !prefetch_off && grad_lds_bytes(L, 0, 8, 1, obs_dim + 2) <= 160 * 1024 ? 2 : 1;
}

int64_t rp_sym_workspace_floats(int obs_dim, int act_dim, int64_t batch) {
    if (rp_train_packed_floats(obs_dim, act_dim) < 0 || batch < 1) return RP_EUNSUPPORTED;
    return grad_blocks(2 * batch) * WAVES_PER_BLOCK * int64_t(gstride_of(obs_dim, act_dim));
}

int rp_sym_grad_norm_dev(const float *d_packed_train, const float *d_obs, const float *d_obs_image, const int64_t *d_index, int64_t batch,
                         int obs_dim, int act_dim, const int32_t *act_src, float coef, const float *d_norm, float clip, float *d_grad_pi,
                         int accumulate, float *d_workspace, void *stream) {
    if (d_norm && !(clip > 0.0f)) return fail(RP_EINVAL, "clip must be > 0");
    if (!d_packed_train || !d_obs || !d_obs_image || !act_src || !d_grad_pi || !d_workspace) return fail(RP_EINVAL, "null argument");
    if (batch < 1) return fail(RP_EINVAL, "batch must be >= 1");
    if (!(coef >= 0.0f) || !(coef <= 3.0e38f)) return fail(RP_EINVAL, "coef must be finite and >= 0");
    if (rp_train_packed_floats(obs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    SymArgs sym;
    for (int j = 0; j < 64; ++j) sym.act_src[j] = 0;
    for (int j = 0; j < act_dim; ++j) {
        const int p = act_src[j];
        if (p < 0 || p >= act_dim || act_src[p] != j)
            return fail(RP_EINVAL, "act_src must be an involution of [0, act_dim): act_src[act_src[j]] == j for every j");
        sym.act_src[j] = p;
    }
    sym.obs_image = d_obs_image;
    sym.lscale = float(double(coef) / (double(batch) * double(act_dim)));
    sym.c2 = float(2.0 * double(coef) / (double(batch) * double(act_dim)));
    DeviceScope scope(d_packed_train); if (scope.rc) return scope.rc;
    const int dev = scope.dev;
    const int gs = gstride_of(obs_dim, act_dim);
    const long blocks = grad_blocks(2 * batch);                         // ceil(batch / 32) pair tiles, four waves per workgroup
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainArgs a;
    a.packed = d_packed_train; a.obs = d_obs; a.act = nullptr; a.adv = nullptr; a.adv_stats = nullptr; a.logp_old = nullptr; a.val_old = nullptr;
    a.ret = nullptr; a.index = reinterpret_cast<const long long *>(d_index); a.B = batch; a.obs_dim = obs_dim; a.act_dim = act_dim; a.gstride = gs;
    a.cliprange = 0.0f; a.vf_coef = 0.0f; a.inv_B = 1.0f / float(batch);
    a.partials = d_workspace;
    const Layout L = layout_of(obs_dim, act_dim);
    const int form = rp_sym_grad_form(obs_dim, act_dim);
    int rc;
    if (form == 2) rc = launch_sym<1, 8, true>(a, sym, d_norm, clip, blocks, grad_lds_bytes(L, 0, 8, 1, obs_dim + 2), dev, st);
    else if (form == 1) rc = launch_sym<1, 8, false>(a, sym, d_norm, clip, blocks, grad_lds_bytes(L, 0, 8, 1), dev, st);
    else rc = launch_sym<2, 64, false>(a, sym, d_norm, clip, blocks, grad_lds_bytes(L, 0, 64, 2), dev, st);
    if (rc) return rc;
    const GOff g = goff_of(obs_dim, act_dim);
    hipLaunchKernelGGL(reduce_sym_kernel, dim3((g.loss + 1 + 255) / 256), dim3(256), 0, st, d_workspace, int(blocks), WAVES_PER_BLOCK * gs, g.loss,
                       g.loss + RP_SYM_LOSS_SLOT, accumulate != 0 ? 1 : 0, d_grad_pi);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("reduce_sym_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

int rp_sym_grad_dev(const float *d_packed_train, const float *d_obs, const float *d_obs_image, const int64_t *d_index, int64_t batch,
                    int obs_dim, int act_dim, const int32_t *act_src, float coef, float *d_grad_pi, int accumulate, float *d_workspace,
                    void *stream) {
    return rp_sym_grad_norm_dev(d_packed_train, d_obs, d_obs_image, d_index, batch, obs_dim, act_dim, act_src, coef, nullptr, 0.0f, d_grad_pi,
                                accumulate, d_workspace, stream);
}

// ---- the asymmetric critic: the value net on rows and a blob of its own, the same kernel instances ----
int64_t rp_grad_asym_floats(int obs_dim, int cobs_dim, int act_dim) {
    if (rp_train_packed_floats(obs_dim, act_dim) < 0 || rp_train_packed_floats(cobs_dim, act_dim) < 0) return RP_EUNSUPPORTED;
    return int64_t(gstride_of(obs_dim, act_dim)) + int64_t(gstride_of(cobs_dim, act_dim));
}

int64_t rp_ppo_asym_workspace_floats(int obs_dim, int cobs_dim, int act_dim, int64_t batch) {
    const int64_t n = rp_grad_asym_floats(obs_dim, cobs_dim, act_dim);
    if (n < 0 || batch < 1) return RP_EUNSUPPORTED;
    return grad_blocks(batch) * WAVES_PER_BLOCK * n;
}

int rp_ppo_grad_asym_dev(const float *d_packed_pi, const float *d_packed_vf, const float *d_obs, const float *d_cobs, const float *d_act,
                         const float *d_adv, const float *d_adv_stats, const float *d_logp_old, const float *d_val_old, const float *d_ret,
                         const int64_t *d_index, int64_t batch, int obs_dim, int cobs_dim, int act_dim, float cliprange, float vf_coef,
                         const float *d_norm_pi, const float *d_norm_vf, float clip_pi, float clip_vf, int diag, float *d_grad,
                         float *d_workspace, void *stream) {
    if ((d_norm_pi == nullptr) != (d_norm_vf == nullptr)) return fail(RP_EINVAL, "statistics for both nets, or for neither");
    return ppo_grad_launch(diag != 0, d_packed_pi, d_packed_vf, d_obs, d_cobs, d_act, d_adv, d_adv_stats, d_logp_old, d_val_old, d_ret, d_index,
                           batch, obs_dim, cobs_dim, act_dim, cliprange, vf_coef, d_norm_pi, clip_pi, d_norm_vf, clip_vf, d_grad, d_workspace, stream);
}

}  // extern "C"
