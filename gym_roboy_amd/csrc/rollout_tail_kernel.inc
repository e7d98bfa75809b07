// rollout_tail_kernel.inc - the text of the rollout tail's kernel, included by mlp_update.hip once per instance (as mlp_act_kernel.inc
// is by mlp_policy.hip): RP_BOOT 0 is rollout_tail_kernel, the instruction stream it has always been; RP_BOOT 1 is
// rollout_tail_boot_kernel, whose done words are episode-end codes (0 none, 1 terminated, 2 truncated) and whose backward scan
// bootstraps the truncated steps (DESIGN.md §17).  The forward scan is the same text: it resets on any non-zero word.
#if RP_BOOT
#define RP_TAIL_KERNEL rollout_tail_boot_kernel
#else
#define RP_TAIL_KERNEL rollout_tail_kernel
#endif
__global__ void __launch_bounds__(256, 4)                  // four waves per SIMD: 262 144 envs are one resident grid of 1 024 workgroups
RP_TAIL_KERNEL(const float *__restrict__ rew_raw, const int *__restrict__ done_i, const float *__restrict__ val,
                    const float *__restrict__ last_val, float scale, const float *__restrict__ norm2, float clip,
                    const double *__restrict__ shift, double gamma, float lam, double *__restrict__ ret_carry, float *__restrict__ rew,
                    float *__restrict__ done, float *__restrict__ adv, float *__restrict__ ret, double *__restrict__ sums3,
                    double *scratch, int T, long long n) {
    const float rstd = norm2 ? norm2[1] : 1.0f, gamma_f = float(gamma);
    const double sft = shift ? shift[0] : 0.0;
    double s = 0.0, ss = 0.0;
    // Addresses: the base of a chunk's first row, t0 * n, is wave-uniform (a scalar pair per array and chunk); the lane adds one
    // 32-bit byte offset per step of the chunk, 4 (u n + i), shared by all seven arrays (n < 2^26, checked by the caller: the offsets
    // of TAIL_UNROLL rows fit 32 bits) - instead of a 64-bit register pair per array and step
    const unsigned rowb = unsigned(n) * 4u;
    // (the row base goes through readfirstlane: it stays a scalar pair, and the loop optimiser does not turn every (array, step) into
    // a 64-bit induction pointer per lane of its own)
    TAIL_ADDRESSING
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned boff = unsigned(i) * 4u;
        double R = ret_carry[i];
        int t = 0;
        for (; t + TAIL_UNROLL <= T; t += TAIL_UNROLL) {
            const long long row = (long long)t * n;
            float r[TAIL_UNROLL]; int dn[TAIL_UNROLL];
#pragma unroll
            for (int u = 0; u < TAIL_UNROLL; ++u) { r[u] = ldf(rew_raw + row, boff + u * rowb); dn[u] = ldi(done_i + row, boff + u * rowb); }
#pragma unroll
            for (int u = 0; u < TAIL_UNROLL; ++u) {
                R = gamma * R + double(__fmul_rn(r[u], scale));
                const double d = R - sft;
                s += d; ss += d * d;
                R = dn[u] ? 0.0 : R;
            }
        }
#pragma unroll 1
        for (; t < T; ++t) {
            const long long row = (long long)t * n;
            R = gamma * R + double(__fmul_rn(ldf(rew_raw + row, boff), scale));
            const double d = R - sft;
            s += d; ss += d * d;
            R = ldi(done_i + row, boff) ? 0.0 : R;
        }
        ret_carry[i] = R;

        float next_value = last_val[i], lastgae = 0.0f;
        auto step = [&](long long row, unsigned off, float rr, int dd, float v) {
            const float rt = __builtin_amdgcn_fmed3f(__fmul_rn(__fmul_rn(rr, scale), rstd), -clip, clip);
#if RP_BOOT
            // dd is an episode-end code: any non-zero one ends the episode; a truncated step (2) bootstraps the value of the state it was
            // cut at into its reward, r^ = fl32(r~ + fl32(gamma v)) - two roundings, no contraction; rew below still receives r~
            const float df = dd ? 1.0f : 0.0f, nonterminal = 1.0f - df;
            const float rb = dd == 2 ? __fadd_rn(rt, __fmul_rn(gamma_f, v)) : rt;
            const float delta = rb + gamma_f * next_value * nonterminal - v;
#else
            const float df = float(dd), nonterminal = 1.0f - df;
            const float delta = rt + gamma_f * next_value * nonterminal - v;
#endif
            lastgae = delta + gamma_f * lam * nonterminal * lastgae;
            st(rew + row, off, rt); st(done + row, off, df); st(adv + row, off, lastgae); st(ret + row, off, lastgae + v);
            next_value = v;
        };
        t = T - 1;
        for (; t - (TAIL_UNROLL - 1) >= 0; t -= TAIL_UNROLL) {
            const long long row = (long long)(t - (TAIL_UNROLL - 1)) * n;      // the chunk's lowest row; step u is row TAIL_UNROLL - 1 - u of it
            float r[TAIL_UNROLL], v[TAIL_UNROLL]; int dn[TAIL_UNROLL];
#pragma unroll
            for (int u = 0; u < TAIL_UNROLL; ++u) {
                const unsigned off = boff + (TAIL_UNROLL - 1 - u) * rowb;
                r[u] = ldf(rew_raw + row, off); dn[u] = ldi(done_i + row, off); v[u] = ldf(val + row, off);
            }
#pragma unroll
            for (int u = 0; u < TAIL_UNROLL; ++u) step(row, boff + (TAIL_UNROLL - 1 - u) * rowb, r[u], dn[u], v[u]);
        }
#pragma unroll 1
        for (; t >= 0; --t) {
            const long long row = (long long)t * n;
            step(row, boff, ldf(rew_raw + row, boff), ldi(done_i + row, boff), ldf(val + row, boff));
        }
    }
    tail_reduce<256>(s, ss, scratch, sums3, T, n);
}
#undef RP_TAIL_KERNEL
#undef RP_BOOT
