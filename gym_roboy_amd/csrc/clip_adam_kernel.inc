// clip_adam_kernel.inc - the text of the clip + Adam kernel, included by mlp_update.hip once per instance: RP_KL 0 is clip_adam_kernel
// (const AdamArgs), RP_KL 1 is clip_adam_kl_kernel (const AdamArgs, const KlArgs): every thread reads the learning rate and the KL slot
// from the device and computes the new rate redundantly (adapt_lr); one thread stores it behind the barrier, when every thread has read
// the old one; Adam then steps with the new rate.  Everything else - the norm, the clipping coefficient, the moments - is one text.
#if RP_KL
#define RP_KERNEL clip_adam_kl_kernel
#define RP_KL_PARAMS , const KlArgs k
#define RP_LR lr
#else
#define RP_KERNEL clip_adam_kernel
#define RP_KL_PARAMS
#define RP_LR a.lr
#endif
__global__ void __launch_bounds__(1024)
RP_KERNEL(const AdamArgs a RP_KL_PARAMS) {
    __shared__ float sh[16];
#if RP_KL
    const float lr = adapt_lr(k.lr[0], a.g[k.kl_slot] * a.gscale, k);
#endif
    auto grad = [&](int i) {
        if (!(i < a.pi_end || (i >= a.vf_begin && i < a.vf_end))) return 0.0f;
        float g = a.g[i] * a.gscale;
        if (i >= a.ls_off && i < a.ls_off + a.ls_len) g -= a.ent_coef;
        return g;
    };
    float ss = 0.0f;
    for (int i = threadIdx.x; i < a.n; i += 1024) { const float g = grad(i); ss += g * g; }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ss;
    __syncthreads();
#if RP_KL
    if (threadIdx.x == 0) k.lr[0] = lr;
#endif
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += sh[w];
    // torch.nn.utils.clip_grad_norm_: coefficient max_norm / (norm + 1e-6), clamped to 1
    const float coef = fminf(a.max_norm / (sqrtf(tot) + 1e-6f), 1.0f);
    const float step = RP_LR / a.bc1, isb2 = 1.0f / sqrtf(a.bc2);
    for (int i = threadIdx.x; i < a.n; i += 1024) {
        if (!(i < a.pi_end || (i >= a.vf_begin && i < a.vf_end))) continue;
        const float g = grad(i) * coef;
        const float m = a.beta1 * a.m[i] + (1.0f - a.beta1) * g;
        const float v = a.beta2 * a.v[i] + (1.0f - a.beta2) * g * g;
        a.m[i] = m; a.v[i] = v;
        a.p[i] -= step * m / (sqrtf(v) * isb2 + a.eps);     // torch.optim.Adam: denom = sqrt(v) / sqrt(bc2) + eps
    }
}
#undef RP_KERNEL
#undef RP_KL_PARAMS
#undef RP_LR
#undef RP_KL
