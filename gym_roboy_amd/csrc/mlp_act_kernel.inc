// mlp_act_kernel.inc - the text of the policy-step kernel, included by mlp_policy.hip once per instance: RP_NORM 0 is mlp_act_kernel
// (no statistics in its signature: the instruction stream it has always been), RP_NORM 1 is mlp_act_norm_kernel, whose observation
// operands are normalised as net_forward fetches them.
#if RP_NORM
#define RP_KERNEL mlp_act_norm_kernel
#define RP_NORM_PARAMS , const float *__restrict__ norm, float clip
#define RP_NORM_ARGS , norm, clip
#else
#define RP_KERNEL mlp_act_kernel
#define RP_NORM_PARAMS
#define RP_NORM_ARGS
#endif
__global__ void __launch_bounds__(256, 2)
RP_KERNEL(const float *__restrict__ packed, const float *__restrict__ obs, float *__restrict__ act,
          float *__restrict__ logp, float *__restrict__ value, float *__restrict__ mean_out, long n, int obs_dim,
          int act_dim, uint64_t seed, uint64_t sample_offset, uint32_t step, const uint32_t *__restrict__ step_base,
          int deterministic RP_NORM_PARAMS) {
    extern __shared__ float4 lds4[];
    if (step_base) step += *step_base;
    float *lds = reinterpret_cast<float *>(lds4);
    const Layout L = layout_of(obs_dim, act_dim);
    for (int k = threadIdx.x; k < L.total / 4; k += blockDim.x) lds4[k] = reinterpret_cast<const float4 *>(packed)[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const float onehot = half ? 0.0f : 1.0f;
    const long n_tiles = (n + 63) / 64;
    // work item = (tile, net): the two nets of a tile share nothing but the observation, so they go to different
    // waves - twice the items, half the dependent MFMA chain per item (what a small batch waits for: 4 096 samples are
    // 64 tiles for 1 024 SIMDs)
    for (long item = long(blockIdx.x) * nw + wave; item < 2 * n_tiles; item += long(gridDim.x) * nw) {
        const long tile = item >> 1;
        long s0 = tile * 64 + col, s1 = s0 + 32;                    // this lane's samples in column tile 0 / 1
        s0 = s0 < n ? s0 : n - 1; s1 = s1 < n ? s1 : n - 1;         // past the end: shadow the last sample
        const float *x0 = obs + s0 * obs_dim, *x1 = obs + s1 * obs_dim;
        const long i = tile * 64 + lane;
        const bool live = i < n;
        f32x16 ypi[2][2];
        if (item & 1) {                                              // the value net
            net_forward<RP_NORM>(lds, L, 1, 1, lane, onehot, x0, x1, obs_dim, ypi RP_NORM_ARGS);
            if (live) value[i] = ypi[0][0][0];                       // row 0 of its output tile
            continue;
        }
        net_forward<RP_NORM>(lds, L, 0, L.ot_pi, lane, onehot, x0, x1, obs_dim, ypi RP_NORM_ARGS);    // the action-mean net
        // ---- epilogue: this lane's sample ----
        float lp = -0.91893853320467274f * float(act_dim);          // -1/2 log(2 pi) per dimension
        float *arow = act + (live ? i : 0) * act_dim, *mrow = mean_out ? mean_out + (live ? i : 0) * act_dim : nullptr;
        const uint64_t gid = sample_offset + uint64_t(i);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    // rows 32 q + 8 g + 4 hh + (0..3): one Philox block gives their four normals
                    const int j0 = 32 * q + 8 * g + 4 * hh;
                    if (j0 < act_dim) {
                        float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (!deterministic) {
                            const rb::Philox4 u = rb::philox_draw(seed, gid, step, STREAM_POLICY, uint32_t(j0 >> 2));
#pragma unroll
                            for (int pr = 0; pr < 2; ++pr) {           // Box-Muller on (u1 in (0,1], u2 in [0,1))
                                const float u1 = float((u.v[2 * pr] >> 8) + 1u) * (1.0f / 16777216.0f);
                                const float u2 = rb::u01(u.v[2 * pr + 1]);
                                const float rad = __builtin_amdgcn_sqrtf(-2.0f * __logf(u1));
                                float sn, cs;
                                __sincosf(6.2831853071795865f * u2, &sn, &cs);
                                eps[2 * pr] = rad * cs; eps[2 * pr + 1] = rad * sn;
                            }
                        }
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int j = j0 + c;
                            if (j < act_dim) {
                                const float mu = hh ? ypi[q][1][4 * g + c] : ypi[q][0][4 * g + c];
                                const float ls = lds[L.o_logstd + j];
                                const float a = mu + __expf(ls) * eps[c];
                                lp -= 0.5f * eps[c] * eps[c] + ls;
                                if (live) { arow[j] = a; if (mrow) mrow[j] = mu; }
                            }
                        }
                    }
                }
        if (live) logp[i] = lp;
    }
}
#undef RP_KERNEL
#undef RP_NORM_PARAMS
#undef RP_NORM_ARGS
#undef RP_NORM
