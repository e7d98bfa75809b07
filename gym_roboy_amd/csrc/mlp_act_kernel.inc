// mlp_act_kernel.inc - the text of the policy-step kernel, included by mlp_policy.hip once per instance: RP_NORM 0 is mlp_act_kernel
// (no statistics in its signature: the instruction stream it has always been), RP_NORM 1 is mlp_act_norm_kernel, whose observation
// operands are normalised as net_forward fetches them.
// RP_ASYM 1 (DESIGN.md §20): mlp_act_asym_kernel / mlp_act_asym_norm_kernel, the policy step of an asymmetric critic - the value net
// reads rows of its own (cobs, cobs_dim columns) through a blob packed for (cobs_dim, act_dim), and in the norm instance its own
// statistics and clip.  ONE NET PER WORKGROUP: the first pi_blocks workgroups run the action net over the tiles, the others the value
// net, and each stages only its net's operand blocks (offsets of the blob rebased, as mlp_grad_kernel.inc does) - the two nets share
// nothing, not even the observation.  Work items, net_forward and the epilogue are the text below; RP_ASYM 0 expands to the text as it
// was.
#if RP_ASYM && RP_NORM
#define RP_KERNEL mlp_act_asym_norm_kernel
#define RP_NORM_PARAMS , const float *__restrict__ norm, float clip, const float *__restrict__ norm_vf, float clip_vf
#define RP_NORM_ARGS , norm, clip
#define RP_NORM_ARGS_VF , norm_vf, clip_vf
#elif RP_ASYM
#define RP_KERNEL mlp_act_asym_kernel
#define RP_NORM_PARAMS
#define RP_NORM_ARGS
#define RP_NORM_ARGS_VF
#elif RP_NORM
#define RP_KERNEL mlp_act_norm_kernel
#define RP_NORM_PARAMS , const float *__restrict__ norm, float clip
#define RP_NORM_ARGS , norm, clip
#define RP_NORM_ARGS_VF , norm, clip
#else
#define RP_KERNEL mlp_act_kernel
#define RP_NORM_PARAMS
#define RP_NORM_ARGS
#define RP_NORM_ARGS_VF
#endif
// The epilogue's loop-invariant scalars - the 64 `j < act_dim` masks, the Philox key schedule of `seed` - are hoisted in front of
// the tile loop by hipcc and live across net_forward, where the symmetric instances park them in spare VGPR lanes (101 / 111 SGPR
// spills, no scratch).  RP_ASYM 1 re-reads the two values through an empty asm statement once per tile, so nothing derived from them
// is loop-invariant: the epilogue forms them where it uses them.  RP_ASYM 0 names the arguments themselves: the text as it was.
#if RP_ASYM
#define RP_ASYM_PARAMS , const float *__restrict__ packed_vf, const float *__restrict__ cobs, int cobs_dim, int pi_blocks
#define RP_ACT_DIM act_dim_tile
#define RP_SEED seed_tile
#else
#define RP_ASYM_PARAMS
#define RP_ACT_DIM act_dim
#define RP_SEED seed
#endif
__global__ void __launch_bounds__(256, 2)
RP_KERNEL(const float *__restrict__ packed, const float *__restrict__ obs, float *__restrict__ act,
          float *__restrict__ logp, float *__restrict__ value, float *__restrict__ mean_out, long n, int obs_dim,
          int act_dim, uint64_t seed, uint64_t sample_offset, uint32_t step, const uint32_t *__restrict__ step_base,
          int deterministic RP_ASYM_PARAMS RP_NORM_PARAMS) {
    extern __shared__ float4 lds4[];
    if (step_base) step += *step_base;
    float *lds = reinterpret_cast<float *>(lds4);
#if RP_ASYM
    const bool value_net = int(blockIdx.x) >= pi_blocks;           // (workgroup-uniform)
    Layout L;
    {   // this net's operand blocks of its blob -> LDS, one behind the other (all blocks are multiples of 4 floats)
        const float *blob = value_net ? packed_vf : packed;
        const Layout G = layout_of(value_net ? cobs_dim : obs_dim, act_dim);
        L = G;
        int used = 0;
        auto stage = [&](int src, int n_floats) {
            const float4 *s4 = reinterpret_cast<const float4 *>(blob + src);
            for (int k = threadIdx.x; k < n_floats / 4; k += blockDim.x) lds4[used / 4 + k] = s4[k];
            const int at = used;
            used += n_floats;
            return at;
        };
        // (the blocks of fixed size first: their LDS offsets are compile-time constants, not scalar registers)
        if (value_net) {
            L.o_l2[1] = stage(G.o_l2[1], HT * HT * 16 * 64);
            L.o_b2[1] = stage(G.o_b2[1], HT * 64);
            L.o_l3[1] = stage(G.o_l3[1], HT * 16 * 64);
            L.o_b3[1] = stage(G.o_b3[1], 64);
            L.o_l1 = stage(G.o_l1 + HT * G.k1s * 64, HT * G.k1s * 64) - HT * G.k1s * 64;     // (net_forward adds the net's row tiles)
        } else {
            L.o_l2[0] = stage(G.o_l2[0], HT * HT * 16 * 64);
            L.o_b2[0] = stage(G.o_b2[0], HT * 64);
            L.o_logstd = stage(G.o_logstd, 64);
            L.o_l3[0] = stage(G.o_l3[0], G.ot_pi * HT * 16 * 64);
            L.o_b3[0] = stage(G.o_b3[0], G.ot_pi * 64);
            L.o_l1 = stage(G.o_l1, HT * G.k1s * 64);
        }
    }
#else
    const Layout L = layout_of(obs_dim, act_dim);
    for (int k = threadIdx.x; k < L.total / 4; k += blockDim.x) lds4[k] = reinterpret_cast<const float4 *>(packed)[k];
#endif
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const float onehot = half ? 0.0f : 1.0f;
    const long n_tiles = (n + 63) / 64;
    // work item = (tile, net): the two nets of a tile share nothing but the observation, so they go to different
    // waves - twice the items, half the dependent MFMA chain per item (what a small batch waits for: 4 096 samples are
    // 64 tiles for 1 024 SIMDs)
#if RP_ASYM
    // work item = a tile of this workgroup's net: the net's workgroups stride over the tiles
    const long first_block = value_net ? pi_blocks : 0, net_blocks = value_net ? long(gridDim.x) - pi_blocks : pi_blocks;
    for (long tile = (long(blockIdx.x) - first_block) * nw + wave; tile < n_tiles; tile += net_blocks * nw) {
#else
    for (long item = long(blockIdx.x) * nw + wave; item < 2 * n_tiles; item += long(gridDim.x) * nw) {
        const long tile = item >> 1;
#endif
        long s0 = tile * 64 + col, s1 = s0 + 32;                    // this lane's samples in column tile 0 / 1
        s0 = s0 < n ? s0 : n - 1; s1 = s1 < n ? s1 : n - 1;         // past the end: shadow the last sample
#if !RP_ASYM
        const float *x0 = obs + s0 * obs_dim, *x1 = obs + s1 * obs_dim;
#endif
        const long i = tile * 64 + lane;
        const bool live = i < n;
        f32x16 ypi[2][2];
#if RP_ASYM
        if (value_net) {                                             // the value net, on the critic's rows
            const float *x0 = cobs + s0 * cobs_dim, *x1 = cobs + s1 * cobs_dim;
            net_forward<RP_NORM>(lds, L, 1, 1, lane, onehot, x0, x1, cobs_dim, ypi RP_NORM_ARGS_VF);
            if (live) value[i] = ypi[0][0][0];                       // row 0 of its output tile
            continue;
        }
        const float *x0 = obs + s0 * obs_dim, *x1 = obs + s1 * obs_dim;
        int act_dim_tile = act_dim;
        uint32_t seed_lo = uint32_t(seed), seed_hi = uint32_t(seed >> 32);
        asm volatile("" : "+s"(act_dim_tile), "+s"(seed_lo), "+s"(seed_hi));
        const uint64_t seed_tile = uint64_t(seed_hi) << 32 | seed_lo;
#else
        if (item & 1) {                                              // the value net
            net_forward<RP_NORM>(lds, L, 1, 1, lane, onehot, x0, x1, obs_dim, ypi RP_NORM_ARGS);
            if (live) value[i] = ypi[0][0][0];                       // row 0 of its output tile
            continue;
        }
#endif
        net_forward<RP_NORM>(lds, L, 0, L.ot_pi, lane, onehot, x0, x1, obs_dim, ypi RP_NORM_ARGS);    // the action-mean net
        // ---- epilogue: this lane's sample ----
        float lp = -0.91893853320467274f * float(RP_ACT_DIM);          // -1/2 log(2 pi) per dimension
        float *arow = act + (live ? i : 0) * RP_ACT_DIM, *mrow = mean_out ? mean_out + (live ? i : 0) * RP_ACT_DIM : nullptr;
        const uint64_t gid = sample_offset + uint64_t(i);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    // rows 32 q + 8 g + 4 hh + (0..3): one Philox block gives their four normals
                    const int j0 = 32 * q + 8 * g + 4 * hh;
                    if (j0 < RP_ACT_DIM) {
                        float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (!deterministic) {
                            const rb::Philox4 u = rb::philox_draw(RP_SEED, gid, step, STREAM_POLICY, uint32_t(j0 >> 2));
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
                            if (j < RP_ACT_DIM) {
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
#undef RP_NORM_ARGS_VF
#undef RP_ASYM_PARAMS
#undef RP_ACT_DIM
#undef RP_SEED
#undef RP_NORM
#undef RP_ASYM
