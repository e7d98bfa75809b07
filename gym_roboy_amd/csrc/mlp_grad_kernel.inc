// mlp_grad_kernel.inc - the text of the PPO-gradient kernel, included by mlp_train.hip once per instance family: RP_NORM 0 is
// mlp_grad_kernel<NET, KX, NJ, PF> (no statistics in its signature: the instruction streams it has always had), RP_NORM 1 is
// mlp_grad_norm_kernel<...>.
// RP_NORM 1: every observation operand - the layer-1 B operands and the dW1 operands, staged, direct or prefetched - goes through
// obs_operand() (mlp_common.hpp) with the statistics norm = float[2][obs_dim]: the staged form normalises the rows once as they go to
// LDS; the direct and the prefetched form where the raw value is read (scalar loads of the K step's pair in the forward pass, the
// lane's column pair loaded per tile for dW1).  No LDS for the statistics: the budget of every form is what it was.
// RP_DIAG 1 (the action net only; DESIGN.md §19): mlp_grad_diag_kernel / mlp_grad_norm_diag_kernel also leave the update's diagnostics
// in the spare slots behind the loss term: x = logp - logp_old, approx_kl = sum 0.5 x^2 / B at loss + 1 - one more per-lane sum beside
// loss_sum, under the same `live` guard, kept in the lane's pad word of the delta3 staging (row stride NJ + 1: word NJ is never staged)
// instead of a register the tile loop has not got - and clip_frac = #{rc != ratio} / B at loss + 2, counted per tile over the wave (a
// ballot of the live lanes the clamp acted on: the running count is wave-uniform and costs no vector register).  RP_DIAG 0 expands
// to the text as it was.
// RP_SYM 1 (the action net only; DESIGN.md §26): mlp_sym_kernel / mlp_sym_norm_kernel, the gradient of the mirror-symmetry loss
//     L_sym = coef / (B A) sum_i sum_j (mu(M s_i)[j] - mu(s_i)[P j])^2
// A wave tile is 32 PAIRS: column tile 0 holds the rows s_i of `obs`, column tile 1 the same rows of `obs_image` (M s_i), through the
// same staged, direct or prefetched operand paths.  After the forward pass lane l holds mu(s_l) and lane l ^ 32 mu(M s_l): every lane
// stages its output row in S3, reads its partner's entry P[j] and forms d3[j] = c' (out[j] - partner[P j]), c' = 2 coef / (B A) - the
// derivative for BOTH branches (P is an involution).  The image half adds the loss term, so a pair counts once.  Everything behind d3
// is the text of the PPO kernel.  P comes in the kernel arguments (scalar loads at constant offsets: no vector register holds it).
// RP_SYM 0 expands to the text as it was.
#if RP_SYM
#define RP_TW 32                                           /* samples (pairs) of a wave tile */
#define RP_IN_TILE(l) ((l) & 31)                           /* a lane's sample within the tile */
#define RP_OBS_OF(t) ((t) ? sym.obs_image : a.obs)         /* the rows of column tile t */
#define RP_SYM_PARAMS , const SymArgs sym
#else
#define RP_TW 64
#define RP_IN_TILE(l) (l)
#define RP_OBS_OF(t) a.obs
#define RP_SYM_PARAMS
#endif
#if RP_SYM && RP_NORM
#define RP_KERNEL mlp_sym_norm_kernel
#elif RP_SYM
#define RP_KERNEL mlp_sym_kernel
#elif RP_NORM && RP_DIAG
#define RP_KERNEL mlp_grad_norm_diag_kernel
#elif RP_NORM
#define RP_KERNEL mlp_grad_norm_kernel
#elif RP_DIAG
#define RP_KERNEL mlp_grad_diag_kernel
#else
#define RP_KERNEL mlp_grad_kernel
#endif
#if RP_NORM
#define RP_NORM_PARAMS , const float *__restrict__ norm, float clip
#else
#define RP_NORM_PARAMS
#endif
template <int NET, int KX, int NJ, bool PF>
__global__ void __launch_bounds__(256, 1)
RP_KERNEL(const TrainArgs a RP_NORM_PARAMS RP_SYM_PARAMS) {
    static_assert(!PF || KX == 1, "the prefetching form is the small instance's");
#if RP_DIAG
    static_assert(NET == 0, "the diagnostics are the action net's");
#endif
#if RP_SYM
    static_assert(NET == 0, "the symmetry loss is the action net's");
#endif
    constexpr int OT = (NJ + 31) / 32;                     // 32-row tiles of the outputs
    extern __shared__ float4 lds4[];
    float *lds = reinterpret_cast<float *>(lds4);
    const int obs_dim = a.obs_dim, act_dim = a.act_dim, n_out = NET == 0 ? a.act_dim : 1;
    // LDS holds THIS net's operand blocks only (offsets of the blob rebased), then per-wave scratch
    const Layout G = layout_of(obs_dim, act_dim);
    Layout L = G;
    const int ot_net = NET == 0 ? G.ot_pi : 1;
    int lds_used = 0;
    auto stage = [&](int src, int n_floats) {              // blob block -> LDS at lds_used; all blocks are multiples of 4 floats
        const float4 *s4 = reinterpret_cast<const float4 *>(a.packed + src);
        for (int k = threadIdx.x; k < n_floats / 4; k += blockDim.x) lds4[lds_used / 4 + k] = s4[k];
        const int at = lds_used;
        lds_used += n_floats;
        return at;
    };
    L.o_l1 = stage(G.o_l1 + (NET == 0 ? 0 : HT) * G.k1s * 64, HT * G.k1s * 64) - 0;
    L.o_l2[NET] = stage(G.o_l2[NET], HT * HT * 16 * 64);
    L.o_b2[NET] = stage(G.o_b2[NET], HT * 64);
    L.o_l3[NET] = stage(G.o_l3[NET], ot_net * HT * 16 * 64);
    L.o_b3[NET] = stage(G.o_b3[NET], ot_net * 64);
    L.o_logstd = stage(G.o_logstd, 64);
    L.o_l3t[NET] = stage(G.o_l3t[NET], HT * G.k3s[NET] * 64);
    L.o_l2t[NET] = stage(G.o_l2t[NET], HT * HT * 16 * 64);
    __syncthreads();
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform: the tile arithmetic stays in scalar registers
    const int col = lane & 31, half = lane >> 5;
    constexpr int S3S = NJ + 1;                            // row stride of the delta3 staging (odd)
    // KX == 1: the tile's observations [64 samples][33], staged once - or (PF) two buffers of pf_rows rows of the tile's inputs:
    // rows [0, obs_dim) observation columns, then NET 0: act_dim action columns, advantage, old log-probability; NET 1: old value, return;
#if RP_SYM
    const int pf_rows = obs_dim + 2;                       // the observation columns (rows of obs | of obs_image) and the next tile's row index
#else
    const int pf_rows = obs_dim + (NET == 0 ? act_dim + 2 : 2) + 2;   // (+ 2: the next tile's row index, low and high words)
#endif
    const int XSN = PF ? 2 * pf_rows * PFS : (KX == 1 ? 64 * 33 : 0);
    float *T = lds + lds_used + wave * (32 * 33 + 64 * S3S + XSN);   // transpose scratch, the delta3 staging [64][S3S], observations
    float *S3 = T + 32 * 33;
    float *XS = S3 + 64 * S3S;
    const float onehot = half ? 0.0f : 1.0f;
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long B = a.B, n_tiles = (B + RP_TW - 1) / RP_TW;
    const int mrow = 0;                                     // (the staged layer-1 block holds this net's two row tiles)
    const int k3s = L.k3s[NET];

    // gradient accumulators, alive across the wave's tiles
    f32x16 G1[HT][KX], G2[HT][HT], G3[OT][HT];
    float db2[HT];                                          // bias 2: this lane's unit (col) of tile o, summed over its half's samples
    float db3[NJ], gls[NJ];
    float acc3[HT][16];                                     // value net: per-lane sums of dW3 (see the forward pass)
#pragma unroll
    for (int m = 0; m < HT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc3[m][r] = 0.0f;
    float loss_sum = 0.0f;
#if RP_DIAG
    S3[lane * S3S + NJ] = 0.0f;                             // this lane's sum of 0.5 x^2 / B
    int n_clipped = 0;                                      // wave-uniform: samples of this wave's tiles whose ratio the clamp changed
#endif
#pragma unroll
    for (int o = 0; o < HT; ++o) {
        db2[o] = 0.0f;
#pragma unroll
        for (int k = 0; k < KX; ++k) G1[o][k] = zero;
#pragma unroll
        for (int m = 0; m < HT; ++m) G2[o][m] = zero;
    }
#pragma unroll
    for (int q = 0; q < OT; ++q)
#pragma unroll
        for (int m = 0; m < HT; ++m) G3[q][m] = zero;
#pragma unroll
    for (int j = 0; j < NJ; ++j) { db3[j] = 0.0f; gls[j] = 0.0f; }

    const long tile0 = long(blockIdx.x) * nw + wave, tstep = long(gridDim.x) * nw;
    // (PF) this lane's sample of tile t: position in the minibatch and row in the rollout tensors
    auto pos_of = [&](long t) { const long p = t * RP_TW + RP_IN_TILE(lane); return p < B ? p : B - 1; };
    auto row_of = [&](long t) { const long p = pos_of(t); return a.index ? long(a.index[p]) : p; };
    auto prefetch = [&](long t, long row, int buf) {        // tile t's rows (this lane's sample at `row`) + the sample order of the tile after it
        float *dst = XS + buf * pf_rows * PFS;
        const float *xr = RP_OBS_OF(lane >> 5) + row * obs_dim;
        for (int k = 0; k < obs_dim; ++k) dma_dword(xr + k, dst + k * PFS);
        dst += obs_dim * PFS;
        if (RP_SYM) {
        } else if (NET == 0) {
            const float *ar = a.act + row * act_dim;
            for (int j = 0; j < act_dim; ++j) dma_dword(ar + j, dst + j * PFS);
            dma_dword(a.adv + (a.adv_stats ? row : pos_of(t)), dst + act_dim * PFS);
            dma_dword(a.logp_old + row, dst + (act_dim + 1) * PFS);
            dst += (act_dim + 2) * PFS;
        } else {
            dma_dword(a.val_old + row, dst);
            dma_dword(a.ret + row, dst + PFS);
            dst += 2 * PFS;
        }
        // the next tile's row index travels the same way (two rows: low and high words): an ordinary load in this loop
        // would have the compiler wait - vmcnt(0) - behind the DMAs wherever it moves the loaded register
        if (a.index && t + tstep < n_tiles) {
            const float *ip = reinterpret_cast<const float *>(a.index + pos_of(t + tstep));
            dma_dword(ip, dst);
            dma_dword(ip + 1, dst + PFS);
        }
    };
    // the minibatch's advantage statistics, read once (uniform: scalar registers)
    float adv_mean = 0.0f, adv_istd = 1.0f;
    if (NET == 0 && a.adv_stats) {
        adv_mean = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(a.adv_stats[0])));
        adv_istd = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(a.adv_stats[1])));
    }
    int buf = 0;
    if (PF && tile0 < n_tiles) prefetch(tile0, row_of(tile0), 0);
    const int lane_id = lane;
    for (long tile = tile0; tile < n_tiles; tile += tstep, buf ^= 1) {
        // the lane-derived indices are recomputed per tile from an opaque copy of the lane id: hoisted out of the loop they
        // are a dozen registers the allocator spills, and a scratch reload waits for every DMA issued before it
        int lane = lane_id;
        asm volatile("" : "+v"(lane));
        const int col = lane & 31, half = lane >> 5;
        const float onehot = half ? 0.0f : 1.0f;
        const float *PB = XS + buf * pf_rows * PFS;         // (PF) this tile's inputs
#if RP_NORM
        // the statistics are read per tile through an opaque copy of their address, like the lane id above: hoisted out of the loop
        // the pairs of every column would be registers the allocator spills
        norm_ptr np = norm_of(norm);
        asm volatile("" : "+s"(np));
#endif
        if (PF) {
            wait_dma();                                     // this tile's rows have landed (issued one tile ago)
            if (tile + tstep < n_tiles) {                   // the next tile's go out now and have this tile's arithmetic to arrive
                long row_n = pos_of(tile + tstep);
                if (a.index) {
                    const unsigned lo = __float_as_uint(PB[(pf_rows - 2) * PFS + lane]), hi = __float_as_uint(PB[(pf_rows - 1) * PFS + lane]);
                    row_n = long((static_cast<unsigned long long>(hi) << 32) | lo);
                }
                prefetch(tile + tstep, row_n, buf ^ 1);
            }
        }
        // ================= forward =================
        long s0 = tile * RP_TW + col, s1 = s0 + (RP_SYM ? 0 : 32);     // (RP_SYM: the pair - row s0 of obs and of obs_image)
        s0 = s0 < B ? s0 : B - 1; s1 = s1 < B ? s1 : B - 1;
        if (!PF && a.index) { s0 = a.index[s0]; s1 = a.index[s1]; }
        const float *x0 = a.obs + s0 * obs_dim, *x1 = RP_OBS_OF(1) + s1 * obs_dim;
        if (KX == 1 && !PF) {
            // the tile's observation rows (gathered when indexed) go to LDS once: lane = sample reads its whole row with
            // all loads in flight together; the K loop of layer 1 and the dW1 operands then come from LDS instead of
            // one dependent global load per step (the indexed minibatch cost 10.4 ms against 7.6 contiguous before)
            long sr = tile * RP_TW + RP_IN_TILE(lane);
            sr = sr < B ? sr : B - 1;
            if (a.index) sr = a.index[sr];
            const float *xr = RP_OBS_OF(half) + sr * obs_dim;
#pragma unroll
            for (int k0 = 0; k0 < 32; k0 += 8) {                 // eight loads in flight at a time (registers are scarce here)
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = k0 + k < obs_dim ? xr[k0 + k] : (k0 + k == obs_dim ? 1.0f : 0.0f);
#if RP_NORM
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float mu, rs;
                    norm_at(np, obs_dim, k0 + k, mu, rs);
                    if (k0 + k < obs_dim) v[k] = obs_operand<true>(v[k], mu, rs, clip);
                }
#endif
#pragma unroll
                for (int k = 0; k < 8; ++k) XS[lane * 33 + k0 + k] = v[k];
            }
            wave_fence();
        }
        f32x16 h1[HT][2], h2[HT][2];
#pragma unroll
        for (int m = 0; m < HT; ++m) { h1[m][0] = zero; h1[m][1] = zero; }
        const float *w1 = lds + L.o_l1 + lane;
        for (int s = 0; s < L.k1s; ++s) {
            const int k = 2 * s + half;
            float b0, b1;
            if (PF) {
                const int kk = k < obs_dim ? k : obs_dim - 1;
                const float v0 = pinned(PB[kk * PFS + col]), v1 = pinned(PB[kk * PFS + 32 + col]);
                const float pad = k == obs_dim ? 1.0f : 0.0f;
                b0 = k < obs_dim ? v0 : pad; b1 = k < obs_dim ? v1 : pad;
            } else if (KX == 1) { b0 = XS[col * 33 + k]; b1 = XS[(32 + col) * 33 + k]; }
            else {
                b0 = k < obs_dim ? x0[k] : (k == obs_dim ? 1.0f : 0.0f);
                b1 = k < obs_dim ? x1[k] : (k == obs_dim ? 1.0f : 0.0f);
            }
#if RP_NORM
            if (PF || KX != 1) {                            // (the staged rows are normalised already)
                float mu, rs;
                norm_of_step(np, obs_dim, s, half, mu, rs);
                if (k < obs_dim) { b0 = obs_operand<true>(b0, mu, rs, clip); b1 = obs_operand<true>(b1, mu, rs, clip); }
            }
#endif
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                const float w = w1[((mrow + m) * L.k1s + s) * 64];
                h1[m][0] = mfma(w, b0, h1[m][0]);
                h1[m][1] = mfma(w, b1, h1[m][1]);
            }
        }
#pragma unroll
        for (int m = 0; m < HT; ++m) { tanh_tile(h1[m][0]); tanh_tile(h1[m][1]); }
#pragma unroll
        for (int o = 0; o < HT; ++o) {
            h2[o][0] = zero; h2[o][1] = zero;
            const float *w = lds + L.o_l2[NET] + o * (HT * 16 * 64) + lane;
            mfma_stream<HT * 16>(w, [&](int k) { return h1[k >> 4][0][k & 15]; }, [&](int k) { return h1[k >> 4][1][k & 15]; },
                                 h2[o][0], h2[o][1]);
            const float b = lds[L.o_b2[NET] + o * 64 + lane];
            h2[o][0] = mfma(b, onehot, h2[o][0]);
            h2[o][1] = mfma(b, onehot, h2[o][1]);
            tanh_tile(h2[o][0]); tanh_tile(h2[o][1]);
        }
        float out[NJ];                                      // this lane's sample: output row j
        // The value net has ONE output: as 32-row MFMA tiles its output layer, W3^T delta3 and dW3 would be 31/32
        // padding (134 of the net's 602 MFMAs per tile).  They run on the VALU instead: every lane holds 32 of the 64
        // h2 units of its column's sample, so the output is a 32-term dot product per half-wave plus the other half's.
        float wv[HT][16];                                   // W3[0][unit of (m, r, this half)]
        float bt0 = 0.0f, bt1 = 0.0f;                       // delta3 of this lane's column sample in tile 0 / 1
        if (NET == 1) {
            float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    wv[m][r] = lds[L.o_l3[NET] + (m * 16 + r) * 64 + 32 * half];      // row 0 of the A operand: lane 0 / 32
                    p0 += wv[m][r] * h2[m][0][r];
                    p1 += wv[m][r] * h2[m][1][r];
                }
            half_swap(p0, p1);                               // (tile 0 | tile 1) x (lower | upper units) -> one sample per lane
            out[0] = p0 + p1 + lds[L.o_b3[NET]];
        }
#pragma unroll
        for (int q = 0; q < (NET == 1 ? 0 : OT); ++q) {
            f32x16 y0 = zero, y1 = zero;
            const float *w = lds + L.o_l3[NET] + q * (HT * 16 * 64) + lane;
            mfma_stream<HT * 16>(w, [&](int k) { return h2[k >> 4][0][k & 15]; }, [&](int k) { return h2[k >> 4][1][k & 15]; }, y0, y1);
            const float b = lds[L.o_b3[NET] + q * 64 + lane];
            y0 = mfma(b, onehot, y0);
            y1 = mfma(b, onehot, y1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {                  // one sample per lane: rows 32 q + U(r) and + 4
                float lo = y0[r], hi = y1[r];
                half_swap(lo, hi);
                if (32 * q + unit_of(r) < NJ) out[32 * q + unit_of(r)] = lo;
                if (32 * q + unit_of(r) + 4 < NJ) out[32 * q + unit_of(r) + 4] = hi;
            }
        }
        // ================= loss derivative of this lane's sample =================
        const long i = tile * RP_TW + RP_IN_TILE(lane);
        const bool live = i < B;
        const long im = live ? i : B - 1;                    // position in the minibatch
        const long ii = PF ? im : (a.index ? long(a.index[im]) : im);     // row in the rollout tensors (PF: the inputs are in PB)
        float d3[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) d3[j] = 0.0f;
#if RP_SYM
        {
            // every lane's output row to its S3 row; the partner (the pair's other branch) is lane ^ 32
            (void)ii; (void)adv_mean; (void)adv_istd;        // (the PPO epilogue's)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j < act_dim) S3[lane * S3S + j] = out[j];
            wave_fence();
            float e2 = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j < act_dim) {
                    const float e = out[j] - S3[(lane ^ 32) * S3S + sym.act_src[j]];
                    d3[j] = live ? sym.c2 * e : 0.0f;
                    e2 += e * e;
                }
            if (live && half) loss_sum += sym.lscale * e2;   // the image half alone: each pair once
            wave_fence();                                    // the partner reads above, the delta3 staging below
        }
#else
        if (NET == 0) {
            float lp = -0.91893853320467274f * float(act_dim);
            float z[NJ], iv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                z[j] = 0.0f; iv[j] = 0.0f;
                if (j < act_dim) {
                    const float ls = lds[L.o_logstd + j];
                    iv[j] = __expf(-2.0f * ls);
                    z[j] = (PF ? PB[(obs_dim + j) * PFS + lane] : a.act[ii * act_dim + j]) - out[j];
                    lp -= 0.5f * z[j] * z[j] * iv[j] + ls;
                }
            }
            const float araw = PF ? PB[(obs_dim + act_dim) * PFS + lane] : (a.adv_stats ? a.adv[ii] : a.adv[im]);
            const float A = (araw - adv_mean) * adv_istd;
            const float ratio = __expf(lp - (PF ? PB[(obs_dim + act_dim + 1) * PFS + lane] : a.logp_old[ii]));
            const float rc = __builtin_amdgcn_fmed3f(ratio, 1.0f - a.cliprange, 1.0f + a.cliprange);
            const float t1 = -A * ratio, t2 = -A * rc;
            const float g = live ? (t1 >= t2 ? -A : 0.0f) * ratio * a.inv_B : 0.0f;      // dL / dlogp
            if (live) loss_sum += fmaxf(t1, t2) * a.inv_B;
#if RP_DIAG
            {
                const float x = lp - (PF ? PB[(obs_dim + act_dim + 1) * PFS + lane] : a.logp_old[ii]);
                S3[lane * S3S + NJ] += live ? 0.5f * x * x * a.inv_B : 0.0f;
                n_clipped += __builtin_popcountll(__ballot(live && rc != ratio));
            }
#endif
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j < act_dim) {
                    d3[j] = g * z[j] * iv[j];
                    gls[j] += g * (z[j] * z[j] * iv[j] - 1.0f);
                }
        } else {
            const float v = out[0], vo = PF ? PB[obs_dim * PFS + lane] : a.val_old[ii], R = PF ? PB[(obs_dim + 1) * PFS + lane] : a.ret[ii];
            const float dv = v - vo, vc = vo + __builtin_amdgcn_fmed3f(dv, -a.cliprange, a.cliprange);
            const float e1 = (v - R) * (v - R), e2 = (vc - R) * (vc - R);
            const float dvl = e1 >= e2 ? (v - R) : (fabsf(dv) < a.cliprange ? (vc - R) : 0.0f);
            d3[0] = live ? a.vf_coef * a.inv_B * dvl : 0.0f;
            if (live) loss_sum += 0.5f * fmaxf(e1, e2) * a.inv_B;
        }
#endif
#pragma unroll
        for (int j = 0; j < NJ; ++j) db3[j] += d3[j];
        // delta3 staged [sample][row] for the transposed (row-on-lane) reads of dW3
        if (NET == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j < n_out) S3[lane * S3S + j] = d3[j];
        } else {
            bt0 = d3[0]; bt1 = d3[0];
            half_swap(bt0, bt1);                             // this lane's column sample of tile 0 / tile 1
        }
        // ================= delta2 = (W3^T delta3) (1 - h2^2) =================
        f32x16 d2[HT][2];
#pragma unroll
        for (int m = 0; m < HT; ++m) { d2[m][0] = zero; d2[m][1] = zero; }
        if (NET == 1) {
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    d2[m][0][r] = wv[m][r] * bt0;
                    d2[m][1][r] = wv[m][r] * bt1;
                    acc3[m][r] += bt0 * h2[m][0][r] + bt1 * h2[m][1][r];     // dW3, reduced over the lanes at the end
                }
        }
#pragma unroll
        for (int s = 0; s < (NET == 1 ? 0 : NJ / 2); ++s)
            if (s < k3s) {                                   // K pair = outputs (2 s, 2 s + 1)
                float b0 = d3[2 * s], b1 = d3[2 * s + 1];
                half_swap(b0, b1);                           // b0: column tile 0, b1: column tile 1
#pragma unroll
                for (int m = 0; m < HT; ++m) {
                    const float w = lds[L.o_l3t[NET] + (m * k3s + s) * 64 + lane];
                    d2[m][0] = mfma(w, b0, d2[m][0]);
                    d2[m][1] = mfma(w, b1, d2[m][1]);
                }
            }
#pragma unroll
        for (int m = 0; m < HT; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) d2[m][t][r] *= 1.0f - h2[m][t][r] * h2[m][t][r];
        wave_fence();                                        // S3 written above is read below
        // ================= dW3 += delta3 h2^T, per column tile =================
#pragma unroll
        for (int t = 0; t < (NET == 1 ? 0 : 2); ++t) {
            f32x16 h2T[HT];
#pragma unroll
            for (int m = 0; m < HT; ++m) h2T[m] = transpose_tile(h2[m][t], T, col, half);
#pragma unroll
            for (int q = 0; q < OT; ++q) {
                const int j = 32 * q + col;                  // row on this lane
                const int jj = j < n_out ? j : 0;            // (an unconditional read + select: a guarded read is a branch per element,
                                                             //  32 basic blocks that the MFMAs cannot be scheduled across)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float d3raw = pinned(S3[(32 * t + unit_of(r) + 4 * half) * S3S + jj]);
                    const float d3t = j < n_out ? d3raw : 0.0f;
#pragma unroll
                    for (int m = 0; m < HT; ++m) G3[q][m] = mfma(d3t, h2T[m][r], G3[q][m]);
                }
            }
        }
        // ================= delta1 = (W2^T delta2) (1 - h1^2) =================
        f32x16 d1[HT][2];
#pragma unroll
        for (int ip = 0; ip < HT; ++ip) {
            d1[ip][0] = zero; d1[ip][1] = zero;
            const float *w = lds + L.o_l2t[NET] + ip * (HT * 16 * 64) + lane;
            mfma_stream<HT * 16>(w, [&](int k) { return d2[k >> 4][0][k & 15]; }, [&](int k) { return d2[k >> 4][1][k & 15]; },
                                 d1[ip][0], d1[ip][1]);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) d1[ip][t][r] *= 1.0f - h1[ip][t][r] * h1[ip][t][r];
        }
        // ================= dW2 += delta2 h1^T, db2, dW1 += delta1 [obs | 1]^T =================
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x16 h1T[HT], dT[HT];
#pragma unroll
            for (int m = 0; m < HT; ++m) { h1T[m] = transpose_tile(h1[m][t], T, col, half); dT[m] = transpose_tile(d2[m][t], T, col, half); }
            // bias 2 from the transposed delta2 (units on the lanes, samples in the registers): one accumulator per row tile
            // instead of a 16-register tile of per-sample sums
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                float sum = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += dT[m][r];
                db2[m] += sum;
            }
#pragma unroll
            for (int o = 0; o < HT; ++o)
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) G2[o][m] = mfma(dT[o][r], h1T[m][r], G2[o][m]);
#pragma unroll
            for (int m = 0; m < HT; ++m) dT[m] = transpose_tile(d1[m][t], T, col, half);
#if RP_NORM
            float nmu[KX], nrs[KX];                                              // the pair of this lane's column(s)
            if (PF || KX != 1) {
#pragma unroll
                for (int kx = 0; kx < KX; ++kx) norm_at(np, obs_dim, 32 * kx + col, nmu[kx], nrs[kx]);
            }
#endif
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                long sn = tile * RP_TW + (RP_SYM ? 0 : 32 * t) + unit_of(r) + 4 * half;    // sample of this K slot (RP_SYM: the pair)
                sn = sn < B ? sn : B - 1;
                if (KX != 1 && a.index) sn = a.index[sn];
#pragma unroll
                for (int kx = 0; kx < KX; ++kx) {
                    const int k = 32 * kx + col;
                    float xv;
                    if (PF) {
                        const float v = pinned(PB[(col < obs_dim ? col : obs_dim - 1) * PFS + 32 * t + unit_of(r) + 4 * half]);
                        xv = col < obs_dim ? v : (col == obs_dim ? 1.0f : 0.0f);
                    } else
                        xv = KX == 1 ? XS[(32 * t + unit_of(r) + 4 * half) * 33 + col]
                                     : (k < obs_dim ? RP_OBS_OF(t)[sn * obs_dim + k] : (k == obs_dim ? 1.0f : 0.0f));
#if RP_NORM
                    if ((PF || KX != 1) && k < obs_dim) xv = obs_operand<true>(xv, nmu[kx], nrs[kx], clip);
#endif
#pragma unroll
                    for (int o = 0; o < HT; ++o) G1[o][kx] = mfma(dT[o][r], xv, G1[o][kx]);
                }
            }
        }
    }
    // ================= this wave's partial gradient, torch parameter order =================
    const GOff g = goff_of(obs_dim, n_out);
    float *P = a.partials + (long(blockIdx.x) * nw + wave) * a.gstride;
    for (int k = lane; k < a.gstride; k += 64) P[k] = 0.0f;
    wave_fence();
    __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
    for (int o = 0; o < HT; ++o)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * o + unit_of(r) + 4 * half;              // out unit
#pragma unroll
            for (int m = 0; m < HT; ++m) P[g.w2 + row * H + 32 * m + col] = G2[o][m][r];
#pragma unroll
            for (int kx = 0; kx < KX; ++kx) {
                const int k = 32 * kx + col;
                if (k < obs_dim) P[g.w1 + row * obs_dim + k] = G1[o][kx][r];
                else if (k == obs_dim) P[g.b1 + row] = G1[o][kx][r];
            }
        }
#pragma unroll
    for (int o = 0; o < HT; ++o) {                                       // bias 2: unit 32 o + col, the two halves' samples
        const float v = db2[o] + __shfl_xor(db2[o], 32, 64);
        if (half == 0) P[g.b2 + 32 * o + col] = v;
    }
    if (NET == 1) {
#pragma unroll
        for (int m = 0; m < HT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc3[m][r];                                    // sum over the 32 samples-lanes of the half-wave
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                if (col == 0) P[g.w3 + 32 * m + unit_of(r) + 4 * half] = v;
            }
    }
#pragma unroll
    for (int q = 0; q < (NET == 1 ? 0 : OT); ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * q + unit_of(r) + 4 * half;              // output
            if (row < n_out) {
#pragma unroll
                for (int m = 0; m < HT; ++m) P[g.w3 + row * H + 32 * m + col] = G3[q][m][r];
            }
        }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (j < n_out) {
            float v = db3[j], w = gls[j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { v += __shfl_xor(v, off, 64); w += __shfl_xor(w, off, 64); }
            if (lane == 0) { P[g.b3 + j] = v; P[g.ls + j] = NET == 0 ? w : 0.0f; }
        }
    float ls = loss_sum;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ls += __shfl_xor(ls, off, 64);
    if (lane == 0) P[g.loss + (RP_SYM ? RP_SYM_LOSS_SLOT : 0)] = ls;
#if RP_DIAG
    float kl = S3[lane * S3S + NJ];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kl += __shfl_xor(kl, off, 64);
    if (lane == 0) { P[g.loss + 1] = kl; P[g.loss + 2] = float(n_clipped) * a.inv_B; }
#endif
    // the workgroup's waves fold their partials into wave 0's (fixed order: bit-reproducible), so the reduction
    // kernel reads one partial per workgroup instead of one per wave
    __syncthreads();
    float *P0 = a.partials + long(blockIdx.x) * nw * a.gstride;
    for (int k = threadIdx.x; k < a.gstride; k += blockDim.x) {
        float v = P0[k];
        for (int w = 1; w < nw; ++w) v += P0[w * a.gstride + k];
        P0[k] = v;
    }
}
#undef RP_KERNEL
#undef RP_NORM_PARAMS
#undef RP_SYM_PARAMS
#undef RP_OBS_OF
#undef RP_TW
#undef RP_IN_TILE
#undef RP_NORM
#undef RP_DIAG
#undef RP_SYM
