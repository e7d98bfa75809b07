// mlp_symmetry.hip - the streaming pass of PPO's mirror-symmetry augmentation (gym_roboy_amd/ppo.py: PPO.augment; DESIGN.md §25;
// include/roboy_policy.h: rp_mirror_rows_dev).  For rows of `width` floats it writes
//     mirror[r][c] = col_sign[c] * src[r][col_src[c]]          (one IEEE multiply: a flipped 0 is -0)
//     plain[r][c]  = src[r][c]                                 (where a plain output is given)
// which is gym_roboy_amd/envs/symmetry.py's mirror_rows(), the statement the kernel is tested against bit for bit.  The two outputs
// are the halves of the [2 n, width] tensors the unchanged gradient kernels then read, so the mirrored half starts wherever n * width
// floats end: 4-byte aligned and no more in general.
//
// A 256-thread workgroup takes a contiguous run of whole rows (at most TILE floats, a multiple of four rows so that every run
// starts on the alignment of the tensor it belongs to), loads it coalesced into LDS - float4 from the first 16-byte boundary of the
// run on, single floats in front of and behind that - and writes each output as one contiguous run in the same way, the boundary
// taken from THAT output's address.  The column map and the signs sit in LDS (read once per workgroup); the column permutation is an
// LDS read at [row * width + col_src[col]], never a global gather.  Row and column of a run's element come from a multiply-high with
// a host-computed reciprocal, once per four elements.  No scratch, no spills: 17 KB of LDS, 64 VGPRs.
#include <hip/hip_runtime.h>

#include "../../include/roboy_policy.h"
#include "mlp_common.hpp"

namespace {
using namespace rpd;

constexpr int MIRROR_TILE = 4096;        // floats of one workgroup's run (16 KB of LDS)
constexpr int MIRROR_MAX_WIDTH = 128;

// rows of one run: whole rows, a multiple of four (every run then starts 16-byte aligned relative to the tensor's base)
inline int mirror_rows_per_block(int width) { return (MIRROR_TILE / width) & ~3; }

// floats in front of the first 16-byte boundary at or behind p, at most cnt
__device__ __forceinline__ int head_floats(const float *p, int cnt) {
    const int h = int(((16u - unsigned(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
    return h < cnt ? h : cnt;
}

__global__ void __launch_bounds__(256)
mirror_rows_kernel(const float *__restrict__ src, float *__restrict__ plain, float *__restrict__ mirror, long long rows, int width,
                   int rows_per_block, unsigned int width_rcp, const int *__restrict__ col_src, const float *__restrict__ col_sign) {
    __shared__ __attribute__((aligned(16))) float tile[MIRROR_TILE];
    __shared__ int s_src[MIRROR_MAX_WIDTH];
    __shared__ float s_sign[MIRROR_MAX_WIDTH];
    const int t = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    const long long left = rows - row0;
    const int cnt = int(left < rows_per_block ? left : rows_per_block) * width;      // floats of this run, <= MIRROR_TILE
    const long long base = row0 * width;
    if (t < width) {
        // (a map entry outside the row would read LDS outside the run: held inside it, whatever the caller handed in)
        const unsigned int c = (unsigned int)col_src[t];
        s_src[t] = int(c < (unsigned int)width ? c : (unsigned int)(width - 1));
        s_sign[t] = col_sign[t];
    }
    {   // the run into LDS
        const float *p = src + base;
        const int head = head_floats(p, cnt), quads = (cnt - head) >> 2, tail = head + 4 * quads;
        if (t < head) tile[t] = p[t];
        if (head == 0) {                   // the run starts on a 16-byte boundary (the usual case): 16-byte LDS stores, no bank conflict
            for (int i = t; i < quads; i += 256)
                *reinterpret_cast<float4 *>(tile + 4 * i) = *reinterpret_cast<const float4 *>(p + 4 * i);
        } else {
            for (int i = t; i < quads; i += 256) {
                const float4 v = *reinterpret_cast<const float4 *>(p + head + 4 * i);
                float *d = tile + head + 4 * i;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
        if (t < cnt - tail) tile[tail + t] = p[tail + t];
    }
    __syncthreads();
    if (plain) {
        float *p = plain + base;
        const int head = head_floats(p, cnt), quads = (cnt - head) >> 2, tail = head + 4 * quads;
        if (t < head) p[t] = tile[t];
        if (head == 0) {
            for (int i = t; i < quads; i += 256)
                *reinterpret_cast<float4 *>(p + 4 * i) = *reinterpret_cast<const float4 *>(tile + 4 * i);
        } else {
            for (int i = t; i < quads; i += 256) {
                const float *s = tile + head + 4 * i;
                *reinterpret_cast<float4 *>(p + head + 4 * i) = make_float4(s[0], s[1], s[2], s[3]);
            }
        }
        if (t < cnt - tail) p[tail + t] = tile[tail + t];
    }
    {
        float *p = mirror + base;
        // element e of the run: row e / width (width_rcp = floor(2^32 / width) + 1: exact for e * width < 2^32), column the rest
        auto at = [&](int r_off, int c) { return __fmul_rn(s_sign[c], tile[r_off + s_src[c]]); };
        auto split = [&](int e, int &r_off, int &c) {
            const int r = width == 1 ? e : int(__umulhi((unsigned int)e, width_rcp));
            r_off = r * width; c = e - r_off;
        };
        const int head = head_floats(p, cnt), quads = (cnt - head) >> 2, tail = head + 4 * quads;
        if (t < head) { int ro, c; split(t, ro, c); p[t] = at(ro, c); }
        for (int i = t; i < quads; i += 256) {
            const int e = head + 4 * i;
            int ro, c;
            split(e, ro, c);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = at(ro, c);
                if (++c == width) { c = 0; ro += width; }
            }
            *reinterpret_cast<float4 *>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
        }
        if (t < cnt - tail) { int ro, c; split(tail + t, ro, c); p[tail + t] = at(ro, c); }
    }
}

}  // namespace

extern "C" {

int rp_mirror_rows_dev(const float *d_src, float *d_plain, float *d_mirror, int64_t rows, int width, const int32_t *d_col_src,
                       const float *d_col_sign, void *stream) {
    if (!d_src || !d_mirror || !d_col_src || !d_col_sign) return fail(RP_EINVAL, "null argument");
    if (width < 1 || width > MIRROR_MAX_WIDTH) return fail(RP_EINVAL, "need 1 <= width <= 128");
    if (rows < 0) return fail(RP_EINVAL, "rows must be >= 0");
    if (rows == 0) return RP_OK;
    {   // the three arrays of rows x width floats may not overlap - every workgroup reads its run of the source while others write
        // theirs - except that the plain output may BE the source
        const uintptr_t bytes = uintptr_t(rows) * uintptr_t(width) * sizeof(float);
        auto overlap = [bytes](const void *a, const void *b) {
            const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
            return x < y + bytes && y < x + bytes;
        };
        if (overlap(d_mirror, d_src)) return fail(RP_EINVAL, "the mirrored rows overlap their source");
        if (d_plain && d_plain != d_src && overlap(d_plain, d_src)) return fail(RP_EINVAL, "the plain rows overlap their source without being it");
        if (d_plain && overlap(d_plain, d_mirror)) return fail(RP_EINVAL, "the plain and the mirrored rows overlap");
    }
    const int rpb = mirror_rows_per_block(width);
    const int64_t blocks = (rows + rpb - 1) / rpb;
    if (blocks > 0x7FFFFFFFll) return fail(RP_EINVAL, "too many rows for one launch");
    DeviceScope scope(d_src); if (scope.rc) return scope.rc;
    const unsigned int rcp = width == 1 ? 0u : (unsigned int)((1ull << 32) / (unsigned long long)width) + 1u;
    hipLaunchKernelGGL(mirror_rows_kernel, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), d_src,
                       d_plain == d_src ? nullptr : d_plain, d_mirror, (long long)rows, width, rpb, rcp, d_col_src, d_col_sign);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RP_EHIP, std::string("mirror_rows_kernel: ") + hipGetErrorString(e));
    return RP_OK;
}

}  // extern "C"
