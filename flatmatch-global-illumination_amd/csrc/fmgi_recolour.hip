/*
 * fmgi_recolour.hip -- a bake's per-state photon histogram folded with the colour tables of up to
 * kRecolourMaxK lighting scenarios at once:
 *   lm[k][t][c] += sum_s counts[s][t] * table[s][k][c]          (exact, mod 2^64)
 * a skinny integer matrix product bound by reading counts (8 KiB per texel). Lanes run over consecutive
 * texels, so every state row is read with one coalesced 512-B load per wave; the state index is uniform in a
 * wave, so the table row comes through scalar loads. A workgroup owns 64 texels and one slab of the states
 * (blockIdx.y); its four waves take a quarter of the slab each, keep 3 x K int64 sums per lane in registers,
 * add them up through LDS, and wave 0 adds the non-zero sums to the lightmaps with 64-bit integer atomics
 * (other slabs add to the same texels; integer sums are order-free). A state whose 64 counts are all zero is
 * skipped (most are: a bake reaches a few hundred of the 1024 states).
 * counts are u64 and table values < 2^30: lo32(count) * value is one 32 x 32 -> 64 multiply-add; the high half
 * of a count >= 2^32 contributes (hi32(count) * value mod 2^32) << 32, taken only by waves that hold one.
 */
#include <hip/hip_runtime.h>

#include "fmgi_recolour.h"

namespace {

constexpr int kUnroll = 4; /* state rows in flight per wave; divides every wave's slice (>= 4 states) */

template <int K>
__global__ __launch_bounds__(64 * kRecolourWaves) void k_recolour(RecolourArgs a) {
    __shared__ unsigned long long red[(kRecolourWaves - 1) * K * 3 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const bool live = t < a.num_texels;
    const size_t T = (size_t)a.num_texels;
    const int per = kRecolourStates / (a.slabs * kRecolourWaves); /* states of this wave: 4 .. 256 */
    const int s0 = ((int)blockIdx.y * kRecolourWaves + wave) * per;
    unsigned long long acc[K][3];
#pragma unroll
    for (int k = 0; k < K; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0;
    const unsigned long long *p = a.counts + (size_t)s0 * T + (size_t)t;
    for (int s = s0; s < s0 + per; s += kUnroll, p += kUnroll * T) {
        unsigned long long c[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) c[u] = live ? p[(size_t)u * T] : 0ull;
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            if (__ballot(c[u] != 0) == 0) continue; /* no lane of the wave deposited in this state */
            const uint32_t *row = a.table + (size_t)(s + u) * (K * 3);
            const uint32_t lo = (uint32_t)c[u], hi = (uint32_t)(c[u] >> 32);
#pragma unroll
            for (int k = 0; k < K; k++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) acc[k][ch] += (unsigned long long)lo * row[3 * k + ch];
            if (__ballot(hi != 0) != 0) { /* a count of 2^32 or more */
#pragma unroll
                for (int k = 0; k < K; k++)
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) acc[k][ch] += (unsigned long long)(hi * row[3 * k + ch]) << 32;
            }
        }
    }
    if (wave != 0) {
#pragma unroll
        for (int j = 0; j < K * 3; j++) red[((wave - 1) * K * 3 + j) * 64 + lane] = acc[j / 3][j % 3];
    }
    __syncthreads();
    if (wave != 0 || !live) return;
#pragma unroll
    for (int k = 0; k < K; k++) {
        unsigned long long *q = a.lm[k] + 4 * (size_t)t;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            unsigned long long v = acc[k][ch];
#pragma unroll
            for (int w = 0; w < kRecolourWaves - 1; w++) v += red[((w * K + k) * 3 + ch) * 64 + lane];
            if (v) atomicAdd(q + ch, v);
        }
    }
}

template <int K>
void launch(const RecolourArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)a.num_texels + 63) / 64), (unsigned)a.slabs);
    hipLaunchKernelGGL(k_recolour<K>, grid, dim3(64 * kRecolourWaves), 0, s, a);
}

} // namespace

/* enough state slabs that the launch has about eight waves per SIMD-pair of the chip (8 per CU), so a small
   lightmap still reads its histogram on every CU: 2,152 texels = 34 workgroups per slab -> 16 slabs */
int fmgi_recolour_slabs(int num_texels, int num_cus) {
    const int64_t groups = ((int64_t)num_texels + 63) / 64;
    const int64_t want = (int64_t)(num_cus > 0 ? num_cus : 256) * 2; /* workgroups of 4 waves */
    int slabs = 1;
    while (slabs < 64 && groups * slabs < want) slabs *= 2;
    return slabs;
}

hipError_t fmgi_launch_recolour(const RecolourArgs &a, hipStream_t s) {
    if (a.num_texels <= 0) return hipSuccess;
    if (a.slabs < 1 || a.slabs > 64 || (a.slabs & (a.slabs - 1)) != 0) return hipErrorInvalidValue;
    switch (a.k) {
    case 1: launch<1>(a, s); break;
    case 2: launch<2>(a, s); break;
    case 3: launch<3>(a, s); break;
    case 4: launch<4>(a, s); break;
    case 5: launch<5>(a, s); break;
    case 6: launch<6>(a, s); break;
    case 7: launch<7>(a, s); break;
    case 8: launch<8>(a, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
