/*
 * fmgi_sparse.hip -- the sparse, blocked form of a per-state photon histogram.
 *   blob = uint64 off[B + 1], uint64 entry[64 * rows];  B = blocks of 64 consecutive texels
 *   slot j of texel 64 b + l = entry[(off[b] + j) * 64 + l] = state << 54 | count, a texel's non-zero states in
 *   ascending order, then zeros up to the block's row count r_b = off[b + 1] - off[b]
 * Every kernel gives one wave (a workgroup of 64 lanes) to a block and one lane to a texel, so a row of the dense
 * histogram and a row of the blob are both one coalesced 512-B access, a lane owns its texel (no atomics on
 * counts or lightmaps) and blocks of very different row counts are handed out by the dispatcher one by one.
 *   count   1024 dense rows, kDenseUnroll in flight: per-lane non-zeros, wave max -> r_b, wave sums -> the info
 *   scan    one workgroup: off[1..B] row counts -> inclusive prefix sums in place, any B
 *   fill    the count loop again, every lane storing its packed cells at its own slot counter, then zeros
 *   expand  rows in order, one load-add-store per lane and entry
 *   recolour_sparse<K>  rows in order; each lane gathers the table row of its own state from global memory (the
 *           table is 12 KB x K and stays in the caches: nothing is staged in LDS, so occupancy is not bound by
 *           it), lo32(count) * value as one 32 x 32 -> 64 multiply-add and the high half as in k_recolour
 * Every kernel that reads a blob clamps the block's [off[b], off[b + 1]) to [0, rows] (rows comes from the
 * host) and skips a block whose begin exceeds its end; the state field has 10 bits: a blob of
 * fmgi_sparse_bytes(T, rows) bytes cannot cause an access outside itself, the table or the histogram.
 */
#include <hip/hip_runtime.h>

#include "fmgi_sparse.h"

namespace {

typedef unsigned long long u64;

constexpr int kDenseUnroll = 8; /* dense state rows in flight per wave (divides 1024) */
constexpr int kRowUnroll = 4;   /* blob rows in flight per wave */
constexpr int kScanThreads = 256;

__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ inline uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline u64 min64(u64 a, u64 b) { return a < b ? a : b; }

__global__ __launch_bounds__(64) void k_sparse_count(const u64 *__restrict__ counts, int num_texels,
                                                     u64 *__restrict__ off, SparseSums *__restrict__ sums) {
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const bool live = t < num_texels;
    const size_t T = (size_t)num_texels;
    const u64 *p = counts + (live ? (size_t)t : 0);
    uint32_t n = 0, big = 0;
    u64 dep = 0;
    for (int s = 0; s < kRecolourStates; s += kDenseUnroll, p += kDenseUnroll * T) {
        u64 c[kDenseUnroll];
#pragma unroll
        for (int u = 0; u < kDenseUnroll; u++) c[u] = live ? p[(size_t)u * T] : 0ull;
#pragma unroll
        for (int u = 0; u < kDenseUnroll; u++) {
            n += c[u] != 0;
            big += c[u] > kSparseCountMask;
            dep += c[u];
        }
    }
    const uint32_t r = wave_max(n);
    const u64 cells = wave_sum(n), deposits = wave_sum(dep), too_large = wave_sum(big);
    if (lane != 0) return;
    if (off) off[(size_t)blockIdx.x + 1] = r;
    if (!sums) return;
    if (r) atomicAdd(&sums->rows, (u64)r);
    if (cells) atomicAdd(&sums->cells, cells);
    if (deposits) atomicAdd(&sums->deposits, deposits);
    if (too_large) atomicAdd(&sums->too_large, too_large);
}

/* one workgroup walks off[1 .. blocks] in tiles of kScanThreads, carrying the running sum: exact for any count */
__global__ __launch_bounds__(kScanThreads) void k_sparse_scan(u64 *off, int blocks, u64 rows) {
    __shared__ u64 wsum[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) off[0] = 0;
    u64 carry = 0;
    for (int64_t base = 0; base < blocks; base += kScanThreads) {
        const int64_t i = base + tid;
        u64 x = i < blocks ? off[i + 1] : 0ull;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        u64 before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; w++) {
            const u64 ws = wsum[w];
            if (w < wave) before += ws;
            total += ws;
        }
        if (i < blocks) off[i + 1] = min64(carry + before + x, rows);
        carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_sparse_fill(const u64 *__restrict__ counts, int num_texels, u64 *blob,
                                                    u64 rows) {
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const bool live = t < num_texels;
    const size_t T = (size_t)num_texels;
    const u64 begin = min64(blob[blockIdx.x], rows), end = min64(blob[(size_t)blockIdx.x + 1], rows);
    if (begin >= end) return; /* no rows (or offsets that do not belong to this histogram) */
    const u64 r = end - begin;
    u64 *e = blob + (size_t)gridDim.x + 1 + (size_t)begin * 64 + lane; /* this lane's slot 0; slot j < r only */
    const u64 *p = counts + (live ? (size_t)t : 0);
    u64 j = 0;
    for (int s = 0; s < kRecolourStates; s += kDenseUnroll, p += kDenseUnroll * T) {
        u64 c[kDenseUnroll];
#pragma unroll
        for (int u = 0; u < kDenseUnroll; u++) c[u] = live ? p[(size_t)u * T] : 0ull;
#pragma unroll
        for (int u = 0; u < kDenseUnroll; u++) {
            if (c[u] != 0 && j < r) {
                e[(size_t)j * 64] = ((u64)(s + u) << kSparseCountBits) | (c[u] & kSparseCountMask);
                j++;
            }
        }
    }
    for (; j < r; j++) e[(size_t)j * 64] = 0; /* padding: the whole blob is written */
}

__global__ __launch_bounds__(64) void k_sparse_expand(const u64 *__restrict__ blob, int num_texels, u64 rows,
                                                      u64 *__restrict__ counts) {
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const bool live = t < num_texels;
    const size_t T = (size_t)num_texels;
    const u64 begin = min64(blob[blockIdx.x], rows), end = min64(blob[(size_t)blockIdx.x + 1], rows);
    if (begin >= end) return;
    const u64 *e = blob + (size_t)gridDim.x + 1 + lane;
    for (u64 j = begin; j < end; j += kRowUnroll) {
        u64 v[kRowUnroll];
#pragma unroll
        for (int u = 0; u < kRowUnroll; u++) v[u] = j + u < end ? e[(size_t)(j + u) * 64] : 0ull;
#pragma unroll
        for (int u = 0; u < kRowUnroll; u++) { /* in order: a duplicate state of a lane adds twice */
            if (v[u] == 0 || !live) continue;
            u64 *q = counts + (size_t)(v[u] >> kSparseCountBits) * T + (size_t)t;
            *q += v[u] & kSparseCountMask;
        }
    }
}

template <int K>
__global__ __launch_bounds__(64) void k_recolour_sparse(SparseRecolourArgs a) {
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const u64 begin = min64(a.blob[blockIdx.x], a.rows), end = min64(a.blob[(size_t)blockIdx.x + 1], a.rows);
    if (begin >= end) return;
    const u64 *e = a.blob + (size_t)gridDim.x + 1 + lane;
    const uint32_t *__restrict__ table = a.table;
    u64 acc[K][3];
#pragma unroll
    for (int k = 0; k < K; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0;
    for (u64 j = begin; j < end; j += kRowUnroll) {
        u64 v[kRowUnroll];
#pragma unroll
        for (int u = 0; u < kRowUnroll; u++) v[u] = j + u < end ? e[(size_t)(j + u) * 64] : 0ull;
#pragma unroll
        for (int u = 0; u < kRowUnroll; u++) {
            if (__ballot(v[u] != 0) == 0) continue; /* a row past the end */
            /* padding (0) reads table row 0 with a count of 0; the state has 10 bits: always inside the table */
            const uint32_t *row = table + (size_t)(v[u] >> kSparseCountBits) * (K * 3);
            const uint32_t lo = (uint32_t)v[u], hi = (uint32_t)((v[u] & kSparseCountMask) >> 32);
            uint32_t val[K * 3];
#pragma unroll
            for (int i = 0; i < K * 3; i++) val[i] = row[i];
#pragma unroll
            for (int k = 0; k < K; k++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) acc[k][ch] += (u64)lo * val[3 * k + ch];
            if (__ballot(hi != 0) != 0) { /* a count of 2^32 or more */
#pragma unroll
                for (int k = 0; k < K; k++)
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) acc[k][ch] += (u64)(hi * val[3 * k + ch]) << 32;
            }
        }
    }
    if (t >= a.num_texels) return;
#pragma unroll
    for (int k = 0; k < K; k++) {
        u64 *q = a.lm[k] + 4 * (size_t)t;
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            if (acc[k][ch]) q[ch] += acc[k][ch]; /* this wave owns the texel: groups are launches of one stream */
    }
}

template <int K>
void launch(const SparseRecolourArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_recolour_sparse<K>, dim3((unsigned)fmgi_sparse_blocks(a.num_texels)), dim3(64), 0, s, a);
}

} // namespace

hipError_t fmgi_launch_sparse_count(const unsigned long long *counts, int num_texels, unsigned long long *off,
                                    SparseSums *sums, hipStream_t s) {
    if (num_texels <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sparse_count, dim3((unsigned)fmgi_sparse_blocks(num_texels)), dim3(64), 0, s, counts,
                       num_texels, off, sums);
    return hipGetLastError();
}

hipError_t fmgi_launch_sparse_scan(unsigned long long *off, int blocks, unsigned long long rows, hipStream_t s) {
    if (blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sparse_scan, dim3(1), dim3(kScanThreads), 0, s, off, blocks, rows);
    return hipGetLastError();
}

hipError_t fmgi_launch_sparse_fill(const unsigned long long *counts, int num_texels, unsigned long long *blob,
                                   unsigned long long rows, hipStream_t s) {
    if (num_texels <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sparse_fill, dim3((unsigned)fmgi_sparse_blocks(num_texels)), dim3(64), 0, s, counts,
                       num_texels, blob, rows);
    return hipGetLastError();
}

hipError_t fmgi_launch_sparse_expand(const unsigned long long *blob, int num_texels, unsigned long long rows,
                                     unsigned long long *counts, hipStream_t s) {
    if (num_texels <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sparse_expand, dim3((unsigned)fmgi_sparse_blocks(num_texels)), dim3(64), 0, s, blob,
                       num_texels, rows, counts);
    return hipGetLastError();
}

hipError_t fmgi_launch_recolour_sparse(const SparseRecolourArgs &a, hipStream_t s) {
    if (a.num_texels <= 0) return hipSuccess;
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
