/*
 * fmgi_hist.hip -- the sparse photon histogram of a set of deposit codes (texel << 10 | colour state), and the
 * sum of two sparse histograms. Nothing here is proportional to 1024 x texels.
 *
 *   bins     every code counted per half-block (32 texels, code >> 15) in a workgroup's LDS histogram, the
 *            touched range added to the global counts: the host then knows every half-block's codes exactly
 *   scatter  the codes of a batch of half-blocks moved to a scratch, each half-block's contiguous: a workgroup
 *            ranks its 4096 codes per half-block in LDS, reserves each half-block's run with one global atomic
 *            and stores the codes there (the order inside a half-block does not matter to a count); it walks
 *            only the pool blocks of the batch's tiles, through the bake's block list
 *   count    one workgroup per half-block: one non-returning LDS add per code into u32 [1024][32] (128 KB), then
 *            every texel's non-zero states -> nz[]. A half-block of 2^32 codes or more never gets here (the
 *            host sends its chunk to the dense route), so no counter can wrap
 *   rows     one wave per block: r_b = the largest nz of its 64 texels, and the sums
 *   fill     the count again, then every slot of the block's rows: a texel's cells in ascending state order
 *            from its 32 state groups' prefix sums, zeros after them
 *   add      one wave per block, one lane per texel: a two-pointer merge of two ascending lists (count, fill)
 * The codes come from the bake's bucket pool (blocks of 1024 codes, tile and length per block, codes of
 * 0xFFFFFFFF and codes at or past the length skipped, as k_bucket_fold) or from a plain array. A code whose
 * texel is >= num_texels is never counted, so every index derived from a code stays inside its table; every
 * offset read from memory is clamped to the size the host allocated.
 */
#include <hip/hip_runtime.h>

#include "fmgi_hist.h"
#include "fmgi_lds_attr.h"

namespace {

typedef unsigned long long u64;

constexpr uint32_t kPad = 0xFFFFFFFFu;
constexpr int kBinThreads = 256;
constexpr int kBinSegs = 4;                                             /* segments per binning workgroup */
constexpr int kBinPerSeg = kHistSegCodes / kBinThreads;                 /* codes per lane and segment */
constexpr int kBinPer = kBinSegs * kBinPerSeg;                          /* codes per lane */
constexpr int kCountThreads = 1024;
constexpr int kStates = 1024;
constexpr int kGroups = kCountThreads / kHistHalfTexels;                /* state groups of a texel: 32 */
constexpr int kGroupStates = kStates / kGroups;                         /* states per group: 32 */
constexpr size_t kCountLds = (size_t)kStates * kHistHalfTexels * sizeof(uint32_t);

__device__ inline u64 wsum(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ inline uint32_t wmax(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}
__device__ inline uint32_t wmin(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline u64 min64(u64 a, u64 b) { return a < b ? a : b; }

/* code k (< kBinPer) of this lane, or kPad: a pad, a code past its block's length, or a texel outside the
   lightmap (counted in oob) */
__device__ inline uint32_t load_code(const HistSource &src, int k, uint32_t &oob) {
    const u64 seg = (u64)blockIdx.x * kBinSegs + (u64)(k / kBinPerSeg);
    if (seg >= src.nseg) return kPad;
    const uint32_t o = (uint32_t)(k % kBinPerSeg) * kBinThreads + threadIdx.x;
    uint32_t len;
    u64 first;
    if (src.block_len) {
        const u64 blk = src.list ? (u64)src.list[src.list_lo + seg] : seg;
        if (blk >= src.pool_blocks) return kPad;
        const uint32_t l = src.block_len[blk];
        len = l < (uint32_t)kHistSegCodes ? l : (uint32_t)kHistSegCodes;
        first = blk * kHistSegCodes;
    } else {
        first = seg * kHistSegCodes;
        if (first >= src.n) return kPad;
        len = (uint32_t)min64(src.n - first, (u64)kHistSegCodes);
    }
    if (o >= len) return kPad;
    const uint32_t c = src.codes[first + o];
    if (c == kPad) return kPad;
    if ((c >> 10) >= (uint32_t)src.num_texels) {
        oob++;
        return kPad;
    }
    return c;
}

__global__ __launch_bounds__(kBinThreads) void k_hist_bins(HistSource src, uint32_t halves, u64 *__restrict__ half_count,
                                                           u64 *__restrict__ skipped) {
    __shared__ uint32_t h[kHistMaxHalves];
    __shared__ uint32_t range[2];
    for (uint32_t i = threadIdx.x; i < halves; i += kBinThreads) h[i] = 0;
    if (threadIdx.x == 0) range[0] = kPad, range[1] = 0;
    __syncthreads();
    uint32_t c[kBinPer], oob = 0, lo = kPad, hi = 0;
#pragma unroll
    for (int k = 0; k < kBinPer; k++) c[k] = load_code(src, k, oob);
#pragma unroll
    for (int k = 0; k < kBinPer; k++) {
        if (c[k] == kPad) continue;
        const uint32_t b = c[k] >> kHistHalfShift;
        if (b >= halves) continue; /* (texel < num_texels <= 32 halves: never) */
        atomicAdd(&h[b], 1u);
        lo = b < lo ? b : lo;
        hi = b > hi ? b : hi;
    }
    lo = wmin(lo), hi = wmax(hi);
    const u64 out = wsum(oob);
    if ((threadIdx.x & 63) == 0) {
        if (lo <= hi) atomicMin(&range[0], lo), atomicMax(&range[1], hi);
        if (out && skipped) atomicAdd(skipped, out);
    }
    __syncthreads();
    const uint32_t r0 = range[0], r1 = range[1];
    if (r0 > r1) return; /* no code */
    for (uint32_t i = r0 + threadIdx.x; i <= r1; i += kBinThreads)
        if (h[i]) atomicAdd(&half_count[i], (u64)h[i]);
}

__global__ __launch_bounds__(kBinThreads) void k_hist_scatter(HistSource src, uint32_t half_lo, uint32_t half_hi,
                                                              uint32_t *__restrict__ cursor, uint32_t *__restrict__ scratch,
                                                              uint32_t scratch_cap) {
    __shared__ uint32_t h[kHistMaxHalves];
    __shared__ uint32_t range[2];
    const uint32_t nb = half_hi - half_lo; /* <= kHistMaxHalves (host) */
    for (uint32_t i = threadIdx.x; i < nb; i += kBinThreads) h[i] = 0;
    if (threadIdx.x == 0) range[0] = kPad, range[1] = 0;
    __syncthreads();
    uint32_t c[kBinPer], rank[kBinPer], oob = 0, lo = kPad, hi = 0;
#pragma unroll
    for (int k = 0; k < kBinPer; k++) c[k] = load_code(src, k, oob);
#pragma unroll
    for (int k = 0; k < kBinPer; k++) {
        rank[k] = 0;
        if (c[k] == kPad) continue;
        const uint32_t b = c[k] >> kHistHalfShift;
        if (b < half_lo || b >= half_hi) { /* another batch's */
            c[k] = kPad;
            continue;
        }
        rank[k] = atomicAdd(&h[b - half_lo], 1u);
        lo = b - half_lo < lo ? b - half_lo : lo;
        hi = b - half_lo > hi ? b - half_lo : hi;
    }
    lo = wmin(lo), hi = wmax(hi);
    if ((threadIdx.x & 63) == 0 && lo <= hi) atomicMin(&range[0], lo), atomicMax(&range[1], hi);
    __syncthreads();
    const uint32_t r0 = range[0], r1 = range[1];
    if (r0 > r1) return; /* uniform: no code of this batch */
    for (uint32_t i = r0 + threadIdx.x; i <= r1; i += kBinThreads)
        if (h[i]) h[i] = atomicAdd(&cursor[i], h[i]); /* the run's first index */
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBinPer; k++) {
        if (c[k] == kPad) continue;
        const u64 pos = (u64)h[(c[k] >> kHistHalfShift) - half_lo] + rank[k];
        if (pos < scratch_cap) scratch[pos] = c[k];
    }
}

/* FILL = false: nz[]; FILL = true: the rows of the half-block's lanes in its block's piece */
template <bool FILL>
__global__ __launch_bounds__(kCountThreads) void k_hist_count(const uint32_t *__restrict__ scratch,
                                                              const uint32_t *__restrict__ start, uint32_t scratch_cap,
                                                              uint32_t half_lo, uint32_t *__restrict__ nz,
                                                              const u64 *__restrict__ off, u64 piece_rows,
                                                              u64 *__restrict__ piece) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cnt[]; /* [state][texel of the half-block] */
    __shared__ uint32_t part[kGroups][kHistHalfTexels];
    const uint32_t half = half_lo + blockIdx.x;
    const uint32_t a0 = start[blockIdx.x], a1 = start[blockIdx.x + 1];
    const uint32_t s1 = a1 < scratch_cap ? a1 : scratch_cap, s0 = a0 < s1 ? a0 : s1;
    u64 begin = 0, r = 0;
    if (FILL) {
        const uint32_t b = (half >> 1) - (half_lo >> 1);
        begin = min64(off[b], piece_rows);
        const u64 end = min64(off[b + 1], piece_rows);
        if (begin >= end) return; /* uniform: the block has no rows */
        r = end - begin;
    } else if (s0 == s1) {
        return; /* uniform: nz[] was zeroed */
    }
    for (int i = threadIdx.x; i < kStates * kHistHalfTexels; i += kCountThreads) cnt[i] = 0;
    __syncthreads();
    for (u64 i0 = s0; i0 < s1; i0 += 4 * kCountThreads) {
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const u64 i = i0 + (u64)u * kCountThreads + threadIdx.x;
            v[u] = i < s1 ? scratch[i] : kPad;
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (v[u] != kPad && (v[u] >> kHistHalfShift) == half)
                atomicAdd(&cnt[(v[u] & (kStates - 1)) * kHistHalfTexels + ((v[u] >> 10) & (kHistHalfTexels - 1))], 1u);
    }
    __syncthreads();
    /* lane (g, l): states [32 g, 32 g + 32) of texel l */
    const int l = threadIdx.x & (kHistHalfTexels - 1), g = threadIdx.x / kHistHalfTexels;
    const uint32_t *col = cnt + (size_t)g * kGroupStates * kHistHalfTexels + l;
    uint32_t n = 0;
#pragma unroll 8
    for (int k = 0; k < kGroupStates; k++) n += col[k * kHistHalfTexels] != 0;
    part[g][l] = n;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int q = 0; q < kGroups; q++) {
        const uint32_t p = part[q][l];
        before += q < g ? p : 0u;
        total += p;
    }
    if (!FILL) {
        if (g == 0) nz[(size_t)half * kHistHalfTexels + l] = total;
        return;
    }
    u64 *e = piece + (size_t)begin * 64 + (half & 1) * kHistHalfTexels + l; /* slot 0 of this texel; slot j < r only */
    u64 j = before;
    for (int k = 0; k < kGroupStates; k++) {
        const uint32_t v = col[k * kHistHalfTexels];
        if (v != 0 && j < r) {
            e[(size_t)j * 64] = ((u64)(g * kGroupStates + k) << kSparseCountBits) | v;
            j++;
        }
    }
    for (j = (u64)total + g; j < r; j += kGroups) e[(size_t)j * 64] = 0; /* padding: every slot is written */
}

__global__ __launch_bounds__(64) void k_hist_rows(const uint32_t *__restrict__ nz, uint32_t block_lo,
                                                  u64 *__restrict__ rows_local, u64 *__restrict__ rows_all,
                                                  SparseSums *__restrict__ sums) {
    const uint32_t b = block_lo + blockIdx.x;
    const uint32_t n = nz[(size_t)b * 64 + threadIdx.x];
    const uint32_t r = wmax(n);
    const u64 cells = wsum(n);
    if (threadIdx.x != 0) return;
    rows_local[(size_t)blockIdx.x + 1] = r;
    rows_all[(size_t)b + 1] = r;
    if (r) atomicAdd(&sums->rows, (u64)r);
    if (cells) atomicAdd(&sums->cells, cells);
}

/* FILL = false: out = off (r_b in off[b + 1], may be null) and sums (may be null); FILL = true: out = the sum's
   blob whose off[] the scan has written */
template <bool FILL>
__global__ __launch_bounds__(64) void k_sparse_add(const u64 *__restrict__ a, u64 a_rows, const u64 *__restrict__ b,
                                                   u64 b_rows, u64 *out, u64 out_rows, SparseSums *__restrict__ sums) {
    const int lane = threadIdx.x;
    const size_t blk = blockIdx.x, B = gridDim.x;
    const u64 ab = min64(a[blk], a_rows), ae = min64(a[blk + 1], a_rows);
    const u64 bb = min64(b[blk], b_rows), be = min64(b[blk + 1], b_rows);
    const u64 *ea = a + B + 1 + lane, *eb = b + B + 1 + lane;
    u64 ia = ab, ib = bb; /* (a block whose begin exceeds its end has no row: ia < ae never holds) */
    u64 va = ia < ae ? ea[(size_t)ia * 64] : 0ull, vb = ib < be ? eb[(size_t)ib * 64] : 0ull;
    u64 r = 0;
    u64 *eo = nullptr;
    if (FILL) {
        const u64 ob = min64(out[blk], out_rows), oe = min64(out[blk + 1], out_rows);
        if (ob >= oe) return;
        r = oe - ob;
        eo = out + B + 1 + (size_t)ob * 64 + lane;
    }
    uint32_t n = 0, big = 0;
    u64 dep = 0, j = 0;
    while (va | vb) { /* an entry of 0 is padding: the end of a lane's list */
        const u64 sa = va >> kSparseCountBits, sb = vb >> kSparseCountBits;
        const bool ta = va != 0 && (vb == 0 || sa <= sb), tb = vb != 0 && (va == 0 || sb <= sa);
        const u64 c = (ta ? va & kSparseCountMask : 0ull) + (tb ? vb & kSparseCountMask : 0ull);
        const u64 st = ta ? sa : sb;
        if (ta) {
            ia++;
            va = ia < ae ? ea[(size_t)ia * 64] : 0ull;
        }
        if (tb) {
            ib++;
            vb = ib < be ? eb[(size_t)ib * 64] : 0ull;
        }
        if (c == 0) continue; /* (a state with a count of 0: not canonical, no cell) */
        if (FILL) {
            if (j < r) eo[(size_t)j * 64] = (st << kSparseCountBits) | (c & kSparseCountMask);
            j++;
        } else {
            n++;
            big += c > kSparseCountMask;
            dep += c;
        }
    }
    if (FILL) {
        for (; j < r; j++) eo[(size_t)j * 64] = 0;
        return;
    }
    const uint32_t rb = wmax(n);
    const u64 cells = wsum(n), deposits = wsum(dep), too_large = wsum(big);
    if (lane != 0) return;
    if (out) out[blk + 1] = rb;
    if (!sums) return;
    if (rb) atomicAdd(&sums->rows, (u64)rb);
    if (cells) atomicAdd(&sums->cells, cells);
    if (deposits) atomicAdd(&sums->deposits, deposits);
    if (too_large) atomicAdd(&sums->too_large, too_large);
}

unsigned bin_grid(const HistSource &src) { return (unsigned)((src.nseg + kBinSegs - 1) / kBinSegs); }

} // namespace

hipError_t fmgi_launch_hist_bins(const HistSource &src, uint32_t halves, unsigned long long *half_count,
                                 unsigned long long *skipped, hipStream_t s) {
    if (halves > (uint32_t)kHistMaxHalves) return hipErrorInvalidValue;
    if (src.nseg == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hist_bins, dim3(bin_grid(src)), dim3(kBinThreads), 0, s, src, halves, half_count, skipped);
    return hipGetLastError();
}

hipError_t fmgi_launch_hist_scatter(const HistSource &src, uint32_t half_lo, uint32_t half_hi, uint32_t *cursor,
                                    uint32_t *scratch, uint32_t scratch_cap, hipStream_t s) {
    if (half_hi < half_lo || half_hi - half_lo > (uint32_t)kHistMaxHalves) return hipErrorInvalidValue;
    if (src.nseg == 0 || half_lo == half_hi) return hipSuccess;
    hipLaunchKernelGGL(k_hist_scatter, dim3(bin_grid(src)), dim3(kBinThreads), 0, s, src, half_lo, half_hi, cursor,
                       scratch, scratch_cap);
    return hipGetLastError();
}

hipError_t fmgi_launch_hist_count(const uint32_t *scratch, const uint32_t *start, uint32_t scratch_cap,
                                  uint32_t half_lo, uint32_t half_hi, uint32_t *nz, hipStream_t s) {
    if (half_hi <= half_lo) return hipSuccess;
    hipError_t e = fmgi_set_lds_attr_fn((const void *)k_hist_count<false>, (int)kCountLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hist_count<false>, dim3(half_hi - half_lo), dim3(kCountThreads), kCountLds, s, scratch, start,
                       scratch_cap, half_lo, nz, (const u64 *)nullptr, 0ull, (u64 *)nullptr);
    return hipGetLastError();
}

hipError_t fmgi_launch_hist_rows(const uint32_t *nz, uint32_t block_lo, uint32_t block_hi,
                                 unsigned long long *rows_local, unsigned long long *rows_all, SparseSums *sums,
                                 hipStream_t s) {
    if (block_hi <= block_lo) return hipSuccess;
    hipLaunchKernelGGL(k_hist_rows, dim3(block_hi - block_lo), dim3(64), 0, s, nz, block_lo, rows_local, rows_all, sums);
    return hipGetLastError();
}

hipError_t fmgi_launch_hist_fill(const uint32_t *scratch, const uint32_t *start, uint32_t scratch_cap,
                                 uint32_t half_lo, uint32_t half_hi, const unsigned long long *off,
                                 unsigned long long piece_rows, unsigned long long *piece, hipStream_t s) {
    if (half_hi <= half_lo || piece_rows == 0) return hipSuccess;
    hipError_t e = fmgi_set_lds_attr_fn((const void *)k_hist_count<true>, (int)kCountLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hist_count<true>, dim3(half_hi - half_lo), dim3(kCountThreads), kCountLds, s, scratch, start,
                       scratch_cap, half_lo, (uint32_t *)nullptr, off, piece_rows, piece);
    return hipGetLastError();
}

hipError_t fmgi_launch_sparse_add_count(const unsigned long long *a, unsigned long long a_rows,
                                        const unsigned long long *b, unsigned long long b_rows, int num_texels,
                                        unsigned long long *off, SparseSums *sums, hipStream_t s) {
    if (num_texels <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sparse_add<false>, dim3((unsigned)fmgi_sparse_blocks(num_texels)), dim3(64), 0, s, a, a_rows, b,
                       b_rows, off, 0ull, sums);
    return hipGetLastError();
}

hipError_t fmgi_launch_sparse_add_fill(const unsigned long long *a, unsigned long long a_rows,
                                       const unsigned long long *b, unsigned long long b_rows, int num_texels,
                                       unsigned long long *sum, unsigned long long sum_rows, hipStream_t s) {
    if (num_texels <= 0 || sum_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sparse_add<true>, dim3((unsigned)fmgi_sparse_blocks(num_texels)), dim3(64), 0, s, a, a_rows, b,
                       b_rows, sum, sum_rows, (SparseSums *)nullptr);
    return hipGetLastError();
}
