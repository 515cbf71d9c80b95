/*
 * fmgi_filter.hip -- the adaptive density filter of the int64 fixed-point lightmap: per
 * level-0 texel a square window, grown until it holds enough energy of a guide lightmap and clipped to the
 * texel's own wall, then the mean of every map over that window, all in exact 64-bit integers.
 *
 * Window sums come from per-wall inclusive 2-D prefix sums (summed-area tables) kept in the context's
 * scratch, one plane [num_texels] per summed quantity. The sums are taken mod 2^64: a table entry may wrap,
 * the four-corner difference of a window whose true sum is below 2^64 is still that sum.
 *   k_filter_rows   one lane per texel in flat texel order. A wall's rows are consecutive runs of texels, so a
 *                   wave scans its 64 texels with a segmented shuffle scan (lane i takes lane i - d's partial
 *                   sum only if d <= x, its column); a row that began before the wave's first texel brings a
 *                   carry, the sum of its x0 earlier texels, which the wave reads and reduces itself.
 *   k_filter_cols   one lane per wall column walking down the rows (neighbouring lanes = neighbouring x, so
 *                   every step is a coalesced load and store).
 *   k_filter_radii  one lane per texel: the smallest r whose window sum reaches min_energy, four lookups per r.
 *   k_filter_apply  one lane per texel and map: four lookups per channel and one unsigned 64-bit division by
 *                   the window's texel count (the compiler's exact division; r = 0 copies the texel).
 * No kernel launches work per wall: walls of 1 x 1 texels cost a lane, not a workgroup. Planes and maps are
 * gridDim.y. Every index is inside [0, num_texels): fmgi_set_scene checks s0 + s1 * s2 <= num_texels.
 */
#include <hip/hip_runtime.h>

#include "fmgi_filter.h"

namespace {

typedef unsigned long long u64;
constexpr int kBlock = 256;

/* plane j's value of texel t: the guide's energy, or channel j % 3 of map j / 3 */
__device__ __forceinline__ u64 plane_value(const FilterArgs &a, int j, int64_t t) {
    if (a.guide) {
        const u64 *g = a.guide + 4 * t;
        return g[0] + g[1] + g[2];
    }
    return a.in[j / 3][4 * t + j % 3];
}

__global__ __launch_bounds__(kBlock) void k_filter_rows(FilterArgs a) {
    const int j = (int)blockIdx.y;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < a.num_texels;
    int x = 0;
    u64 v = 0;
    if (live) {
        const FilterTex tx = a.tex[t];
        if (tx.wall >= 0) {
            const FilterWall w = a.walls[tx.wall];
            x = (int)(t - w.s0) - tx.y * w.s1;
            v = plane_value(a, j, t);
        }
    }
    /* the row of lane 0 began x0 texels before this wave: their sum */
    const int x0 = __shfl(x, 0);
    u64 carry = 0;
    if (x0 > 0) {
        const int64_t first = t - lane - x0; /* >= the wall's s0 */
        for (int i = lane; i < x0; i += 64) carry += plane_value(a, j, first + i);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) carry += __shfl_xor(carry, d);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 u = __shfl_up(v, d);
        if (d <= x && d <= lane) v += u;
    }
    if (x > lane) v += carry; /* lanes of lane 0's row */
    if (live) a.sat[(size_t)j * (size_t)a.num_texels + (size_t)t] = v;
}

__global__ __launch_bounds__(kBlock) void k_filter_cols(FilterArgs a) {
    const int ci = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (ci >= a.num_cols) return;
    const FilterCol c = a.cols[ci];
    const FilterWall w = a.walls[c.wall];
    u64 *p = a.sat + (size_t)blockIdx.y * (size_t)a.num_texels + (size_t)w.s0 + (size_t)c.x;
    const size_t s1 = (size_t)w.s1;
    u64 acc = 0;
    int y = 0;
    for (; y + 4 <= w.s2; y += 4, p += 4 * s1) {
        const u64 v0 = p[0], v1 = p[s1], v2 = p[2 * s1], v3 = p[3 * s1];
        p[0] = acc += v0;
        p[s1] = acc += v1;
        p[2 * s1] = acc += v2;
        p[3 * s1] = acc += v3;
    }
    for (; y < w.s2; y++, p += s1) *p = acc += *p;
}

/* the sum of plane P (a wall's table, texel (x, y) at P[y * s1 + x]) over the window of radius r around (x, y),
   clipped to the wall; n = the window's texel count */
__device__ __forceinline__ u64 window_sum(const u64 *P, int s1, int s2, int x, int y, int r, int &n) {
    const int xa = max(x - r, 0), xb = min(x + r, s1 - 1), ya = max(y - r, 0), yb = min(y + r, s2 - 1);
    n = (xb - xa + 1) * (yb - ya + 1);
    const size_t S = (size_t)s1;
    u64 s = P[yb * S + xb];
    if (xa > 0) s -= P[yb * S + (xa - 1)];
    if (ya > 0) s -= P[(ya - 1) * S + xb];
    if (xa > 0 && ya > 0) s += P[(ya - 1) * S + (xa - 1)];
    return s;
}

__global__ __launch_bounds__(kBlock) void k_filter_radii(FilterArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= a.num_texels) return;
    const FilterTex tx = a.tex[t];
    int r = 0;
    if (tx.wall >= 0) {
        const FilterWall w = a.walls[tx.wall];
        const int x = (int)(t - w.s0) - tx.y * w.s1;
        const u64 *P = a.sat + w.s0;
        r = a.max_radius;
        for (int q = 0; q < a.max_radius; q++) {
            int n;
            if (window_sum(P, w.s1, w.s2, x, tx.y, q, n) >= a.min_energy) {
                r = q;
                break;
            }
        }
    }
    a.radii_out[t] = (uint8_t)r;
}

__global__ __launch_bounds__(kBlock) void k_filter_apply(FilterArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= a.num_texels) return;
    const int k = (int)blockIdx.y;
    const u64 *in = a.in[k] + 4 * t;
    u64 v[4] = {in[0], in[1], in[2], in[3]};
    const FilterTex tx = a.tex[t];
    if (tx.wall >= 0) {
        const int r = min((int)a.radii_in[t], kFilterMaxRadius);
        if (r > 0) { /* (r = 0: the window is the texel, its count 1) */
            const FilterWall w = a.walls[tx.wall];
            const int x = (int)(t - w.s0) - tx.y * w.s1;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                int n;
                const u64 s = window_sum(a.sat + (size_t)(3 * k + c) * (size_t)a.num_texels + w.s0, w.s1, w.s2, x,
                                         tx.y, r, n);
                v[c] = n == 1 ? s : s / (u64)n;
            }
        }
    }
    u64 *out = a.out[k] + 4 * t;
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
    out[3] = v[3];
}

unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

} // namespace

hipError_t fmgi_launch_filter_sat(const FilterArgs &a, int planes, hipStream_t s) {
    if (a.num_texels <= 0) return hipSuccess;
    if (planes < 1 || planes > 3 * kFilterMaxMaps) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_rows, dim3(blocks(a.num_texels), (unsigned)planes), dim3(kBlock), 0, s, a);
    if (a.num_cols > 0)
        hipLaunchKernelGGL(k_filter_cols, dim3(blocks(a.num_cols), (unsigned)planes), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t fmgi_launch_filter_radii(const FilterArgs &a, hipStream_t s) {
    if (a.num_texels <= 0) return hipSuccess;
    if (a.max_radius < 0 || a.max_radius > kFilterMaxRadius) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_radii, dim3(blocks(a.num_texels)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t fmgi_launch_filter_apply(const FilterArgs &a, hipStream_t s) {
    if (a.num_texels <= 0) return hipSuccess;
    if (a.maps < 1 || a.maps > kFilterMaxMaps) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_apply, dim3(blocks(a.num_texels), (unsigned)a.maps), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
