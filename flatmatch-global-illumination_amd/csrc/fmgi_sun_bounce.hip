/*
 * fmgi_sun_bounce.hip -- the bounced-sun layer's kernels (semantics: include/flatmatch_gi.h "Bounced
 * sunlight"). fp32 is IEEE in the order the header states, contraction off; the add is in doubles.
 *
 * Layout of a pass of K directions: kp = 1, 2, 4, 8, 16 or 32 >= K slots per texel, `[texel][kp]` floats, so a
 * texel's values are kp * 4 contiguous bytes (one 128-B line at kp = 32). Slots K .. kp-1 are padding: +0
 * everywhere, never written out. No slot reads another, so a direction's rows depend on nothing but its own map.
 *
 *   k_sun_e0           the start table: ((float)cover * c_w) / (float)(S * S) on the level-0 texels of the walls
 *                      that face direction k, c_w from the cache's own rectangles; the table was zeroed before.
 *   k_sun_gather<KP>   max(1, KP / 4) neighbouring lanes per job; a lane loads up to four directions of a ray's
 *                      texel at once and keeps as many sequential sums over the job's 10000 rays.
 *   k_sun_unpack       slot k of texels [0, numTexels) -> row n - 1 of direction k's output.
 *   k_sun_add_bounced  one lane per level-0 texel of every wall: the reflectance's power chain and the deposit.
 *
 * Memory safety: an id is used only if 0 <= id < num_texels <= ntex, a job's texel is stored to only below ntex, a
 * wall's texel is written only below ntex (e0) or num_texels (add); all bounds are kernel arguments.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fmgi_sun_bounce.h"

#pragma clang fp contract(off)

namespace {

/* the ids keep k_rad_gather_sets' block prefetch: GATHER_B ids of the next block in flight while this block's
   texels load */
constexpr int GATHER_B = 25;
static_assert(FMGI_RAD_RAYS % GATHER_B == 0, "gather blocks must tile the rays");

/* W floats a lane loads per ray: the directions it sums */
template <int W> struct Vec;
template <> struct Vec<1> { using type = float; };
template <> struct Vec<2> { using type = float2; };
template <> struct Vec<4> { using type = float4; };

__device__ __forceinline__ float comp(float v, int) { return v; }
__device__ __forceinline__ float comp(float2 v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ float comp(float4 v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

__global__ __launch_bounds__(256) void k_sun_e0(SunBounce b, SunBounceDirs d) {
    const int w = (int)blockIdx.y;
    if (w >= b.nwalls) return;
    const RadRect r = b.rects[w];
    const int64_t n = (int64_t)r.s1 * r.s2 * b.kp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = (int64_t)r.s0 + e / b.kp;
        const int k = (int)(e % b.kp);
        if (k >= b.ndirs || t < 0 || t >= b.num_texels || t >= b.ntex) continue;
        const float c = (r.nx * d.sx[k] + r.ny * d.sy[k]) + r.nz * d.sz[k];
        if (!(c > 0)) continue;
        b.dst[t * b.kp + k] = ((float)d.cover[k][t] * c) / d.s2[k];
    }
}

template <int KP> __global__ __launch_bounds__(256) void k_sun_gather(SunBounce b) {
    constexpr int L = KP >= 4 ? KP / 4 : 1; /* lanes per job */
    constexpr int W = KP / L;               /* directions per lane */
    using V = typename Vec<W>::type;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t job = g / L;
    const int sub = (int)(g % L);
    if (job >= b.njobs) return;
    const int32_t *s = b.sids + job;
    const int64_t stride = b.njobs;
    const V *src = (const V *)b.src + sub;
    const uint32_t lim = (uint32_t)b.num_texels;
    float sum[W];
#pragma unroll
    for (int c = 0; c < W; c++) sum[c] = 0.0f;
    int32_t nxt[GATHER_B];
#pragma unroll
    for (int i = 0; i < GATHER_B; i++) nxt[i] = __builtin_nontemporal_load(s + (int64_t)i * stride);
    for (int k0 = 0; k0 < FMGI_RAD_RAYS; k0 += GATHER_B) {
        int32_t id[GATHER_B];
#pragma unroll
        for (int i = 0; i < GATHER_B; i++) id[i] = nxt[i];
        if (k0 + GATHER_B < FMGI_RAD_RAYS) {
#pragma unroll
            for (int i = 0; i < GATHER_B; i++)
                nxt[i] = __builtin_nontemporal_load(s + (int64_t)(k0 + GATHER_B + i) * stride);
        }
        V t[GATHER_B];
#pragma unroll
        for (int i = 0; i < GATHER_B; i++) t[i] = src[(int64_t)((uint32_t)id[i] < lim ? id[i] : 0) * L];
#pragma unroll
        for (int i = 0; i < GATHER_B; i++) {
            const bool hit = (uint32_t)id[i] < lim; /* -1, and the window and light texels behind numTexels, add nothing */
#pragma unroll
            for (int c = 0; c < W; c++) sum[c] = hit ? sum[c] + comp(t[i], c) : sum[c];
        }
    }
    const int64_t texel = b.jobs[job].texel;
    if (texel < 0 || texel >= b.ntex) return;
    float *o = b.dst + texel * KP + sub * W;
#pragma unroll
    for (int c = 0; c < W; c++) o[c] = sum[c] / 10000.0f;
}

/* lanes along the texels: coalesced stores to the direction's row, blockIdx.y is the slot */
__global__ __launch_bounds__(256) void k_sun_unpack(SunBounce b, SunBounceDirs d) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = (int)blockIdx.y;
    if (t >= b.num_texels || k >= b.ndirs) return;
    d.out[k][(int64_t)b.row * b.num_texels + t] = b.src[t * b.kp + k];
}

/* the wall that holds level-0 texel g of the running count (0 <= g < total): the last one whose first is <= g */
__device__ __forceinline__ int wall_of(const SunBounceWall *__restrict__ walls, int nwalls, int g) {
    int lo = 0, hi = nwalls;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (walls[mid].first <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_sun_add_bounced(SunBounceAdd a) {
    const long long g64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g64 >= a.total) return;
    const int g = (int)g64;
    const SunBounceWall w = a.walls[wall_of(a.walls, a.nwalls, g)];
    const int local = g - w.first;
    if (local < 0 || local >= w.n) return;
    const int t = w.s0 + local;
    if ((unsigned)t >= (unsigned)a.num_texels) return;
    float gn[FMGI_SUN_BOUNCES];
    bool any = false;
#pragma unroll
    for (int n = 0; n < FMGI_SUN_BOUNCES; n++) {
        gn[n] = n < a.bounces ? a.bounce[(size_t)n * (size_t)a.num_texels + (size_t)t] : 0.0f;
        any = any || gn[n] != 0.0f;
    }
    if (!any) return;
#pragma unroll
    for (int m = 0; m < FMGI_SUN_BOUNCE_MAPS; m++) {
        if (m >= a.maps) break;
        unsigned long long *p = a.lm[m] + 4 * (size_t)t;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double refl = (double)a.refl[m][c];
            double pw = refl, v = 0.0;
#pragma unroll
            for (int n = 0; n < FMGI_SUN_BOUNCES; n++) {
                if (n < a.bounces) {
                    v = v + (double)gn[n] * pw;
                    pw = pw * refl;
                }
            }
            const double q = floor(ldexp((((double)a.rgb[m][c] * v) * a.flux) * w.area_t, 25));
            p[c] += (unsigned long long)(long long)q;
        }
    }
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

bool valid(const SunBounce &b) {
    return (b.kp == 1 || b.kp == 2 || b.kp == 4 || b.kp == 8 || b.kp == 16 || b.kp == 32) && b.ndirs >= 1 &&
           b.ndirs <= b.kp && b.num_texels >= 0 && b.num_texels <= b.ntex && b.njobs >= 0 && b.nwalls >= 0;
}

} // namespace

hipError_t fmgi_sun_bounce_launch_e0(const SunBounce &b, const SunBounceDirs &d, hipStream_t s) {
    if (!valid(b) || !b.dst) return hipErrorInvalidValue;
    if (b.nwalls < 1 || b.num_texels < 1) return hipSuccess;
    /* a wall's elements go round a fixed number of workgroups: at most 64 * 256 lanes per wall */
    const int64_t per_wall = std::min<int64_t>((b.njobs * b.kp + 255) / 256, 64);
    hipLaunchKernelGGL(k_sun_e0, dim3((unsigned)std::max<int64_t>(per_wall, 1), (unsigned)b.nwalls), dim3(256), 0, s, b, d);
    return hipGetLastError();
}

hipError_t fmgi_sun_bounce_launch_gather(const SunBounce &b, hipStream_t s) {
    if (!valid(b) || !b.src || !b.dst) return hipErrorInvalidValue;
    if (b.njobs < 1) return hipSuccess;
    const dim3 block(256);
    switch (b.kp) {
    case 1: hipLaunchKernelGGL(k_sun_gather<1>, dim3(blocks_of(b.njobs)), block, 0, s, b); break;
    case 2: hipLaunchKernelGGL(k_sun_gather<2>, dim3(blocks_of(b.njobs)), block, 0, s, b); break;
    case 4: hipLaunchKernelGGL(k_sun_gather<4>, dim3(blocks_of(b.njobs)), block, 0, s, b); break;
    case 8: hipLaunchKernelGGL(k_sun_gather<8>, dim3(blocks_of(b.njobs * 2)), block, 0, s, b); break;
    case 16: hipLaunchKernelGGL(k_sun_gather<16>, dim3(blocks_of(b.njobs * 4)), block, 0, s, b); break;
    default: hipLaunchKernelGGL(k_sun_gather<32>, dim3(blocks_of(b.njobs * 8)), block, 0, s, b); break;
    }
    return hipGetLastError();
}

hipError_t fmgi_sun_bounce_launch_unpack(const SunBounce &b, const SunBounceDirs &d, hipStream_t s) {
    if (!valid(b) || !b.src || b.row < 0 || b.row >= FMGI_SUN_BOUNCES) return hipErrorInvalidValue;
    if (b.num_texels < 1) return hipSuccess;
    hipLaunchKernelGGL(k_sun_unpack, dim3(blocks_of(b.num_texels), (unsigned)b.ndirs), dim3(256), 0, s, b, d);
    return hipGetLastError();
}

hipError_t fmgi_sun_bounce_launch_add(const SunBounceAdd &a, hipStream_t s) {
    if (a.bounces < 1 || a.bounces > FMGI_SUN_BOUNCES || a.maps < 1 || a.maps > FMGI_SUN_BOUNCE_MAPS || !a.bounce)
        return hipErrorInvalidValue;
    if (a.total < 1 || a.nwalls < 1) return hipSuccess;
    hipLaunchKernelGGL(k_sun_add_bounced, dim3((unsigned)(((long long)a.total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
