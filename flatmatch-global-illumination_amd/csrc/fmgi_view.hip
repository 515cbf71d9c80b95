/*
 * fmgi_view.hip -- the view renderer's kernels, bit-identical to the reference's debug raycaster
 * (debugRaytracer.cc:121-176 over radiosityNative.c:25-90); see fmgi_view.h for the kernel plan.
 *
 * Arithmetic: IEEE fp32 in the reference's source order (gcc -O2 -msse3, no FMA), contraction off, with
 * the helpers the radiosity backend uses (fmgi_rect_dev.h). The orthographic and equirectangular cameras
 * (no reference program) are the _proj instances; they call the pin-hole kernels' device functions.
 * The glossy floor's mirror bounce (no reference program) is the _gloss kernels on the same functions.
 */
#include <hip/hip_runtime.h>

#include "fmgi_lds_attr.h"
#include "fmgi_view.h"

#pragma clang fp contract(off)

#include "fmgi_math.h"
#include "fmgi_rect_dev.h"

namespace {

using namespace fmgi_dev;

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

/*
 * One workgroup per camera: k_rad_rays's prologue. LDS: sort_n 64-bit keys (distance bits << 32 | wall
 * index; ~0 for culled walls). getSortedIntersectableRects (radiosityNative.c:25-61) filters in wall order
 * and glibc's qsort is a stable merge sort, so the list is ordered by (distance, index).
 */
__global__ __launch_bounds__(256) void k_view_candidates(ViewArgs a) {
    extern __shared__ unsigned long long keys[];
    __shared__ int ncand;
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const ViewCam V = a.cams[c];
    const v3 cam = mk(V.px, V.py, V.pz), n = mk(V.dx, V.dy, V.dz);
    if (tid == 0) ncand = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < a.sort_n; i += blockDim.x) {
        unsigned long long key = ~0ull;
        if (i < a.nrects) {
            const RadRect r = a.rects[i];
            const v3 pos = mk(r.px, r.py, r.pz), w = mk(r.wx, r.wy, r.wz), h = mk(r.hx, r.hy, r.hz),
                     rn = mk(r.nx, r.ny, r.nz);
            if (!(dot(rn, sub(pos, cam)) > 0) && !behind_ray(pos, w, h, cam, n)) {
                key = ((unsigned long long)__float_as_uint(min_dist(pos, w, h, rn, cam)) << 32) | (uint32_t)i;
                mine++;
            }
        }
        keys[i] = key;
    }
    if (mine) atomicAdd(&ncand, mine);
    __syncthreads();
    /* bitonic sort, ascending */
    for (int k = 2; k <= a.sort_n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < a.sort_n / 2; i += blockDim.x) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                const unsigned long long x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    keys[lo] = y;
                    keys[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    unsigned long long *out = a.keys + (size_t)c * a.sort_n;
    for (int i = tid; i < a.sort_n; i += blockDim.x) out[i] = keys[i];
    if (tid == 0) a.counts[c] = ncand;
}

/* debugRaytracer.cc:154-155: the ray through the screen point (fx, fy); add3 sums left to right */
__device__ __forceinline__ v3 view_dir(const ViewCam &V, v3 cam, float fx, float fy) {
    const v3 screen = add(add(mk(V.cx, V.cy, V.cz), mul(mk(V.rx, V.ry, V.rz), fx)), mul(mk(V.ux, V.uy, V.uz), fy));
    return unit(sub(screen, cam));
}

/*
 * findClosestIntersectionSorted (radiosityNative.c:67-90), the ray starting at camPos itself: the hit wall or
 * -1, its distance in dist. The candidate index is uniform over the wave's lanes that are still walking (they
 * all started at 0 together), so keys and rectangles are read once per wave.
 */
__device__ __forceinline__ int view_walk(const ViewArgs &a, const unsigned long long *keys, int C, v3 cam, v3 dir,
                                         float &dist, unsigned long long &tests) {
    dist = INFINITY;
    int target = -1;
    for (int i = 0; i < C; i++) {
        const unsigned long long key = keys[i];
        const float md = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32)));
        if (dist < md) break;
        const int idx = __builtin_amdgcn_readfirstlane((int)(uint32_t)key);
        tests++;
        const float dn = rect_intersects(a.hits[idx], cam, dir, dist);
        if (dn < 0) continue;
        if (dn <= dist) {
            target = idx;
            dist = dn;
        }
    }
    return target;
}

/* getTileIdAt's tile coordinates before the cast (rectangle.c:205-230) */
__device__ __forceinline__ void view_uv(const AoRect &t, const RadRect &tr, v3 cam, v3 dir, float dist, float &u,
                                        float &v) {
    const v3 pd = sub(add(cam, mul(dir, dist)), mk(t.px, t.py, t.pz));
    const float dx = dot(mk(t.wx, t.wy, t.wz), pd), dy = dot(mk(t.hx, t.hy, t.hz), pd);
    u = dx * (float)tr.s1 / t.wl;
    v = dy * (float)tr.s2 / t.hl;
}

/*
 * One lane per pixel; a wave is an 8x8 pixel block, a workgroup 2x2 of them; blockIdx.z is the camera.
 * A lane outside the image does nothing but join the wave's sum of its test counter with a zero.
 */
__global__ __launch_bounds__(256) void k_view_rays(ViewArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    unsigned long long tests = 0;
    if (x < a.width && y < a.height) {
        const ViewCam V = a.cams[c];
        const v3 cam = mk(V.px, V.py, V.pz);
        const float fx = V.pixel * (float)(x - a.width / 2), fy = -V.pixel * (float)(y - a.height / 2);
        const v3 dir = view_dir(V, cam, fx, fy);
        float dist;
        const int target = view_walk(a, a.keys + (size_t)c * a.sort_n, a.counts[c], cam, dir, dist, tests);
        int sid = -1;
        uint32_t rgb = a.background;
        if (target >= 0) {
            const RadRect tr = a.rects[target];
            float u, v;
            view_uv(a.hits[target], tr, cam, dir, dist, u, v);
            const int tx = clampi(cvt_x86(u), 0, tr.s1 - 1);
            const int ty = clampi(cvt_x86(v), 0, tr.s2 - 1);
            const int tile = ty * tr.s1 + tx;
            sid = tr.s0 + tile;
            if (a.rgb_out) {
                const uint8_t *p = a.tiles_rgb + 3 * (a.first_tile[target] + tile);
                rgb = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            }
        }
        const int64_t o = ((int64_t)c * a.height + y) * a.width + x;
        if (a.wall_out) a.wall_out[o] = target;
        if (a.texel_out) a.texel_out[o] = sid;
        if (a.dist_out) a.dist_out[o] = dist;
        if (a.rgb_out) {
            uint8_t *q = a.rgb_out + 3 * o;
            q[0] = (uint8_t)rgb;
            q[1] = (uint8_t)(rgb >> 8);
            q[2] = (uint8_t)(rgb >> 16);
        }
    }
    /* intersects() evaluations: counted per lane, one atomic per wave */
    const unsigned long long s = wave_sum(tests);
    if (lane == 0 && s) atomicAdd(a.tests, s);
}

__global__ __launch_bounds__(256) void k_view_pack(const uint8_t *rgb, uint32_t *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (uint32_t)rgb[3 * i] | ((uint32_t)rgb[3 * i + 1] << 8) | ((uint32_t)rgb[3 * i + 2] << 16);
}

/* one axis of the bilinear footprint: the two tile columns (clamped to the wall's grid) and the weight of the second */
__device__ __forceinline__ void tap_axis(float u, int n, int &a, int &b, float &f) {
    const float t = u - 0.5f, t0 = floorf(t);
    f = t - t0;
    a = clampi((int)t0, 0, n - 1);
    b = clampi((int)t0 + 1, 0, n - 1);
}

__device__ __forceinline__ float lerp2(float f, float a, float b) { return (1.0f - f) * a + f * b; }

/* the sample's fixed-point colour: (int)(val * 256 + 0.5) */
__device__ __forceinline__ int fix8(float val) { return (int)(val * 256.0f + 0.5f); }

/*
 * k_view_rays's pixel mapping over the window [x0, x1) x [y0, y1). A lane loops its pixel's samples x samples
 * rays: every lane of the wave starts each ray's walk at candidate 0 together, so view_walk's wave-uniform
 * reads hold. Colours are summed as 24.8 fixed point, so the result does not depend on the sample order.
 */
__global__ __launch_bounds__(256) void k_view_shade(ShadeArgs s) {
    const ViewArgs &a = s.v;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = s.x0 + (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = s.y0 + (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    unsigned long long tests = 0;
    if (x < s.x1 && y < s.y1) {
        const ViewCam V = a.cams[c];
        const v3 cam = mk(V.px, V.py, V.pz);
        const unsigned long long *keys = a.keys + (size_t)c * a.sort_n;
        const int C = a.counts[c], S = s.samples;
        const bool colour = a.rgb_out != nullptr, bilinear = s.filter != 0;
        const float px = (float)(x - a.width / 2), py = (float)(y - a.height / 2);
        const int bg0 = fix8((float)(a.background & 255)), bg1 = fix8((float)((a.background >> 8) & 255)),
                  bg2 = fix8((float)((a.background >> 16) & 255));
        int sum0 = 0, sum1 = 0, sum2 = 0, cov = 0;
        for (int j = 0; j < S; j++) {
            const float fy = -V.pixel * (py + s.offs[j]);
            for (int i = 0; i < S; i++) {
                const float fx = V.pixel * (px + s.offs[i]);
                const v3 dir = view_dir(V, cam, fx, fy);
                float dist;
                const int target = view_walk(a, keys, C, cam, dir, dist, tests);
                if (target < 0) {
                    sum0 += bg0, sum1 += bg1, sum2 += bg2;
                    continue;
                }
                cov++;
                if (!colour) continue;
                const RadRect tr = a.rects[target];
                float u, v;
                view_uv(a.hits[target], tr, cam, dir, dist, u, v);
                const uint32_t *T = s.tiles + a.first_tile[target];
                if (!bilinear) {
                    const uint32_t w = T[clampi(cvt_x86(v), 0, tr.s2 - 1) * tr.s1 + clampi(cvt_x86(u), 0, tr.s1 - 1)];
                    sum0 += fix8((float)(w & 255)), sum1 += fix8((float)((w >> 8) & 255)), sum2 += fix8((float)((w >> 16) & 255));
                    continue;
                }
                int xa, xb, ya, yb;
                float fu, fv;
                tap_axis(u, tr.s1, xa, xb, fu);
                tap_axis(v, tr.s2, ya, yb, fv);
                const uint32_t w00 = T[ya * tr.s1 + xa], w01 = T[ya * tr.s1 + xb], w10 = T[yb * tr.s1 + xa],
                               w11 = T[yb * tr.s1 + xb];
#define FMGI_CH(sh)                                                                                        \
    fix8(lerp2(fv, lerp2(fu, (float)((w00 >> sh) & 255), (float)((w01 >> sh) & 255)),                    \
               lerp2(fu, (float)((w10 >> sh) & 255), (float)((w11 >> sh) & 255))))
                sum0 += FMGI_CH(0), sum1 += FMGI_CH(8), sum2 += FMGI_CH(16);
#undef FMGI_CH
            }
        }
        const int64_t o = ((int64_t)c * a.height + y) * a.width + x;
        if (colour) {
            const int half = 128 * S * S, den = 256 * S * S;
            uint8_t *q = a.rgb_out + 3 * o;
            q[0] = (uint8_t)((sum0 + half) / den);
            q[1] = (uint8_t)((sum1 + half) / den);
            q[2] = (uint8_t)((sum2 + half) / den);
        }
        if (s.cov_out) s.cov_out[o] = (uint8_t)cov;
    }
    const unsigned long long n = wave_sum(tests);
    if (lane == 0 && n) atomicAdd(a.tests, n);
}

/*
 * The orthographic and equirectangular cameras. The host puts the orthonormal frame into the
 * ViewCam: d = f, r = normalized(cross(f, up)), u = cross(r, f), c = pos + f.
 *
 * The candidate lists of the two projections, k_view_candidates' sort and output:
 *   ORTHO     walls that face against f and have a corner at depth >= 0 along f; the key is the smallest
 *             corner depth, clamped to 0 from below (every ray of the camera has direction f, so a hit's
 *             distance is a depth between its wall's corner depths);
 *   EQUIRECT  the pin-hole's list without isBehindRay: the rays leave the camera in every direction;
 *   MIRROR    every wall, keyed as the pin-hole keys it: the list the mirror rays of any projection walk.
 */
template <int P>
__global__ __launch_bounds__(256) void k_view_candidates_proj(ViewArgs a) {
    extern __shared__ unsigned long long keys[];
    __shared__ int ncand;
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const ViewCam V = a.cams[c];
    const v3 cam = mk(V.px, V.py, V.pz), f = mk(V.dx, V.dy, V.dz);
    if (tid == 0) ncand = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < a.sort_n; i += blockDim.x) {
        unsigned long long key = ~0ull;
        if (i < a.nrects) {
            const RadRect r = a.rects[i];
            const v3 pos = mk(r.px, r.py, r.pz), w = mk(r.wx, r.wy, r.wz), h = mk(r.hx, r.hy, r.hz),
                     rn = mk(r.nx, r.ny, r.nz);
            bool keep;
            float md;
            if constexpr (P == FMGI_VIEW_ORTHO) {
                /* the corners in behind_ray's order */
                const float e1 = dot(sub(pos, cam), f), e2 = dot(sub(add(pos, w), cam), f),
                            e3 = dot(sub(add(pos, h), cam), f), e4 = dot(sub(add(add(pos, w), h), cam), f);
                const float m12 = e1 < e2 ? e1 : e2, m34 = e3 < e4 ? e3 : e4, m = m12 < m34 ? m12 : m34;
                keep = dot(rn, f) < 0 && !(e1 < 0 && e2 < 0 && e3 < 0 && e4 < 0);
                md = m < 0 ? 0.0f : m;
            } else if constexpr (P == FMGI_VIEW_MIRROR) {
                keep = true;
                md = min_dist(pos, w, h, rn, cam);
            } else {
                keep = !(dot(rn, sub(pos, cam)) > 0);
                md = keep ? min_dist(pos, w, h, rn, cam) : 0.0f;
            }
            if (keep) {
                key = ((unsigned long long)__float_as_uint(md) << 32) | (uint32_t)i;
                mine++;
            }
        }
        keys[i] = key;
    }
    if (mine) atomicAdd(&ncand, mine);
    __syncthreads();
    /* bitonic sort, ascending */
    for (int k = 2; k <= a.sort_n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < a.sort_n / 2; i += blockDim.x) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                const unsigned long long x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    keys[lo] = y;
                    keys[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    unsigned long long *out = a.keys + (size_t)c * a.sort_n;
    for (int i = tid; i < a.sort_n; i += blockDim.x) out[i] = keys[i];
    if (tid == 0) a.counts[c] = ncand;
}

/* ORTHO: the origin of the ray through the screen point (fx, fy) */
__device__ __forceinline__ v3 ortho_origin(const ViewCam &V, v3 cam, float fx, float fy) {
    return add(add(cam, mul(mk(V.rx, V.ry, V.rz), fx)), mul(mk(V.ux, V.uy, V.uz), fy));
}

/* EQUIRECT: the ray of longitude phi (sp, cp) and polar angle theta (st, ct): column width / 2 looks along f,
   x grows to the right, row 0 is straight up */
__device__ __forceinline__ v3 equirect_dir(const ViewCam &V, float sp, float cp, float st, float ct) {
    const float ea = (-cp) * st, eb = (-sp) * st;
    return unit(add(add(mul(mk(V.dx, V.dy, V.dz), ea), mul(mk(V.rx, V.ry, V.rz), eb)), mul(mk(V.ux, V.uy, V.uz), ct)));
}

/* EQUIRECT: the sines and cosines of a column's sample longitudes, once per lane. A lane keeps its S pairs in
   its own LDS slots ([sample][lane], 16 KB per workgroup, no bank conflicts, no barrier: nobody else reads
   them); registers indexed by the sample loop would cost the kernel half its occupancy. */
struct PhiTable {
    float2 sc[FMGI_VIEW_SAMPLES][256];
};
__device__ __forceinline__ void phi_table(PhiTable &t, int tid, int x, int S, const float *offs, float kphi) {
    for (int i = 0; i < S; i++) {
        float sn, cs;
        fmgi_sincosf(((float)x + (0.5f + offs[i])) * kphi, &sn, &cs);
        t.sc[i][tid] = make_float2(sn, cs);
    }
}

/*
 * k_view_shade for the two projections: the same pixel mapping, sample loop, walk, taps and fixed-point resolve;
 * only the sample's ray differs. ORTHO moves the origin over the screen plane and keeps the direction f;
 * EQUIRECT keeps the origin and takes theta's sine and cosine once per sample row, phi's once per lane and column.
 */
template <int P>
__global__ __launch_bounds__(256) void k_view_shade_proj(ShadeProjArgs q) {
    const ShadeArgs &s = q.s;
    const ViewArgs &a = s.v;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = s.x0 + (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = s.y0 + (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    __shared__ PhiTable phis; /* EQUIRECT only; ORTHO never touches it and the compiler drops it */
    unsigned long long tests = 0;
    if (x < s.x1 && y < s.y1) {
        const ViewCam V = a.cams[c];
        const v3 cam = mk(V.px, V.py, V.pz), f = mk(V.dx, V.dy, V.dz);
        const unsigned long long *keys = a.keys + (size_t)c * a.sort_n;
        const int C = a.counts[c], S = s.samples;
        const bool colour = a.rgb_out != nullptr, bilinear = s.filter != 0;
        const float px = (float)(x - a.width / 2), py = (float)(y - a.height / 2);
        const int bg0 = fix8((float)(a.background & 255)), bg1 = fix8((float)((a.background >> 8) & 255)),
                  bg2 = fix8((float)((a.background >> 16) & 255));
        if constexpr (P == FMGI_VIEW_EQUIRECT) phi_table(phis, tid, x, S, s.offs, q.kphi);
        int sum0 = 0, sum1 = 0, sum2 = 0, cov = 0;
        for (int j = 0; j < S; j++) {
            float fy = 0.0f, st = 0.0f, ct = 0.0f;
            if constexpr (P == FMGI_VIEW_ORTHO) fy = -V.pixel * (py + s.offs[j]);
            else fmgi_sincosf(((float)y + (0.5f + s.offs[j])) * q.ktheta, &st, &ct);
            for (int i = 0; i < S; i++) {
                v3 src = cam, dir = f;
                if constexpr (P == FMGI_VIEW_ORTHO) src = ortho_origin(V, cam, V.pixel * (px + s.offs[i]), fy);
                else dir = equirect_dir(V, phis.sc[i][tid].x, phis.sc[i][tid].y, st, ct);
                float dist;
                const int target = view_walk(a, keys, C, src, dir, dist, tests);
                if (target < 0) {
                    sum0 += bg0, sum1 += bg1, sum2 += bg2;
                    continue;
                }
                cov++;
                if (!colour) continue;
                const RadRect tr = a.rects[target];
                float u, v;
                view_uv(a.hits[target], tr, src, dir, dist, u, v);
                const uint32_t *T = s.tiles + a.first_tile[target];
                if (!bilinear) {
                    const uint32_t w = T[clampi(cvt_x86(v), 0, tr.s2 - 1) * tr.s1 + clampi(cvt_x86(u), 0, tr.s1 - 1)];
                    sum0 += fix8((float)(w & 255)), sum1 += fix8((float)((w >> 8) & 255)), sum2 += fix8((float)((w >> 16) & 255));
                    continue;
                }
                int xa, xb, ya, yb;
                float fu, fv;
                tap_axis(u, tr.s1, xa, xb, fu);
                tap_axis(v, tr.s2, ya, yb, fv);
                const uint32_t w00 = T[ya * tr.s1 + xa], w01 = T[ya * tr.s1 + xb], w10 = T[yb * tr.s1 + xa],
                               w11 = T[yb * tr.s1 + xb];
#define FMGI_CH(sh)                                                                                        \
    fix8(lerp2(fv, lerp2(fu, (float)((w00 >> sh) & 255), (float)((w01 >> sh) & 255)),                    \
               lerp2(fu, (float)((w10 >> sh) & 255), (float)((w11 >> sh) & 255))))
                sum0 += FMGI_CH(0), sum1 += FMGI_CH(8), sum2 += FMGI_CH(16);
#undef FMGI_CH
            }
        }
        const int64_t o = ((int64_t)c * a.height + y) * a.width + x;
        if (colour) {
            const int half = 128 * S * S, den = 256 * S * S;
            uint8_t *p = a.rgb_out + 3 * o;
            p[0] = (uint8_t)((sum0 + half) / den);
            p[1] = (uint8_t)((sum1 + half) / den);
            p[2] = (uint8_t)((sum2 + half) / den);
        }
        if (s.cov_out) s.cov_out[o] = (uint8_t)cov;
    }
    const unsigned long long n = wave_sum(tests);
    if (lane == 0 && n) atomicAdd(a.tests, n);
}

/* sample n of camera c, pixel (y, x): its record's index in [c][n][y][x] */
__device__ __forceinline__ int64_t record_index(int c, int spp, int n, int height, int width, int y, int x) {
    return (((int64_t)c * spp + n) * height + y) * width + x;
}

/*
 * k_view_shade's rays without its colours (fmgi_view_cache_create): the same pixel mapping, sample loop and
 * walk, so the candidate index stays wave-uniform; every sample's taps go to its record (fmgi_view.h) and
 * nothing is shaded. tests and hits are counted per lane, one atomic per wave each.
 */
__global__ __launch_bounds__(256) void k_view_trace(TraceArgs t) {
    const ShadeArgs &s = t.s;
    const ViewArgs &a = s.v;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = s.x0 + (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = s.y0 + (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    unsigned long long tests = 0, hits = 0;
    if (x < s.x1 && y < s.y1) {
        const ViewCam V = a.cams[c];
        const v3 cam = mk(V.px, V.py, V.pz);
        const unsigned long long *keys = a.keys + (size_t)c * a.sort_n;
        const int C = a.counts[c], S = s.samples;
        const bool bilinear = s.filter != 0;
        const float px = (float)(x - a.width / 2), py = (float)(y - a.height / 2);
        for (int j = 0; j < S; j++) {
            const float fy = -V.pixel * (py + s.offs[j]);
            for (int i = 0; i < S; i++) {
                const float fx = V.pixel * (px + s.offs[i]);
                const v3 dir = view_dir(V, cam, fx, fy);
                float dist;
                const int target = view_walk(a, keys, C, cam, dir, dist, tests);
                const int64_t o = record_index(c, S * S, j * S + i, a.height, a.width, y, x);
                uint4 rec = make_uint4(FMGI_VIEW_MISS, 0u, 0u, 0u);
                if (target >= 0) {
                    hits++;
                    const RadRect tr = a.rects[target];
                    float u, v;
                    view_uv(a.hits[target], tr, cam, dir, dist, u, v);
                    const uint32_t first = (uint32_t)a.first_tile[target];
                    if (!bilinear) {
                        rec.x = first + (uint32_t)(clampi(cvt_x86(v), 0, tr.s2 - 1) * tr.s1 + clampi(cvt_x86(u), 0, tr.s1 - 1));
                    } else {
                        int xa, xb, ya, yb;
                        float fu, fv;
                        tap_axis(u, tr.s1, xa, xb, fu);
                        tap_axis(v, tr.s2, ya, yb, fv);
                        rec.x = (first + (uint32_t)(ya * tr.s1 + xa)) | ((uint32_t)(xb != xa) << 31);
                        rec.y = first + (uint32_t)(yb * tr.s1 + xa);
                        rec.z = __float_as_uint(fu);
                        rec.w = __float_as_uint(fv);
                    }
                }
                if (bilinear) ((uint4 *)t.records)[o] = rec;
                else ((uint32_t *)t.records)[o] = rec.x;
            }
        }
    }
    const unsigned long long n = wave_sum(tests), h = wave_sum(hits);
    if (lane == 0 && n) atomicAdd(a.tests, n);
    if (lane == 0 && h) atomicAdd(t.hits, h);
}

/* k_view_trace for the two projections: k_view_shade_proj's rays, k_view_trace's records */
template <int P>
__global__ __launch_bounds__(256) void k_view_trace_proj(TraceProjArgs q) {
    const TraceArgs &t = q.t;
    const ShadeArgs &s = t.s;
    const ViewArgs &a = s.v;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = s.x0 + (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = s.y0 + (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    __shared__ PhiTable phis; /* EQUIRECT only */
    unsigned long long tests = 0, hits = 0;
    if (x < s.x1 && y < s.y1) {
        const ViewCam V = a.cams[c];
        const v3 cam = mk(V.px, V.py, V.pz), f = mk(V.dx, V.dy, V.dz);
        const unsigned long long *keys = a.keys + (size_t)c * a.sort_n;
        const int C = a.counts[c], S = s.samples;
        const bool bilinear = s.filter != 0;
        const float px = (float)(x - a.width / 2), py = (float)(y - a.height / 2);
        if constexpr (P == FMGI_VIEW_EQUIRECT) phi_table(phis, tid, x, S, s.offs, q.kphi);
        for (int j = 0; j < S; j++) {
            float fy = 0.0f, st = 0.0f, ct = 0.0f;
            if constexpr (P == FMGI_VIEW_ORTHO) fy = -V.pixel * (py + s.offs[j]);
            else fmgi_sincosf(((float)y + (0.5f + s.offs[j])) * q.ktheta, &st, &ct);
            for (int i = 0; i < S; i++) {
                v3 src = cam, dir = f;
                if constexpr (P == FMGI_VIEW_ORTHO) src = ortho_origin(V, cam, V.pixel * (px + s.offs[i]), fy);
                else dir = equirect_dir(V, phis.sc[i][tid].x, phis.sc[i][tid].y, st, ct);
                float dist;
                const int target = view_walk(a, keys, C, src, dir, dist, tests);
                const int64_t o = record_index(c, S * S, j * S + i, a.height, a.width, y, x);
                uint4 rec = make_uint4(FMGI_VIEW_MISS, 0u, 0u, 0u);
                if (target >= 0) {
                    hits++;
                    const RadRect tr = a.rects[target];
                    float u, v;
                    view_uv(a.hits[target], tr, src, dir, dist, u, v);
                    const uint32_t first = (uint32_t)a.first_tile[target];
                    if (!bilinear) {
                        rec.x = first + (uint32_t)(clampi(cvt_x86(v), 0, tr.s2 - 1) * tr.s1 + clampi(cvt_x86(u), 0, tr.s1 - 1));
                    } else {
                        int xa, xb, ya, yb;
                        float fu, fv;
                        tap_axis(u, tr.s1, xa, xb, fu);
                        tap_axis(v, tr.s2, ya, yb, fv);
                        rec.x = (first + (uint32_t)(ya * tr.s1 + xa)) | ((uint32_t)(xb != xa) << 31);
                        rec.y = first + (uint32_t)(yb * tr.s1 + xa);
                        rec.z = __float_as_uint(fu);
                        rec.w = __float_as_uint(fv);
                    }
                }
                if (bilinear) ((uint4 *)t.records)[o] = rec;
                else ((uint32_t *)t.records)[o] = rec.x;
            }
        }
    }
    const unsigned long long n = wave_sum(tests), h = wave_sum(hits);
    if (lane == 0 && n) atomicAdd(a.tests, n);
    if (lane == 0 && h) atomicAdd(t.hits, h);
}

/*
 * The gather (fmgi_view_cache_shade): one lane per pixel, k_view_shade's pixel mapping over the whole image. Per
 * sample the record is read once and every tile set of the pass gathers its tap words (4 B each, served by L2)
 * and adds k_view_shade's fixed-point colour to its own integer sums. The loop over the sets is unrolled with a
 * uniform guard, so the sums stay in registers.
 */
template <bool BILINEAR>
__global__ __launch_bounds__(256) void k_view_resolve(ResolveArgs r) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    if (x >= r.width || y >= r.height) return;
    const int spp = r.samples * r.samples;
    const int bg0 = fix8((float)(r.background & 255)), bg1 = fix8((float)((r.background >> 8) & 255)),
              bg2 = fix8((float)((r.background >> 16) & 255));
    int sum0[FMGI_VIEW_SETS], sum1[FMGI_VIEW_SETS], sum2[FMGI_VIEW_SETS], cov = 0;
#pragma unroll
    for (int k = 0; k < FMGI_VIEW_SETS; k++) sum0[k] = sum1[k] = sum2[k] = 0;
    for (int n = 0; n < spp; n++) {
        const int64_t o = record_index(c, spp, n, r.height, r.width, y, x);
        if constexpr (BILINEAR) {
            /* a native vector, so that the record stays one 16-byte load */
            typedef uint32_t rec4 __attribute__((ext_vector_type(4)));
            const rec4 rec = ((const rec4 *)r.records)[o];
            const bool hit = rec.x != FMGI_VIEW_MISS;
            cov += hit;
            const uint32_t t00 = rec.x & 0x7FFFFFFFu, dx = rec.x >> 31, t10 = rec.y;
            const float fu = __uint_as_float(rec.z), fv = __uint_as_float(rec.w);
#pragma unroll
            for (int k = 0; k < FMGI_VIEW_SETS; k++) {
                if (k >= r.nsets) break;
                if (!hit) {
                    sum0[k] += bg0, sum1[k] += bg1, sum2[k] += bg2;
                    continue;
                }
                const uint32_t *T = r.tiles[k];
                const uint32_t w00 = T[t00], w01 = T[t00 + dx], w10 = T[t10], w11 = T[t10 + dx];
#define FMGI_CH(sh)                                                                                        \
    fix8(lerp2(fv, lerp2(fu, (float)((w00 >> sh) & 255), (float)((w01 >> sh) & 255)),                    \
               lerp2(fu, (float)((w10 >> sh) & 255), (float)((w11 >> sh) & 255))))
                sum0[k] += FMGI_CH(0), sum1[k] += FMGI_CH(8), sum2[k] += FMGI_CH(16);
#undef FMGI_CH
            }
        } else {
            const uint32_t rec = ((const uint32_t *)r.records)[o];
            const bool hit = rec != FMGI_VIEW_MISS;
            cov += hit;
#pragma unroll
            for (int k = 0; k < FMGI_VIEW_SETS; k++) {
                if (k >= r.nsets) break;
                if (!hit) {
                    sum0[k] += bg0, sum1[k] += bg1, sum2[k] += bg2;
                    continue;
                }
                const uint32_t w = r.tiles[k][rec];
                sum0[k] += fix8((float)(w & 255)), sum1[k] += fix8((float)((w >> 8) & 255)), sum2[k] += fix8((float)((w >> 16) & 255));
            }
        }
    }
    const int64_t o = ((int64_t)c * r.height + y) * r.width + x;
    const int half = 128 * spp, den = 256 * spp;
#pragma unroll
    for (int k = 0; k < FMGI_VIEW_SETS; k++) {
        if (k >= r.nsets) break;
        uint8_t *q = r.rgb[k] + 3 * o;
        q[0] = (uint8_t)((sum0[k] + half) / den);
        q[1] = (uint8_t)((sum1[k] + half) / den);
        q[2] = (uint8_t)((sum2[k] + half) / den);
    }
    if (r.cov_out) r.cov_out[o] = (uint8_t)cov;
}

/*
 * The glossy floor. view_walk over the mirror list, the lower bound moved to the camera position:
 * base = |Q - camPos|, so base + best is the length of the path camera -> floor -> hit, and no wall is nearer to
 * the camera than its key. The lanes of a wave that mirror enter together at entry 0, so the entry's index is
 * uniform over the lanes still walking and keys and rectangles are read once per wave; Q, d2, base and best are
 * the lane's own. The loop ends after the N walls of the list at the latest.
 */
__device__ __forceinline__ int view_walk_mirror(const ViewArgs &a, const unsigned long long *mkeys, int N, v3 Q, v3 d2,
                                                float base, float &best, unsigned long long &tests) {
    best = INFINITY;
    int wall2 = -1;
    for (int i = 0; i < N; i++) {
        const unsigned long long key = mkeys[i];
        const float md = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32)));
        if ((base + best) < md) break;
        const int idx = __builtin_amdgcn_readfirstlane((int)(uint32_t)key);
        tests++;
        const float dn = rect_intersects(a.hits[idx], Q, d2, best);
        if (dn < 0) continue;
        if (dn <= best) {
            wall2 = idx;
            best = dn;
        }
    }
    return wall2;
}

/* does the sample that hit at P mirror: the bake's test (k_bake, photonmap.cl:236), whatever the wall */
__device__ __forceinline__ bool mirrors(v3 P) { return !(P.z > FMGI_VIEW_MIRROR_Z); }

/* the mirror ray of a hit at P on wall t (photonmap.cl:253, :261; d2 keeps its length) and its walk */
__device__ __forceinline__ int mirror_walk(const ViewArgs &a, const unsigned long long *mkeys, v3 cam, const AoRect &t, v3 P,
                                           v3 dir, v3 &Q, v3 &d2, float &best, unsigned long long &tests) {
    const v3 n = mk(t.nx, t.ny, t.nz);
    const float two = 2.0f * dot(n, dir);
    d2 = sub(dir, mul(n, two));
    Q = add(P, mul(d2, 1e-5f));
    return view_walk_mirror(a, mkeys, a.nrects, Q, d2, len3(sub(Q, cam)), best, tests);
}

/* sample (j, i)'s ray of pixel (px, py): the pin-hole's, k_view_shade_proj's ORTHO and EQUIRECT */
template <int P>
__device__ __forceinline__ void sample_ray(const ViewCam &V, v3 cam, float fx, float fy, float2 phi, float st, float ct,
                                           v3 &src, v3 &dir) {
    src = cam;
    if constexpr (P == FMGI_VIEW_PINHOLE) {
        dir = view_dir(V, cam, fx, fy);
    } else if constexpr (P == FMGI_VIEW_ORTHO) {
        src = ortho_origin(V, cam, fx, fy);
        dir = mk(V.dx, V.dy, V.dz);
    } else {
        dir = equirect_dir(V, phi.x, phi.y, st, ct);
    }
}

/* a hit's colour as k_view_shade taps it, before fix8 */
__device__ __forceinline__ void tap_colour(const uint32_t *T, const RadRect &tr, float u, float v, bool bilinear, float &c0,
                                           float &c1, float &c2) {
    if (!bilinear) {
        const uint32_t w = T[clampi(cvt_x86(v), 0, tr.s2 - 1) * tr.s1 + clampi(cvt_x86(u), 0, tr.s1 - 1)];
        c0 = (float)(w & 255), c1 = (float)((w >> 8) & 255), c2 = (float)((w >> 16) & 255);
        return;
    }
    int xa, xb, ya, yb;
    float fu, fv;
    tap_axis(u, tr.s1, xa, xb, fu);
    tap_axis(v, tr.s2, ya, yb, fv);
    const uint32_t w00 = T[ya * tr.s1 + xa], w01 = T[ya * tr.s1 + xb], w10 = T[yb * tr.s1 + xa], w11 = T[yb * tr.s1 + xb];
#define FMGI_CH(sh)                                                                                        \
    lerp2(fv, lerp2(fu, (float)((w00 >> sh) & 255), (float)((w01 >> sh) & 255)),                         \
          lerp2(fu, (float)((w10 >> sh) & 255), (float)((w11 >> sh) & 255)))
    c0 = FMGI_CH(0), c1 = FMGI_CH(8), c2 = FMGI_CH(16);
#undef FMGI_CH
}

/* a hit's record as k_view_trace writes it */
__device__ __forceinline__ uint4 tap_record(uint32_t first, const RadRect &tr, float u, float v, bool bilinear) {
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (!bilinear) {
        rec.x = first + (uint32_t)(clampi(cvt_x86(v), 0, tr.s2 - 1) * tr.s1 + clampi(cvt_x86(u), 0, tr.s1 - 1));
    } else {
        int xa, xb, ya, yb;
        float fu, fv;
        tap_axis(u, tr.s1, xa, xb, fu);
        tap_axis(v, tr.s2, ya, yb, fv);
        rec.x = (first + (uint32_t)(ya * tr.s1 + xa)) | ((uint32_t)(xb != xa) << 31);
        rec.y = first + (uint32_t)(yb * tr.s1 + xa);
        rec.z = __float_as_uint(fu);
        rec.w = __float_as_uint(fv);
    }
    return rec;
}

/*
 * k_view_shade / k_view_shade_proj with the mirror bounce: the same pixel mapping, sample loop, primary walk and
 * taps. A sample that hit and mirrors walks the mirror list inside one branch after the primary walk, taps the
 * wall its mirror ray hit (or takes the background) and blends the two colours before fix8. The second walk runs
 * whether or not a picture is asked for, so that the counts do not depend on the outputs.
 */
template <int P>
__global__ __launch_bounds__(256) void k_view_shade_gloss(ShadeGlossArgs ga) {
    const ShadeProjArgs &q = ga.q;
    const ShadeArgs &s = q.s;
    const ViewArgs &a = s.v;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = s.x0 + (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = s.y0 + (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    __shared__ PhiTable phis; /* EQUIRECT only */
    unsigned long long tests = 0, mtests = 0;
    unsigned int mrays = 0, mhits = 0;
    if (x < s.x1 && y < s.y1) {
        const ViewCam V = a.cams[c];
        const v3 cam = mk(V.px, V.py, V.pz);
        const unsigned long long *keys = a.keys + (size_t)c * a.sort_n, *mkeys = ga.g.mkeys + (size_t)c * a.sort_n;
        const int C = a.counts[c], S = s.samples;
        const bool colour = a.rgb_out != nullptr, bilinear = s.filter != 0;
        const float gloss = ga.g.gloss;
        const float px = (float)(x - a.width / 2), py = (float)(y - a.height / 2);
        const float b0 = (float)(a.background & 255), b1 = (float)((a.background >> 8) & 255),
                    b2 = (float)((a.background >> 16) & 255);
        const int bg0 = fix8(b0), bg1 = fix8(b1), bg2 = fix8(b2);
        if constexpr (P == FMGI_VIEW_EQUIRECT) phi_table(phis, tid, x, S, s.offs, q.kphi);
        int sum0 = 0, sum1 = 0, sum2 = 0, cov = 0;
        for (int j = 0; j < S; j++) {
            float fy = 0.0f, st = 0.0f, ct = 0.0f;
            if constexpr (P == FMGI_VIEW_EQUIRECT) fmgi_sincosf(((float)y + (0.5f + s.offs[j])) * q.ktheta, &st, &ct);
            else fy = -V.pixel * (py + s.offs[j]);
            for (int i = 0; i < S; i++) {
                float fx = 0.0f;
                float2 phi = make_float2(0.0f, 0.0f);
                if constexpr (P == FMGI_VIEW_EQUIRECT) phi = phis.sc[i][tid];
                else fx = V.pixel * (px + s.offs[i]);
                v3 src, dir;
                sample_ray<P>(V, cam, fx, fy, phi, st, ct, src, dir);
                float dist;
                const int target = view_walk(a, keys, C, src, dir, dist, tests);
                if (target < 0) {
                    sum0 += bg0, sum1 += bg1, sum2 += bg2;
                    continue;
                }
                cov++;
                float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
                if (colour) {
                    const RadRect tr = a.rects[target];
                    float u, v;
                    view_uv(a.hits[target], tr, src, dir, dist, u, v);
                    tap_colour(s.tiles + a.first_tile[target], tr, u, v, bilinear, v0, v1, v2);
                }
                const v3 Pt = add(src, mul(dir, dist));
                if (mirrors(Pt)) {
                    v3 Q, d2;
                    float best;
                    const int wall2 = mirror_walk(a, mkeys, cam, a.hits[target], Pt, dir, Q, d2, best, mtests);
                    mrays++;
                    float m0 = b0, m1 = b1, m2 = b2;
                    if (wall2 >= 0) {
                        mhits++;
                        if (colour) {
                            const RadRect tr = a.rects[wall2];
                            float u, v;
                            view_uv(a.hits[wall2], tr, Q, d2, best, u, v);
                            tap_colour(s.tiles + a.first_tile[wall2], tr, u, v, bilinear, m0, m1, m2);
                        }
                    }
                    v0 = lerp2(gloss, v0, m0), v1 = lerp2(gloss, v1, m1), v2 = lerp2(gloss, v2, m2);
                }
                sum0 += fix8(v0), sum1 += fix8(v1), sum2 += fix8(v2);
            }
        }
        const int64_t o = ((int64_t)c * a.height + y) * a.width + x;
        if (colour) {
            const int half = 128 * S * S, den = 256 * S * S;
            uint8_t *p = a.rgb_out + 3 * o;
            p[0] = (uint8_t)((sum0 + half) / den);
            p[1] = (uint8_t)((sum1 + half) / den);
            p[2] = (uint8_t)((sum2 + half) / den);
        }
        if (s.cov_out) s.cov_out[o] = (uint8_t)cov;
    }
    /* a.tests counts both walks; the three counters are the mirror rays' own */
    const unsigned long long mt = wave_sum(mtests), n = wave_sum(tests) + mt,
                             rh = wave_sum(((unsigned long long)mrays << 32) | mhits);
    if (lane == 0 && n) atomicAdd(a.tests, n);
    if (lane == 0 && rh) {
        atomicAdd(ga.g.counters, rh >> 32);
        if (rh & 0xFFFFFFFFull) atomicAdd(ga.g.counters + 1, rh & 0xFFFFFFFFull);
        if (mt) atomicAdd(ga.g.counters + 2, mt);
    }
}

/*
 * k_view_trace / k_view_trace_proj with the mirror bounce: the primary records as they write them and, at the same
 * index of a second plane, a mirror record per sample: tap_record of the wall the mirror ray hit, FMGI_VIEW_MISS
 * if it hit nothing, FMGI_VIEW_NO_MIRROR for a sample that does not mirror. Nothing here depends on gloss.
 */
template <int P>
__global__ __launch_bounds__(256) void k_view_trace_gloss(TraceGlossArgs ga) {
    const TraceProjArgs &q = ga.q;
    const TraceArgs &t = q.t;
    const ShadeArgs &s = t.s;
    const ViewArgs &a = s.v;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = s.x0 + (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = s.y0 + (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    __shared__ PhiTable phis; /* EQUIRECT only */
    unsigned long long tests = 0, mtests = 0, hits = 0;
    unsigned int mrays = 0, mhits = 0;
    if (x < s.x1 && y < s.y1) {
        const ViewCam V = a.cams[c];
        const v3 cam = mk(V.px, V.py, V.pz);
        const unsigned long long *keys = a.keys + (size_t)c * a.sort_n, *mkeys = ga.g.mkeys + (size_t)c * a.sort_n;
        const int C = a.counts[c], S = s.samples;
        const bool bilinear = s.filter != 0;
        const float px = (float)(x - a.width / 2), py = (float)(y - a.height / 2);
        if constexpr (P == FMGI_VIEW_EQUIRECT) phi_table(phis, tid, x, S, s.offs, q.kphi);
        for (int j = 0; j < S; j++) {
            float fy = 0.0f, st = 0.0f, ct = 0.0f;
            if constexpr (P == FMGI_VIEW_EQUIRECT) fmgi_sincosf(((float)y + (0.5f + s.offs[j])) * q.ktheta, &st, &ct);
            else fy = -V.pixel * (py + s.offs[j]);
            for (int i = 0; i < S; i++) {
                float fx = 0.0f;
                float2 phi = make_float2(0.0f, 0.0f);
                if constexpr (P == FMGI_VIEW_EQUIRECT) phi = phis.sc[i][tid];
                else fx = V.pixel * (px + s.offs[i]);
                v3 src, dir;
                sample_ray<P>(V, cam, fx, fy, phi, st, ct, src, dir);
                float dist;
                const int target = view_walk(a, keys, C, src, dir, dist, tests);
                const int64_t o = record_index(c, S * S, j * S + i, a.height, a.width, y, x);
                uint4 rec = make_uint4(FMGI_VIEW_MISS, 0u, 0u, 0u), mrec = make_uint4(FMGI_VIEW_NO_MIRROR, 0u, 0u, 0u);
                if (target >= 0) {
                    hits++;
                    const RadRect tr = a.rects[target];
                    float u, v;
                    view_uv(a.hits[target], tr, src, dir, dist, u, v);
                    rec = tap_record((uint32_t)a.first_tile[target], tr, u, v, bilinear);
                    const v3 Pt = add(src, mul(dir, dist));
                    if (mirrors(Pt)) {
                        v3 Q, d2;
                        float best;
                        const int wall2 = mirror_walk(a, mkeys, cam, a.hits[target], Pt, dir, Q, d2, best, mtests);
                        mrays++;
                        mrec.x = FMGI_VIEW_MISS;
                        if (wall2 >= 0) {
                            mhits++;
                            const RadRect mr = a.rects[wall2];
                            view_uv(a.hits[wall2], mr, Q, d2, best, u, v);
                            mrec = tap_record((uint32_t)a.first_tile[wall2], mr, u, v, bilinear);
                        }
                    }
                }
                if (bilinear) {
                    ((uint4 *)t.records)[o] = rec;
                    ((uint4 *)ga.mrecords)[o] = mrec;
                } else {
                    ((uint32_t *)t.records)[o] = rec.x;
                    ((uint32_t *)ga.mrecords)[o] = mrec.x;
                }
            }
        }
    }
    const unsigned long long mt = wave_sum(mtests), n = wave_sum(tests) + mt, h = wave_sum(hits),
                             rh = wave_sum(((unsigned long long)mrays << 32) | mhits);
    if (lane == 0 && n) atomicAdd(a.tests, n);
    if (lane == 0 && h) atomicAdd(t.hits, h);
    if (lane == 0 && rh) {
        atomicAdd(ga.g.counters, rh >> 32);
        if (rh & 0xFFFFFFFFull) atomicAdd(ga.g.counters + 1, rh & 0xFFFFFFFFull);
        if (mt) atomicAdd(ga.g.counters + 2, mt);
    }
}

/* a record's colour from one tile set, before fix8: k_view_resolve's gather */
template <bool BILINEAR>
__device__ __forceinline__ void record_colour(const uint32_t *T, uint32_t t00, uint32_t dx, uint32_t t10, float fu, float fv,
                                              float &c0, float &c1, float &c2) {
    if constexpr (BILINEAR) {
        const uint32_t w00 = T[t00], w01 = T[t00 + dx], w10 = T[t10], w11 = T[t10 + dx];
#define FMGI_CH(sh)                                                                                        \
    lerp2(fv, lerp2(fu, (float)((w00 >> sh) & 255), (float)((w01 >> sh) & 255)),                         \
          lerp2(fu, (float)((w10 >> sh) & 255), (float)((w11 >> sh) & 255)))
        c0 = FMGI_CH(0), c1 = FMGI_CH(8), c2 = FMGI_CH(16);
#undef FMGI_CH
    } else {
        const uint32_t w = T[t00];
        c0 = (float)(w & 255), c1 = (float)((w >> 8) & 255), c2 = (float)((w >> 16) & 255);
    }
}

/*
 * k_view_resolve with the mirror records: per sample both records are read once, every tile set gathers the
 * primary colour and, for a sample that mirrors, the mirror colour (or the background), blends them with gloss
 * and adds k_view_shade_gloss's fixed-point colour to its sums.
 */
template <bool BILINEAR>
__global__ __launch_bounds__(256) void k_view_resolve_gloss(ResolveGlossArgs ga) {
    const ResolveArgs &r = ga.r;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = (int)blockIdx.x * FMGI_VIEW_BLOCK + (wave & 1) * FMGI_VIEW_TILE + (lane & (FMGI_VIEW_TILE - 1));
    const int y = (int)blockIdx.y * FMGI_VIEW_BLOCK + (wave >> 1) * FMGI_VIEW_TILE + lane / FMGI_VIEW_TILE;
    const int c = blockIdx.z;
    if (x >= r.width || y >= r.height) return;
    const int spp = r.samples * r.samples;
    const float gloss = ga.gloss;
    const float b0 = (float)(r.background & 255), b1 = (float)((r.background >> 8) & 255),
                b2 = (float)((r.background >> 16) & 255);
    const int bg0 = fix8(b0), bg1 = fix8(b1), bg2 = fix8(b2);
    int sum0[FMGI_VIEW_SETS], sum1[FMGI_VIEW_SETS], sum2[FMGI_VIEW_SETS], cov = 0;
#pragma unroll
    for (int k = 0; k < FMGI_VIEW_SETS; k++) sum0[k] = sum1[k] = sum2[k] = 0;
    for (int n = 0; n < spp; n++) {
        const int64_t o = record_index(c, spp, n, r.height, r.width, y, x);
        typedef uint32_t rec4 __attribute__((ext_vector_type(4)));
        rec4 rec = {0u, 0u, 0u, 0u}, mrec = {0u, 0u, 0u, 0u};
        if constexpr (BILINEAR) {
            rec = ((const rec4 *)r.records)[o];
            mrec = ((const rec4 *)ga.mrecords)[o];
        } else {
            rec.x = ((const uint32_t *)r.records)[o];
            mrec.x = ((const uint32_t *)ga.mrecords)[o];
        }
        const bool hit = rec.x != FMGI_VIEW_MISS, mirror = mrec.x != FMGI_VIEW_NO_MIRROR, mhit = mrec.x != FMGI_VIEW_MISS;
        cov += hit;
        const uint32_t t00 = BILINEAR ? rec.x & 0x7FFFFFFFu : rec.x, dx = BILINEAR ? rec.x >> 31 : 0u, t10 = rec.y;
        const uint32_t m00 = BILINEAR ? mrec.x & 0x7FFFFFFFu : mrec.x, mdx = BILINEAR ? mrec.x >> 31 : 0u, m10 = mrec.y;
        const float fu = __uint_as_float(rec.z), fv = __uint_as_float(rec.w);
        const float mfu = __uint_as_float(mrec.z), mfv = __uint_as_float(mrec.w);
#pragma unroll
        for (int k = 0; k < FMGI_VIEW_SETS; k++) {
            if (k >= r.nsets) break;
            if (!hit) {
                sum0[k] += bg0, sum1[k] += bg1, sum2[k] += bg2;
                continue;
            }
            float v0, v1, v2;
            record_colour<BILINEAR>(r.tiles[k], t00, dx, t10, fu, fv, v0, v1, v2);
            if (mirror) {
                float m0 = b0, m1 = b1, m2 = b2;
                if (mhit) record_colour<BILINEAR>(r.tiles[k], m00, mdx, m10, mfu, mfv, m0, m1, m2);
                v0 = lerp2(gloss, v0, m0), v1 = lerp2(gloss, v1, m1), v2 = lerp2(gloss, v2, m2);
            }
            sum0[k] += fix8(v0), sum1[k] += fix8(v1), sum2[k] += fix8(v2);
        }
    }
    const int64_t o = ((int64_t)c * r.height + y) * r.width + x;
    const int half = 128 * spp, den = 256 * spp;
#pragma unroll
    for (int k = 0; k < FMGI_VIEW_SETS; k++) {
        if (k >= r.nsets) break;
        uint8_t *q = r.rgb[k] + 3 * o;
        q[0] = (uint8_t)((sum0[k] + half) / den);
        q[1] = (uint8_t)((sum1[k] + half) / den);
        q[2] = (uint8_t)((sum2[k] + half) / den);
    }
    if (r.cov_out) r.cov_out[o] = (uint8_t)cov;
}

bool bad_sort(const ViewArgs &a) {
    return a.sort_n < 2 || a.sort_n > FMGI_RAD_MAX_SORT || (a.sort_n & (a.sort_n - 1)) || a.nrects > a.sort_n;
}

} // namespace

hipError_t fmgi_view_launch_candidates(const ViewArgs &a, hipStream_t s) {
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a)) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.sort_n * 8;
    hipError_t e = fmgi_set_lds_attr_once<7>((const void *)k_view_candidates, FMGI_RAD_MAX_SORT * 8);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_view_candidates, dim3((unsigned)a.ncams), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_rays(const ViewArgs &a, hipStream_t s) {
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a) || a.ncams > FMGI_VIEW_MAX_BATCH || a.width < 1 || a.height < 1 ||
        a.width > FMGI_VIEW_MAX_DIM || a.height > FMGI_VIEW_MAX_DIM || (a.rgb_out && (!a.tiles_rgb || !a.first_tile)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.width + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((a.height + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)a.ncams);
    hipLaunchKernelGGL(k_view_rays, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_pack(const uint8_t *tiles_rgb, uint32_t *tiles, int64_t ntiles, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    if (!tiles_rgb || !tiles || ntiles > (int64_t)0x7FFFFFFF * 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_view_pack, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, s, tiles_rgb, tiles, ntiles);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_shade(const ShadeArgs &s, hipStream_t st) {
    const ViewArgs &a = s.v;
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a) || a.ncams > FMGI_VIEW_MAX_BATCH || a.width < 1 || a.height < 1 ||
        a.width > FMGI_VIEW_MAX_DIM || a.height > FMGI_VIEW_MAX_DIM || (a.rgb_out && (!s.tiles || !a.first_tile)) ||
        s.samples < 1 || s.samples > FMGI_VIEW_SAMPLES || (s.filter != 0 && s.filter != 1) || s.x0 < 0 || s.y0 < 0 ||
        s.x1 <= s.x0 || s.y1 <= s.y0 || s.x1 > a.width || s.y1 > a.height)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((s.x1 - s.x0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((s.y1 - s.y0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)a.ncams);
    hipLaunchKernelGGL(k_view_shade, grid, dim3(256), 0, st, s);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_trace(const TraceArgs &t, hipStream_t st) {
    const ShadeArgs &s = t.s;
    const ViewArgs &a = s.v;
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a) || a.ncams > FMGI_VIEW_MAX_BATCH || a.width < 1 || a.height < 1 ||
        a.width > FMGI_VIEW_MAX_DIM || a.height > FMGI_VIEW_MAX_DIM || !a.first_tile || !t.records || !t.hits ||
        s.samples < 1 || s.samples > FMGI_VIEW_SAMPLES || (s.filter != 0 && s.filter != 1) || s.x0 < 0 || s.y0 < 0 ||
        s.x1 <= s.x0 || s.y1 <= s.y0 || s.x1 > a.width || s.y1 > a.height)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((s.x1 - s.x0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((s.y1 - s.y0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)a.ncams);
    hipLaunchKernelGGL(k_view_trace, grid, dim3(256), 0, st, t);
    return hipGetLastError();
}

static bool bad_proj(int projection) { return projection != FMGI_VIEW_ORTHO && projection != FMGI_VIEW_EQUIRECT; }

hipError_t fmgi_view_launch_candidates_proj(const ViewArgs &a, int projection, hipStream_t s) {
    if (bad_proj(projection)) return hipErrorInvalidValue;
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a)) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.sort_n * 8;
    if (projection == FMGI_VIEW_ORTHO) {
        hipError_t e = fmgi_set_lds_attr_once<8>((const void *)k_view_candidates_proj<FMGI_VIEW_ORTHO>, FMGI_RAD_MAX_SORT * 8);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_view_candidates_proj<FMGI_VIEW_ORTHO>, dim3((unsigned)a.ncams), dim3(256), lds, s, a);
    } else {
        hipError_t e = fmgi_set_lds_attr_once<9>((const void *)k_view_candidates_proj<FMGI_VIEW_EQUIRECT>, FMGI_RAD_MAX_SORT * 8);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_view_candidates_proj<FMGI_VIEW_EQUIRECT>, dim3((unsigned)a.ncams), dim3(256), lds, s, a);
    }
    return hipGetLastError();
}

hipError_t fmgi_view_launch_shade_proj(const ShadeProjArgs &q, int projection, hipStream_t st) {
    const ShadeArgs &s = q.s;
    const ViewArgs &a = s.v;
    if (bad_proj(projection)) return hipErrorInvalidValue;
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a) || a.ncams > FMGI_VIEW_MAX_BATCH || a.width < 1 || a.height < 1 ||
        a.width > FMGI_VIEW_MAX_DIM || a.height > FMGI_VIEW_MAX_DIM || (a.rgb_out && (!s.tiles || !a.first_tile)) ||
        s.samples < 1 || s.samples > FMGI_VIEW_SAMPLES || (s.filter != 0 && s.filter != 1) || s.x0 < 0 || s.y0 < 0 ||
        s.x1 <= s.x0 || s.y1 <= s.y0 || s.x1 > a.width || s.y1 > a.height)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((s.x1 - s.x0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((s.y1 - s.y0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)a.ncams);
    if (projection == FMGI_VIEW_ORTHO) hipLaunchKernelGGL(k_view_shade_proj<FMGI_VIEW_ORTHO>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(k_view_shade_proj<FMGI_VIEW_EQUIRECT>, grid, dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_trace_proj(const TraceProjArgs &q, int projection, hipStream_t st) {
    const TraceArgs &t = q.t;
    const ShadeArgs &s = t.s;
    const ViewArgs &a = s.v;
    if (bad_proj(projection)) return hipErrorInvalidValue;
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a) || a.ncams > FMGI_VIEW_MAX_BATCH || a.width < 1 || a.height < 1 ||
        a.width > FMGI_VIEW_MAX_DIM || a.height > FMGI_VIEW_MAX_DIM || !a.first_tile || !t.records || !t.hits ||
        s.samples < 1 || s.samples > FMGI_VIEW_SAMPLES || (s.filter != 0 && s.filter != 1) || s.x0 < 0 || s.y0 < 0 ||
        s.x1 <= s.x0 || s.y1 <= s.y0 || s.x1 > a.width || s.y1 > a.height)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((s.x1 - s.x0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((s.y1 - s.y0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)a.ncams);
    if (projection == FMGI_VIEW_ORTHO) hipLaunchKernelGGL(k_view_trace_proj<FMGI_VIEW_ORTHO>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(k_view_trace_proj<FMGI_VIEW_EQUIRECT>, grid, dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_resolve(const ResolveArgs &r, hipStream_t st) {
    if (r.ncams <= 0) return hipSuccess;
    if (r.ncams > FMGI_VIEW_MAX_BATCH || r.width < 1 || r.height < 1 || r.width > FMGI_VIEW_MAX_DIM ||
        r.height > FMGI_VIEW_MAX_DIM || r.samples < 1 || r.samples > FMGI_VIEW_SAMPLES ||
        (r.filter != 0 && r.filter != 1) || !r.records || r.nsets < 1 || r.nsets > FMGI_VIEW_SETS)
        return hipErrorInvalidValue;
    for (int k = 0; k < r.nsets; k++)
        if (!r.tiles[k] || !r.rgb[k]) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((r.width + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((r.height + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)r.ncams);
    if (r.filter) hipLaunchKernelGGL(k_view_resolve<true>, grid, dim3(256), 0, st, r);
    else hipLaunchKernelGGL(k_view_resolve<false>, grid, dim3(256), 0, st, r);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_candidates_mirror(const ViewArgs &a, hipStream_t s) {
    if (a.ncams <= 0) return hipSuccess;
    if (bad_sort(a)) return hipErrorInvalidValue;
    hipError_t e = fmgi_set_lds_attr_once<10>((const void *)k_view_candidates_proj<FMGI_VIEW_MIRROR>, FMGI_RAD_MAX_SORT * 8);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_view_candidates_proj<FMGI_VIEW_MIRROR>, dim3((unsigned)a.ncams), dim3(256), (size_t)a.sort_n * 8, s, a);
    return hipGetLastError();
}

static bool bad_gloss_proj(int projection) {
    return projection != FMGI_VIEW_PINHOLE && projection != FMGI_VIEW_ORTHO && projection != FMGI_VIEW_EQUIRECT;
}

/* what the shade and trace launches check of their windows and shapes */
static bool bad_window(const ShadeArgs &s) {
    const ViewArgs &a = s.v;
    return bad_sort(a) || a.ncams > FMGI_VIEW_MAX_BATCH || a.width < 1 || a.height < 1 || a.width > FMGI_VIEW_MAX_DIM ||
           a.height > FMGI_VIEW_MAX_DIM || s.samples < 1 || s.samples > FMGI_VIEW_SAMPLES || (s.filter != 0 && s.filter != 1) ||
           s.x0 < 0 || s.y0 < 0 || s.x1 <= s.x0 || s.y1 <= s.y0 || s.x1 > a.width || s.y1 > a.height;
}

hipError_t fmgi_view_launch_shade_gloss(const ShadeGlossArgs &g, int projection, hipStream_t st) {
    const ShadeArgs &s = g.q.s;
    const ViewArgs &a = s.v;
    if (bad_gloss_proj(projection)) return hipErrorInvalidValue;
    if (a.ncams <= 0) return hipSuccess;
    if (bad_window(s) || (a.rgb_out && (!s.tiles || !a.first_tile)) || !g.g.mkeys || !g.g.counters || !(g.g.gloss >= 0.0f) ||
        !(g.g.gloss <= 1.0f))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((s.x1 - s.x0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((s.y1 - s.y0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)a.ncams);
    if (projection == FMGI_VIEW_PINHOLE) hipLaunchKernelGGL(k_view_shade_gloss<FMGI_VIEW_PINHOLE>, grid, dim3(256), 0, st, g);
    else if (projection == FMGI_VIEW_ORTHO) hipLaunchKernelGGL(k_view_shade_gloss<FMGI_VIEW_ORTHO>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_view_shade_gloss<FMGI_VIEW_EQUIRECT>, grid, dim3(256), 0, st, g);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_trace_gloss(const TraceGlossArgs &g, int projection, hipStream_t st) {
    const TraceArgs &t = g.q.t;
    const ShadeArgs &s = t.s;
    const ViewArgs &a = s.v;
    if (bad_gloss_proj(projection)) return hipErrorInvalidValue;
    if (a.ncams <= 0) return hipSuccess;
    if (bad_window(s) || !a.first_tile || !t.records || !t.hits || !g.mrecords || !g.g.mkeys || !g.g.counters)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((s.x1 - s.x0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((s.y1 - s.y0 + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)a.ncams);
    if (projection == FMGI_VIEW_PINHOLE) hipLaunchKernelGGL(k_view_trace_gloss<FMGI_VIEW_PINHOLE>, grid, dim3(256), 0, st, g);
    else if (projection == FMGI_VIEW_ORTHO) hipLaunchKernelGGL(k_view_trace_gloss<FMGI_VIEW_ORTHO>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_view_trace_gloss<FMGI_VIEW_EQUIRECT>, grid, dim3(256), 0, st, g);
    return hipGetLastError();
}

hipError_t fmgi_view_launch_resolve_gloss(const ResolveGlossArgs &g, hipStream_t st) {
    const ResolveArgs &r = g.r;
    if (r.ncams <= 0) return hipSuccess;
    if (r.ncams > FMGI_VIEW_MAX_BATCH || r.width < 1 || r.height < 1 || r.width > FMGI_VIEW_MAX_DIM ||
        r.height > FMGI_VIEW_MAX_DIM || r.samples < 1 || r.samples > FMGI_VIEW_SAMPLES ||
        (r.filter != 0 && r.filter != 1) || !r.records || !g.mrecords || r.nsets < 1 || r.nsets > FMGI_VIEW_SETS ||
        !(g.gloss >= 0.0f) || !(g.gloss <= 1.0f))
        return hipErrorInvalidValue;
    for (int k = 0; k < r.nsets; k++)
        if (!r.tiles[k] || !r.rgb[k]) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((r.width + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK),
                    (unsigned)((r.height + FMGI_VIEW_BLOCK - 1) / FMGI_VIEW_BLOCK), (unsigned)r.ncams);
    if (r.filter) hipLaunchKernelGGL(k_view_resolve_gloss<true>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_view_resolve_gloss<false>, grid, dim3(256), 0, st, g);
    return hipGetLastError();
}
