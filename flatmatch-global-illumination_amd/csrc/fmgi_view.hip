/*
 * fmgi_view.hip -- the view renderer's kernels, bit-identical to the reference's debug raycaster
 * (debugRaytracer.cc:121-176 over radiosityNative.c:25-90); see fmgi_view.h for the kernel plan.
 *
 * Arithmetic: IEEE fp32 in the reference's source order (gcc -O2 -msse3, no FMA), contraction off, with
 * the helpers the radiosity backend uses (fmgi_rect_dev.h).
 */
#include <hip/hip_runtime.h>

#include "fmgi_lds_attr.h"
#include "fmgi_view.h"

#pragma clang fp contract(off)

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

/*
 * One lane per pixel; a wave is an 8x8 pixel block, a workgroup 2x2 of them; blockIdx.z is the camera.
 * The candidate index is uniform over the wave's lanes that are still walking (they all started at 0), so
 * keys and rectangles are read once per wave. A lane outside the image does nothing but join the wave's
 * sum of its test counter with a zero.
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
        /* debugRaytracer.cc:154-155: add3 sums left to right */
        const float fx = V.pixel * (float)(x - a.width / 2), fy = -V.pixel * (float)(y - a.height / 2);
        const v3 screen = add(add(mk(V.cx, V.cy, V.cz), mul(mk(V.rx, V.ry, V.rz), fx)), mul(mk(V.ux, V.uy, V.uz), fy));
        const v3 dir = unit(sub(screen, cam));
        /* findClosestIntersectionSorted (radiosityNative.c:67-90), the ray starting at camPos itself */
        const unsigned long long *keys = a.keys + (size_t)c * a.sort_n;
        const int C = a.counts[c];
        float dist = INFINITY;
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
        int sid = -1;
        uint32_t rgb = a.background;
        if (target >= 0) {
            /* getTileIdAt (rectangle.c:205-230) */
            const AoRect t = a.hits[target];
            const RadRect tr = a.rects[target];
            const v3 pd = sub(add(cam, mul(dir, dist)), mk(t.px, t.py, t.pz));
            const float dx = dot(mk(t.wx, t.wy, t.wz), pd), dy = dot(mk(t.hx, t.hy, t.hz), pd);
            const int tx = clampi(cvt_x86(dx * (float)tr.s1 / t.wl), 0, tr.s1 - 1);
            const int ty = clampi(cvt_x86(dy * (float)tr.s2 / t.hl), 0, tr.s2 - 1);
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
