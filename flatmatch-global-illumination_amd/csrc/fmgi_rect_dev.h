/*
 * fmgi_rect_dev.h -- device-side fp32 vector helpers and the ray/rectangle test of the native C
 * backends (vector3_cl.c, rectangle.c:67-95 intersects), shared by the ambient-occlusion (fmgi_ao.hip),
 * radiosity (fmgi_rad.hip) and view (fmgi_view.hip) kernels; the candidate-list helpers (isBehindRay,
 * getShortestDistanceRectToPoint, the x86 cast) serve the last two. Every operation is IEEE fp32 in the reference's source order;
 * the including file turns contraction off (#pragma clang fp contract(off)) before including this.
 */
#ifndef FMGI_RECT_DEV_H
#define FMGI_RECT_DEV_H

#include <hip/hip_runtime.h>

#include "fmgi_ao.h"

namespace fmgi_dev {

struct v3 {
    float x, y, z;
};
__device__ __forceinline__ v3 mk(float x, float y, float z) { return v3{x, y, z}; }
__device__ __forceinline__ v3 add(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 mul(v3 a, float f) { return mk(a.x * f, a.y * f, a.z * f); }
__device__ __forceinline__ float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

/* rectangle.c:67-95 intersects() on an AoRect (normalised edges and lengths precomputed with the same
   IEEE ops as the per-call div_vec3/length): the hit distance, or -1 for no hit */
__device__ __forceinline__ float rect_intersects(const AoRect &r, v3 src, v3 dir, float closest) {
    const v3 n = mk(r.nx, r.ny, r.nz), pos = mk(r.px, r.py, r.pz);
    const float denom = dot(n, dir);
    if (denom >= 0) return -1;
    const float fac = dot(n, sub(pos, src)) / denom;
    if (fac < 0) return -1;
    const v3 ray = mul(dir, fac);
    if (closest * closest < dot(ray, ray)) return -1; /* squaredLength */
    const v3 pdir = sub(add(src, ray), pos);
    const float dx = dot(mk(r.wx, r.wy, r.wz), pdir);
    const float dy = dot(mk(r.hx, r.hy, r.hz), pdir);
    if (dx < 0 || dy < 0 || dx > r.wl || dy > r.hl) return -1;
    return fac;
}

/* rectangle.c:97-113 isBehindRay */
__device__ __forceinline__ bool behind_ray(v3 p, v3 w, v3 h, v3 src, v3 dir) {
    const v3 d1 = sub(p, src), d2 = sub(add(p, w), src), d3 = sub(add(p, h), src), d4 = sub(add(add(p, w), h), src);
    return dot(d1, dir) < 0 && dot(d2, dir) < 0 && dot(d3, dir) < 0 && dot(d4, dir) < 0;
}

__device__ __forceinline__ float len3(v3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ v3 unit(v3 a) { return mul(a, 1.0f / len3(a)); }

/* rectangle.c:442-470 getShortestDistanceRectToPoint */
__device__ __forceinline__ float min_dist(v3 pos, v3 w, v3 h, v3 n, v3 p) {
    const v3 vd = sub(p, pos);
    const v3 on_plane = sub(p, mul(n, dot(vd, n)));
    const v3 pd = sub(on_plane, pos);
    float u = dot(pd, unit(h)) / len3(h);
    float v = dot(pd, unit(w)) / len3(w);
    u = (u < 0) ? 0.0f : ((u > 1) ? 1.0f : u);
    v = (v < 0) ? 0.0f : ((v > 1) ? 1.0f : v);
    return len3(sub(p, add(add(pos, mul(w, v)), mul(h, u))));
}

/* x86-64 cvttss2si, the reference's (int) cast: out of range and NaN give INT_MIN */
__device__ __forceinline__ int cvt_x86(float f) {
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

} // namespace fmgi_dev

#endif
