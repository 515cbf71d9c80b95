/*
 * fmgi_sun.hip -- the direct-sun layer's kernels (semantics: include/flatmatch_gi.h "Direct sunlight
 * through windows"). Every operation on a sample is IEEE fp32 in the order the header states, contraction off.
 *
 *   k_sun_lists  one wave per occluder list: the walls that can block a ray towards the sun (dot(n, s) < 0, the
 *                exact cull of intersects()' first line) and, per window, whose projection along s onto the
 *                window's plane overlaps the window within a margin and that are not wholly beyond the plane.
 *                Wall indices in ascending order, so a list is the same whatever the launch.
 *   k_sun_rays   one lane per sample, the S * S samples of a texel on adjacent lanes, floor(64 / S^2) texels per
 *                wave. The wall and window records are wave-uniform (scalar loads, or LDS for the staged lists);
 *                a texel's count is a ballot masked to its lanes; one lane per texel stores the byte.
 *   k_sun_add    one lane per level-0 texel of a facing wall: lm[m][t] += (cover * unit + S^2 / 2) / S^2.
 *
 * Memory safety: a job index is below njobs, a list entry is used only if it is below nwalls, a list's length is
 * clamped to list_cap, a texel index is stored to only below num_texels; all four bounds come from the host.
 */
#include <hip/hip_runtime.h>

#include "fmgi_sun.h"

#pragma clang fp contract(off)

#include "fmgi_rect_dev.h"

using namespace fmgi_dev;

namespace {

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

/* the job that holds job texel g (0 <= g < total): the last one whose first is <= g */
__device__ __forceinline__ int job_of(const SunJob *__restrict__ jobs, int njobs, int g) {
    int lo = 0, hi = njobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].first <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float max3abs(float x, float y, float z) { return fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z)); }

} // namespace

__global__ __launch_bounds__(64) void k_sun_lists(SunArgs a) {
    const int l = (int)blockIdx.x, lane = lane_id();
    const v3 s = mk(a.sx, a.sy, a.sz);
    int32_t *list = a.lists + (size_t)l * a.list_cap;
    int n = 0;
    bool dead = false, cull = false;
    AoRect w = {};
    float dn = -1.0f;
    if (!a.all) {
        w = a.wins[l];
        dn = dot(mk(w.nx, w.ny, w.nz), s);
        dead = dn >= 0;                 /* intersects() returns -1 on its first line: no ray crosses this window */
        cull = fabsf(dn) >= 1e-3f;      /* a grazing (or NaN) window keeps every wall */
    }
    if (!dead)
        for (int base = 0; base < a.nwalls; base += 64) {
            const int i = base + lane;
            bool keep = false;
            if (i < a.nwalls) {
                const AoRect r = a.hits[i];
                keep = !(dot(mk(r.nx, r.ny, r.nz), s) >= 0);
                if (keep && cull) {
                    const v3 wp = mk(w.px, w.py, w.pz), wn = mk(w.nx, w.ny, w.nz);
                    const v3 rp = mk(r.px, r.py, r.pz);
                    const float R = fmaxf(max3abs(w.px, w.py, w.pz) + w.wl + w.hl, max3abs(r.px, r.py, r.pz) + r.wl + r.hl);
                    const float m = 1e-3f * (1.0f + R) / fabsf(dn);
                    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, tmax = -INFINITY;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        v3 c = rp;
                        if (k & 1) c = add(c, mul(mk(r.wx, r.wy, r.wz), r.wl));
                        if (k & 2) c = add(c, mul(mk(r.hx, r.hy, r.hz), r.hl));
                        const float t = dot(wn, sub(wp, c)) / dn; /* along s from the corner to the window's plane */
                        const v3 d = sub(add(c, mul(s, t)), wp);
                        const float u = dot(mk(w.wx, w.wy, w.wz), d), v = dot(mk(w.hx, w.hy, w.hz), d);
                        umin = fminf(umin, u), umax = fmaxf(umax, u);
                        vmin = fminf(vmin, v), vmax = fmaxf(vmax, v);
                        tmax = fmaxf(tmax, t);
                    }
                    /* finite numbers only: anything else keeps the wall */
                    if (R < 1e30f && m < 1e30f)
                        keep = !(tmax < -m || umax < -m || umin > w.wl + m || vmax < -m || vmin > w.hl + m);
                }
            }
            const unsigned long long b = __ballot(keep);
            const int at = n + __popcll(b & ((1ull << lane) - 1ull));
            if (keep && at < a.list_cap) list[at] = i;
            n += __popcll(b);
        }
    if (lane == 0) {
        a.list_len[l] = n < a.list_cap ? n : a.list_cap;
        atomicAdd(&a.counters[SUN_CTR_ENTRIES], (unsigned long long)n);
    }
}

extern __shared__ __attribute__((aligned(16))) char sun_smem[];

__global__ __launch_bounds__(FMGI_SUN_BLOCK) void k_sun_rays(SunArgs a) {
    const int lane = lane_id();
    const int waves = FMGI_SUN_BLOCK / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const v3 s = mk(a.sx, a.sy, a.sz);
    const int S = a.S, S2 = S * S, tpw = 64 / S2;

    /* the lists' records into LDS, if the launch has room for all of them */
    int *off = (int *)sun_smem;
    AoRect *lrec = (AoRect *)(sun_smem + (((size_t)(a.nlists + 1) * 4 + 15) & ~(size_t)15));
    bool staged = false;
    if (a.lds_entries > 0) {
        if (threadIdx.x == 0) {
            int e = 0;
            for (int l = 0; l < a.nlists; l++) {
                off[l] = e;
                const int len = a.list_len[l];
                e += len < 0 ? 0 : (len < a.list_cap ? len : a.list_cap);
            }
            off[a.nlists] = e;
        }
        __syncthreads();
        staged = off[a.nlists] <= a.lds_entries;
        if (staged) {
            for (int l = 0; l < a.nlists; l++) {
                const int o = off[l], len = off[l + 1] - o;
                for (int k = (int)threadIdx.x; k < len; k += FMGI_SUN_BLOCK) {
                    const int i = a.lists[(size_t)l * a.list_cap + k];
                    AoRect r;
                    if ((unsigned)i < (unsigned)a.nwalls) r = a.hits[i];
                    else r = AoRect{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; /* n = 0: never hit */
                    lrec[o + k] = r;
                }
            }
        }
        __syncthreads();
    }

    const int k = lane / S2, q = lane - k * S2, si = q % S, sj = q / S;
    const float fu = (float)(2 * si + 1) / (float)(2 * S), fv = (float)(2 * sj + 1) / (float)(2 * S);
    const long long nwaves = ((long long)a.total + tpw - 1) / tpw;
    unsigned long long n_cross = 0, n_lit = 0, n_tests = 0;

    for (long long wj = (long long)blockIdx.x * waves + wave; wj < nwaves; wj += (long long)gridDim.x * waves) {
        const int g0 = (int)(wj * tpw);
        const int g1 = (a.total - g0 < tpw ? a.total : g0 + tpw) - 1; /* the wave's last job texel */
        const int g = g0 + k;
        const bool live = k < tpw && g <= g1;
        const int j_lo = job_of(a.jobs, a.njobs, g0), j_hi = job_of(a.jobs, a.njobs, g1);
        v3 Q = mk(0, 0, 0);
        int texel = -1;
        for (int j = j_lo; j <= j_hi; j++) { /* nearly always one wall */
            const SunJob w = a.jobs[j];
            const int end = j + 1 < a.njobs ? a.jobs[j + 1].first : a.total;
            if (live && g >= w.first && g < end) {
                const int local = g - w.first, ty = local / w.s1, tx = local - ty * w.s1;
                const float ca = ((float)tx + fu) / (float)w.s1, cb = ((float)ty + fv) / (float)w.s2;
                const v3 P = add(add(mk(w.px, w.py, w.pz), mul(mk(w.wx, w.wy, w.wz), ca)), mul(mk(w.hx, w.hy, w.hz), cb));
                Q = add(P, mul(s, 1e-5f));
                texel = w.s0 + local;
            }
        }
        const bool has = live && texel >= 0;

        /* the nearest window the ray leaves through */
        float dw = INFINITY;
        int vwin = -1;
        for (int v = 0; v < a.nwins; v++) {
            const AoRect w = a.wins[v];
            if (has) {
                const float d = rect_intersects(w, Q, s, INFINITY);
                if (d != -1.0f && (vwin < 0 || d < dw)) {
                    dw = d;
                    vwin = v;
                }
            }
        }
        const bool crossing = has && vwin >= 0;
        const int lid = a.all ? 0 : vwin;

        /* any wall before the window blocks; the wave walks list by list */
        bool blocked = false;
        for (int l = 0; l < a.nlists; l++) {
            const bool mine = crossing && lid == l;
            unsigned long long act = __ballot(mine);
            if (!act) continue;
            int len = staged ? off[l + 1] - off[l] : a.list_len[l];
            len = len < a.list_cap ? len : a.list_cap;
            const int o = staged ? off[l] : 0;
            for (int e = 0; e < len && act; e++) {
                AoRect r;
                if (staged) {
                    r = lrec[o + e];
                } else {
                    const int i = a.lists[(size_t)l * a.list_cap + e];
                    if ((unsigned)i >= (unsigned)a.nwalls) continue;
                    r = a.hits[i];
                }
                n_tests += (unsigned long long)__popcll(act);
                if (mine && !blocked && rect_intersects(r, Q, s, dw) != -1.0f) blocked = true;
                act = __ballot(mine && !blocked);
            }
        }
        const bool lit = crossing && !blocked;
        const unsigned long long lit_b = __ballot(lit);
        n_cross += (unsigned long long)__popcll(__ballot(crossing));
        n_lit += (unsigned long long)__popcll(lit_b);
        if (has && q == 0 && (unsigned)texel < (unsigned)a.num_texels) {
            const unsigned long long m = S2 == 64 ? ~0ull : (((1ull << S2) - 1ull) << (k * S2));
            a.cover[texel] = (uint8_t)__popcll(lit_b & m);
        }
    }
    if (lane == 0 && (n_cross | n_lit | n_tests)) {
        atomicAdd(&a.counters[SUN_CTR_CROSSING], n_cross);
        atomicAdd(&a.counters[SUN_CTR_LIT], n_lit);
        atomicAdd(&a.counters[SUN_CTR_TESTS], n_tests);
    }
}

__global__ __launch_bounds__(256) void k_sun_add(SunAddArgs a) {
    const long long g64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g64 >= a.total) return;
    const int g = (int)g64;
    const int j = job_of(a.jobs, a.njobs, g);
    const int t = a.jobs[j].s0 + (g - a.jobs[j].first);
    if ((unsigned)t >= (unsigned)a.num_texels) return;
    unsigned cv = a.cover[t];
    if (cv == 0) return;
    const unsigned S2 = (unsigned)a.S2;
    cv = cv < S2 ? cv : S2;
    const long long *u = a.units + (size_t)j * a.maps * 3;
#pragma unroll
    for (int m = 0; m < FMGI_SUN_MAPS; m++) {
        if (m >= a.maps) break;
        unsigned long long *p = a.lm[m] + 4 * (size_t)t;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const unsigned long long unit = (unsigned long long)u[m * 3 + c];
            p[c] += cv == S2 ? unit : (cv * unit + S2 / 2) / S2; /* a full texel: (S2 * unit + S2 / 2) / S2 == unit */
        }
    }
}

size_t fmgi_sun_lds_bytes(const SunArgs &a) {
    if (a.lds_entries <= 0) return 0;
    return (((size_t)(a.nlists + 1) * 4 + 15) & ~(size_t)15) + (size_t)a.lds_entries * sizeof(AoRect);
}

hipError_t fmgi_sun_launch_lists(const SunArgs &a, hipStream_t s) {
    if (a.nlists < 1) return hipSuccess;
    hipLaunchKernelGGL(k_sun_lists, dim3((unsigned)a.nlists), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t fmgi_sun_launch_rays(const SunArgs &a, int num_cus, hipStream_t s) {
    if (a.total < 1 || a.njobs < 1) return hipSuccess;
    const int tpw = 64 / (a.S * a.S), waves = FMGI_SUN_BLOCK / 64;
    const long long nwaves = ((long long)a.total + tpw - 1) / tpw;
    const size_t lds = fmgi_sun_lds_bytes(a);
    /* resident workgroups only, so that a workgroup's staging serves many wave jobs: 160 KB of LDS and 32 waves
       per CU */
    long long per_cu = lds ? (long long)((160u << 10) / lds) : 4;
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    long long blocks = (nwaves + waves - 1) / waves;
    const long long resident = (long long)(num_cus > 0 ? num_cus : 256) * per_cu;
    if (blocks > resident) blocks = resident;
    hipLaunchKernelGGL(k_sun_rays, dim3((unsigned)blocks), dim3(FMGI_SUN_BLOCK), lds, s, a);
    return hipGetLastError();
}

hipError_t fmgi_sun_launch_add(const SunAddArgs &a, hipStream_t s) {
    if (a.total < 1 || a.njobs < 1 || a.maps < 1) return hipSuccess;
    hipLaunchKernelGGL(k_sun_add, dim3((unsigned)(((long long)a.total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
