/*
 * fmgi_rad_solve.hip -- the bounce half of the radiosity backend for several emitter palettes at once
 * (fmgi_rad_cache_solve). The arithmetic is fmgi_rad.hip's k_rad_gather / k_rad_update / k_rad_mip,
 * which restate radiosityNative.c:230-251 and rectangle.c:508-575 in fp32 and in the reference's order; only the
 * layout differs. Contraction is off, as in fmgi_rad.hip.
 *
 * Layout of a pass of K sets: kp = 1, 2, 4 or 8 >= K slots per texel, `[texel][kp]` float4, so a texel's values
 * are kp * 16 contiguous bytes (64 B at kp = 4, one 128-B line at kp = 8). Slots K .. kp-1 are padding: they start
 * at 0 everywhere, stay 0 and are never written out. No slot reads another, so a set's result depends on nothing
 * but its own palette.
 */
#include <hip/hip_runtime.h>

#include "fmgi_rad.h"

#pragma clang fp contract(off)

namespace {

/*
 * kp neighbouring lanes per job, lane = (job, slot): each lane keeps its own sequential fp32 sum over the job's
 * 10000 rays, skipping -1, exactly as k_rad_gather's lane does. The kp lanes of a job load the same id (one dword
 * per job and ray, as before) and then kp * 16 contiguous bytes of one texel, so one gather instruction touches
 * 64 / kp texels' lines instead of 64. The ids keep k_rad_gather's block prefetch (GATHER_B ids of the next block in
 * flight while this block's texels load).
 */
constexpr int GATHER_B = 25;
static_assert(FMGI_RAD_RAYS % GATHER_B == 0, "gather blocks must tile the rays");

template <int KP> __global__ __launch_bounds__(256) void k_rad_gather_sets(RadSolve b) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t job = g / KP;
    const int slot = (int)(g % KP);
    if (job >= b.njobs) return;
    const int32_t *s = b.sids + job;
    const int64_t stride = b.njobs;
    const float4 *src = b.src + slot;
    float x = 0, y = 0, z = 0;
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
        float4 t[GATHER_B];
#pragma unroll
        for (int i = 0; i < GATHER_B; i++) t[i] = src[(int64_t)(id[i] < 0 ? 0 : id[i]) * KP];
#pragma unroll
        for (int i = 0; i < GATHER_B; i++) {
            const bool hit = id[i] >= 0;
            x = hit ? x + t[i].x : x;
            y = hit ? y + t[i].y : y;
            z = hit ? z + t[i].z : z;
        }
    }
    b.dest[(int64_t)b.jobs[job].texel * KP + slot] = make_float4(x, y, z, 0.0f);
}

/* radiosityNative.c:242-247 on every slot of every texel */
__global__ __launch_bounds__(256) void k_rad_update_sets(RadSolve b) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.ntex * b.kp) return;
    const float4 s = b.src[i], d = b.dest[i];
    b.dst[i] = make_float4(s.x * b.keep + d.x * b.gain, s.y * b.keep + d.y * b.gain, s.z * b.keep + d.z * b.gain, 0.0f);
}

/* rectangle.c:508-575 mipmap(): one workgroup per rectangle, one level per step, every slot of a texel */
__global__ __launch_bounds__(256) void k_rad_mip_sets(RadSolve b) {
    const RadRect r = b.rects[blockIdx.x];
    float4 *t = b.dst;
    const int kp = b.kp;
    int64_t base = r.s0;
    int w = r.s1, h = r.s2;
    while (w > 1 || h > 1) {
        if (w == 1 || h == 1) { /* mipmapInternalHorizontal / Vertical (:508-533) */
            const int m = (h == 1) ? w : h, tm = m / 2;
            for (int e = threadIdx.x; e < tm * kp; e += blockDim.x) {
                const int i = e / kp, c = e % kp;
                const float4 p = t[(base + 2 * i) * kp + c], q = t[(base + 2 * i + 1) * kp + c];
                t[(base + m + i) * kp + c] = make_float4((p.x + q.x) * 0.5f, (p.y + q.y) * 0.5f, (p.z + q.z) * 0.5f, 0.0f);
            }
            base += m;
            if (h == 1) w = tm;
            else h = tm;
        } else { /* mipmapInternal 2-D step (:535-569), add4 order */
            const int tw = w / 2, th = h / 2;
            for (int e = threadIdx.x; e < tw * th * kp; e += blockDim.x) {
                const int idx = e / kp, c = e % kp;
                const int i = idx % tw, j = idx / tw;
                const float4 p = t[(base + (2 * j) * w + 2 * i) * kp + c], q = t[(base + (2 * j + 1) * w + 2 * i) * kp + c];
                const float4 u = t[(base + (2 * j) * w + 2 * i + 1) * kp + c],
                             d = t[(base + (2 * j + 1) * w + 2 * i + 1) * kp + c];
                t[(base + (int64_t)w * h + j * tw + i) * kp + c] =
                    make_float4((p.x + q.x + u.x + d.x) * 0.25f, (p.y + q.y + u.y + d.y) * 0.25f,
                                (p.z + q.z + u.z + d.z) * 0.25f, 0.0f);
            }
            base += (int64_t)w * h;
            w = tw;
            h = th;
        }
        __syncthreads();
    }
}

/*
 * radiosityNative.c:135-145 with the palette as a parameter: one workgroup per emitter rectangle writes every
 * texel of its mip chain, slot k = emit[k][e]; the table was zeroed before (walls, padding slots).
 */
__global__ __launch_bounds__(256) void k_rad_init_sets(RadSolve b, const float *__restrict__ emit, int nsets, int nemit,
                                                       int first_emit) {
    const int e = blockIdx.x;
    const RadRect r = b.rects[first_emit + e];
    int w = r.s1, h = r.s2;
    int64_t n = (int64_t)w * h; /* getNumMipmapTexels, rectangle.c:166-190 */
    while (w > 1 || h > 1) {
        if (w > 1) w /= 2;
        if (h > 1) h /= 2;
        n += (int64_t)w * h;
    }
    float4 *dst = b.dst + (int64_t)r.s0 * b.kp;
    for (int64_t i = threadIdx.x; i < n * b.kp; i += blockDim.x) {
        const int k = (int)(i % b.kp);
        if (k >= nsets) continue;
        const float *c = emit + ((int64_t)k * nemit + e) * 3;
        dst[i] = make_float4(c[0], c[1], c[2], 0.0f);
    }
}

/* slot k of texels [0, numTexels) -> the caller's planar float [numTexels][4] of set k, w = 0 */
__global__ __launch_bounds__(256) void k_rad_unpack_sets(RadSolve b, float4 *const *__restrict__ out, int nsets) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.num_texels * b.kp) return;
    const int k = (int)(i % b.kp);
    if (k >= nsets) return;
    const float4 v = b.src[i];
    out[k][i / b.kp] = make_float4(v.x, v.y, v.z, 0.0f);
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

bool valid(const RadSolve &b) { return b.kp == 1 || b.kp == 2 || b.kp == 4 || b.kp == 8; }

} // namespace

hipError_t fmgi_rad_launch_init_sets(const RadSolve &b, const float *emit_dev, int nsets, int nemit, int first_emit,
                                     hipStream_t s) {
    if (!valid(b) || nsets < 1 || nsets > b.kp || nemit < 0 || first_emit < 0 || first_emit + nemit > b.nrects)
        return hipErrorInvalidValue;
    if (nemit > 0) hipLaunchKernelGGL(k_rad_init_sets, dim3((unsigned)nemit), dim3(256), 0, s, b, emit_dev, nsets, nemit, first_emit);
    return hipGetLastError();
}

hipError_t fmgi_rad_launch_bounce_sets(const RadSolve &b, hipStream_t s) {
    if (!valid(b)) return hipErrorInvalidValue;
    if (b.njobs > 0) {
        const dim3 grid(blocks_of(b.njobs * b.kp)), block(256);
        switch (b.kp) {
        case 1: hipLaunchKernelGGL(k_rad_gather_sets<1>, grid, block, 0, s, b); break;
        case 2: hipLaunchKernelGGL(k_rad_gather_sets<2>, grid, block, 0, s, b); break;
        case 4: hipLaunchKernelGGL(k_rad_gather_sets<4>, grid, block, 0, s, b); break;
        default: hipLaunchKernelGGL(k_rad_gather_sets<8>, grid, block, 0, s, b); break;
        }
    }
    if (b.ntex > 0) hipLaunchKernelGGL(k_rad_update_sets, dim3(blocks_of(b.ntex * b.kp)), dim3(256), 0, s, b);
    if (b.nrects > 0) hipLaunchKernelGGL(k_rad_mip_sets, dim3((unsigned)b.nrects), dim3(256), 0, s, b);
    return hipGetLastError();
}

hipError_t fmgi_rad_launch_unpack_sets(const RadSolve &b, void *const *out_dev, int nsets, hipStream_t s) {
    if (!valid(b) || nsets < 1 || nsets > b.kp) return hipErrorInvalidValue;
    if (b.num_texels > 0)
        hipLaunchKernelGGL(k_rad_unpack_sets, dim3(blocks_of(b.num_texels * b.kp)), dim3(256), 0, s, b,
                           (float4 *const *)out_dev, nsets);
    return hipGetLastError();
}
