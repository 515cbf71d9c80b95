/*
 * fmgi_rad_host.cpp -- host side of the radiosity backend (§8f rank 4) and its C ABI
 * (include/flatmatch_gi.h: performRadiosityGpu, fmgi_radiosity, fmgi_radiosity_jobs,
 * fmgi_radiosity_stats). The reference is performRadiosityNative (radiosityNative.c:92-268).
 *
 * The host
 *   - reads the caller's libc rand() state (glibc TYPE_3: 31 words and a read position), before any HIP
 *     call, since the HIP runtime's first initialisation itself draws a rand() value;
 *   - builds the rectangle list with the window/light texel bases appended after numTexels
 *     (radiosityNative.c:108-131) and one job per level-0 wall texel, in the reference's wall/tile
 *     order, which is also its rand() order;
 *   - builds the jump matrices M^(2500 * 2^b) of the generator's linear recurrence;
 *   - runs the device phases (fmgi_rad.hip) and copies texels [0, numTexels) back;
 *   - leaves the libc generator exactly where 2 x 10000 x jobs rand() calls would have left it.
 * fmgi_rad_cache_*  runs the same trace once (rad_prepare, rad_trace), keeps its ids on the device and
 * solves any emitter palettes from them, asynchronously on the caller's stream; fmgi_rad_cache_sun_bounce
 * gathers sun coverage maps through the same ids (fmgi_sun_bounce.hip).
 * Geometry precomputation is fp32 in the reference's order (built with -ffp-contract=off, no FMA).
 */
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/flatmatch_gi.h"
#include "fmgi_rad.h"
#include "fmgi_sun_bounce.h"
#include "fmgi_view.h"

#define FMGI_API extern "C" __attribute__((visibility("default")))

int internal_set_err(int code, const char *msg);

namespace {

struct F3 {
    float x, y, z;
};
F3 f3of(const fmgi_vec3 &v) { return F3{v.s[0], v.s[1], v.s[2]}; }
F3 add(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
F3 mul(F3 a, float f) { return F3{a.x * f, a.y * f, a.z * f}; }
float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
F3 cross(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float length(F3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
F3 div_vec3(F3 a, float b) { return mul(a, 1.0f / b); } /* vector3_cl.c:53-58 */
F3 normalized(F3 a) { return mul(a, 1.0f / length(a)); } /* vector3_cl.c:95-101 */

constexpr int DEG = FMGI_RAND_DEG;
using Mat = std::vector<uint32_t>; /* 31x31 row-major over Z/2^32 */

/* one step of glibc random_r TYPE_3 on the window (x[n-31] .. x[n-1]): shift, append x[n-31] + x[n-3] */
Mat step_matrix() {
    Mat m((size_t)DEG * DEG, 0);
    for (int i = 0; i + 1 < DEG; i++) m[(size_t)i * DEG + i + 1] = 1;
    m[(size_t)(DEG - 1) * DEG + 0] += 1;
    m[(size_t)(DEG - 1) * DEG + 28] += 1;
    return m;
}

Mat mat_mul(const Mat &a, const Mat &b) {
    Mat c((size_t)DEG * DEG, 0);
    for (int i = 0; i < DEG; i++)
        for (int k = 0; k < DEG; k++) {
            const uint32_t aik = a[(size_t)i * DEG + k];
            if (!aik) continue;
            for (int j = 0; j < DEG; j++) c[(size_t)i * DEG + j] += aik * b[(size_t)k * DEG + j];
        }
    return c;
}

void mat_vec(const Mat &a, const uint32_t *x, uint32_t *y) {
    uint32_t t[DEG];
    for (int i = 0; i < DEG; i++) {
        uint32_t s = 0;
        for (int k = 0; k < DEG; k++) s += a[(size_t)i * DEG + k] * x[k];
        t[i] = s;
    }
    memcpy(y, t, sizeof t);
}

Mat mat_pow(Mat base, uint64_t e) {
    Mat r((size_t)DEG * DEG, 0);
    for (int i = 0; i < DEG; i++) r[(size_t)i * DEG + i] = 1;
    while (e) {
        if (e & 1) r = mat_mul(r, base);
        e >>= 1;
        if (e) base = mat_mul(base, base);
    }
    return r;
}

/*
 * The caller's glibc rand() generator. glibc keeps the TYPE_3 state as an int32 header word followed
 * by 31 words; initstate() on another buffer records the read position in that header (5 * rear + type,
 * random_r.c __initstate_r) and setstate() reloads it (the front index is rear + 3 mod 31).
 */
struct LibcRand {
    int32_t *hdr = nullptr;
    int rear = 0, front = 0;
    bool read(uint32_t v[DEG]) {
#ifdef __GLIBC__
        static char scratch[128];
        hdr = (int32_t *)initstate(1, scratch, sizeof scratch);
        if (!hdr) return false;
        const int32_t h = hdr[0];
        setstate((char *)hdr);
        if (h % 5 != 3) return false; /* TYPE_3 only: the default state and srand() keep it */
        rear = h / 5;
        front = (rear + 3) % DEG;
        const uint32_t *st = (const uint32_t *)(hdr + 1);
        for (int j = 0; j < DEG; j++) v[j] = st[(front + j) % DEG]; /* oldest (the next front) first */
        return true;
#else
        return false;
#endif
    }
    /* install window v as the state after `steps` calls from the one read() saw */
    void write(const uint32_t v[DEG], uint64_t steps) {
#ifdef __GLIBC__
        static char scratch2[128];
        initstate(1, scratch2, sizeof scratch2); /* leave the caller's array (its header is rewritten) */
        const int f = (int)((front + steps) % DEG), r = (int)((rear + steps) % DEG);
        uint32_t *st = (uint32_t *)(hdr + 1);
        for (int j = 0; j < DEG; j++) st[(f + j) % DEG] = v[j];
        hdr[0] = 5 * r + 3;
        setstate((char *)hdr);
#endif
    }
};

int num_mip_texels(const int32_t *lm) { /* rectangle.c:166-190 (asserts compiled out) */
    int w = lm[1], h = lm[2], n = w * h;
    while (w > 1 || h > 1) {
        if (w > 1) w /= 2;
        if (h > 1) h /= 2;
        n += w * h;
    }
    return n;
}

fmgi_rad_stats g_stats;

#define RADCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            char b_[256];                                                                              \
            snprintf(b_, sizeof b_, "%s: %s", #expr, hipGetErrorString(e_));                           \
            rc = internal_set_err(FMGI_ERR_HIP, b_);                                                   \
            goto done;                                                                                 \
        }                                                                                              \
    } while (0)

int64_t count_jobs(const fmgi_geometry *geo) {
    int64_t n = 0;
    for (int i = 0; i < geo->numWalls; i++) n += (int64_t)geo->walls[i].lightmapSetup[1] * geo->walls[i].lightmapSetup[2];
    return n;
}

/* an argument error of the entry point fn */
int arg_err(const char *fn, const char *msg) {
    char b[256];
    snprintf(b, sizeof b, "%s: %s", fn, msg);
    return internal_set_err(FMGI_ERR_ARG, b);
}

int check_geometry(const fmgi_geometry *geo, const char *fn) {
    if (!geo) return arg_err(fn, "null geometry");
    if (geo->numWalls < 0 || geo->numWindows < 0 || geo->numLights < 0 || geo->numTexels < 0 ||
        (geo->numWalls && !geo->walls) || (geo->numWindows && !geo->windows) || (geo->numLights && !geo->lights) ||
        (geo->numTexels && !geo->texels))
        return arg_err(fn, "bad geometry");
    std::vector<std::pair<int64_t, int64_t>> spans;
    const fmgi_rect *sets[3] = {geo->walls, geo->windows, geo->lights};
    const int counts[3] = {geo->numWalls, geo->numWindows, geo->numLights};
    for (int s = 0; s < 3; s++)
        for (int i = 0; i < counts[s]; i++) {
            const int32_t *lm = sets[s][i].lightmapSetup;
            if (lm[1] < 1 || lm[2] < 1 || (int64_t)lm[1] * lm[2] > (1 << 28))
                return arg_err(fn, "a rectangle has an empty or huge lightmap");
            if (s == 0) {
                if (lm[0] < 0 || (int64_t)lm[0] + num_mip_texels(lm) > geo->numTexels)
                    return arg_err(fn, "a wall's texels lie outside numTexels");
                spans.push_back({lm[0], (int64_t)lm[0] + (int64_t)lm[1] * lm[2]});
            }
        }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++)
        if (spans[i].first < spans[i - 1].second) return arg_err(fn, "two walls share level-0 texels");
    const int64_t nr = (int64_t)geo->numWalls + geo->numWindows + geo->numLights;
    if (nr > FMGI_RAD_MAX_SORT) return arg_err(fn, "more rectangles than the candidate sort holds (16384)");
    return FMGI_OK;
}

/* a device allocation that lives as long as its scope */
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 1)); }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
    }
    template <class T> T *as() const { return (T *)p; }
};

/*
 * The lighting-independent half of a run on the host: the caller's rand() position, the rectangle list
 * (radiosityNative.c:108-131), the jobs, the jump matrices and the generator's window after the run's draws.
 * fmgi_radiosity and fmgi_rad_cache_create share it, and rad_trace below.
 */
struct RadPrep {
    LibcRand libc;
    uint32_t v0[DEG], vend[DEG];
    int nr = 0, sort_n = 2;
    int64_t ntex = 0, first_light = 0, njobs = 0;
    std::vector<RadRect> rects;
    std::vector<AoRect> hits;
    std::vector<RadJob> jobs;
    std::vector<uint32_t> jump;
    void restore() { libc.write(v0, 0); }                                    /* as if nothing had been drawn */
    void advance() { libc.write(vend, 2ull * FMGI_RAD_RAYS * (uint64_t)njobs); } /* as after the reference's draws */
};

/* what rad_trace leaves on the device; draws, jump, v0 and hits serve the trace only */
struct RadDev {
    DevBuf rects, hits, jobs, jump, v0, draws, sids;
};

/* geo has passed check_geometry; reads the libc state before any HIP call */
int rad_prepare(const fmgi_geometry *geo, const char *fn, RadPrep &p) {
    if (!p.libc.read(p.v0)) return arg_err(fn, "libc rand() is not in glibc's default TYPE_3 state");

    /* the rectangle list, radiosityNative.c:108-131 */
    const int nr = p.nr = geo->numWalls + geo->numWindows + geo->numLights;
    std::vector<fmgi_rect> all;
    all.reserve((size_t)nr);
    for (int i = 0; i < geo->numWalls; i++) all.push_back(geo->walls[i]);
    for (int i = 0; i < geo->numWindows; i++) all.push_back(geo->windows[i]);
    for (int i = 0; i < geo->numLights; i++) all.push_back(geo->lights[i]);
    int64_t ntex = geo->numTexels;
    for (int i = geo->numWalls; i < nr; i++) {
        if (ntex > INT32_MAX) return arg_err(fn, "too many texels");
        all[(size_t)i].lightmapSetup[0] = (int32_t)ntex;
        ntex += num_mip_texels(all[(size_t)i].lightmapSetup);
    }
    p.ntex = ntex;
    p.first_light = geo->numLights ? all[(size_t)(geo->numWalls + geo->numWindows)].lightmapSetup[0] : ntex;
    p.rects.resize((size_t)std::max(nr, 1));
    p.hits.resize((size_t)std::max(nr, 1));
    for (int i = 0; i < nr; i++) {
        const fmgi_rect &r = all[(size_t)i];
        p.rects[(size_t)i] = fmgi_rad_rect(r);
        p.hits[(size_t)i] = fmgi_rad_hit_rect(r);
    }
    while (p.sort_n < nr) p.sort_n <<= 1;

    /* jobs: every level-0 wall texel, wall/tile order (radiosityNative.c:166-176) */
    const int64_t njobs = p.njobs = count_jobs(geo);
    p.jobs.resize((size_t)std::max<int64_t>(njobs, 1));
    {
        int64_t j = 0;
        for (int w = 0; w < geo->numWalls; w++) {
            const fmgi_rect &r = geo->walls[w];
            const int s1 = r.lightmapSetup[1], s2 = r.lightmapSetup[2];
            const F3 vw = div_vec3(f3of(r.width), (float)s1), vh = div_vec3(f3of(r.height), (float)s2);
            const F3 n = f3of(r.n);
            /* getCosineDistributedRandomRay's basis (vector3_cl.c:140-145) */
            F3 ud{0, 0, 1};
            if (fabs(dot(ud, n)) >= 0.999999f) ud = F3{0, 1, 0};
            const F3 vd = normalized(cross(ud, n));
            ud = normalized(cross(vd, n));
            for (int t = 0; t < s1 * s2; t++, j++) {
                RadJob &o = p.jobs[(size_t)j];
                memset(&o, 0, sizeof o);
                const int tx = t % s1, ty = t / s1; /* getTileCenter (rectangle.c:140-153) */
                const F3 c = add(add(f3of(r.pos), mul(vw, (float)(tx + 0.5))), mul(vh, (float)(ty + 0.5)));
                o.cx = c.x, o.cy = c.y, o.cz = c.z;
                o.nx = n.x, o.ny = n.y, o.nz = n.z;
                o.ux = ud.x, o.uy = ud.y, o.uz = ud.z;
                o.vx = vd.x, o.vy = vd.y, o.vz = vd.z;
                o.texel = r.lightmapSetup[0] + t;
            }
        }
    }

    /* jump matrices and the generator's final window after 20000 draws per job */
    p.jump.resize((size_t)FMGI_RAD_JUMP_BITS * DEG * DEG);
    Mat m = mat_pow(step_matrix(), FMGI_RAD_SUBLEN);
    for (int b = 0; b < FMGI_RAD_JUMP_BITS; b++) {
        memcpy(&p.jump[(size_t)b * DEG * DEG], m.data(), (size_t)DEG * DEG * 4);
        if (b + 1 < FMGI_RAD_JUMP_BITS) m = mat_mul(m, m);
    }
    const uint64_t qend = (uint64_t)njobs * FMGI_RAD_SUBS;
    if (qend >> FMGI_RAD_JUMP_BITS) return arg_err(fn, "too many texels");
    memcpy(p.vend, p.v0, sizeof p.vend);
    for (int b = 0; b < FMGI_RAD_JUMP_BITS; b++)
        if ((qend >> b) & 1) {
            Mat pb(p.jump.begin() + (size_t)b * DEG * DEG, p.jump.begin() + (size_t)(b + 1) * DEG * DEG);
            mat_vec(pb, p.vend, p.vend);
        }
    return FMGI_OK;
}

/* no device: the caller's stream goes back where it was */
int rad_no_device(RadPrep &p) {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) == hipSuccess && dev_count > 0) return FMGI_OK;
    p.restore();
    return internal_set_err(FMGI_ERR_NO_DEVICE, "no HIP device visible");
}

/*
 * The trace on the device: uploads, the rand() replay and the rays, in chunks of jobs. Records ev[0] before the
 * first upload and ev[3] after the last ray launch on the null stream; ev[1] and ev[2] time the replays.
 * Fills jobs, rects, texels, rays, rand_ms and rays_ms (rays + uploads) of st.
 */
int rad_trace(const RadPrep &p, RadDev &d, fmgi_rad_stats &st, hipEvent_t (&ev)[4]) {
    int rc = FMGI_OK;
    const int64_t njobs = p.njobs;
    int64_t chunk = 1;
    RadArgs a;
    memset(&a, 0, sizeof a);
    st.jobs = njobs;
    st.rects = p.nr;
    st.texels = p.ntex;
    st.rays = njobs * FMGI_RAD_RAYS;
    RADCHK(hipEventRecord(ev[0], nullptr));
    RADCHK(d.rects.alloc(p.rects.size() * sizeof(RadRect)));
    RADCHK(hipMemcpy(d.rects.p, p.rects.data(), p.rects.size() * sizeof(RadRect), hipMemcpyHostToDevice));
    RADCHK(d.hits.alloc(p.hits.size() * sizeof(AoRect)));
    RADCHK(hipMemcpy(d.hits.p, p.hits.data(), p.hits.size() * sizeof(AoRect), hipMemcpyHostToDevice));
    RADCHK(d.jobs.alloc(p.jobs.size() * sizeof(RadJob)));
    RADCHK(hipMemcpy(d.jobs.p, p.jobs.data(), p.jobs.size() * sizeof(RadJob), hipMemcpyHostToDevice));
    RADCHK(d.jump.alloc(p.jump.size() * 4));
    RADCHK(hipMemcpy(d.jump.p, p.jump.data(), p.jump.size() * 4, hipMemcpyHostToDevice));
    RADCHK(d.v0.alloc(DEG * 4));
    RADCHK(hipMemcpy(d.v0.p, p.v0, DEG * 4, hipMemcpyHostToDevice));
    RADCHK(d.sids.alloc((size_t)std::max<int64_t>(njobs, 1) * FMGI_RAD_RAYS * 4));
    {
        /* rand() draws of a chunk of jobs: at most 1/8 of free memory, at most 4 GiB */
        size_t fr = 0, tot = 0;
        RADCHK(hipMemGetInfo(&fr, &tot));
        const size_t cap = std::min<size_t>(fr / 8, (size_t)4 << 30);
        chunk = std::max<int64_t>(1, std::min<int64_t>(njobs, (int64_t)(cap / ((size_t)FMGI_RAD_DRAWS * 4))));
        const char *ce = getenv("FMGI_RAD_CHUNK"); /* tests: force several chunks */
        if (ce && atoll(ce) > 0) chunk = std::min<int64_t>(std::max<int64_t>(njobs, 1), atoll(ce));
    }
    RADCHK(d.draws.alloc((size_t)chunk * FMGI_RAD_DRAWS * 4));
    a.rects = d.rects.as<RadRect>();
    a.hits = d.hits.as<AoRect>();
    a.nrects = p.nr;
    a.sort_n = p.sort_n;
    a.jobs = d.jobs.as<RadJob>();
    a.njobs = njobs;
    a.jump = d.jump.as<uint32_t>();
    a.v0 = d.v0.as<uint32_t>();
    a.draws = d.draws.as<uint32_t>();
    a.sids = d.sids.as<int32_t>();
    {
        float rand_ms = 0;
        for (int64_t j0 = 0; j0 < njobs; j0 += chunk) {
            a.job0 = j0;
            a.nchunk = std::min(chunk, njobs - j0);
            RADCHK(hipEventRecord(ev[1], nullptr));
            RADCHK(fmgi_rad_launch_rand(a, nullptr));
            RADCHK(hipEventRecord(ev[2], nullptr));
            RADCHK(fmgi_rad_launch_rays(a, nullptr));
            RADCHK(hipEventSynchronize(ev[2]));
            float ms = 0;
            RADCHK(hipEventElapsedTime(&ms, ev[1], ev[2]));
            rand_ms += ms;
        }
        st.rand_ms = rand_ms;
    }
    RADCHK(hipEventRecord(ev[3], nullptr));
    {
        float ms = 0;
        RADCHK(hipEventSynchronize(ev[3]));
        RADCHK(hipEventElapsedTime(&ms, ev[0], ev[3]));
        st.rays_ms = ms - st.rand_ms; /* rays + uploads */
    }
done:
    return rc;
}

/* device ray-major ids -> the reference's per-texel rows */
int download_sids(const int32_t *d_sids, int64_t njobs, int32_t *sids_out) {
    int rc = FMGI_OK;
    std::vector<int32_t> h((size_t)njobs * FMGI_RAD_RAYS);
    if (!njobs) return rc;
    RADCHK(hipMemcpy(h.data(), d_sids, h.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < FMGI_RAD_RAYS; k++)
        for (int64_t j = 0; j < njobs; j++) sids_out[j * FMGI_RAD_RAYS + k] = h[(size_t)(k * njobs + j)];
done:
    return rc;
}

int rad_run(const fmgi_geometry *geo, fmgi_vec3 *texels_out, int32_t *sids_out) {
    static const char fn[] = "fmgi_radiosity";
    int rc = check_geometry(geo, fn);
    if (rc != FMGI_OK) return rc;
    if (!texels_out && geo->numTexels) return arg_err(fn, "null texels_out");
    RadPrep p;
    if ((rc = rad_prepare(geo, fn, p)) != FMGI_OK) return rc;
    const int64_t njobs = p.njobs, ntex = p.ntex;

    memset(&g_stats, 0, sizeof g_stats);
    g_stats.jobs = njobs;
    g_stats.rects = p.nr;
    g_stats.texels = ntex;
    g_stats.rays = njobs * FMGI_RAD_RAYS;
    if ((rc = rad_no_device(p)) != FMGI_OK) return rc;

    RadDev d;
    DevBuf b_src, b_dst, b_dest;
    float4 *d_src = nullptr, *d_dst = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}, ev_b[2] = {nullptr, nullptr};
    std::vector<float4> init((size_t)std::max<int64_t>(ntex, 1));
    RadBounce bb;
    memset(&bb, 0, sizeof bb);
    {
        const char *dv = getenv("FMGI_DEVICE");
        RADCHK(hipSetDevice(dv ? atoi(dv) : 0));
    }
    for (auto &e : ev) RADCHK(hipEventCreate(&e));
    for (auto &e : ev_b) RADCHK(hipEventCreate(&e));
    if ((rc = rad_trace(p, d, g_stats, ev)) != FMGI_OK) goto done;

    /* radiosity: walls 0, windows 30, lights (28, 28, 32) (radiosityNative.c:139-149) */
    for (int64_t i = 0; i < ntex; i++)
        init[(size_t)i] = i < geo->numTexels  ? make_float4(0, 0, 0, 0)
                          : i < p.first_light ? make_float4(FMGI_RAD_WINDOW, FMGI_RAD_WINDOW, FMGI_RAD_WINDOW, 0)
                                              : make_float4(FMGI_RAD_LIGHT_R, FMGI_RAD_LIGHT_G, FMGI_RAD_LIGHT_B, 0);
    RADCHK(b_src.alloc(init.size() * 16));
    RADCHK(b_dst.alloc(init.size() * 16));
    RADCHK(b_dest.alloc(init.size() * 16));
    d_src = b_src.as<float4>(), d_dst = b_dst.as<float4>();
    RADCHK(hipMemcpy(d_src, init.data(), init.size() * 16, hipMemcpyHostToDevice));
    RADCHK(hipMemset(b_dest.p, 0, init.size() * 16));
    RADCHK(hipEventRecord(ev_b[0], nullptr));
    bb.sids = d.sids.as<int32_t>();
    bb.jobs = d.jobs.as<RadJob>();
    bb.njobs = njobs;
    bb.rects = d.rects.as<RadRect>();
    bb.nrects = p.nr;
    bb.ntex = ntex;
    bb.dest = b_dest.as<float4>();
    bb.keep = 1 - FMGI_RAD_REFLECTANCE; /* reflectance = 0.3 (float), radiosityNative.c:103 */
    bb.gain = FMGI_RAD_REFLECTANCE / FMGI_RAD_RAYS;
    for (int it = 0; it < FMGI_RAD_ITERS; it++) {
        bb.src = d_src;
        bb.dst = d_dst;
        RADCHK(fmgi_rad_launch_bounce(bb, nullptr));
        std::swap(d_src, d_dst);
    }
    RADCHK(hipEventRecord(ev_b[1], nullptr));
    if (geo->numTexels) RADCHK(hipMemcpy(texels_out, d_src, (size_t)geo->numTexels * 16, hipMemcpyDeviceToHost));
    if (sids_out && (rc = download_sids(d.sids.as<int32_t>(), njobs, sids_out)) != FMGI_OK) goto done;
    {
        float ms = 0;
        RADCHK(hipEventSynchronize(ev_b[1]));
        RADCHK(hipEventElapsedTime(&ms, ev_b[0], ev_b[1]));
        g_stats.bounce_ms = ms;
        RADCHK(hipEventElapsedTime(&ms, ev[0], ev_b[1]));
        g_stats.total_ms = ms;
    }
    p.advance();
done:
    if (rc != FMGI_OK) p.restore();
    for (auto &e : ev)
        if (e) hipEventDestroy(e);
    for (auto &e : ev_b)
        if (e) hipEventDestroy(e);
    return rc;
}

} // namespace

/* the two device images of a rectangle; the view renderer uploads its walls as the same (fmgi_view.h) */
AoRect fmgi_rad_hit_rect(const fmgi_rect &r) { /* intersects()'s per-call values, rectangle.c:67-95 */
    AoRect a;
    memset(&a, 0, sizeof a);
    a.nx = r.n.s[0], a.ny = r.n.s[1], a.nz = r.n.s[2];
    a.px = r.pos.s[0], a.py = r.pos.s[1], a.pz = r.pos.s[2];
    const F3 w = f3of(r.width), h = f3of(r.height);
    const float wl = length(w), hl = length(h);
    const F3 wn = div_vec3(w, wl), hn = div_vec3(h, hl);
    a.wx = wn.x, a.wy = wn.y, a.wz = wn.z, a.wl = wl;
    a.hx = hn.x, a.hy = hn.y, a.hz = hn.z, a.hl = hl;
    return a;
}

RadRect fmgi_rad_rect(const fmgi_rect &r) { /* the candidate tests' values, rectangle.c:97-113, :442-470 */
    RadRect o;
    o.px = r.pos.s[0], o.py = r.pos.s[1], o.pz = r.pos.s[2];
    o.wx = r.width.s[0], o.wy = r.width.s[1], o.wz = r.width.s[2];
    o.hx = r.height.s[0], o.hy = r.height.s[1], o.hz = r.height.s[2];
    o.nx = r.n.s[0], o.ny = r.n.s[1], o.nz = r.n.s[2];
    o.s0 = r.lightmapSetup[0], o.s1 = r.lightmapSetup[1], o.s2 = r.lightmapSetup[2], o.pad = 0;
    return o;
}

/*
 * The radiosity cache: rad_trace's ids, jobs and rectangles kept on the device, and the scratch of a
 * solve. A call's palette and pointer array go through a pinned staging block of their own, so that a call never
 * writes what an earlier call's copy may still read.
 */
struct fmgi_rad_cache {
    struct Stage {
        void *host = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr; /* recorded after the call that used the block */
        bool used = false;
    };
    int device = 0;
    struct fmgi_rad_cache_info info;
    int nr = 0, nemit = 0, first_emit = 0;
    int64_t njobs = 0, ntex = 0, num_texels = 0;
    DevBuf rects, jobs, sids;
    DevBuf src, dst, dest, params; /* the scratch: three tables of a pass, and a call's pointers and palette */
    int table_kp = 0;              /* slots per texel the tables have room for */
    size_t params_cap = 0;
    std::vector<Stage> stages;
    hipEvent_t ev_solve = nullptr; /* the last launch that uses the scratch */
    bool pending = false;
    ~fmgi_rad_cache() {
        for (auto &s : stages) {
            if (s.done) hipEventDestroy(s.done);
            if (s.host) hipHostFree(s.host);
        }
        if (ev_solve) hipEventDestroy(ev_solve);
    }
};

namespace {

constexpr int RAD_MAX_STAGES = 8;

int64_t rad_cache_bytes(int64_t njobs, int64_t nr) {
    return njobs * FMGI_RAD_RAYS * 4 + njobs * (int64_t)sizeof(RadJob) + nr * (int64_t)sizeof(RadRect);
}

int rad_cache_create(const fmgi_geometry *geo, fmgi_rad_cache **out) {
    static const char fn[] = "fmgi_rad_cache_create";
    if (!out) return arg_err(fn, "null out");
    *out = nullptr;
    int rc = check_geometry(geo, fn);
    if (rc != FMGI_OK) return rc;
    RadPrep p;
    if ((rc = rad_prepare(geo, fn, p)) != FMGI_OK) return rc;
    if ((rc = rad_no_device(p)) != FMGI_OK) return rc;

    fmgi_rad_cache *c = new fmgi_rad_cache;
    RadDev d;
    fmgi_rad_stats st;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    memset(&st, 0, sizeof st);
    memset(&c->info, 0, sizeof c->info);
    {
        const char *dv = getenv("FMGI_DEVICE");
        c->device = dv ? atoi(dv) : 0;
        RADCHK(hipSetDevice(c->device));
    }
    for (auto &e : ev) RADCHK(hipEventCreate(&e));
    RADCHK(hipEventCreateWithFlags(&c->ev_solve, hipEventDisableTiming));
    if ((rc = rad_trace(p, d, st, ev)) != FMGI_OK) goto done;
    std::swap(c->rects.p, d.rects.p);
    std::swap(c->jobs.p, d.jobs.p);
    std::swap(c->sids.p, d.sids.p);
    c->nr = p.nr;
    c->nemit = geo->numWindows + geo->numLights;
    c->first_emit = geo->numWalls;
    c->njobs = p.njobs;
    c->ntex = p.ntex;
    c->num_texels = geo->numTexels;
    c->info.jobs = p.njobs;
    c->info.rects = p.nr;
    c->info.windows = geo->numWindows;
    c->info.lights = geo->numLights;
    c->info.texels = p.ntex;
    c->info.rays = st.rays;
    c->info.bytes = rad_cache_bytes(p.njobs, p.nr);
    c->info.rand_ms = st.rand_ms;
    c->info.rays_ms = st.rays_ms;
    p.advance();
    *out = c;
    c = nullptr;
done:
    if (rc != FMGI_OK) p.restore();
    for (auto &e : ev)
        if (e) hipEventDestroy(e);
    delete c; /* on an error: nothing stays allocated */
    return rc;
}

/* a pinned block of `bytes` that no earlier call's copy still reads */
int rad_stage(fmgi_rad_cache *c, size_t bytes, fmgi_rad_cache::Stage **out) {
    int rc = FMGI_OK;
    fmgi_rad_cache::Stage *s = nullptr;
    for (auto &t : c->stages)
        if (!t.used || hipEventQuery(t.done) == hipSuccess) {
            t.used = false;
            if (!s) s = &t;
        }
    if (!s && (int)c->stages.size() >= RAD_MAX_STAGES) { /* that many calls in flight: wait for the oldest block */
        s = &c->stages[0];
        RADCHK(hipEventSynchronize(s->done));
        s->used = false;
    }
    if (!s) {
        c->stages.reserve(RAD_MAX_STAGES);
        c->stages.emplace_back();
        s = &c->stages.back();
        RADCHK(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
    }
    if (s->cap < bytes) {
        if (s->host) hipHostFree(s->host);
        s->host = nullptr;
        s->cap = 0;
        RADCHK(hipHostMalloc(&s->host, bytes, hipHostMallocDefault));
        s->cap = bytes;
    }
    *out = s;
done:
    return rc;
}

/* the scratch tables with room for kp_need slots of 16 B per texel; the caller has waited for what used them */
int rad_tables(fmgi_rad_cache *c, int kp_need) {
    int rc = FMGI_OK;
    if (c->table_kp < kp_need) {
        const size_t tb = (size_t)c->ntex * (size_t)kp_need * 16;
        c->table_kp = 0;
        c->src.release(), c->dst.release(), c->dest.release();
        RADCHK(c->src.alloc(tb));
        RADCHK(c->dst.alloc(tb));
        RADCHK(c->dest.alloc(tb));
        c->table_kp = kp_need;
    }
done:
    return rc;
}

int rad_cache_solve(fmgi_rad_cache *c, const float *emit, int num_sets, int iterations, void *const *texels_dev,
                    hipStream_t st) {
    static const char fn[] = "fmgi_rad_cache_solve";
    if (!c || !texels_dev || (c->nemit && !emit)) return arg_err(fn, "null argument");
    if (num_sets < 1) return arg_err(fn, "num_sets < 1");
    if (iterations < 1 || iterations > FMGI_RAD_CACHE_MAX_ITERATIONS) return arg_err(fn, "iterations outside 1..64");
    for (int k = 0; k < num_sets; k++)
        if (!texels_dev[k] && c->num_texels) return arg_err(fn, "null set");
    const size_t nvals = (size_t)num_sets * (size_t)c->nemit * 3;
    for (size_t i = 0; i < nvals; i++)
        if (!(emit[i] >= 0) || isinf(emit[i])) return arg_err(fn, "an emit value is negative, NaN or infinite");
    if (c->num_texels == 0) return FMGI_OK; /* no walls: nothing to solve and nothing to write */

    int rc = FMGI_OK;
    const int first_pass = std::min(num_sets, FMGI_RAD_CACHE_MAX_SETS);
    int kp_need = 1;
    while (kp_need < first_pass) kp_need <<= 1;
    const size_t ptr_bytes = ((size_t)num_sets * sizeof(void *) + 15) / 16 * 16, bytes = ptr_bytes + std::max<size_t>(nvals, 1) * 4;
    fmgi_rad_cache::Stage *stage = nullptr;
    RadSolve b;
    memset(&b, 0, sizeof b);
    RADCHK(hipSetDevice(c->device));
    if (c->table_kp < kp_need || c->params_cap < bytes) { /* grow the scratch once nothing uses it any more */
        if (c->pending) RADCHK(hipEventSynchronize(c->ev_solve));
        c->pending = false;
        if ((rc = rad_tables(c, kp_need)) != FMGI_OK) goto done;
        if (c->params_cap < bytes) {
            c->params_cap = 0;
            c->params.release();
            RADCHK(c->params.alloc(bytes));
            c->params_cap = bytes;
        }
    }
    if ((rc = rad_stage(c, bytes, &stage)) != FMGI_OK) goto done;
    memcpy(stage->host, texels_dev, (size_t)num_sets * sizeof(void *));
    if (nvals) memcpy((char *)stage->host + ptr_bytes, emit, nvals * 4);
    /* an earlier call, maybe on another stream, may still use the scratch */
    if (c->pending) RADCHK(hipStreamWaitEvent(st, c->ev_solve, 0));
    RADCHK(hipMemcpyAsync(c->params.p, stage->host, bytes, hipMemcpyHostToDevice, st));
    stage->used = true;
    RADCHK(hipEventRecord(stage->done, st)); /* the kernels read the device copy: the block is free after the copy */
    b.sids = c->sids.as<int32_t>();
    b.jobs = c->jobs.as<RadJob>();
    b.njobs = c->njobs;
    b.rects = c->rects.as<RadRect>();
    b.nrects = c->nr;
    b.ntex = c->ntex;
    b.num_texels = c->num_texels;
    b.dest = c->dest.as<float4>();
    b.keep = 1 - FMGI_RAD_REFLECTANCE;
    b.gain = FMGI_RAD_REFLECTANCE / FMGI_RAD_RAYS;
    for (int k0 = 0; k0 < num_sets; k0 += FMGI_RAD_CACHE_MAX_SETS) {
        const int n = std::min(FMGI_RAD_CACHE_MAX_SETS, num_sets - k0);
        float4 *src = c->src.as<float4>(), *dst = c->dst.as<float4>();
        b.kp = 1;
        while (b.kp < n) b.kp <<= 1;
        const size_t tb = (size_t)c->ntex * (size_t)b.kp * 16;
        /* walls and padding slots start at 0; the sums of texels no ray starts from stay 0 */
        RADCHK(hipMemsetAsync(src, 0, tb, st));
        RADCHK(hipMemsetAsync(b.dest, 0, tb, st));
        b.src = nullptr;
        b.dst = src;
        RADCHK(fmgi_rad_launch_init_sets(b, (const float *)((const char *)c->params.p + ptr_bytes) + (size_t)k0 * c->nemit * 3,
                                         n, c->nemit, c->first_emit, st));
        /* every round builds the mip levels, as the reference does: only the last round's are read, but they
           cost one small launch per round next to the gather */
        for (int it = 0; it < iterations; it++) {
            b.src = src;
            b.dst = dst;
            RADCHK(fmgi_rad_launch_bounce_sets(b, st));
            std::swap(src, dst);
        }
        b.src = src;
        RADCHK(fmgi_rad_launch_unpack_sets(b, (void *const *)c->params.p + k0, n, st));
    }
    RADCHK(hipEventRecord(c->ev_solve, st));
    c->pending = true;
done:
    return rc;
}


static_assert(FMGI_SUN_BOUNCE_DIRS == FMGI_SUN_BOUNCE_MAX_DIRS && FMGI_SUN_BOUNCES == FMGI_SUN_MAX_BOUNCES,
              "kernel and ABI limits differ");

/* DESIGN §21. The per-direction values go to the kernels as arguments: nothing of the caller's is read later. */
int rad_cache_sun_bounce(fmgi_rad_cache *c, void *const *cover_dev, const float *to_sun, const int *samples, int num_dirs,
                         int bounces, void *const *bounce_dev, hipStream_t st) {
    static const char fn[] = "fmgi_rad_cache_sun_bounce";
    if (!c || !cover_dev || !to_sun || !samples || !bounce_dev) return arg_err(fn, "null argument");
    if (num_dirs < 1) return arg_err(fn, "num_dirs < 1");
    if (bounces < 1 || bounces > FMGI_SUN_MAX_BOUNCES) return arg_err(fn, "bounces outside 1..8");
    std::vector<float> s((size_t)num_dirs * 3);
    for (int k = 0; k < num_dirs; k++) {
        if ((!cover_dev[k] || !bounce_dev[k]) && c->num_texels) return arg_err(fn, "a coverage map or an output is NULL");
        if (samples[k] < 1 || samples[k] > FMGI_SUN_MAX_SAMPLES) return arg_err(fn, "samples outside 1..8");
        if (!fmgi_sun_unit_vector(to_sun + 3 * (size_t)k, &s[3 * (size_t)k]))
            return arg_err(fn, "to_sun has a zero or non-finite length");
    }
    {
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count < 1)
            return internal_set_err(FMGI_ERR_NO_DEVICE, "no HIP device visible");
    }
    if (c->num_texels == 0) return FMGI_OK; /* no walls: nothing to gather and nothing to write */

    int rc = FMGI_OK;
    const int first_pass = std::min(num_dirs, FMGI_SUN_BOUNCE_MAX_DIRS);
    int kp_first = 1;
    while (kp_first < first_pass) kp_first <<= 1;
    const int kp_need = std::max(1, kp_first / 4); /* the scratch counts slots of 16 B */
    SunBounce b;
    memset(&b, 0, sizeof b);
    RADCHK(hipSetDevice(c->device));
    if (c->table_kp < kp_need) { /* grow the scratch once nothing uses it any more */
        if (c->pending) RADCHK(hipEventSynchronize(c->ev_solve));
        c->pending = false;
        if ((rc = rad_tables(c, kp_need)) != FMGI_OK) goto done;
    }
    /* an earlier call, maybe on another stream, may still use the scratch */
    if (c->pending) RADCHK(hipStreamWaitEvent(st, c->ev_solve, 0));
    b.sids = c->sids.as<int32_t>();
    b.jobs = c->jobs.as<RadJob>();
    b.njobs = c->njobs;
    b.rects = c->rects.as<RadRect>();
    b.nwalls = c->first_emit;
    b.ntex = c->ntex;
    b.num_texels = c->num_texels;
    for (int k0 = 0; k0 < num_dirs; k0 += FMGI_SUN_BOUNCE_MAX_DIRS) {
        const int n = std::min(FMGI_SUN_BOUNCE_MAX_DIRS, num_dirs - k0);
        float *src = c->src.as<float>(), *dst = c->dst.as<float>();
        SunBounceDirs d;
        memset(&d, 0, sizeof d);
        for (int k = 0; k < n; k++) {
            d.cover[k] = (const uint8_t *)cover_dev[k0 + k];
            d.out[k] = (float *)bounce_dev[k0 + k];
            d.sx[k] = s[3 * (size_t)(k0 + k)], d.sy[k] = s[3 * (size_t)(k0 + k) + 1], d.sz[k] = s[3 * (size_t)(k0 + k) + 2];
            d.s2[k] = (float)(samples[k0 + k] * samples[k0 + k]);
        }
        b.kp = 1;
        while (b.kp < n) b.kp <<= 1;
        b.ndirs = n;
        const size_t tb = (size_t)c->ntex * (size_t)b.kp * 4;
        /* both tables start at +0: the padding slots, the texels no wall faces and no ray starts from. Every later
           round overwrites exactly the jobs' texels, which are the level-0 texels the start table fills. */
        RADCHK(hipMemsetAsync(src, 0, tb, st));
        RADCHK(hipMemsetAsync(dst, 0, tb, st));
        b.src = nullptr;
        b.dst = src;
        RADCHK(fmgi_sun_bounce_launch_e0(b, d, st));
        for (int it = 0; it < bounces; it++) {
            b.src = src;
            b.dst = dst;
            RADCHK(fmgi_sun_bounce_launch_gather(b, st));
            b.src = dst;
            b.row = it;
            RADCHK(fmgi_sun_bounce_launch_unpack(b, d, st));
            std::swap(src, dst);
        }
    }
    RADCHK(hipEventRecord(c->ev_solve, st));
    c->pending = true;
done:
    return rc;
}

} // namespace

FMGI_API int64_t fmgi_rad_cache_bytes(const fmgi_geometry *geo) {
    const int rc = check_geometry(geo, "fmgi_rad_cache_bytes");
    if (rc != FMGI_OK) return rc;
    return rad_cache_bytes(count_jobs(geo), (int64_t)geo->numWalls + geo->numWindows + geo->numLights);
}

FMGI_API int fmgi_rad_cache_create(const fmgi_geometry *geo, fmgi_rad_cache **out) { return rad_cache_create(geo, out); }

FMGI_API void fmgi_rad_cache_destroy(fmgi_rad_cache *c) {
    if (!c) return;
    if (c->pending) hipEventSynchronize(c->ev_solve); /* launches may still use what the handle owns */
    delete c;
}

FMGI_API int fmgi_rad_cache_info(const fmgi_rad_cache *c, struct fmgi_rad_cache_info *out) {
    if (!c || !out) return arg_err("fmgi_rad_cache_info", "null argument");
    *out = c->info;
    return FMGI_OK;
}

FMGI_API int fmgi_rad_cache_sids(const fmgi_rad_cache *c, int32_t *sids_out) {
    if (!c || (!sids_out && c->njobs)) return arg_err("fmgi_rad_cache_sids", "null argument");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return internal_set_err(FMGI_ERR_HIP, hipGetErrorString(e));
    return download_sids(c->sids.as<int32_t>(), c->njobs, sids_out);
}

FMGI_API int fmgi_rad_reference_emit(const fmgi_geometry *geo, float *emit) {
    static const char fn[] = "fmgi_rad_reference_emit";
    if (!geo) return arg_err(fn, "null geometry");
    if (geo->numWindows < 0 || geo->numLights < 0) return arg_err(fn, "bad geometry");
    if (!emit && geo->numWindows + geo->numLights) return arg_err(fn, "null emit");
    for (int i = 0; i < geo->numWindows; i++) emit[3 * i] = emit[3 * i + 1] = emit[3 * i + 2] = FMGI_RAD_WINDOW;
    for (int i = geo->numWindows; i < geo->numWindows + geo->numLights; i++)
        emit[3 * i] = FMGI_RAD_LIGHT_R, emit[3 * i + 1] = FMGI_RAD_LIGHT_G, emit[3 * i + 2] = FMGI_RAD_LIGHT_B;
    return FMGI_OK;
}

FMGI_API int fmgi_rad_cache_solve(const fmgi_rad_cache *c, const float *emit, int num_sets, int iterations,
                                  void *const *texels_dev, void *stream) {
    return rad_cache_solve(const_cast<fmgi_rad_cache *>(c), emit, num_sets, iterations, texels_dev, (hipStream_t)stream);
}

FMGI_API int fmgi_rad_cache_sun_bounce(const fmgi_rad_cache *c, void *const *cover_dev, const float *to_sun,
                                       const int *samples, int num_dirs, int bounces, void *const *bounce_dev,
                                       void *stream) {
    return rad_cache_sun_bounce(const_cast<fmgi_rad_cache *>(c), cover_dev, to_sun, samples, num_dirs, bounces, bounce_dev,
                                (hipStream_t)stream);
}

FMGI_API int fmgi_radiosity(const fmgi_geometry *geo, fmgi_vec3 *texels_out, int32_t *sids_out) {
    return rad_run(geo, texels_out, sids_out);
}

FMGI_API int fmgi_rand_skip(uint64_t n) {
    LibcRand libc;
    uint32_t v[DEG];
    if (!libc.read(v)) return internal_set_err(FMGI_ERR_ARG, "fmgi_rand_skip: libc rand() is not in glibc's TYPE_3 state");
    mat_vec(mat_pow(step_matrix(), n), v, v);
    libc.write(v, n);
    return FMGI_OK;
}

FMGI_API int64_t fmgi_radiosity_jobs(const fmgi_geometry *geo) {
    if (!geo || (geo->numWalls && !geo->walls)) return internal_set_err(FMGI_ERR_ARG, "bad geometry");
    return count_jobs(geo);
}

FMGI_API int fmgi_radiosity_stats(fmgi_rad_stats *out) {
    if (!out) return internal_set_err(FMGI_ERR_ARG, "null stats");
    *out = g_stats;
    return FMGI_OK;
}

FMGI_API void performRadiosityGpu(fmgi_geometry *geo) {
    const int rc = rad_run(geo, geo ? geo->texels : nullptr, nullptr);
    if (rc != FMGI_OK) {
        printf("[Err] performRadiosityGpu: %s\n", fmgi_last_error());
        fflush(stdout);
        exit(-1);
    }
}
