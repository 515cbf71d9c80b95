/*
 * fmgi_view_host.cpp -- host side of the view renderer and its C ABI (include/flatmatch_gi.h:
 * fmgi_render_views, fmgi_view_candidates, fmgi_view_stats). The reference is the debug raycaster
 * (debugRaytracer.cc:121-176) over getSortedIntersectableRects / findClosestIntersectionSorted
 * (radiosityNative.c:25-90).
 *
 * The host checks every argument before the first device call, sets each camera up in fp32 in the
 * reference's order (built with -ffp-contract=off, no FMA), uploads the walls as the radiosity backend's
 * RadRect / AoRect images, runs the two kernels (fmgi_view.hip) over chunks of cameras and copies the
 * requested outputs back. fmgi_shade_views (supersampled, filtered views; no reference program) takes the same
 * path into k_view_shade, in launches of a bounded number of rays. fmgi_view_cache_* (traced views)
 * casts the same rays once with k_view_trace and shades device-resident lightmaps with k_output's read-only form
 * and k_view_resolve, asynchronously on the caller's stream. The *_proj entry points pass a projection
 * through the same functions: the pin-hole takes the calls above unchanged, the orthographic and equirectangular
 * cameras get an orthonormal frame in their ViewCam and the _proj instances of the three kernels. The *_gloss entry
 * points pass a mirror weight through the same functions: with gloss > 0 (or for create_gloss) they build
 * the mirror lists and launch the _gloss kernels, with gloss == 0 they are the calls above.
 */
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/flatmatch_gi.h"
#include "fmgi_output.h"
#include "fmgi_view.h"

#define FMGI_API extern "C" __attribute__((visibility("default")))

int internal_set_err(int code, const char *msg);

namespace {

struct F3 {
    float x, y, z;
};
F3 add(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
F3 mul(F3 a, float f) { return F3{a.x * f, a.y * f, a.z * f}; }
F3 cross(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float length(F3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
F3 normalized(F3 a) { return mul(a, 1.0f / length(a)); } /* vector3_cl.c:95-101 */

struct fmgi_view_stats g_stats;
struct fmgi_view_gloss_stats g_gloss; /* of the last gloss call; any other view call zeroes it */

#define VIEWCHK(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            char b_[256];                                                                              \
            snprintf(b_, sizeof b_, "%s: %s", #expr, hipGetErrorString(e_));                           \
            rc = internal_set_err(e_ == hipErrorOutOfMemory ? FMGI_ERR_OOM : FMGI_ERR_HIP, b_);        \
            goto done;                                                                                 \
        }                                                                                              \
    } while (0)

/* the walls as both backends' device images, and the tiles' running sum */
struct Walls {
    std::vector<RadRect> rects;
    std::vector<AoRect> hits;
    std::vector<int64_t> first_tile;
    int sort_n = 2;
};

/* an argument error of the entry point fn */
int arg_err(const char *fn, const char *msg) {
    char b[256];
    snprintf(b, sizeof b, "%s: %s", fn, msg);
    return internal_set_err(FMGI_ERR_ARG, b);
}

int check_geometry(const fmgi_geometry *geo, Walls &w, const char *fn) {
    if (!geo) return arg_err(fn, "null geometry");
    if (geo->numWalls < 0 || geo->numTexels < 0 || (geo->numWalls && !geo->walls))
        return arg_err(fn, "bad geometry");
    if (geo->numWalls > FMGI_RAD_MAX_SORT)
        return arg_err(fn, "more walls than the candidate sort holds (16384)");
    const int nr = geo->numWalls;
    w.rects.resize((size_t)std::max(nr, 1));
    w.hits.resize((size_t)std::max(nr, 1));
    w.first_tile.resize((size_t)std::max(nr, 1));
    int64_t tiles = 0;
    for (int i = 0; i < nr; i++) {
        const fmgi_rect &r = geo->walls[i];
        const int32_t *lm = r.lightmapSetup;
        if (lm[1] < 1 || lm[2] < 1 || lm[0] < 0 || (int64_t)lm[1] * lm[2] > (1 << 28) ||
            (int64_t)lm[0] + (int64_t)lm[1] * lm[2] > geo->numTexels)
            return arg_err(fn, "a wall's texels lie outside numTexels");
        w.rects[(size_t)i] = fmgi_rad_rect(r);
        w.hits[(size_t)i] = fmgi_rad_hit_rect(r);
        w.first_tile[(size_t)i] = tiles;
        tiles += (int64_t)lm[1] * lm[2];
    }
    while (w.sort_n < nr) w.sort_n <<= 1;
    return FMGI_OK;
}

/* debugRaytracer.cc:121-125 */
int make_cam(const fmgi_camera &c, ViewCam &o, const char *fn, bool reads_pixel = true) {
    if (reads_pixel && (!(c.pixel > 0) || !isfinite(c.pixel)))
        return arg_err(fn, "a camera's pixel size is not finite and positive");
    const F3 pos{c.pos[0], c.pos[1], c.pos[2]}, d{c.dir[0], c.dir[1], c.dir[2]}, up{c.up[0], c.up[1], c.up[2]};
    const float len = length(d);
    if (!(len > 0) || !isfinite(len))
        return arg_err(fn, "a camera's direction has no length");
    const F3 dir = normalized(d);
    const F3 centre = add(pos, dir);
    const F3 right = cross(dir, up);
    o.px = pos.x, o.py = pos.y, o.pz = pos.z;
    o.dx = dir.x, o.dy = dir.y, o.dz = dir.z;
    o.cx = centre.x, o.cy = centre.y, o.cz = centre.z;
    o.rx = right.x, o.ry = right.y, o.rz = right.z;
    o.ux = up.x, o.uy = up.y, o.uz = up.z;
    o.pixel = reads_pixel ? c.pixel : 0.0f;
    return FMGI_OK;
}

static_assert(FMGI_VIEW_PINHOLE == FMGI_PROJ_PINHOLE && FMGI_VIEW_ORTHO == FMGI_PROJ_ORTHO &&
                  FMGI_VIEW_EQUIRECT == FMGI_PROJ_EQUIRECT, "kernel and ABI projections differ");

/* a call's cameras: make_cam's checks for every camera (EQUIRECT does not read the pixel size), then the
   projection, then, for ORTHO and EQUIRECT, the orthonormal frame: r = normalized(cross(f, up)),
   u = cross(r, f) */
int make_cams(const fmgi_camera *cams, int n, int projection, std::vector<ViewCam> &vc, const char *fn) {
    int rc;
    for (int i = 0; i < n; i++)
        if ((rc = make_cam(cams[i], vc[(size_t)i], fn, projection != FMGI_PROJ_EQUIRECT)) != FMGI_OK) return rc;
    if (projection == FMGI_PROJ_PINHOLE) return FMGI_OK;
    if (projection != FMGI_PROJ_ORTHO && projection != FMGI_PROJ_EQUIRECT)
        return arg_err(fn, "projection is none of pinhole, ortho and equirect");
    for (int i = 0; i < n; i++) {
        ViewCam &o = vc[(size_t)i];
        const F3 f{o.dx, o.dy, o.dz}, r0{o.rx, o.ry, o.rz}; /* make_cam's cross(f, up) */
        const float len = length(r0);
        if (!(len > 0) || !isfinite(len) || !isfinite(1.0f / len))
            return arg_err(fn, "a camera's up vector is parallel to its direction: cross(dir, up) has no length");
        const F3 r = normalized(r0), u = cross(r, f);
        o.rx = r.x, o.ry = r.y, o.rz = r.z;
        o.ux = u.x, o.uy = u.y, o.uz = u.z;
    }
    return FMGI_OK;
}

int no_device() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count <= 0)
        return internal_set_err(FMGI_ERR_NO_DEVICE, "no HIP device visible");
    return FMGI_OK;
}

int view_run(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
             const uint8_t *tiles_rgb, const uint8_t *background, int32_t *wall_out, int32_t *texel_out,
             float *dist_out, uint8_t *rgb_out) {
    static const char fn[] = "fmgi_render_views";
    Walls w;
    int rc = check_geometry(geo, w, fn);
    if (rc != FMGI_OK) return rc;
    if (width < 1 || height < 1 || width > FMGI_VIEW_MAX_DIM || height > FMGI_VIEW_MAX_DIM)
        return internal_set_err(FMGI_ERR_ARG, "fmgi_render_views: bad image size");
    if (num_cams < 0 || (num_cams && !cams)) return internal_set_err(FMGI_ERR_ARG, "fmgi_render_views: bad cameras");
    if (rgb_out && !tiles_rgb) return internal_set_err(FMGI_ERR_ARG, "fmgi_render_views: rgb_out needs tiles_rgb");
    std::vector<ViewCam> vc((size_t)std::max(num_cams, 1));
    for (int i = 0; i < num_cams; i++)
        if ((rc = make_cam(cams[i], vc[(size_t)i], fn)) != FMGI_OK) return rc;
    memset(&g_stats, 0, sizeof g_stats);
    memset(&g_gloss, 0, sizeof g_gloss);
    if (num_cams == 0) return FMGI_OK;
    if ((rc = no_device()) != FMGI_OK) return rc;

    const int nr = geo->numWalls;
    const int64_t pix = (int64_t)width * height;
    /* cameras per launch: at most 2^26 pixels of outputs on the device at a time */
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)num_cams, FMGI_VIEW_MAX_BATCH, ((int64_t)1 << 26) / pix}));
    const int64_t tile_bytes = 3 * (w.first_tile[(size_t)std::max(nr, 1) - 1] +
                                    (nr ? (int64_t)geo->walls[nr - 1].lightmapSetup[1] * geo->walls[nr - 1].lightmapSetup[2] : 0));
    RadRect *d_rects = nullptr;
    AoRect *d_hits = nullptr;
    ViewCam *d_cams = nullptr;
    unsigned long long *d_keys = nullptr, *d_tests = nullptr;
    int32_t *d_counts = nullptr, *d_wall = nullptr, *d_texel = nullptr;
    int64_t *d_first = nullptr;
    uint8_t *d_tiles = nullptr, *d_rgb = nullptr;
    float *d_dist = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<int32_t> counts((size_t)batch);
    unsigned long long tests = 0;
    ViewArgs a;
    memset(&a, 0, sizeof a);
    {
        const char *dv = getenv("FMGI_DEVICE");
        VIEWCHK(hipSetDevice(dv ? atoi(dv) : 0));
    }
    for (auto &e : ev) VIEWCHK(hipEventCreate(&e));
    VIEWCHK(hipEventRecord(ev[0], nullptr));
    VIEWCHK(hipMalloc(&d_rects, w.rects.size() * sizeof(RadRect)));
    VIEWCHK(hipMemcpy(d_rects, w.rects.data(), w.rects.size() * sizeof(RadRect), hipMemcpyHostToDevice));
    VIEWCHK(hipMalloc(&d_hits, w.hits.size() * sizeof(AoRect)));
    VIEWCHK(hipMemcpy(d_hits, w.hits.data(), w.hits.size() * sizeof(AoRect), hipMemcpyHostToDevice));
    VIEWCHK(hipMalloc(&d_cams, (size_t)batch * sizeof(ViewCam)));
    VIEWCHK(hipMalloc(&d_keys, (size_t)batch * w.sort_n * 8));
    VIEWCHK(hipMalloc(&d_counts, (size_t)batch * 4));
    VIEWCHK(hipMalloc(&d_tests, 8));
    VIEWCHK(hipMemset(d_tests, 0, 8));
    if (wall_out) VIEWCHK(hipMalloc(&d_wall, (size_t)batch * pix * 4));
    if (texel_out) VIEWCHK(hipMalloc(&d_texel, (size_t)batch * pix * 4));
    if (dist_out) VIEWCHK(hipMalloc(&d_dist, (size_t)batch * pix * 4));
    if (rgb_out) {
        VIEWCHK(hipMalloc(&d_rgb, (size_t)batch * pix * 3));
        VIEWCHK(hipMalloc(&d_first, w.first_tile.size() * 8));
        VIEWCHK(hipMemcpy(d_first, w.first_tile.data(), w.first_tile.size() * 8, hipMemcpyHostToDevice));
        VIEWCHK(hipMalloc(&d_tiles, (size_t)std::max<int64_t>(tile_bytes, 1)));
        if (tile_bytes) VIEWCHK(hipMemcpy(d_tiles, tiles_rgb, (size_t)tile_bytes, hipMemcpyHostToDevice));
    }
    a.rects = d_rects;
    a.hits = d_hits;
    a.nrects = nr;
    a.sort_n = w.sort_n;
    a.cams = d_cams;
    a.width = width;
    a.height = height;
    a.keys = d_keys;
    a.counts = d_counts;
    a.first_tile = d_first;
    a.tiles_rgb = d_tiles;
    a.background = background ? ((uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16)) : 0;
    a.wall_out = d_wall;
    a.texel_out = d_texel;
    a.dist_out = d_dist;
    a.rgb_out = d_rgb;
    a.tests = d_tests;
    for (int c0 = 0; c0 < num_cams; c0 += batch) {
        const int n = std::min(batch, num_cams - c0);
        const size_t px = (size_t)n * pix, o = (size_t)c0 * pix;
        a.ncams = n;
        VIEWCHK(hipMemcpy(d_cams, vc.data() + c0, (size_t)n * sizeof(ViewCam), hipMemcpyHostToDevice));
        VIEWCHK(hipEventRecord(ev[1], nullptr));
        VIEWCHK(fmgi_view_launch_candidates(a, nullptr));
        VIEWCHK(hipEventRecord(ev[2], nullptr));
        VIEWCHK(fmgi_view_launch_rays(a, nullptr));
        VIEWCHK(hipEventRecord(ev[3], nullptr));
        VIEWCHK(hipEventSynchronize(ev[3]));
        float ms = 0;
        VIEWCHK(hipEventElapsedTime(&ms, ev[1], ev[2]));
        g_stats.cand_ms += ms;
        VIEWCHK(hipEventElapsedTime(&ms, ev[2], ev[3]));
        g_stats.rays_ms += ms;
        VIEWCHK(hipEventElapsedTime(&ms, ev[0], ev[3]));
        g_stats.total_ms = ms;
        VIEWCHK(hipMemcpy(counts.data(), d_counts, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) g_stats.candidates += counts[(size_t)i];
        if (wall_out) VIEWCHK(hipMemcpy(wall_out + o, d_wall, px * 4, hipMemcpyDeviceToHost));
        if (texel_out) VIEWCHK(hipMemcpy(texel_out + o, d_texel, px * 4, hipMemcpyDeviceToHost));
        if (dist_out) VIEWCHK(hipMemcpy(dist_out + o, d_dist, px * 4, hipMemcpyDeviceToHost));
        if (rgb_out) VIEWCHK(hipMemcpy(rgb_out + 3 * o, d_rgb, px * 3, hipMemcpyDeviceToHost));
    }
    VIEWCHK(hipMemcpy(&tests, d_tests, 8, hipMemcpyDeviceToHost));
    g_stats.cameras = num_cams;
    g_stats.rays = (int64_t)num_cams * pix;
    g_stats.tests = (int64_t)tests;
done:
    for (auto &e : ev)
        if (e) hipEventDestroy(e);
    hipFree(d_rects);
    hipFree(d_hits);
    hipFree(d_cams);
    hipFree(d_keys);
    hipFree(d_counts);
    hipFree(d_tests);
    hipFree(d_wall);
    hipFree(d_texel);
    hipFree(d_dist);
    hipFree(d_rgb);
    hipFree(d_first);
    hipFree(d_tiles);
    return rc;
}

int candidates_run(const fmgi_geometry *geo, const fmgi_camera *cam, int projection, int32_t *wall_idx,
                   float *min_dist, int cap) {
    Walls w;
    int rc = check_geometry(geo, w, "fmgi_view_candidates");
    if (rc != FMGI_OK) return rc;
    if (!cam) return internal_set_err(FMGI_ERR_ARG, "fmgi_view_candidates: null camera");
    std::vector<ViewCam> one(1);
    if ((rc = make_cams(cam, 1, projection, one, "fmgi_view_candidates")) != FMGI_OK) return rc;
    const ViewCam vc = one[0];
    if ((rc = no_device()) != FMGI_OK) return rc;
    RadRect *d_rects = nullptr;
    ViewCam *d_cams = nullptr;
    unsigned long long *d_keys = nullptr;
    int32_t *d_counts = nullptr;
    std::vector<unsigned long long> keys((size_t)w.sort_n);
    int32_t count = 0;
    ViewArgs a;
    memset(&a, 0, sizeof a);
    {
        const char *dv = getenv("FMGI_DEVICE");
        VIEWCHK(hipSetDevice(dv ? atoi(dv) : 0));
    }
    VIEWCHK(hipMalloc(&d_rects, w.rects.size() * sizeof(RadRect)));
    VIEWCHK(hipMemcpy(d_rects, w.rects.data(), w.rects.size() * sizeof(RadRect), hipMemcpyHostToDevice));
    VIEWCHK(hipMalloc(&d_cams, sizeof(ViewCam)));
    VIEWCHK(hipMemcpy(d_cams, &vc, sizeof(ViewCam), hipMemcpyHostToDevice));
    VIEWCHK(hipMalloc(&d_keys, (size_t)w.sort_n * 8));
    VIEWCHK(hipMalloc(&d_counts, 4));
    a.rects = d_rects;
    a.nrects = geo->numWalls;
    a.sort_n = w.sort_n;
    a.cams = d_cams;
    a.ncams = 1;
    a.keys = d_keys;
    a.counts = d_counts;
    if (projection == FMGI_PROJ_PINHOLE) VIEWCHK(fmgi_view_launch_candidates(a, nullptr));
    else VIEWCHK(fmgi_view_launch_candidates_proj(a, projection, nullptr));
    VIEWCHK(hipMemcpy(keys.data(), d_keys, keys.size() * 8, hipMemcpyDeviceToHost));
    VIEWCHK(hipMemcpy(&count, d_counts, 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < std::min(count, std::max(cap, 0)); i++) {
        const uint32_t bits = (uint32_t)(keys[(size_t)i] >> 32);
        if (wall_idx) wall_idx[i] = (int32_t)(uint32_t)keys[(size_t)i];
        if (min_dist) memcpy(&min_dist[i], &bits, 4);
    }
    rc = count;
done:
    hipFree(d_rects);
    hipFree(d_cams);
    hipFree(d_keys);
    hipFree(d_counts);
    return rc;
}

static_assert(FMGI_VIEW_SAMPLES == FMGI_VIEW_MAX_SAMPLES, "kernel and ABI sample limits differ");

/* a device allocation that lives as long as its scope */
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 1)); }
    template <class T> T *as() const { return (T *)p; }
};

/* a mirror weight the gloss calls take: a number in [0, 1] */
bool bad_gloss(float gloss) { return !(gloss >= 0.0f && gloss <= 1.0f); }

/* rays per k_view_shade launch: FMGI_VIEW_MAX_RAYS, or FMGI_VIEW_RAYS_PER_LAUNCH from the environment (tests
   use it to reach the windowed launches with small images) */
int64_t shade_ray_budget() {
    const char *e = getenv("FMGI_VIEW_RAYS_PER_LAUNCH");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? std::min<int64_t>(v, FMGI_VIEW_MAX_RAYS) : FMGI_VIEW_MAX_RAYS;
}

int shade_run(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
              int projection, const uint8_t *tiles_rgb, const uint8_t *background, int samples, int filter, uint8_t *rgb_out,
              uint8_t *coverage_out, float gloss = 0.0f, const char *fn = "fmgi_shade_views") {
    Walls w;
    int rc = check_geometry(geo, w, fn);
    if (rc != FMGI_OK) return rc;
    if (width < 1 || height < 1 || width > FMGI_VIEW_MAX_DIM || height > FMGI_VIEW_MAX_DIM)
        return arg_err(fn, "bad image size");
    if (num_cams < 0 || (num_cams && !cams)) return arg_err(fn, "bad cameras");
    if (rgb_out && !tiles_rgb) return arg_err(fn, "rgb_out needs tiles_rgb");
    if (samples < 1 || samples > FMGI_VIEW_MAX_SAMPLES) return arg_err(fn, "samples outside 1..8");
    if (filter != FMGI_VIEW_NEAREST && filter != FMGI_VIEW_BILINEAR) return arg_err(fn, "filter is neither nearest nor bilinear");
    std::vector<ViewCam> vc((size_t)std::max(num_cams, 1));
    if ((rc = make_cams(cams, num_cams, projection, vc, fn)) != FMGI_OK) return rc;
    if (bad_gloss(gloss)) return arg_err(fn, "gloss is not a number in [0, 1]");
    memset(&g_stats, 0, sizeof g_stats);
    memset(&g_gloss, 0, sizeof g_gloss);
    if (num_cams == 0) return FMGI_OK;
    if ((rc = no_device()) != FMGI_OK) return rc;

    const bool mirror = gloss > 0.0f; /* gloss == 0 is the call without it: no mirror list, no second walk */
    const int nr = geo->numWalls;
    const int64_t pix = (int64_t)width * height, spp = (int64_t)samples * samples, budget = shade_ray_budget();
    /* cameras per launch: at most 2^26 pixels of outputs on the device, and at most `budget` primary rays */
    const int batch = (int)std::max<int64_t>(
        1, std::min<int64_t>({(int64_t)num_cams, FMGI_VIEW_MAX_BATCH, ((int64_t)1 << 26) / pix, budget / (pix * spp)}));
    /* one camera over the budget: windows of whole workgroup rows, then of workgroup columns */
    int rows = height, cols = width;
    if (pix * spp > budget) {
        const int64_t B = FMGI_VIEW_BLOCK;
        rows = (int)std::min<int64_t>(height, std::max<int64_t>(B, budget / ((int64_t)width * spp) / B * B));
        cols = (int)std::min<int64_t>(width, std::max<int64_t>(B, budget / ((int64_t)rows * spp) / B * B));
    }
    const int64_t ntiles = nr ? w.first_tile[(size_t)nr - 1] + (int64_t)geo->walls[nr - 1].lightmapSetup[1] * geo->walls[nr - 1].lightmapSetup[2] : 0;
    DevBuf d_rects, d_hits, d_cams, d_keys, d_counts, d_tests, d_rgb, d_cov, d_first, d_tiles, d_mkeys, d_mcounts;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<int32_t> counts((size_t)batch);
    unsigned long long tests[4] = {0, 0, 0, 0}; /* tests, then the mirror rays, hits and tests */
    ShadeGlossArgs gq;
    memset(&gq, 0, sizeof gq);
    ShadeProjArgs &q = gq.q;
    ShadeArgs &s = q.s;
    ViewArgs &a = s.v;
    q.kphi = 6.2831855f / (float)width;
    q.ktheta = 3.1415927f / (float)height;
    {
        const char *dv = getenv("FMGI_DEVICE");
        VIEWCHK(hipSetDevice(dv ? atoi(dv) : 0));
    }
    for (auto &e : ev) VIEWCHK(hipEventCreate(&e));
    VIEWCHK(hipEventRecord(ev[0], nullptr));
    VIEWCHK(d_rects.alloc(w.rects.size() * sizeof(RadRect)));
    VIEWCHK(hipMemcpy(d_rects.p, w.rects.data(), w.rects.size() * sizeof(RadRect), hipMemcpyHostToDevice));
    VIEWCHK(d_hits.alloc(w.hits.size() * sizeof(AoRect)));
    VIEWCHK(hipMemcpy(d_hits.p, w.hits.data(), w.hits.size() * sizeof(AoRect), hipMemcpyHostToDevice));
    VIEWCHK(d_cams.alloc((size_t)batch * sizeof(ViewCam)));
    VIEWCHK(d_keys.alloc((size_t)batch * w.sort_n * 8));
    VIEWCHK(d_counts.alloc((size_t)batch * 4));
    VIEWCHK(d_tests.alloc(32));
    VIEWCHK(hipMemset(d_tests.p, 0, 32));
    if (mirror) {
        VIEWCHK(d_mkeys.alloc((size_t)batch * w.sort_n * 8));
        VIEWCHK(d_mcounts.alloc((size_t)batch * 4));
    }
    if (coverage_out) VIEWCHK(d_cov.alloc((size_t)batch * pix));
    if (rgb_out) {
        VIEWCHK(d_rgb.alloc((size_t)batch * pix * 3));
        VIEWCHK(d_first.alloc(w.first_tile.size() * 8));
        VIEWCHK(hipMemcpy(d_first.p, w.first_tile.data(), w.first_tile.size() * 8, hipMemcpyHostToDevice));
        /* the RGB8 tiles go up as they are and are repacked to one word per tile on the device */
        DevBuf d_bytes;
        VIEWCHK(d_bytes.alloc((size_t)ntiles * 3));
        VIEWCHK(d_tiles.alloc((size_t)ntiles * 4));
        if (ntiles) VIEWCHK(hipMemcpy(d_bytes.p, tiles_rgb, (size_t)ntiles * 3, hipMemcpyHostToDevice));
        VIEWCHK(fmgi_view_launch_pack(d_bytes.as<uint8_t>(), d_tiles.as<uint32_t>(), ntiles, nullptr));
        VIEWCHK(hipStreamSynchronize(nullptr));
    }
    a.rects = d_rects.as<RadRect>();
    a.hits = d_hits.as<AoRect>();
    a.nrects = nr;
    a.sort_n = w.sort_n;
    a.cams = d_cams.as<ViewCam>();
    a.width = width;
    a.height = height;
    a.keys = d_keys.as<unsigned long long>();
    a.counts = d_counts.as<int32_t>();
    a.first_tile = d_first.as<int64_t>();
    a.background = background ? ((uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16)) : 0;
    a.rgb_out = d_rgb.as<uint8_t>();
    a.tests = d_tests.as<unsigned long long>();
    s.tiles = d_tiles.as<uint32_t>();
    s.cov_out = d_cov.as<uint8_t>();
    s.samples = samples;
    s.filter = filter;
    for (int i = 0; i < samples; i++) s.offs[i] = (float)(2 * i + 1 - samples) / (float)(2 * samples);
    gq.g.mkeys = d_mkeys.as<unsigned long long>();
    gq.g.counters = d_tests.as<unsigned long long>() + 1;
    gq.g.gloss = gloss;
    for (int c0 = 0; c0 < num_cams; c0 += batch) {
        const int n = std::min(batch, num_cams - c0);
        const size_t px = (size_t)n * pix, o = (size_t)c0 * pix;
        a.ncams = n;
        VIEWCHK(hipMemcpy(d_cams.p, vc.data() + c0, (size_t)n * sizeof(ViewCam), hipMemcpyHostToDevice));
        VIEWCHK(hipEventRecord(ev[1], nullptr));
        if (projection == FMGI_PROJ_PINHOLE) VIEWCHK(fmgi_view_launch_candidates(a, nullptr));
        else VIEWCHK(fmgi_view_launch_candidates_proj(a, projection, nullptr));
        if (mirror) { /* the mirror lists: the same walls and cameras into buffers of their own */
            ViewArgs m = a;
            m.keys = d_mkeys.as<unsigned long long>();
            m.counts = d_mcounts.as<int32_t>();
            VIEWCHK(fmgi_view_launch_candidates_mirror(m, nullptr));
        }
        VIEWCHK(hipEventRecord(ev[2], nullptr));
        for (s.y0 = 0; s.y0 < height; s.y0 += rows)
            for (s.x0 = 0; s.x0 < width; s.x0 += cols) {
                s.y1 = std::min(height, s.y0 + rows);
                s.x1 = std::min(width, s.x0 + cols);
                if (mirror) VIEWCHK(fmgi_view_launch_shade_gloss(gq, projection, nullptr));
                else if (projection == FMGI_PROJ_PINHOLE) VIEWCHK(fmgi_view_launch_shade(s, nullptr));
                else VIEWCHK(fmgi_view_launch_shade_proj(q, projection, nullptr));
            }
        VIEWCHK(hipEventRecord(ev[3], nullptr));
        VIEWCHK(hipEventSynchronize(ev[3]));
        float ms = 0;
        VIEWCHK(hipEventElapsedTime(&ms, ev[1], ev[2]));
        g_stats.cand_ms += ms;
        VIEWCHK(hipEventElapsedTime(&ms, ev[2], ev[3]));
        g_stats.rays_ms += ms;
        VIEWCHK(hipEventElapsedTime(&ms, ev[0], ev[3]));
        g_stats.total_ms = ms;
        VIEWCHK(hipMemcpy(counts.data(), d_counts.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) g_stats.candidates += counts[(size_t)i];
        if (rgb_out) VIEWCHK(hipMemcpy(rgb_out + 3 * o, d_rgb.p, px * 3, hipMemcpyDeviceToHost));
        if (coverage_out) VIEWCHK(hipMemcpy(coverage_out + o, d_cov.p, px, hipMemcpyDeviceToHost));
    }
    VIEWCHK(hipMemcpy(tests, d_tests.p, 32, hipMemcpyDeviceToHost));
    g_stats.cameras = num_cams;
    g_stats.rays = (int64_t)num_cams * pix * spp;
    g_stats.tests = (int64_t)tests[0];
    g_gloss.mirror_rays = (int64_t)tests[1];
    g_gloss.mirror_hits = (int64_t)tests[2];
    g_gloss.mirror_tests = (int64_t)tests[3];
done:
    for (auto &e : ev)
        if (e) hipEventDestroy(e);
    return rc;
}

} // namespace

/*
 * The traced view: fmgi_view_cache_create casts a view's rays once into per-sample records,
 * fmgi_view_cache_tiles runs the output step on device lightmaps and fmgi_view_cache_shade gathers the pictures.
 * The handle owns the records, the output step's wall table and the packed-tile scratch of a pass.
 */
struct fmgi_view_cache {
    int device = 0;
    int projection = FMGI_PROJ_PINHOLE;
    struct fmgi_view_cache_info info;
    std::vector<OutWallIn> walls; /* what the OutWall table is made of; norm follows the call's spa */
    DevBuf records, mrecords, out_walls, packed; /* mrecords: the mirror records' plane, or none */
    bool mirror = false;
    int out_spa = -1;        /* the spa out_walls holds, -1: none yet */
    int packed_sets = 0;     /* sets `packed` has room for */
    hipEvent_t ev_tiles = nullptr, ev_shade = nullptr; /* the last launch that reads out_walls / packed */
    bool tiles_pending = false, shade_pending = false;
    ~fmgi_view_cache() {
        if (ev_tiles) hipEventDestroy(ev_tiles);
        if (ev_shade) hipEventDestroy(ev_shade);
    }
};

static_assert(FMGI_VIEW_SETS == FMGI_VIEW_CACHE_MAX_SETS, "kernel and ABI set limits differ");

namespace {

/* the argument checks fmgi_view_cache_bytes and fmgi_view_cache_create share; nullptr: fine */
const char *cache_shape_error(int num_cams, bool have_cams, int width, int height, int samples, int filter) {
    if (width < 1 || height < 1 || width > FMGI_VIEW_MAX_DIM || height > FMGI_VIEW_MAX_DIM) return "bad image size";
    if (num_cams < 1 || num_cams > FMGI_VIEW_MAX_BATCH || !have_cams) return "bad cameras";
    if (samples < 1 || samples > FMGI_VIEW_MAX_SAMPLES) return "samples outside 1..8";
    if (filter != FMGI_VIEW_NEAREST && filter != FMGI_VIEW_BILINEAR) return "filter is neither nearest nor bilinear";
    return nullptr;
}

int64_t cache_bytes(int num_cams, int width, int height, int samples, int filter) {
    return (int64_t)num_cams * width * height * samples * samples * (filter == FMGI_VIEW_BILINEAR ? 16 : 4);
}

int cache_create(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height, int projection,
                 int samples, int filter, fmgi_view_cache **out, bool mirror = false,
                 const char *fn = "fmgi_view_cache_create") {
    if (!out) return arg_err(fn, "null out");
    *out = nullptr;
    Walls w;
    int rc = check_geometry(geo, w, fn);
    if (rc != FMGI_OK) return rc;
    if (const char *msg = cache_shape_error(num_cams, cams != nullptr, width, height, samples, filter))
        return arg_err(fn, msg);
    std::vector<ViewCam> vc((size_t)num_cams);
    if ((rc = make_cams(cams, num_cams, projection, vc, fn)) != FMGI_OK) return rc;
    const int nr = geo->numWalls;
    std::vector<OutWallIn> ow((size_t)nr);
    int64_t ntiles = 0;
    for (int i = 0; i < nr; i++) {
        ow[(size_t)i] = fmgi_out_wall_in(geo->walls[i], ntiles);
        ntiles += ow[(size_t)i].nt;
    }
    if (ntiles >= ((int64_t)1 << 31)) return arg_err(fn, "2^31 tiles or more: a record holds a tile in 31 bits");
    if ((rc = no_device()) != FMGI_OK) return rc;

    const int64_t pix = (int64_t)width * height, spp = (int64_t)samples * samples, budget = shade_ray_budget();
    const size_t rec = filter == FMGI_VIEW_BILINEAR ? 16 : 4;
    /* cameras per launch and one camera's windows: as shade_run sizes them */
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)num_cams, budget / (pix * spp)));
    int rows = height, cols = width;
    if (pix * spp > budget) {
        const int64_t B = FMGI_VIEW_BLOCK;
        rows = (int)std::min<int64_t>(height, std::max<int64_t>(B, budget / ((int64_t)width * spp) / B * B));
        cols = (int)std::min<int64_t>(width, std::max<int64_t>(B, budget / ((int64_t)rows * spp) / B * B));
    }
    fmgi_view_cache *v = new fmgi_view_cache;
    DevBuf d_rects, d_hits, d_cams, d_keys, d_counts, d_counters, d_first, d_mkeys, d_mcounts;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    unsigned long long counters[5] = {0, 0, 0, 0, 0}; /* tests, hits, then the mirror rays, hits and tests */
    float ms = 0;
    TraceGlossArgs gq;
    memset(&gq, 0, sizeof gq);
    TraceProjArgs &q = gq.q;
    TraceArgs &t = q.t;
    ShadeArgs &s = t.s;
    ViewArgs &a = s.v;
    q.kphi = 6.2831855f / (float)width;
    q.ktheta = 3.1415927f / (float)height;
    v->projection = projection;
    {
        const char *dv = getenv("FMGI_DEVICE");
        v->device = dv ? atoi(dv) : 0;
        VIEWCHK(hipSetDevice(v->device));
    }
    memset(&v->info, 0, sizeof v->info);
    v->info.cameras = num_cams, v->info.width = width, v->info.height = height, v->info.samples = samples;
    v->info.filter = filter, v->info.num_texels = geo->numTexels, v->info.tiles = ntiles;
    v->info.rays = (int64_t)num_cams * pix * spp;
    v->info.bytes = cache_bytes(num_cams, width, height, samples, filter) * (mirror ? 2 : 1);
    v->walls = ow;
    v->mirror = mirror;
    memset(&g_gloss, 0, sizeof g_gloss);
    VIEWCHK(v->records.alloc((size_t)cache_bytes(num_cams, width, height, samples, filter)));
    if (mirror) VIEWCHK(v->mrecords.alloc((size_t)cache_bytes(num_cams, width, height, samples, filter)));
    VIEWCHK(v->out_walls.alloc((size_t)std::max(nr, 1) * sizeof(OutWall)));
    VIEWCHK(hipEventCreateWithFlags(&v->ev_tiles, hipEventDisableTiming));
    VIEWCHK(hipEventCreateWithFlags(&v->ev_shade, hipEventDisableTiming));
    for (auto &e : ev) VIEWCHK(hipEventCreate(&e));
    VIEWCHK(d_rects.alloc(w.rects.size() * sizeof(RadRect)));
    VIEWCHK(hipMemcpy(d_rects.p, w.rects.data(), w.rects.size() * sizeof(RadRect), hipMemcpyHostToDevice));
    VIEWCHK(d_hits.alloc(w.hits.size() * sizeof(AoRect)));
    VIEWCHK(hipMemcpy(d_hits.p, w.hits.data(), w.hits.size() * sizeof(AoRect), hipMemcpyHostToDevice));
    VIEWCHK(d_first.alloc(w.first_tile.size() * 8));
    VIEWCHK(hipMemcpy(d_first.p, w.first_tile.data(), w.first_tile.size() * 8, hipMemcpyHostToDevice));
    VIEWCHK(d_cams.alloc((size_t)num_cams * sizeof(ViewCam)));
    VIEWCHK(hipMemcpy(d_cams.p, vc.data(), (size_t)num_cams * sizeof(ViewCam), hipMemcpyHostToDevice));
    VIEWCHK(d_keys.alloc((size_t)num_cams * w.sort_n * 8));
    VIEWCHK(d_counts.alloc((size_t)num_cams * 4));
    VIEWCHK(d_counters.alloc(40));
    VIEWCHK(hipMemset(d_counters.p, 0, 40));
    if (mirror) {
        VIEWCHK(d_mkeys.alloc((size_t)num_cams * w.sort_n * 8));
        VIEWCHK(d_mcounts.alloc((size_t)num_cams * 4));
    }
    a.rects = d_rects.as<RadRect>();
    a.hits = d_hits.as<AoRect>();
    a.nrects = nr;
    a.sort_n = w.sort_n;
    a.width = width;
    a.height = height;
    a.first_tile = d_first.as<int64_t>();
    a.tests = d_counters.as<unsigned long long>();
    t.hits = d_counters.as<unsigned long long>() + 1;
    s.samples = samples;
    s.filter = filter;
    for (int i = 0; i < samples; i++) s.offs[i] = (float)(2 * i + 1 - samples) / (float)(2 * samples);
    /* every camera's candidate list, then the trace in launches of at most `budget` rays */
    a.cams = d_cams.as<ViewCam>();
    a.keys = d_keys.as<unsigned long long>();
    a.counts = d_counts.as<int32_t>();
    a.ncams = num_cams;
    VIEWCHK(hipEventRecord(ev[0], nullptr));
    if (projection == FMGI_PROJ_PINHOLE) VIEWCHK(fmgi_view_launch_candidates(a, nullptr));
    else VIEWCHK(fmgi_view_launch_candidates_proj(a, projection, nullptr));
    if (mirror) {
        ViewArgs m = a;
        m.keys = d_mkeys.as<unsigned long long>();
        m.counts = d_mcounts.as<int32_t>();
        VIEWCHK(fmgi_view_launch_candidates_mirror(m, nullptr));
    }
    gq.g.counters = d_counters.as<unsigned long long>() + 2;
    VIEWCHK(hipEventRecord(ev[1], nullptr));
    for (int c0 = 0; c0 < num_cams; c0 += batch) {
        a.ncams = std::min(batch, num_cams - c0);
        a.cams = d_cams.as<ViewCam>() + c0;
        a.keys = d_keys.as<unsigned long long>() + (size_t)c0 * w.sort_n;
        a.counts = d_counts.as<int32_t>() + c0;
        t.records = v->records.as<char>() + (size_t)c0 * spp * pix * rec;
        gq.mrecords = mirror ? v->mrecords.as<char>() + (size_t)c0 * spp * pix * rec : nullptr;
        gq.g.mkeys = mirror ? d_mkeys.as<unsigned long long>() + (size_t)c0 * w.sort_n : nullptr;
        for (s.y0 = 0; s.y0 < height; s.y0 += rows)
            for (s.x0 = 0; s.x0 < width; s.x0 += cols) {
                s.y1 = std::min(height, s.y0 + rows);
                s.x1 = std::min(width, s.x0 + cols);
                if (mirror) VIEWCHK(fmgi_view_launch_trace_gloss(gq, projection, nullptr));
                else if (projection == FMGI_PROJ_PINHOLE) VIEWCHK(fmgi_view_launch_trace(t, nullptr));
                else VIEWCHK(fmgi_view_launch_trace_proj(q, projection, nullptr));
            }
    }
    VIEWCHK(hipEventRecord(ev[2], nullptr));
    VIEWCHK(hipEventSynchronize(ev[2]));
    VIEWCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    v->info.cand_ms = ms;
    VIEWCHK(hipEventElapsedTime(&ms, ev[1], ev[2]));
    v->info.trace_ms = ms;
    VIEWCHK(hipMemcpy(counters, d_counters.p, 40, hipMemcpyDeviceToHost));
    v->info.tests = (int64_t)counters[0];
    v->info.hits = (int64_t)counters[1];
    g_gloss.mirror_rays = (int64_t)counters[2];
    g_gloss.mirror_hits = (int64_t)counters[3];
    g_gloss.mirror_tests = (int64_t)counters[4];
    *out = v;
    v = nullptr;
done:
    for (auto &e : ev)
        if (e) hipEventDestroy(e);
    delete v; /* on an error: nothing stays allocated */
    return rc;
}

int cache_tiles(fmgi_view_cache *v, const void *const *texels_dev, int num_sets, int spa, int tint,
                void *const *tiles_dev, hipStream_t st) {
    static const char fn[] = "fmgi_view_cache_tiles";
    if (!v || !texels_dev || !tiles_dev) return arg_err(fn, "null argument");
    if (num_sets < 1) return arg_err(fn, "num_sets < 1");
    if (spa < 0) return arg_err(fn, "numSamplesPerArea < 0");
    for (int k = 0; k < num_sets; k++)
        if (!texels_dev[k] || !tiles_dev[k]) return arg_err(fn, "null set");
    int rc = FMGI_OK;
    OutArgs a;
    memset(&a, 0, sizeof a);
    if (v->info.tiles == 0) return FMGI_OK;
    VIEWCHK(hipSetDevice(v->device));
    if (spa != v->out_spa) { /* another normalisation: the table is rebuilt once its readers are through */
        std::vector<OutWall> ow(v->walls.size());
        for (size_t i = 0; i < ow.size(); i++) ow[i] = fmgi_out_wall(v->walls[i], spa);
        if (v->tiles_pending) VIEWCHK(hipEventSynchronize(v->ev_tiles));
        v->tiles_pending = false;
        v->out_spa = -1;
        VIEWCHK(hipMemcpy(v->out_walls.p, ow.data(), ow.size() * sizeof(OutWall), hipMemcpyHostToDevice));
        v->out_spa = spa;
    }
    /* calls chain on the event, so its last record stands for every launch that reads the table */
    if (v->tiles_pending) VIEWCHK(hipStreamWaitEvent(st, v->ev_tiles, 0));
    a.walls = v->out_walls.as<OutWall>();
    a.nwalls = (int)v->walls.size();
    a.ntexels = v->info.tiles;
    a.normalise = spa > 0;
    a.tint_extra = tint != 0;
    for (int k = 0; k < num_sets; k++) {
        a.texels_in = (const float *)texels_dev[k];
        a.rgb = (uint8_t *)tiles_dev[k];
        VIEWCHK(fmgi_launch_output_const(a, st));
    }
    VIEWCHK(hipEventRecord(v->ev_tiles, st));
    v->tiles_pending = true;
done:
    return rc;
}

int cache_shade(fmgi_view_cache *v, const void *const *tiles_dev, int num_sets, const uint8_t *background,
                void *const *rgb_dev, void *coverage_dev, hipStream_t st, float gloss = 0.0f,
                const char *fn = "fmgi_view_cache_shade") {
    if (!v || !tiles_dev || !rgb_dev || !background) return arg_err(fn, "null argument");
    if (num_sets < 1) return arg_err(fn, "num_sets < 1");
    for (int k = 0; k < num_sets; k++)
        if (!tiles_dev[k] || !rgb_dev[k]) return arg_err(fn, "null set");
    if (bad_gloss(gloss)) return arg_err(fn, "gloss is not a number in [0, 1]");
    if (gloss > 0.0f && !v->mirror) {
        char b[160];
        snprintf(b, sizeof b, "%s: gloss > 0 on a traced view without mirror records (fmgi_view_cache_create_gloss makes them)", fn);
        return internal_set_err(FMGI_ERR_STATE, b);
    }
    int rc = FMGI_OK;
    const int64_t ntiles = v->info.tiles;
    const int per_pass = std::min(num_sets, FMGI_VIEW_SETS);
    ResolveGlossArgs gr;
    memset(&gr, 0, sizeof gr);
    ResolveArgs &r = gr.r;
    gr.mrecords = v->mrecords.p;
    gr.gloss = gloss;
    VIEWCHK(hipSetDevice(v->device));
    if (v->packed_sets < per_pass) { /* grow the scratch once nothing reads it any more */
        if (v->shade_pending) VIEWCHK(hipEventSynchronize(v->ev_shade));
        v->shade_pending = false;
        hipFree(v->packed.p);
        v->packed.p = nullptr;
        v->packed_sets = 0;
        VIEWCHK(v->packed.alloc((size_t)per_pass * (size_t)std::max<int64_t>(ntiles, 1) * 4));
        v->packed_sets = per_pass;
    }
    /* an earlier call, maybe on another stream, may still read the scratch */
    if (v->shade_pending) VIEWCHK(hipStreamWaitEvent(st, v->ev_shade, 0));
    r.records = v->records.p;
    r.ncams = v->info.cameras;
    r.width = v->info.width;
    r.height = v->info.height;
    r.samples = v->info.samples;
    r.filter = v->info.filter;
    r.background = (uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16);
    for (int k0 = 0; k0 < num_sets; k0 += FMGI_VIEW_SETS) {
        r.nsets = std::min(FMGI_VIEW_SETS, num_sets - k0);
        for (int k = 0; k < FMGI_VIEW_SETS; k++) {
            r.tiles[k] = nullptr;
            r.rgb[k] = nullptr;
        }
        for (int k = 0; k < r.nsets; k++) {
            uint32_t *words = v->packed.as<uint32_t>() + (size_t)k * (size_t)std::max<int64_t>(ntiles, 1);
            VIEWCHK(fmgi_view_launch_pack((const uint8_t *)tiles_dev[k0 + k], words, ntiles, st));
            r.tiles[k] = words;
            r.rgb[k] = (uint8_t *)rgb_dev[k0 + k];
        }
        r.cov_out = k0 == 0 ? (uint8_t *)coverage_dev : nullptr;
        /* gloss == 0 is the plain picture, through the plain kernel */
        if (gloss > 0.0f) VIEWCHK(fmgi_view_launch_resolve_gloss(gr, st));
        else VIEWCHK(fmgi_view_launch_resolve(r, st));
    }
    VIEWCHK(hipEventRecord(v->ev_shade, st));
    v->shade_pending = true;
done:
    return rc;
}

} // namespace

FMGI_API int64_t fmgi_view_cache_bytes(int num_cams, int width, int height, int samples, int filter) {
    if (cache_shape_error(num_cams, true, width, height, samples, filter)) return 0;
    return cache_bytes(num_cams, width, height, samples, filter);
}

FMGI_API int fmgi_view_cache_create(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width,
                                    int height, int samples, int filter, fmgi_view_cache **out) {
    return cache_create(geo, cams, num_cams, width, height, FMGI_PROJ_PINHOLE, samples, filter, out);
}

FMGI_API int fmgi_view_cache_create_proj(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width,
                                         int height, int projection, int samples, int filter, fmgi_view_cache **out) {
    return cache_create(geo, cams, num_cams, width, height, projection, samples, filter, out);
}

FMGI_API int fmgi_view_cache_create_gloss(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width,
                                          int height, int projection, int samples, int filter, fmgi_view_cache **out) {
    return cache_create(geo, cams, num_cams, width, height, projection, samples, filter, out, true,
                        "fmgi_view_cache_create_gloss");
}

FMGI_API int fmgi_view_cache_has_mirror(const fmgi_view_cache *vc) {
    if (!vc) return arg_err("fmgi_view_cache_has_mirror", "null argument");
    return vc->mirror ? 1 : 0;
}

FMGI_API int fmgi_view_cache_shade_gloss(const fmgi_view_cache *vc, const void *const *tiles_dev, int num_sets,
                                         const uint8_t background[3], float gloss, void *const *rgb_dev,
                                         void *coverage_dev, void *stream) {
    return cache_shade(const_cast<fmgi_view_cache *>(vc), tiles_dev, num_sets, background, rgb_dev, coverage_dev,
                       (hipStream_t)stream, gloss, "fmgi_view_cache_shade_gloss");
}

FMGI_API int fmgi_shade_views_gloss(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                                    int projection, const uint8_t *tiles_rgb, const uint8_t background[3], int samples,
                                    int filter, float gloss, uint8_t *rgb_out, uint8_t *coverage_out) {
    return shade_run(geo, cams, num_cams, width, height, projection, tiles_rgb, background, samples, filter, rgb_out,
                     coverage_out, gloss, "fmgi_shade_views_gloss");
}

FMGI_API int fmgi_view_gloss_stats(struct fmgi_view_gloss_stats *out) {
    if (!out) return internal_set_err(FMGI_ERR_ARG, "null stats");
    *out = g_gloss;
    return FMGI_OK;
}

FMGI_API int fmgi_view_cache_projection(const fmgi_view_cache *vc) {
    if (!vc) return arg_err("fmgi_view_cache_projection", "null argument");
    return vc->projection;
}

FMGI_API void fmgi_view_cache_destroy(fmgi_view_cache *vc) {
    if (!vc) return;
    /* launches of tiles and shade may still read what the handle owns */
    if (vc->tiles_pending) hipEventSynchronize(vc->ev_tiles);
    if (vc->shade_pending) hipEventSynchronize(vc->ev_shade);
    delete vc;
}

FMGI_API int fmgi_view_cache_info(const fmgi_view_cache *vc, struct fmgi_view_cache_info *out) {
    if (!vc || !out) return arg_err("fmgi_view_cache_info", "null argument");
    *out = vc->info;
    return FMGI_OK;
}

FMGI_API int fmgi_view_cache_tiles(const fmgi_view_cache *vc, const void *const *texels_dev, int num_sets,
                                   int numSamplesPerArea, int tintExtra, void *const *tiles_dev, void *stream) {
    return cache_tiles(const_cast<fmgi_view_cache *>(vc), texels_dev, num_sets, numSamplesPerArea, tintExtra, tiles_dev,
                       (hipStream_t)stream);
}

FMGI_API int fmgi_view_cache_shade(const fmgi_view_cache *vc, const void *const *tiles_dev, int num_sets,
                                   const uint8_t background[3], void *const *rgb_dev, void *coverage_dev, void *stream) {
    return cache_shade(const_cast<fmgi_view_cache *>(vc), tiles_dev, num_sets, background, rgb_dev, coverage_dev,
                       (hipStream_t)stream);
}

FMGI_API int fmgi_shade_views(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                              const uint8_t *tiles_rgb, const uint8_t background[3], int samples, int filter,
                              uint8_t *rgb_out, uint8_t *coverage_out) {
    return shade_run(geo, cams, num_cams, width, height, FMGI_PROJ_PINHOLE, tiles_rgb, background, samples, filter, rgb_out,
                     coverage_out);
}

FMGI_API int fmgi_shade_views_proj(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                                   int projection, const uint8_t *tiles_rgb, const uint8_t background[3], int samples,
                                   int filter, uint8_t *rgb_out, uint8_t *coverage_out) {
    return shade_run(geo, cams, num_cams, width, height, projection, tiles_rgb, background, samples, filter, rgb_out,
                     coverage_out);
}

FMGI_API int fmgi_render_views(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                               const uint8_t *tiles_rgb, const uint8_t background[3], int32_t *wall_out,
                               int32_t *texel_out, float *dist_out, uint8_t *rgb_out) {
    return view_run(geo, cams, num_cams, width, height, tiles_rgb, background, wall_out, texel_out, dist_out, rgb_out);
}

FMGI_API int fmgi_view_candidates(const fmgi_geometry *geo, const fmgi_camera *cam, int32_t *wall_idx, float *min_dist,
                                  int cap) {
    return candidates_run(geo, cam, FMGI_PROJ_PINHOLE, wall_idx, min_dist, cap);
}

FMGI_API int fmgi_view_candidates_proj(const fmgi_geometry *geo, const fmgi_camera *cam, int projection,
                                       int32_t *wall_idx, float *min_dist, int cap) {
    return candidates_run(geo, cam, projection, wall_idx, min_dist, cap);
}

FMGI_API int fmgi_view_stats(struct fmgi_view_stats *out) {
    if (!out) return internal_set_err(FMGI_ERR_ARG, "null stats");
    *out = g_stats;
    return FMGI_OK;
}
