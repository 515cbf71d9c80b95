/*
 * fmgi_sun_host.cpp -- host side of the direct-sun layer and its C ABI (include/flatmatch_gi.h: fmgi_sun_coverage,
 * fmgi_sun_get_stats, fmgi_sun_add, fmgi_sun_units) and of the bounced layer's add (fmgi_sun_add_bounced,
 * DESIGN §21). No reference program has a sun: the header states the semantics, tests/sun_restate.py and
 * tests/sun_bounce_restate.py restate them.
 *
 * The context keeps host copies of the scene's walls and windows (fmgi_sun_set_scene) and, on a device context, their
 * intersects() records, the occluder lists, a call's job table and unit table and the counters. A call checks its
 * arguments on the host, builds its tables in a pinned block of its own (so a call never writes what an earlier
 * call's copy may still read), makes its stream wait for the event of the context's previous sun call (they share the
 * device scratch) and launches; the host waits for nothing. Built with -ffp-contract=off: the sun vector and every
 * wall's cosine are the fp32 values the kernels and the restatement compute.
 */
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/flatmatch_gi.h"
#include "fmgi_sun.h"
#include "fmgi_sun_bounce.h"
#include "fmgi_view.h"

#define FMGI_API extern "C" __attribute__((visibility("default")))

int internal_set_err(int code, const char *msg);

static_assert(FMGI_SUN_SAMPLES == FMGI_SUN_MAX_SAMPLES && FMGI_SUN_MAPS == FMGI_SUN_MAX_MAPS &&
                  FMGI_SUN_BOUNCE_MAPS == FMGI_SUN_MAX_MAPS && FMGI_SUN_BOUNCES == FMGI_SUN_MAX_BOUNCES,
              "kernel and ABI limits differ");

/* a pinned block a call builds its tables in; free again once `done` has completed */
struct SunStage {
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
};

struct SunState {
    bool scene_set = false;
    std::vector<fmgi_rect> walls, windows;
    std::vector<AoRect> hits, wins; /* the walls and the windows as intersects() reads them */
    int64_t level0 = 0;             /* level-0 texels of all walls */
    /* device side */
    bool tables_ready = false; /* d_hits .. d_list_len are those of this scene */
    AoRect *d_hits = nullptr, *d_wins = nullptr;
    int32_t *d_lists = nullptr, *d_list_len = nullptr;
    unsigned long long *d_counters = nullptr;
    SunJob *d_jobs = nullptr;
    size_t jobs_cap = 0;
    long long *d_units = nullptr;
    size_t units_cap = 0;
    SunBounceWall *d_bounce_walls = nullptr; /* fmgi_sun_add_bounced's wall table */
    size_t bounce_walls_cap = 0;
    hipEvent_t ev = nullptr; /* after the last launch of the context's last sun call */
    bool pending = false;
    hipEvent_t ev_t[3] = {nullptr, nullptr, nullptr}; /* around the last coverage call's two kernels */
    bool timed = false;
    bool counted = false; /* d_counters hold a coverage call's counts */
    std::vector<SunStage> stages;
    fmgi_sun_stats stats{}; /* the host's part: samples, facing */
};

namespace {

struct F3 {
    float x, y, z;
};
float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

int err(int code, const char *fn, const char *msg) {
    char b[256];
    snprintf(b, sizeof b, "%s: %s", fn, msg);
    return internal_set_err(code, b);
}

#define SUNCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            char b_[256];                                                                                  \
            snprintf(b_, sizeof b_, "%s: %s", #expr, hipGetErrorString(e_));                               \
            return internal_set_err(e_ == hipErrorOutOfMemory ? FMGI_ERR_OOM : FMGI_ERR_HIP, b_);          \
        }                                                                                                  \
    } while (0)

/* s = to_sun / |to_sun|; false for a zero or non-finite length */
bool sun_dir(const float to_sun[3], F3 &s) {
    const float x = to_sun[0], y = to_sun[1], z = to_sun[2];
    const float l = sqrtf((x * x + y * y) + z * z);
    if (!(l > 0) || !isfinite(l)) return false;
    s = F3{x / l, y / l, z / l};
    return true;
}

float facing_cos(const SunState &st, int i, F3 s) {
    const AoRect &r = st.hits[(size_t)i];
    return dot3(F3{r.nx, r.ny, r.nz}, s);
}

/* the walls with c_w > 0 in scene order, with their running texel count; returns the job texels */
int64_t build_jobs(const SunState &st, F3 s, std::vector<SunJob> &jobs) {
    int64_t total = 0;
    jobs.clear();
    for (int i = 0; i < (int)st.walls.size(); i++) {
        if (!(facing_cos(st, i, s) > 0)) continue;
        const fmgi_rect &r = st.walls[(size_t)i];
        SunJob j;
        memset(&j, 0, sizeof j);
        j.px = r.pos.s[0], j.py = r.pos.s[1], j.pz = r.pos.s[2];
        j.wx = r.width.s[0], j.wy = r.width.s[1], j.wz = r.width.s[2];
        j.hx = r.height.s[0], j.hy = r.height.s[1], j.hz = r.height.s[2];
        j.s0 = r.lightmapSetup[0], j.s1 = r.lightmapSetup[1], j.s2 = r.lightmapSetup[2];
        j.first = (int32_t)total;
        j.wall = i;
        jobs.push_back(j);
        total += (int64_t)j.s1 * j.s2; /* fmgi_set_scene: s0 + s1 * s2 <= numTexels, an int */
    }
    return total;
}

/* unit[c] of wall i under one colour; false if one reaches 2^55 */
bool wall_units(const SunState &st, int i, float c_w, const float rgb[3], double flux, int64_t out[3]) {
    const AoRect &r = st.hits[(size_t)i];
    const int32_t *lm = st.walls[(size_t)i].lightmapSetup;
    const double area_t = ((double)r.wl * (double)r.hl) / (double)((int64_t)lm[1] * lm[2]);
    for (int c = 0; c < 3; c++) {
        const double v = floor(ldexp((double)rgb[c] * (double)c_w * flux * area_t, 25));
        if (!(v < 36028797018963968.0)) return false; /* 2^55 */
        out[c] = (int64_t)v;
    }
    return true;
}

bool bad_rgb(const float *rgb, int n) {
    for (int k = 0; k < 3 * n; k++)
        if (!isfinite(rgb[k]) || !(rgb[k] >= 0.0f && rgb[k] < 32.0f)) return true;
    return false;
}

/* a free pinned block of at least `bytes` */
int stage_acquire(SunState &st, size_t bytes, SunStage **out) {
    bytes = std::max<size_t>(bytes, 64);
    SunStage *pick = nullptr;
    for (SunStage &g : st.stages) {
        if (g.pending && hipEventQuery(g.done) != hipSuccess) continue;
        g.pending = false;
        if (!pick || (g.cap >= bytes && pick->cap < bytes)) pick = &g;
    }
    if (!pick) {
        st.stages.emplace_back();
        pick = &st.stages.back();
        SUNCHK(hipEventCreateWithFlags(&pick->done, hipEventDisableTiming));
    }
    if (pick->cap < bytes) {
        if (pick->host) SUNCHK(hipHostFree(pick->host));
        pick->host = nullptr;
        pick->cap = 0;
        SUNCHK(hipHostMalloc(&pick->host, bytes, hipHostMallocDefault));
        pick->cap = bytes;
    }
    *out = pick;
    return FMGI_OK;
}

template <class T> int grow(T **p, size_t *cap, size_t n) {
    if (*cap >= n && *p) return FMGI_OK;
    if (*p) SUNCHK(hipFree(*p)); /* waits for the device: nothing reads the old block any more */
    *p = nullptr;
    *cap = 0;
    SUNCHK(hipMalloc(p, std::max<size_t>(n, 1) * sizeof(T)));
    *cap = std::max<size_t>(n, 1);
    return FMGI_OK;
}

/* the scene's records, lists and counters on the device; replaced only here, through hipFree */
int device_tables(SunState &st) {
    if (st.tables_ready) return FMGI_OK;
    const size_t nw = std::max<size_t>(st.hits.size(), 1), nwin = std::max<size_t>(st.wins.size(), 1);
    hipFree(st.d_hits);
    hipFree(st.d_wins);
    hipFree(st.d_lists);
    hipFree(st.d_list_len);
    st.d_hits = st.d_wins = nullptr;
    st.d_lists = st.d_list_len = nullptr;
    SUNCHK(hipMalloc(&st.d_hits, nw * sizeof(AoRect)));
    SUNCHK(hipMalloc(&st.d_wins, nwin * sizeof(AoRect)));
    SUNCHK(hipMalloc(&st.d_lists, nwin * nw * sizeof(int32_t)));
    SUNCHK(hipMalloc(&st.d_list_len, nwin * sizeof(int32_t)));
    if (!st.hits.empty()) SUNCHK(hipMemcpy(st.d_hits, st.hits.data(), st.hits.size() * sizeof(AoRect), hipMemcpyHostToDevice));
    if (!st.wins.empty()) SUNCHK(hipMemcpy(st.d_wins, st.wins.data(), st.wins.size() * sizeof(AoRect), hipMemcpyHostToDevice));
    SUNCHK(hipMemset(st.d_list_len, 0, nwin * sizeof(int32_t)));
    if (!st.d_counters) SUNCHK(hipMalloc(&st.d_counters, SUN_CTR_N * sizeof(unsigned long long)));
    if (!st.ev) SUNCHK(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    for (auto &e : st.ev_t)
        if (!e) SUNCHK(hipEventCreate(&e));
    st.tables_ready = true;
    return FMGI_OK;
}

/* the checks every call shares after its own pointer checks; fills s */
int check_sun(const char *fn, const float to_sun[3], F3 &s) {
    s = F3{0, 0, 0};
    if (!sun_dir(to_sun, s)) return err(FMGI_ERR_ARG, fn, "to_sun has a zero or non-finite length");
    return FMGI_OK;
}

} // namespace

SunState *fmgi_sun_new() { return new SunState; }

void fmgi_sun_free(SunState *st, bool has_device) {
    if (!st) return;
    if (has_device) {
        if (st->ev) {
            hipEventSynchronize(st->ev);
            hipEventDestroy(st->ev);
        }
        for (auto &e : st->ev_t)
            if (e) hipEventDestroy(e);
        for (SunStage &g : st->stages) {
            if (g.done) {
                hipEventSynchronize(g.done);
                hipEventDestroy(g.done);
            }
            if (g.host) hipHostFree(g.host);
        }
        hipFree(st->d_hits);
        hipFree(st->d_wins);
        hipFree(st->d_lists);
        hipFree(st->d_list_len);
        hipFree(st->d_counters);
        hipFree(st->d_jobs);
        hipFree(st->d_units);
        hipFree(st->d_bounce_walls);
    }
    delete st;
}

void fmgi_sun_set_scene(SunState *st, const fmgi_rect *walls, int nwalls, const fmgi_rect *windows, int nwins) {
    st->walls.assign(walls, walls + nwalls);
    st->windows.assign(windows, windows + nwins);
    st->hits.resize((size_t)nwalls);
    st->wins.resize((size_t)nwins);
    st->level0 = 0;
    for (int i = 0; i < nwalls; i++) {
        st->hits[(size_t)i] = fmgi_rad_hit_rect(walls[i]);
        st->level0 += (int64_t)walls[i].lightmapSetup[1] * walls[i].lightmapSetup[2];
    }
    for (int i = 0; i < nwins; i++) {
        /* as it is stored: a window's normal points into the room, the ray towards the sun runs against it */
        st->wins[(size_t)i] = fmgi_rad_hit_rect(windows[i]);
    }
    st->scene_set = true;
    st->tables_ready = false;
    st->timed = false;
    st->counted = false;
    memset(&st->stats, 0, sizeof st->stats);
}

FMGI_API int fmgi_sun_coverage(fmgi_context *ctx, const float to_sun[3], int samples, int mode, void *cover_dev,
                               void *stream) {
    static const char fn[] = "fmgi_sun_coverage";
    SunCtx c;
    if (!fmgi_sun_ctx(ctx, &c) || !to_sun || !cover_dev) return err(FMGI_ERR_ARG, fn, "null argument");
    if (samples < 1 || samples > FMGI_SUN_MAX_SAMPLES) return err(FMGI_ERR_ARG, fn, "samples outside 1..8");
    if (mode != FMGI_SUN_LISTS && mode != FMGI_SUN_ALL) return err(FMGI_ERR_ARG, fn, "mode is neither FMGI_SUN_LISTS nor FMGI_SUN_ALL");
    F3 s;
    int rc = check_sun(fn, to_sun, s);
    if (rc != FMGI_OK) return rc;
    SunState &st = *c.sun;
    if (!st.scene_set) return err(FMGI_ERR_STATE, fn, "no scene");
    if (c.device == FMGI_HOST_ONLY) return err(FMGI_ERR_NO_DEVICE, fn, "host-only context");

    SUNCHK(hipSetDevice(c.device));
    hipStream_t q = stream ? (hipStream_t)stream : c.stream;
    if ((rc = device_tables(st)) != FMGI_OK) return rc;
    std::vector<SunJob> jobs;
    const int64_t total = build_jobs(st, s, jobs);
    const int nwalls = (int)st.hits.size(), nwins = (int)st.wins.size();
    if ((rc = grow(&st.d_jobs, &st.jobs_cap, jobs.size())) != FMGI_OK) return rc;
    SunStage *stage = nullptr;
    if (!jobs.empty()) {
        if ((rc = stage_acquire(st, jobs.size() * sizeof(SunJob), &stage)) != FMGI_OK) return rc;
        memcpy(stage->host, jobs.data(), jobs.size() * sizeof(SunJob));
    }
    memset(&st.stats, 0, sizeof st.stats);
    st.stats.samples = st.level0 * samples * samples;
    st.stats.facing = total * samples * samples;
    st.timed = false;

    /* an earlier sun call, maybe on another stream, may still use the job table, the lists and the counters */
    if (st.pending) SUNCHK(hipStreamWaitEvent(q, st.ev, 0));
    st.pending = true;
    st.counted = true;
    hipError_t e = hipSuccess;
    if (c.num_texels > 0) e = hipMemsetAsync(cover_dev, 0, (size_t)c.num_texels, q);
    if (e == hipSuccess) e = hipMemsetAsync(st.d_counters, 0, SUN_CTR_N * sizeof(unsigned long long), q);
    if (e == hipSuccess && stage) {
        e = hipMemcpyAsync(st.d_jobs, stage->host, jobs.size() * sizeof(SunJob), hipMemcpyHostToDevice, q);
        if (e == hipSuccess) e = hipEventRecord(stage->done, q);
        stage->pending = true;
    }
    if (e == hipSuccess && total > 0 && nwins > 0) {
        SunArgs a;
        memset(&a, 0, sizeof a);
        a.jobs = st.d_jobs;
        a.njobs = (int)jobs.size();
        a.total = (int)total;
        a.hits = st.d_hits;
        a.nwalls = nwalls;
        a.wins = st.d_wins;
        a.nwins = nwins;
        a.lists = st.d_lists;
        a.list_len = st.d_list_len;
        a.list_cap = std::max(nwalls, 1);
        a.all = mode == FMGI_SUN_ALL;
        a.nlists = a.all ? 1 : nwins;
        a.sx = s.x, a.sy = s.y, a.sz = s.z;
        a.S = samples;
        a.cover = (uint8_t *)cover_dev;
        a.num_texels = c.num_texels;
        a.counters = st.d_counters;
        /* LDS for the lists' records: every entry they can have, or what 64 KB holds (two workgroups per CU); the
           kernel stages them if the call's lists fit and reads global memory if not */
        if (a.nlists <= FMGI_SUN_LDS_MAX_LISTS) {
            const int64_t room = ((64 << 10) - (((int64_t)(a.nlists + 1) * 4 + 15) & ~(int64_t)15)) / (int64_t)sizeof(AoRect);
            a.lds_entries = (int)std::min<int64_t>((int64_t)a.nlists * a.list_cap, room);
        }
        e = hipEventRecord(st.ev_t[0], q);
        if (e == hipSuccess) e = fmgi_sun_launch_lists(a, q);
        if (e == hipSuccess) e = hipEventRecord(st.ev_t[1], q);
        if (e == hipSuccess) e = fmgi_sun_launch_rays(a, c.num_cus, q);
        if (e == hipSuccess) e = hipEventRecord(st.ev_t[2], q);
        st.timed = e == hipSuccess;
    }
    const hipError_t ev = hipEventRecord(st.ev, q);
    if (e != hipSuccess) return err(FMGI_ERR_HIP, fn, hipGetErrorString(e));
    SUNCHK(ev);
    return FMGI_OK;
}

FMGI_API int fmgi_sun_get_stats(fmgi_context *ctx, struct fmgi_sun_stats *out) {
    static const char fn[] = "fmgi_sun_get_stats";
    SunCtx c;
    if (!fmgi_sun_ctx(ctx, &c) || !out) return err(FMGI_ERR_ARG, fn, "null argument");
    SunState &st = *c.sun;
    *out = st.stats;
    if (c.device == FMGI_HOST_ONLY || !st.counted) return FMGI_OK;
    SUNCHK(hipSetDevice(c.device));
    SUNCHK(hipEventSynchronize(st.ev));
    unsigned long long ctr[SUN_CTR_N];
    SUNCHK(hipMemcpy(ctr, st.d_counters, sizeof ctr, hipMemcpyDeviceToHost));
    out->crossing = (int64_t)ctr[SUN_CTR_CROSSING];
    out->lit = (int64_t)ctr[SUN_CTR_LIT];
    out->tests = (int64_t)ctr[SUN_CTR_TESTS];
    out->list_entries = (int64_t)ctr[SUN_CTR_ENTRIES];
    if (st.timed) {
        float ms = 0;
        SUNCHK(hipEventElapsedTime(&ms, st.ev_t[0], st.ev_t[1]));
        out->list_ms = ms;
        SUNCHK(hipEventElapsedTime(&ms, st.ev_t[1], st.ev_t[2]));
        out->rays_ms = ms;
    }
    return FMGI_OK;
}

FMGI_API int fmgi_sun_add(fmgi_context *ctx, const void *cover_dev, const float to_sun[3], int samples,
                          const float *rgb, int num_maps, double flux, void *const *lm_fx_dev, void *stream) {
    static const char fn[] = "fmgi_sun_add";
    SunCtx c;
    if (!fmgi_sun_ctx(ctx, &c) || !cover_dev || !to_sun || !rgb || !lm_fx_dev) return err(FMGI_ERR_ARG, fn, "null argument");
    if (samples < 1 || samples > FMGI_SUN_MAX_SAMPLES) return err(FMGI_ERR_ARG, fn, "samples outside 1..8");
    F3 s;
    int rc = check_sun(fn, to_sun, s);
    if (rc != FMGI_OK) return rc;
    if (num_maps < 1) return err(FMGI_ERR_ARG, fn, "num_maps < 1");
    for (int k = 0; k < num_maps; k++)
        if (!lm_fx_dev[k]) return err(FMGI_ERR_ARG, fn, "a lightmap is NULL");
    if (bad_rgb(rgb, num_maps)) return err(FMGI_ERR_ARG, fn, "an rgb component is not finite or outside [0, 32)");
    if (!isfinite(flux) || !(flux > 0)) return err(FMGI_ERR_ARG, fn, "flux is not finite and positive");
    SunState &st = *c.sun;
    if (!st.scene_set) return err(FMGI_ERR_STATE, fn, "no scene");
    std::vector<SunJob> jobs;
    const int64_t total = build_jobs(st, s, jobs);
    const size_t nj = jobs.size();
    /* unit tables, one per pass of at most FMGI_SUN_MAPS maps: [pass][job][map in pass][3] */
    std::vector<int64_t> units(nj * (size_t)num_maps * 3);
    for (int k0 = 0; k0 < num_maps; k0 += FMGI_SUN_MAPS) {
        const int maps = std::min(FMGI_SUN_MAPS, num_maps - k0);
        int64_t *u = units.data() + nj * (size_t)k0 * 3;
        for (size_t j = 0; j < nj; j++) {
            const float c_w = facing_cos(st, jobs[j].wall, s);
            for (int m = 0; m < maps; m++)
                if (!wall_units(st, jobs[j].wall, c_w, rgb + 3 * (k0 + m), flux, u + (j * (size_t)maps + (size_t)m) * 3))
                    return err(FMGI_ERR_ARG, fn, "a wall's unit reaches 2^55: flux * rgb * texel area is too large");
        }
    }
    if (c.device == FMGI_HOST_ONLY) return err(FMGI_ERR_NO_DEVICE, fn, "host-only context");

    SUNCHK(hipSetDevice(c.device));
    hipStream_t q = stream ? (hipStream_t)stream : c.stream;
    if (nj == 0 || total == 0) return FMGI_OK; /* no wall faces the sun: nothing to add */
    if ((rc = device_tables(st)) != FMGI_OK) return rc;
    if ((rc = grow(&st.d_jobs, &st.jobs_cap, nj)) != FMGI_OK) return rc;
    if ((rc = grow(&st.d_units, &st.units_cap, units.size())) != FMGI_OK) return rc;
    const size_t job_bytes = nj * sizeof(SunJob), unit_bytes = units.size() * sizeof(int64_t);
    SunStage *stage = nullptr;
    if ((rc = stage_acquire(st, job_bytes + unit_bytes, &stage)) != FMGI_OK) return rc;
    memcpy(stage->host, jobs.data(), job_bytes);
    memcpy((char *)stage->host + job_bytes, units.data(), unit_bytes);
    if (st.pending) SUNCHK(hipStreamWaitEvent(q, st.ev, 0));
    st.pending = true;
    hipError_t e = hipMemcpyAsync(st.d_jobs, stage->host, job_bytes, hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = hipMemcpyAsync(st.d_units, (char *)stage->host + job_bytes, unit_bytes, hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = hipEventRecord(stage->done, q);
    stage->pending = true;
    for (int k0 = 0; k0 < num_maps && e == hipSuccess; k0 += FMGI_SUN_MAPS) {
        SunAddArgs a;
        memset(&a, 0, sizeof a);
        a.jobs = st.d_jobs;
        a.njobs = (int)nj;
        a.total = (int)total;
        a.maps = std::min(FMGI_SUN_MAPS, num_maps - k0);
        a.units = (const long long *)st.d_units + nj * (size_t)k0 * 3;
        a.S2 = samples * samples;
        a.cover = (const uint8_t *)cover_dev;
        a.num_texels = c.num_texels;
        for (int m = 0; m < a.maps; m++) a.lm[m] = (unsigned long long *)lm_fx_dev[k0 + m];
        e = fmgi_sun_launch_add(a, q);
    }
    const hipError_t ev = hipEventRecord(st.ev, q);
    if (e != hipSuccess) return err(FMGI_ERR_HIP, fn, hipGetErrorString(e));
    SUNCHK(ev);
    return FMGI_OK;
}

/* the bounce tables of one direction under num_maps colours and reflectances, onto every wall */
FMGI_API int fmgi_sun_add_bounced(fmgi_context *ctx, const void *bounce_dev, int bounces, const float *rgb,
                                  const float *refl, int num_maps, double flux, void *const *lm_fx_dev, void *stream) {
    static const char fn[] = "fmgi_sun_add_bounced";
    SunCtx c;
    if (!fmgi_sun_ctx(ctx, &c) || !bounce_dev || !rgb || !refl || !lm_fx_dev) return err(FMGI_ERR_ARG, fn, "null argument");
    if (bounces < 1 || bounces > FMGI_SUN_MAX_BOUNCES) return err(FMGI_ERR_ARG, fn, "bounces outside 1..8");
    if (num_maps < 1) return err(FMGI_ERR_ARG, fn, "num_maps < 1");
    for (int k = 0; k < num_maps; k++)
        if (!lm_fx_dev[k]) return err(FMGI_ERR_ARG, fn, "a lightmap is NULL");
    if (bad_rgb(rgb, num_maps)) return err(FMGI_ERR_ARG, fn, "an rgb component is not finite or outside [0, 32)");
    for (int k = 0; k < 3 * num_maps; k++)
        if (!isfinite(refl[k]) || !(refl[k] >= 0.0f && refl[k] <= 1.0f))
            return err(FMGI_ERR_ARG, fn, "a refl component is not finite or outside [0, 1]");
    if (!isfinite(flux) || !(flux > 0)) return err(FMGI_ERR_ARG, fn, "flux is not finite and positive");
    SunState &st = *c.sun;
    if (!st.scene_set) return err(FMGI_ERR_STATE, fn, "no scene");
    const size_t nw = st.walls.size();
    std::vector<SunBounceWall> walls(nw);
    int64_t total = 0;
    double max_area = 0;
    for (size_t i = 0; i < nw; i++) {
        const AoRect &r = st.hits[i];
        const int32_t *lm = st.walls[i].lightmapSetup;
        SunBounceWall &w = walls[i];
        memset(&w, 0, sizeof w);
        w.s0 = lm[0];
        w.n = lm[1] * lm[2];
        w.first = (int32_t)total;
        w.area_t = ((double)r.wl * (double)r.hl) / (double)((int64_t)lm[1] * lm[2]);
        max_area = std::max(max_area, w.area_t);
        total += w.n; /* fmgi_set_scene: s0 + s1 * s2 <= numTexels, an int */
    }
    /* g_n <= 1 up to rounding, a reflectance's powers <= 1, rgb < 32: no deposit reaches 2^55 */
    if (!(ldexp(32.0 * (double)bounces * 1.001 * flux * max_area, 25) < 36028797018963968.0))
        return err(FMGI_ERR_ARG, fn, "a deposit may reach 2^55: flux * texel area is too large");
    if (c.device == FMGI_HOST_ONLY) return err(FMGI_ERR_NO_DEVICE, fn, "host-only context");

    SUNCHK(hipSetDevice(c.device));
    hipStream_t q = stream ? (hipStream_t)stream : c.stream;
    if (nw == 0 || total == 0) return FMGI_OK;
    int rc = device_tables(st);
    if (rc != FMGI_OK) return rc;
    if ((rc = grow(&st.d_bounce_walls, &st.bounce_walls_cap, nw)) != FMGI_OK) return rc;
    SunStage *stage = nullptr;
    if ((rc = stage_acquire(st, nw * sizeof(SunBounceWall), &stage)) != FMGI_OK) return rc;
    memcpy(stage->host, walls.data(), nw * sizeof(SunBounceWall));
    if (st.pending) SUNCHK(hipStreamWaitEvent(q, st.ev, 0));
    st.pending = true;
    hipError_t e = hipMemcpyAsync(st.d_bounce_walls, stage->host, nw * sizeof(SunBounceWall), hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = hipEventRecord(stage->done, q);
    stage->pending = true;
    for (int k0 = 0; k0 < num_maps && e == hipSuccess; k0 += FMGI_SUN_BOUNCE_MAPS) {
        SunBounceAdd a;
        memset(&a, 0, sizeof a);
        a.walls = st.d_bounce_walls;
        a.nwalls = (int)nw;
        a.total = (int)total;
        a.bounce = (const float *)bounce_dev;
        a.bounces = bounces;
        a.maps = std::min(FMGI_SUN_BOUNCE_MAPS, num_maps - k0);
        a.num_texels = c.num_texels;
        a.flux = flux;
        for (int m = 0; m < a.maps; m++) {
            for (int ch = 0; ch < 3; ch++) {
                a.rgb[m][ch] = rgb[3 * (size_t)(k0 + m) + ch];
                a.refl[m][ch] = refl[3 * (size_t)(k0 + m) + ch];
            }
            a.lm[m] = (unsigned long long *)lm_fx_dev[k0 + m];
        }
        e = fmgi_sun_bounce_launch_add(a, q);
    }
    const hipError_t ev = hipEventRecord(st.ev, q);
    if (e != hipSuccess) return err(FMGI_ERR_HIP, fn, hipGetErrorString(e));
    SUNCHK(ev);
    return FMGI_OK;
}

FMGI_API int fmgi_sun_units(fmgi_context *ctx, const float to_sun[3], const float rgb[3], double flux, int64_t *units) {
    static const char fn[] = "fmgi_sun_units";
    SunCtx c;
    if (!fmgi_sun_ctx(ctx, &c) || !to_sun || !rgb || !units) return err(FMGI_ERR_ARG, fn, "null argument");
    F3 s;
    int rc = check_sun(fn, to_sun, s);
    if (rc != FMGI_OK) return rc;
    if (bad_rgb(rgb, 1)) return err(FMGI_ERR_ARG, fn, "an rgb component is not finite or outside [0, 32)");
    if (!isfinite(flux) || !(flux > 0)) return err(FMGI_ERR_ARG, fn, "flux is not finite and positive");
    const SunState &st = *c.sun;
    if (!st.scene_set) return err(FMGI_ERR_STATE, fn, "no scene");
    for (int i = 0; i < (int)st.walls.size(); i++) {
        int64_t *u = units + 3 * (size_t)i;
        u[0] = u[1] = u[2] = 0;
        const float c_w = facing_cos(st, i, s);
        if (!(c_w > 0)) continue;
        if (!wall_units(st, i, c_w, rgb, flux, u))
            return err(FMGI_ERR_ARG, fn, "a wall's unit reaches 2^55: flux * rgb * texel area is too large");
    }
    return FMGI_OK;
}
