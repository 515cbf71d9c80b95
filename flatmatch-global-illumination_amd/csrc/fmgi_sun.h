/*
 * fmgi_sun.h -- shared host/device structures of the direct-sun layer (include/flatmatch_gi.h
 * "Direct sunlight through windows"): fmgi_sun_coverage counts, per level-0 texel of every wall that faces the
 * sun, the sub-texel shadow rays that leave through a window before they meet a wall; fmgi_sun_add turns the
 * counts into deposits of the int64 lightmap. The kernels are in fmgi_sun.hip, the host side and the C ABI in
 * fmgi_sun_host.cpp; the context (fmgi_api.cpp) owns one SunState.
 */
#ifndef FMGI_SUN_H
#define FMGI_SUN_H

#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "fmgi_ao.h"

#define FMGI_SUN_SAMPLES 8 /* == FMGI_SUN_MAX_SAMPLES */
#define FMGI_SUN_MAPS 8    /* == FMGI_SUN_MAX_MAPS: lightmaps one k_sun_add launch carries */
#define FMGI_SUN_BLOCK 512 /* threads of a k_sun_rays workgroup (8 waves) */
#define FMGI_SUN_LDS_MAX_LISTS 1024 /* more lists than this: the records are read from global memory */

/* a wall that faces the sun, as a call's job list holds it (64 B): the rectangle as given (the samples' points
   are pos + width * a + height * b), its level-0 grid, and its first texel in the call's running texel count */
struct SunJob {
    float px, py, pz, wx, wy, wz, hx, hy, hz;
    int32_t s0, s1, s2;
    int32_t first; /* job texels of the walls before this one */
    int32_t wall;  /* its index in the scene */
    int32_t pad0, pad1;
};
static_assert(sizeof(SunJob) == 64, "SunJob must be 64 B");

enum { SUN_CTR_CROSSING = 0, SUN_CTR_LIT, SUN_CTR_TESTS, SUN_CTR_ENTRIES, SUN_CTR_N };

struct SunArgs {
    const SunJob *jobs; /* njobs records, first ascending from 0 */
    int njobs;
    int total;          /* job texels: every first is below it */
    const AoRect *hits; /* the scene's walls as intersects() reads them */
    int nwalls;
    const AoRect *wins; /* the windows, likewise */
    int nwins;
    int32_t *lists;     /* nlists lists of wall indices, list l at lists[l * list_cap] */
    int32_t *list_len;  /* their lengths (the kernels clamp them to list_cap) */
    int list_cap;       /* == max(nwalls, 1) */
    int nlists;         /* FMGI_SUN_LISTS: one per window; FMGI_SUN_ALL: 1 */
    int all;            /* FMGI_SUN_ALL: every lane walks list 0 */
    float sx, sy, sz;   /* the unit vector to the sun */
    int S;              /* samples per texel edge, 1..8 */
    int lds_entries;    /* records the launch's dynamic LDS has room for after the nlists + 1 offsets; 0: none */
    uint8_t *cover;
    int num_texels;
    unsigned long long *counters; /* SUN_CTR_* */
};

struct SunAddArgs {
    const SunJob *jobs;
    int njobs, total;
    const long long *units; /* [njobs][maps][3] */
    int maps;               /* 1..FMGI_SUN_MAPS */
    int S2;                 /* samples * samples */
    const uint8_t *cover;
    int num_texels;
    unsigned long long *lm[FMGI_SUN_MAPS];
};

size_t fmgi_sun_lds_bytes(const SunArgs &a);
hipError_t fmgi_sun_launch_lists(const SunArgs &a, hipStream_t s);
hipError_t fmgi_sun_launch_rays(const SunArgs &a, int num_cus, hipStream_t s);
hipError_t fmgi_sun_launch_add(const SunAddArgs &a, hipStream_t s);

/* the context's side (fmgi_api.cpp): its sun state, created on first use, and what the calls need of it */
struct SunState;
struct fmgi_context;
struct fmgi_rect;
struct SunCtx {
    SunState *sun;
    int device; /* FMGI_HOST_ONLY or the HIP device */
    int num_cus, num_texels;
    hipStream_t stream; /* the context's own */
};
bool fmgi_sun_ctx(fmgi_context *c, SunCtx *out);
SunState *fmgi_sun_new();
void fmgi_sun_free(SunState *s, bool has_device); /* with the device current */
void fmgi_sun_set_scene(SunState *s, const fmgi_rect *walls, int nwalls, const fmgi_rect *windows, int nwins);

#endif
