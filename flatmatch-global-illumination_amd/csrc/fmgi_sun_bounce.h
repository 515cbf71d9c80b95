/*
 * fmgi_sun_bounce.h -- shared host/device structures of the bounced-sun layer (include/flatmatch_gi.h
 * "Bounced sunlight"): fmgi_rad_cache_sun_bounce gathers, per sun direction, a scalar start table made of a
 * coverage map through the radiosity cache's form factors (fmgi_rad.h: the rays' texel ids) into N bounce tables;
 * fmgi_sun_add_bounced adds them, under any colour and reflectance, to the int64 lightmap. The kernels are in
 * fmgi_sun_bounce.hip; the host side of the first call is in fmgi_rad_host.cpp (it owns the cache), that of the
 * second in fmgi_sun_host.cpp (it owns the context's scene).
 */
#ifndef FMGI_SUN_BOUNCE_H
#define FMGI_SUN_BOUNCE_H

#include <stdint.h>

#include <math.h>

#include <hip/hip_runtime_api.h>

#include "fmgi_rad.h"

#define FMGI_SUN_BOUNCE_DIRS 32 /* == FMGI_SUN_BOUNCE_MAX_DIRS: slots of a pass, one 128-B line per texel */
#define FMGI_SUN_BOUNCES 8      /* == FMGI_SUN_MAX_BOUNCES */
#define FMGI_SUN_BOUNCE_MAPS 8  /* == FMGI_SUN_MAX_MAPS: lightmaps one k_sun_add_bounced launch carries */

/* a pass of fmgi_rad_cache_sun_bounce: up to 32 directions over `[texel][kp]` float tables. The per-direction
   values travel as kernel arguments, so the call's host arrays are read before it returns. */
struct SunBounce {
    const int32_t *sids; /* FMGI_RAD_RAYS x njobs, ray-major */
    const RadJob *jobs;
    int64_t njobs;
    const RadRect *rects; /* the cache's rectangles; the first nwalls are the walls */
    int nwalls;
    int kp;              /* slots per texel: 1, 2, 4, 8, 16 or 32 */
    int ndirs;           /* directions of this pass, 1..kp */
    int64_t ntex;        /* entries of a table: texels incl. the window/light texels */
    int64_t num_texels;  /* the walls' texels: the ids a gather may read, the entries a row holds */
    const float *src;    /* e_{n-1} */
    float *dst;          /* g_n: written at the jobs' texels, +0 elsewhere from the pass's memset */
    int row;             /* k_sun_unpack: n - 1 */
};

/* per-direction arguments of a pass; slots ndirs .. 31 are unused */
struct SunBounceDirs {
    const uint8_t *cover[FMGI_SUN_BOUNCE_DIRS]; /* uint8 [num_texels] */
    float *out[FMGI_SUN_BOUNCE_DIRS];           /* float [bounces][num_texels] */
    float sx[FMGI_SUN_BOUNCE_DIRS], sy[FMGI_SUN_BOUNCE_DIRS], sz[FMGI_SUN_BOUNCE_DIRS]; /* unit vectors to the sun */
    float s2[FMGI_SUN_BOUNCE_DIRS];             /* (float)(S * S) */
};

/* a wall as k_sun_add_bounced sees it: its level-0 grid, its first texel in the call's running count, area_t */
struct SunBounceWall {
    int32_t s0, n;   /* the first level-0 texel and their number (s1 * s2) */
    int32_t first;   /* level-0 texels of the walls before this one */
    int32_t pad;
    double area_t;   /* ((double)|width| * (double)|height|) / (double)(s1 * s2) */
};
static_assert(sizeof(SunBounceWall) == 24, "SunBounceWall must be 24 B");

struct SunBounceAdd {
    const SunBounceWall *walls;
    int nwalls, total;     /* total: level-0 texels of all walls; every first is below it */
    const float *bounce;   /* float [bounces][num_texels] */
    int bounces, maps;     /* 1..FMGI_SUN_BOUNCES, 1..FMGI_SUN_BOUNCE_MAPS */
    int num_texels;
    double flux;
    float rgb[FMGI_SUN_BOUNCE_MAPS][3], refl[FMGI_SUN_BOUNCE_MAPS][3];
    unsigned long long *lm[FMGI_SUN_BOUNCE_MAPS];
};

/* s = to_sun / |to_sun| as fmgi_sun_coverage computes it; false for a zero or non-finite length. Host code that
   includes this is built without contraction. */
static inline bool fmgi_sun_unit_vector(const float to_sun[3], float s[3]) {
    const float x = to_sun[0], y = to_sun[1], z = to_sun[2];
    const float l = sqrtf((x * x + y * y) + z * z);
    if (!(l > 0) || !isfinite(l)) return false;
    s[0] = x / l, s[1] = y / l, s[2] = z / l;
    return true;
}

hipError_t fmgi_sun_bounce_launch_e0(const SunBounce &b, const SunBounceDirs &d, hipStream_t s);
hipError_t fmgi_sun_bounce_launch_gather(const SunBounce &b, hipStream_t s);
hipError_t fmgi_sun_bounce_launch_unpack(const SunBounce &b, const SunBounceDirs &d, hipStream_t s);
hipError_t fmgi_sun_bounce_launch_add(const SunBounceAdd &a, hipStream_t s);

#endif
