/*
 * fmgi_view.h -- shared host/device structures of the view renderer: the reference's debug raycaster
 * (debugRaytracer.cc:121-176) on the GPU, for any pin-hole camera and for batches of cameras.
 *
 * The reference builds one sorted candidate list per camera (getSortedIntersectableRects,
 * radiosityNative.c:25-62, over the walls only) and casts one ray per pixel through
 * findClosestIntersectionSorted (radiosityNative.c:67-90). Here:
 *   k_view_candidates  one workgroup per camera: k_rad_rays's prologue (backface / isBehindRay culling,
 *                      getShortestDistanceRectToPoint keys, bitonic sort on (distance, index)) written to a
 *                      global [cameras][sort_n] key array and a per-camera count;
 *   k_view_rays        one lane per pixel, one wave per 8x8 pixel block: the screen position and ray of
 *                      debugRaytracer.cc:154-155, the sorted walk with its early exit, getTileIdAt
 *                      (rectangle.c:205-230) at the hit point, and the RGB8 bytes of the hit tile.
 * The rectangles are the radiosity backend's RadRect / AoRect images of the walls, built by the same host
 * code (fmgi_rad_host.cpp), so edge lengths and unit edges carry the same bits in both backends.
 */
#ifndef FMGI_VIEW_H
#define FMGI_VIEW_H

#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "fmgi_rad.h"

#define FMGI_VIEW_TILE 8   /* a wave covers TILE x TILE pixels */
#define FMGI_VIEW_BLOCK 16 /* a workgroup of 256 lanes covers BLOCK x BLOCK pixels (2 x 2 waves) */
#define FMGI_VIEW_MAX_DIM (65535 * FMGI_VIEW_BLOCK) /* grid limit of the pixel-tile axes */
#define FMGI_VIEW_MAX_BATCH 65535                   /* cameras per launch (grid z) */

/* one camera, set up on the host in fp32 (debugRaytracer.cc:121-125) */
struct ViewCam {
    float px, py, pz; /* camPos */
    float dx, dy, dz; /* camDir = normalized(dir) */
    float cx, cy, cz; /* screenCenter = camPos + camDir */
    float rx, ry, rz; /* camRight = cross(camDir, up) */
    float ux, uy, uz; /* up, as given */
    float pixel;      /* the reference's dx = dy */
};
static_assert(sizeof(ViewCam) == 64, "ViewCam must be 64 B");

struct ViewArgs {
    const RadRect *rects; /* the walls */
    const AoRect *hits;   /* the same walls as intersects() sees them */
    int nrects;
    int sort_n;           /* power of two >= nrects */
    const ViewCam *cams;  /* this launch's cameras */
    int ncams;
    int width, height;
    unsigned long long *keys; /* [ncams][sort_n]: (minDistance bits << 32) | wall index, ~0 for culled walls */
    int32_t *counts;          /* [ncams] */
    const int64_t *first_tile; /* [nrects]: running sum of s1 * s2 (null without tiles) */
    const uint8_t *tiles_rgb;  /* the output step's RGB8 tiles in wall order (null: no rgb) */
    uint32_t background;       /* r | g << 8 | b << 16 */
    int32_t *wall_out;         /* [ncams][height][width] each, or null */
    int32_t *texel_out;
    float *dist_out;
    uint8_t *rgb_out;          /* [ncams][height][width][3], or null */
    unsigned long long *tests; /* one counter: intersects() evaluations */
};

/*
 * k_view_shade (fmgi_shade_views): samples x samples rays per pixel through the same walk, each coloured
 * from the hit wall's tiles (nearest tile, or four taps clamped to the wall's own grid), resolved in fixed
 * point. A lane keeps its pixel and loops the samples, so the candidate index stays wave-uniform; the integer
 * sums make the result independent of the sample order. One launch covers the pixel window [x0, x1) x [y0, y1)
 * of every camera; the host sizes the windows so that a launch casts at most FMGI_VIEW_MAX_RAYS rays.
 */
#define FMGI_VIEW_SAMPLES 8                       /* FMGI_VIEW_MAX_SAMPLES of the C ABI */
#define FMGI_VIEW_MAX_RAYS ((int64_t)1 << 28)     /* rays per k_view_shade launch */

struct ShadeArgs {
    ViewArgs v;            /* as k_view_rays reads it; wall_out, texel_out, dist_out and tiles_rgb unused */
    const uint32_t *tiles; /* one word per tile, r | g << 8 | b << 16, in wall order (null: no rgb) */
    uint8_t *cov_out;      /* [ncams][height][width]: the pixel's rays that hit a wall, or null */
    float offs[FMGI_VIEW_SAMPLES]; /* sample offsets in pixels, (2i + 1 - S) / 2S */
    int samples;           /* S: 1 .. FMGI_VIEW_SAMPLES */
    int filter;            /* 0 nearest, 1 bilinear */
    int x0, y0, x1, y1;    /* this launch's pixels */
};

/*
 * The traced view (fmgi_view_cache_*): k_view_trace casts k_view_shade's rays once and keeps every
 * sample's taps, k_view_resolve shades any number of tile sets from them.
 * Records are sample-major: sample n = j * S + i of camera c, pixel (y, x), lives at [c][n][y][x].
 *   NEAREST   one uint32: first_tile[wall] + ty * s1 + tx, or FMGI_VIEW_MISS
 *   BILINEAR  16 B {uint32 t00, uint32 t10, float fu, float fv}:
 *             t00 = (first_tile + ya * s1 + xa) | (xb != xa) << 31, t10 = first_tile + yb * s1 + xa, fu and fv
 *             tap_axis's weights; a miss is t00 = FMGI_VIEW_MISS
 * so a scene of a traced view holds fewer than 2^31 tiles.
 */
#define FMGI_VIEW_SETS 8 /* tile sets per k_view_resolve pass: FMGI_VIEW_CACHE_MAX_SETS of the C ABI */
#define FMGI_VIEW_MISS 0xFFFFFFFFu

struct TraceArgs {
    ShadeArgs s;               /* as k_view_shade reads it; tiles, cov_out, rgb_out and background unused */
    void *records;             /* [ncams][samples^2][height][width] records of this launch's cameras */
    unsigned long long *hits;  /* one counter: rays that hit a wall */
};

struct ResolveArgs {
    const void *records;                  /* [ncams][samples^2][height][width] */
    const uint32_t *tiles[FMGI_VIEW_SETS]; /* per set: one word per tile, as k_view_pack makes them */
    uint8_t *rgb[FMGI_VIEW_SETS];          /* per set: [ncams][height][width][3] */
    uint8_t *cov_out;                     /* [ncams][height][width], or null */
    int nsets;                            /* 1 .. FMGI_VIEW_SETS */
    int ncams, width, height;
    int samples, filter;
    uint32_t background; /* r | g << 8 | b << 16 */
};

/*
 * The orthographic and equirectangular cameras (fmgi_*_proj). Their ViewCam holds an orthonormal
 * frame: d = f = normalized(dir), r = normalized(cross(f, up)), u = cross(r, f), c = pos + f. The kernels are
 * instances of k_view_candidates_proj, k_view_shade_proj and k_view_trace_proj; the pin-hole keeps its own.
 */
#define FMGI_VIEW_PINHOLE 0 /* FMGI_PROJ_* of the C ABI */
#define FMGI_VIEW_ORTHO 1
#define FMGI_VIEW_EQUIRECT 2

struct ShadeProjArgs {
    ShadeArgs s;
    float kphi, ktheta; /* EQUIRECT: radians per pixel column and row, 2 pi / width and pi / height */
};

struct TraceProjArgs {
    TraceArgs t;
    float kphi, ktheta;
};

/*
 * The glossy floor (fmgi_*_gloss): a sample that lands at the bake's mirror height casts one mirror
 * ray and blends what it sees into its colour. The mirror ray walks a second list per camera, every wall of the
 * scene keyed by its distance to the camera position (k_view_candidates_proj<FMGI_VIEW_MIRROR>: no culls), with
 * the walk's lower bound moved to the camera: the path camera -> floor -> hit is base + best long, and no wall is
 * nearer to the camera than its key. The kernels are k_view_shade_gloss<P>, k_view_trace_gloss<P> and
 * k_view_resolve_gloss<BILINEAR>; the kernels above are not touched.
 *
 * A traced view keeps, next to its primary records, one mirror record per sample at the same [c][n][y][x] index and
 * in the same NEAREST / BILINEAR form; its first word is FMGI_VIEW_NO_MIRROR for a sample that does not mirror and
 * FMGI_VIEW_MISS for a mirror ray that hit nothing.
 */
#define FMGI_VIEW_MIRROR 3 /* k_view_candidates_proj only: the mirror list */
#define FMGI_VIEW_NO_MIRROR 0xFFFFFFFEu
#define FMGI_VIEW_MIRROR_Z 4.99999965541064739227294921875e-4f /* (double)z > 0.0005 in fp32, as k_bake has it */

struct GlossArgs {
    const unsigned long long *mkeys; /* [ncams][sort_n]: the mirror lists, nrects entries each */
    unsigned long long *counters;    /* three counters: mirror rays, mirror hits, mirror tests */
    float gloss;                     /* the mirror's weight; the trace does not read it */
};

struct ShadeGlossArgs {
    ShadeProjArgs q;
    GlossArgs g;
};

struct TraceGlossArgs {
    TraceProjArgs q;
    GlossArgs g;
    void *mrecords; /* the mirror records of this launch's cameras */
};

struct ResolveGlossArgs {
    ResolveArgs r;
    const void *mrecords;
    float gloss;
};

/* a.keys and a.counts: the mirror lists' own buffers */
hipError_t fmgi_view_launch_candidates_mirror(const ViewArgs &a, hipStream_t s);
/* projection: FMGI_VIEW_PINHOLE, _ORTHO or _EQUIRECT */
hipError_t fmgi_view_launch_shade_gloss(const ShadeGlossArgs &a, int projection, hipStream_t s);
hipError_t fmgi_view_launch_trace_gloss(const TraceGlossArgs &t, int projection, hipStream_t s);
hipError_t fmgi_view_launch_resolve_gloss(const ResolveGlossArgs &r, hipStream_t s);

hipError_t fmgi_view_launch_candidates_proj(const ViewArgs &a, int projection, hipStream_t s);
hipError_t fmgi_view_launch_shade_proj(const ShadeProjArgs &a, int projection, hipStream_t s);
hipError_t fmgi_view_launch_trace_proj(const TraceProjArgs &t, int projection, hipStream_t s);

hipError_t fmgi_view_launch_trace(const TraceArgs &t, hipStream_t s);
hipError_t fmgi_view_launch_resolve(const ResolveArgs &r, hipStream_t s);

hipError_t fmgi_view_launch_candidates(const ViewArgs &a, hipStream_t s);
hipError_t fmgi_view_launch_rays(const ViewArgs &a, hipStream_t s);
/* RGB8 tiles -> one word per tile */
hipError_t fmgi_view_launch_pack(const uint8_t *tiles_rgb, uint32_t *tiles, int64_t ntiles, hipStream_t s);
hipError_t fmgi_view_launch_shade(const ShadeArgs &a, hipStream_t s);

/* the radiosity backend's host images of a rectangle (fmgi_rad_host.cpp) */
struct fmgi_rect;
RadRect fmgi_rad_rect(const fmgi_rect &r);
AoRect fmgi_rad_hit_rect(const fmgi_rect &r);

#endif
