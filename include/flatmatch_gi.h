/*
 * flatmatch_gi.h -- C ABI of libflatmatch_gi.so, the MI355X-native drop-in for the reference's
 * OpenCL photon-mapping path (rbuch703/flatmatch-global-illumination).
 *
 * Drop-in entry point (replaces global_illumination_cl.c:275-321, declared at
 * global_illumination_cl.h:10):
 *
 *     void performGlobalIlluminationCl(Geometry *geo, int numSamplesPerArea);
 *
 * The reference's main.c (main.c:63) links against this library unchanged: it includes its own
 * global_illumination_cl.h; the symbol name, argument meaning, in-place texel update and fatal-error
 * behaviour (message on stdout + exit(-1), global_illumination_cl.c:254,263) are the reference's.
 * libc rand() is consumed once per kernel launch of the reference schedule
 * (global_illumination_cl.c:251), so RNG seeds and post-call libc state match the reference.
 *
 * Everything else here is build-defined (prefix fmgi_) and exists so tests and bench.py can drive
 * the device-resident path with plain pointers: no torch or HIP types cross this boundary
 * (streams are passed as void* hipStream_t, device buffers as void*).
 *
 * Environment knobs the reference ABI cannot carry (read by performGlobalIlluminationCl):
 *   FMGI_WG        virtual OpenCL work-group size of the launch schedule (default 256, the value
 *                  ROCm's OpenCL reports for CL_KERNEL_WORK_GROUP_SIZE; global_illumination_cl.c:300)
 *   FMGI_GPUS      number of GPUs one drop-in call shards over (default 1, like the reference; max 8)
 *   FMGI_REDUCE    how a multi-GPU call sums the shard lightmaps: "rccl" (default: one ncclReduce over
 *                  the shard devices) or "peer" (binary tree of xGMI peer copies + adds)
 *   FMGI_KERNEL    "auto" (default), "grid", "fast", "hybrid" or "exact" -- all produce identical bits
 *   FMGI_DROPIN_CACHE  0, 1 (default) or 2: device state kept between calls (fmgi_dropin_release)
 *   FMGI_QUIET     1 = suppress the reference's progress line
 */
#ifndef FLATMATCH_GI_H
#define FLATMATCH_GI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Layout-identical equivalents of the reference ABI types (no CL headers needed). ---------- */
/* Vector3 == cl_float4 (vector3_cl.h:14): 16 B, 16-B aligned; .s[3] unused.                      */
typedef struct __attribute__((aligned(16))) fmgi_vec3 { float s[4]; } fmgi_vec3;
/* Rectangle (rectangle.h:19-26): 80 B, 16-B aligned. lightmapSetup = {texel base, tiles along
   width, tiles along height, 0}. Windows/lights have lightmapSetup.s0 == 0.                       */
typedef struct __attribute__((aligned(16))) fmgi_rect {
    fmgi_vec3 pos, width, height, n;
    int32_t lightmapSetup[4];
} fmgi_rect;
/* Geometry (geometry.h:7-15): 80 B. boxWalls are not used by the photon-mapping path.             */
typedef struct fmgi_geometry {
    fmgi_rect *windows, *lights, *walls, *boxWalls;
    int32_t numWindows, numLights, numWalls, numBoxWalls;
    int32_t width, height;
    float startingPositionX, startingPositionY;
    int32_t numTexels;
    fmgi_vec3 *texels;
} fmgi_geometry;

/* ---- Drop-in entry points ----------------------------------------------------------------------- */
#ifndef GLOBAL_ILLUMINATION_CL /* the reference header declares it with its own Geometry type */
void performGlobalIlluminationCl(fmgi_geometry *geo, int numSamplesPerArea);
#endif
/* North-star name, build-defined (the reference has no such symbol): same bake, but the result is
   written to texels_out[numTexels] (initial values taken from geo->texels, which is not modified).
   Returns 0 on success, a negative fmgi error code otherwise (no exit()). */
int getGlobalIlluminationCl(const fmgi_geometry *geo, int numSamplesPerArea, fmgi_vec3 *texels_out);
/* The drop-in entry points keep their per-geometry device state (contexts, scene tables, lightmaps; a
   few MB per shard) across calls and free the deposit-code stream buffers at the end of every call
   (FMGI_DROPIN_CACHE=1, the default); FMGI_DROPIN_CACHE=0 frees everything after every call, as the
   reference does (global_illumination_cl.c:315-320); FMGI_DROPIN_CACHE=2 keeps the stream buffers too.
   This frees all of it, and the RCCL communicators of a multi-GPU call. */
void fmgi_dropin_release(void);
/* Ranks of the RCCL communicator the last multi-GPU drop-in call reduced over (ncclCommCount; one rank
   per shard device), 0 if that call reduced without RCCL. */
int fmgi_dropin_rccl_ranks(void);
/* The drop-in's multi-GPU layout (host only; for tests): shard k -> device dev[k], work items
   [begin[k], end[k]); and its binary-tree reduction into shard 0 (returns the step count, nshard - 1). */
int fmgi_dropin_shards(uint64_t items, int ngpu, int nshard, int32_t *dev, uint64_t *begin, uint64_t *end);
int fmgi_dropin_reduce_order(int nshard, int32_t *dst, int32_t *src);

/* ---- Ambient occlusion ------------------------------------------------------ */
/* The reference's performAmbientOcclusionNative (global_illumination_native.h:16, photonmap.c:478-490)
   on the GPU, bit-identical: every level-0 texel of every wall becomes (d, d, d, 0), d the
   cosine-weighted mean distance over the 481 geoSphere4 directions (misses count 10), traced through
   the reference's BSP tree. Same argument meaning and in-place update; a different name, because the
   reference's photonmap.o (which main.c also needs for performPhotonMappingNative) already defines
   performAmbientOcclusionNative. Fatal errors print "[Err] ..." and exit(-1).
   Limitation: the BSP build stops at 48 levels (the device traversal stack). The reference's build
   rule does not end on some scenes with off-axis walls: a tilted rect whose own corners are not on its
   own plane in fp32 is handed, as the split plane, to a child together with every other item of the
   node, and that child repeats the node (the reference recurses until it runs out of memory). Such a
   scene is an error here -- FMGI_ERR_ARG with a message naming the BSP depth from
   fmgi_ambient_occlusion and fmgi_ao_tree, before a device is looked for; the "[Err]" exit from
   performAmbientOcclusionGpu -- never a crash. Axis-aligned scenes are not affected. */
void performAmbientOcclusionGpu(fmgi_geometry *geo);
/* Non-mutating form for walls [wall_begin, wall_end) (the BSP always spans every wall):
   texels_out = geo->texels with those walls' level-0 texels replaced. Returns 0 or FMGI_ERR_*. */
int fmgi_ambient_occlusion(const fmgi_geometry *geo, int wall_begin, int wall_end, fmgi_vec3 *texels_out);
/* The direction table of `levels` subdivisions (4 = the AO table, 481 directions) in the reference's
   order, as xyz float triples; returns the count and copies at most `cap` directions. */
int fmgi_geosphere(int levels, float *xyz, int cap);
/* The AO BSP tree, encoded per node as {left, right, plane wall, n, n wall indices}; returns the
   encoding's length and copies at most `cap` ints, or FMGI_ERR_ARG for a scene over the depth bound. */
int64_t fmgi_ao_tree(const fmgi_geometry *geo, int32_t *out, int64_t cap);

/* ---- Output step: what main.c:66-95 does after the bake, minus the PNG encoding */
/* Normalisation for the photon modes (main.c:66-79; numSamplesPerArea = 0 skips it, as the reference
   does for AO/radiosity), then every wall's RGB8 tile as the reference's saveAs()/saveAs_core
   (rectangle.c:295-345) builds it before write_png_file: tone map 1 - exp(-2 L), clamp, floor tint
   (tintExtra: the second tint of the AO/native modes). texels_out = geo->texels normalised;
   rgb_out = the walls' tiles concatenated in wall order, fmgi_output_tile_bytes(geo) bytes.
   Byte-identical to the reference. Returns 0 or FMGI_ERR_*. */
int fmgi_output_tiles(const fmgi_geometry *geo, int numSamplesPerArea, int tintExtra, fmgi_vec3 *texels_out,
                      uint8_t *rgb_out);
int64_t fmgi_output_tile_bytes(const fmgi_geometry *geo);

/* ---- Radiosity --------------------------------------------------------------- */
/* The reference's performRadiosityNative (radiosityNative.h:10, radiosityNative.c:92-268) on the GPU:
   10000 libc-rand() cosine rays per level-0 wall texel against its sorted candidate list, then 7
   gather/update/mipmap bounces; geo->texels[0, numTexels) receive the result (w = 0). The caller's
   libc rand() stream (glibc's default TYPE_3 generator) is replayed on the device and left where the
   reference leaves it (2 x 10000 draws per level-0 wall texel). Same argument meaning and in-place
   update; a different name so that the reference's radiosityNative.o can stay linked. Fatal errors
   print "[Err] ..." and exit(-1). */
void performRadiosityGpu(fmgi_geometry *geo);
/* Non-mutating form: texels_out[numTexels] = the result; sids_out (NULL or jobs x 10000 int32) = the
   reference's sourceTexelIds rows of the level-0 wall texels, wall/tile order (-1: the ray hit
   nothing). Returns 0 or FMGI_ERR_*. */
int fmgi_radiosity(const fmgi_geometry *geo, fmgi_vec3 *texels_out, int32_t *sids_out);
/* number of level-0 wall texels (jobs); the rand() draws of a call are 20000 x this */
int64_t fmgi_radiosity_jobs(const fmgi_geometry *geo);
typedef struct fmgi_rad_stats {
    int64_t jobs, rects, texels, rays; /* texels includes the window/light texels */
    double rand_ms;                    /* device rand() replay */
    double rays_ms;                    /* candidate lists + ray casts (+ uploads) */
    double bounce_ms;                  /* 7 x (gather, update, mipmap) */
    double total_ms;                   /* first upload .. last bounce */
} fmgi_rad_stats;
/* statistics of the last fmgi_radiosity / performRadiosityGpu call */
int fmgi_radiosity_stats(fmgi_rad_stats *out);
/* Host only: advance the caller's libc rand() generator by n draws with the jump matrices the
   radiosity backend uses (as n rand() calls would). Returns 0 or FMGI_ERR_ARG (not glibc TYPE_3). */
int fmgi_rand_skip(uint64_t n);

/* ---- Radiosity scenarios ------------------------------------------------------------- */
/* A radiosity cache of a geometry holds the rectangle list (walls, windows, lights; the windows' and lights'
   texels appended after numTexels, radiosityNative.c:108-131), the jobs (one per level-0 wall texel) and the
   sourceTexelIds of every ray: exactly the values fmgi_radiosity computes from the caller's libc rand() position.
   fmgi_rad_cache_create consumes the stream exactly as fmgi_radiosity does (20000 x jobs draws); on failure it
   puts the stream back. fmgi_rad_cache_solve draws nothing.

   A palette is emit[k][e][3], e over the windows and then the lights, every value finite and >= 0. Scenario k's
   result is what radiosityNative.c:139-149, 230-251 computes when every texel of emitter e, mip levels included,
   starts at emit[k][e] (the reference: 30 for windows, (28, 28, 32) for lights) and the walls' texels at 0:
   `iterations` rounds of gather (the sequential fp32 sum over rays 0..9999, skipping -1), update
   (src * 0.7f + dest * (0.3f / 10000), not contracted) and mipmap (rectangle.c:508-575), in the reference's
   operations and order. The output is texels [0, numTexels) with w = 0. With fmgi_rad_reference_emit's palette
   and iterations = 7 it equals fmgi_radiosity's bit for bit. A set's result depends neither on the other sets of
   the call nor on their number.

   Argument errors are found on the host before any device call: FMGI_ERR_ARG for a NULL handle, geometry or
   pointer, num_sets < 1, iterations outside 1..FMGI_RAD_CACHE_MAX_ITERATIONS, an emit value that is negative, NaN
   or infinite, and a geometry fmgi_radiosity rejects; FMGI_ERR_ARG if libc rand() is not in glibc's TYPE_3 state;
   then FMGI_ERR_NO_DEVICE. */
#define FMGI_RAD_CACHE_MAX_SETS 8        /* palettes one pass carries; solve takes any number */
#define FMGI_RAD_CACHE_MAX_ITERATIONS 64
typedef struct fmgi_rad_cache fmgi_rad_cache;
struct fmgi_rad_cache_info {
    int64_t jobs, rects, windows, lights;
    int64_t texels;                    /* includes the window/light texels */
    int64_t rays;                      /* 10000 x jobs */
    int64_t bytes;                     /* fmgi_rad_cache_bytes */
    double rand_ms, rays_ms;           /* create's device phases, as fmgi_rad_stats */
};
/* Host only: the device bytes create keeps: 40000 per job for the ids, 64 per job and 64 per rectangle.
   FMGI_ERR_ARG (negative) for a geometry fmgi_radiosity rejects. */
int64_t fmgi_rad_cache_bytes(const fmgi_geometry *geo);
int  fmgi_rad_cache_create(const fmgi_geometry *geo, fmgi_rad_cache **out); /* *out is NULL on failure */
void fmgi_rad_cache_destroy(fmgi_rad_cache *rc);               /* NULL is allowed; waits for the handle's launches */
int  fmgi_rad_cache_info(const fmgi_rad_cache *rc, struct fmgi_rad_cache_info *out);
/* sids_out (jobs x 10000 int32): the rows in the reference's per-texel order, as fmgi_radiosity's sids_out */
int  fmgi_rad_cache_sids(const fmgi_rad_cache *rc, int32_t *sids_out);
/* Host only: emit[windows + lights][3] = the reference's palette */
int  fmgi_rad_reference_emit(const fmgi_geometry *geo, float *emit);
/* texels_dev[k]: device float [numTexels][4], the layout fmgi_view_cache_tiles reads (the radiosity mode uses
   numSamplesPerArea = 0, tintExtra = 1, main.c:88-91). Asynchronous on `stream` (a hipStream_t, NULL: the default
   stream); emit and the pointer array are read before the call returns. emit may be NULL for a geometry without
   windows and lights. The scratch (three tables of 16 B x texels x the sets of a pass) belongs to the handle and
   is guarded by an event: a later call's stream waits for the earlier call, the host does not, unless the scratch
   has to grow. More than FMGI_RAD_CACHE_MAX_SETS sets run in further passes. */
int  fmgi_rad_cache_solve(const fmgi_rad_cache *rc, const float *emit, int num_sets, int iterations,
                          void *const *texels_dev, void *stream);

/* ---- View renderer ------------------------------------------------------------ */
/* The reference's debug raycaster (debugRaytracer.cc:121-176) on the GPU, for any pin-hole camera and for
   batches of cameras. dir has any non-zero length, up is used as given, pixel is the size of one pixel on
   the screen plane at distance 1 (the reference's dx = dy = (float)(1/1000.0)). */
typedef struct fmgi_camera {
    float pos[3], dir[3], up[3];
    float pixel;
} fmgi_camera;
/* One image of width x height per camera: one ray per pixel from pos through
   screenCenter + camRight * pixel * (x - width/2) - up * pixel * (y - height/2), traced with the reference's
   getSortedIntersectableRects / findClosestIntersectionSorted (radiosityNative.c:25-90) over geo->walls.
   All pointers are host pointers; outputs are [num_cams][height][width] (rgb_out: a trailing [3]) and any of
   them may be NULL. wall_out = the index in geo->walls, texel_out = lightmapSetup[0] + getTileIdAt at the hit
   point, dist_out = the hit distance; a miss gives -1, -1, +INFINITY. rgb_out = the three bytes of the hit
   tile in tiles_rgb (fmgi_output_tiles' rgb_out, fmgi_output_tile_bytes(geo) bytes), or background.
   Bit-identical to the reference's functions. Returns 0 or FMGI_ERR_*; argument errors (width or height < 1,
   pixel not finite and positive, dir of zero length, more walls than the candidate sort holds, rgb_out
   without tiles_rgb, a wall's texels outside [0, numTexels)) are reported before any device call. */
int fmgi_render_views(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                      const uint8_t *tiles_rgb, const uint8_t background[3], int32_t *wall_out,
                      int32_t *texel_out, float *dist_out, uint8_t *rgb_out);
/* One camera's sorted candidate list, computed on the device: returns its length and copies at most cap
   entries (wall indices, minDistance values); a negative FMGI_ERR_* on failure. */
int fmgi_view_candidates(const fmgi_geometry *geo, const fmgi_camera *cam, int32_t *wall_idx, float *min_dist,
                         int cap);
/* Supersampled, filtered views for looking at a bake: samples x samples rays per pixel, sample (i, j) offset by
   ((2i + 1 - samples) / (2 samples), (2j + 1 - samples) / (2 samples)) pixels from fmgi_render_views' ray, each
   traced by the same walk. A sample that misses has the background's colour; one that hits wall t at tile
   coordinates (u, v) (getTileIdAt's, before the cast) has the tile's bytes (NEAREST), or the bilinear blend of
   the four tiles around (u - 0.5, v - 0.5), taps clamped to t's own s1 x s2 grid (BILINEAR), all fp32. Each
   sample's colour goes to fixed point, q = (int)(colour * 256 + 0.5), and the pixel's byte is
   (sum q + 128 samples^2) / (256 samples^2) in integers, so the result is exact and independent of order.
   rgb_out [num_cams][height][width][3]; coverage_out [num_cams][height][width] = how many of the pixel's rays
   hit a wall (0..samples^2); either may be NULL; rgb_out needs tiles_rgb. Host pointers. samples = 1 with
   NEAREST gives fmgi_render_views' rgb_out. Argument errors: those of fmgi_render_views, samples outside
   1..FMGI_VIEW_MAX_SAMPLES, filter not one of the two; all reported before any device call. */
enum { FMGI_VIEW_NEAREST = 0, FMGI_VIEW_BILINEAR = 1 };
#define FMGI_VIEW_MAX_SAMPLES 8
int fmgi_shade_views(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                     const uint8_t *tiles_rgb, const uint8_t background[3], int samples, int filter,
                     uint8_t *rgb_out, uint8_t *coverage_out);
/* statistics of the last fmgi_render_views or fmgi_shade_views call (rays = cameras * width * height *
   samples^2 after the latter; a struct tag: the function below carries the same name) */
struct fmgi_view_stats {
    int64_t cameras, rays;
    int64_t candidates; /* list lengths summed over the cameras */
    int64_t tests;      /* intersects() evaluations over all rays */
    double cand_ms;     /* candidate lists */
    double rays_ms;     /* ray casts */
    double total_ms;    /* first upload .. last kernel */
};
int fmgi_view_stats(struct fmgi_view_stats *out);

/* A traced view: fmgi_shade_views' rays are cast once and every sample's taps stay on the device;
   any number of lighting scenarios is then shaded from device-resident lightmaps with no host round trip. Each
   picture is, bit for bit, what fmgi_output_tiles followed by fmgi_shade_views gives for that lightmap. Like the
   calls above the cache takes no fmgi_context; its device is FMGI_DEVICE (default 0).
   create makes fmgi_shade_views' argument checks (geometry, image size, cameras, samples, filter, each camera)
   and rejects num_cams < 1, a NULL out and a scene of 2^31 tiles or more, all FMGI_ERR_ARG before any device
   call; then FMGI_ERR_NO_DEVICE; FMGI_ERR_OOM, with nothing left allocated, if the records do not fit. *out is
   NULL after any error. geo->texels is not read and geo may be freed once create returns. The trace runs in
   launches of at most 2^28 rays (FMGI_VIEW_RAYS_PER_LAUNCH in the environment lowers that). */
#define FMGI_VIEW_CACHE_MAX_SETS 8 /* tile sets one gather pass carries; shade takes any number */
typedef struct fmgi_view_cache fmgi_view_cache;
struct fmgi_view_cache_info {
    int32_t cameras, width, height, samples, filter, num_texels;
    int64_t tiles;      /* level-0 tiles of all walls: fmgi_output_tile_bytes / 3 */
    int64_t rays, hits; /* rays = cameras * width * height * samples^2; hits = rays that hit a wall */
    int64_t tests;      /* intersects() evaluations of the trace (== fmgi_view_stats.tests of the same shade call) */
    int64_t bytes;      /* device bytes of the records */
    double cand_ms, trace_ms;
};
/* host only: cameras * width * height * samples^2 * (4 for NEAREST, 16 for BILINEAR); 0 for arguments create rejects */
int64_t fmgi_view_cache_bytes(int num_cams, int width, int height, int samples, int filter);
int  fmgi_view_cache_create(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                            int samples, int filter, fmgi_view_cache **out);
void fmgi_view_cache_destroy(fmgi_view_cache *vc);            /* NULL is allowed; waits for the handle's launches */
int  fmgi_view_cache_info(const fmgi_view_cache *vc, struct fmgi_view_cache_info *out);
/* tiles and shade are asynchronous on `stream`; the pointer arrays and the background are read before they
   return. FMGI_ERR_ARG for a NULL handle or pointer or num_sets < 1 (tiles: numSamplesPerArea < 0), before any
   device call. Sets may not alias each other or the outputs. */
/* tiles_dev[k] (device, tiles * 3 bytes) = the rgb_out of fmgi_output_tiles for this geometry with
   texels = texels_dev[k] (device float [num_texels][4], read only, not normalised in place) */
int  fmgi_view_cache_tiles(const fmgi_view_cache *vc, const void *const *texels_dev, int num_sets,
                           int numSamplesPerArea, int tintExtra, void *const *tiles_dev, void *stream);
/* rgb_dev[k] (device, [cameras][height][width][3]) = fmgi_shade_views' rgb_out for tiles_dev[k];
   coverage_dev (device, [cameras][height][width], may be NULL) = its coverage_out. The sets are repacked to one
   word per tile in scratch memory of the cache (4 B per tile and set of a pass); a later call's stream waits
   for the earlier call before it reuses the scratch, without blocking the host. */
int  fmgi_view_cache_shade(const fmgi_view_cache *vc, const void *const *tiles_dev, int num_sets,
                           const uint8_t background[3], void *const *rgb_dev, void *coverage_dev, void *stream);

/* Two more cameras for the calls above; fmgi_camera is the same record. With FMGI_PROJ_PINHOLE each
   *_proj call is the call without the suffix: same code, bytes, statistics and errors. The other two use the
   orthonormal frame f = normalized(dir), r = normalized(cross(f, up)), u = cross(r, f), all fp32:
     ORTHO     the plan at true scale. Sample (i, j) of pixel (x, y) starts at
               pos + r * pixel * ((x - width/2) + ox_i) - u * pixel * ((y - height/2) + oy_j) and runs along f;
               pixel is metres per pixel. Walls facing f and walls wholly behind the screen plane are not seen.
     EQUIRECT  the 360-degree panorama from pos: phi = (x + 0.5 + ox_i) * 2 pi / width, theta = (y + 0.5 + oy_j)
               * pi / height, ray = normalized(f * (-cos phi sin theta) + r * (-sin phi sin theta) + u * cos theta).
               Column width / 2 looks along dir, x grows to the right, row 0 is straight up. pixel is not read.
   ox, oy are fmgi_shade_views' sample offsets; walk, taps and resolve are fmgi_shade_views'. A traced view made
   by fmgi_view_cache_create_proj gives, through fmgi_view_cache_tiles and _shade, bit for bit what
   fmgi_output_tiles followed by fmgi_shade_views_proj gives, and info.tests / info.hits are that call's counts.
   fmgi_view_candidates_proj returns the projection's list: ORTHO keys are the smallest depth along f of a
   wall's corners (0 if negative), EQUIRECT's list is the pin-hole's without the walls-behind-the-camera cull.
   Argument errors (FMGI_ERR_ARG, before any device call): those of the call without the suffix in its order
   (pixel is not checked for EQUIRECT), then a projection that is none of the three, then, for ORTHO and
   EQUIRECT, a camera whose cross(f, up) has zero or non-finite length. */
enum { FMGI_PROJ_PINHOLE = 0, FMGI_PROJ_ORTHO = 1, FMGI_PROJ_EQUIRECT = 2 };
int fmgi_shade_views_proj(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                          int projection, const uint8_t *tiles_rgb, const uint8_t background[3], int samples,
                          int filter, uint8_t *rgb_out, uint8_t *coverage_out);
int fmgi_view_candidates_proj(const fmgi_geometry *geo, const fmgi_camera *cam, int projection,
                              int32_t *wall_idx, float *min_dist, int cap);
int fmgi_view_cache_create_proj(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width,
                                int height, int projection, int samples, int filter, fmgi_view_cache **out);
/* the projection a traced view was made with (FMGI_PROJ_*), or FMGI_ERR_ARG for a NULL handle */
int fmgi_view_cache_projection(const fmgi_view_cache *vc);

/* The glossy floor: the bake mirrors a photon that lands at z <= 0.0005 three times out of four, and
   these calls draw that floor with one mirror bounce. Everything up to a sample's primary hit is
   fmgi_shade_views_proj's: origin src, direction dir, wall t with normal n_t, distance dist, colour val[c] (the
   tap before its fixed-point step). All arithmetic is fp32 in this order, no FMA:
     mirror sample  the sample hit a wall and !(P.z > 4.99999965541064739227294921875e-4f), P = src + dir * dist
                    (the bake's test; no test on the wall's orientation)
     mirror ray     two = 2 * dot(n_t, dir), d2 = dir - n_t * two (not normalised again), Q = P + d2 * 1e-5f
     mirror list    per camera every wall of the scene, no culls, keyed by its shortest distance to the camera
                    position and sorted by (key bits, wall index); the same list for all three projections
     mirror walk    best = inf, wall2 = -1, base = |Q - pos|; for the list's entries in order: stop if
                    (base + best) < key; count one test; dn = intersects(wall, Q, d2, best); skip if dn < 0;
                    if dn <= best take the wall and best = dn
     colour         mval[c] = background[c] if wall2 < 0, else wall2's tap at Q + d2 * best (nearest or bilinear
                    as the call's filter says); the sample's colour is (1 - gloss) * val[c] + gloss * mval[c], then
                    the fixed-point step and the resolve of fmgi_shade_views. One bounce: the mirror hit is not
                    reflected again. Samples that do not mirror keep val.
   Coverage stays the number of primary hits. fmgi_view_stats.rays stays the primary rays, .tests counts both
   walks; the second walk runs whether or not rgb_out is given. gloss == 0 is fmgi_shade_views_proj: same
   launches, bytes and tests, no mirror list and no second walk.
   Argument errors: those of fmgi_shade_views_proj in its order, then a gloss that is NaN, infinite, below 0 or
   above 1 (FMGI_ERR_ARG before any device call), then FMGI_ERR_NO_DEVICE. */
int fmgi_shade_views_gloss(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width, int height,
                           int projection, const uint8_t *tiles_rgb, const uint8_t background[3], int samples,
                           int filter, float gloss, uint8_t *rgb_out, uint8_t *coverage_out);
/* the mirror rays of the last fmgi_shade_views_gloss (gloss > 0) or fmgi_view_cache_create_gloss call, how many of
   them hit a wall and their intersects() evaluations; zeros after any other render, shade or create call */
struct fmgi_view_gloss_stats {
    int64_t mirror_rays, mirror_hits, mirror_tests;
};
int fmgi_view_gloss_stats(struct fmgi_view_gloss_stats *out);
/* A traced view with mirror records: fmgi_view_cache_create_proj's checks, trace and primary records, and in a
   second allocation, at the same [c][n][y][x] index and in the same NEAREST / BILINEAR form, one mirror record
   per sample (first word 0xFFFFFFFE: the sample does not mirror, 0xFFFFFFFF: its mirror ray missed). The records do
   not depend on gloss. info.bytes covers both planes (twice fmgi_view_cache_bytes), info.tests is the sum of both
   walks (== fmgi_view_stats.tests of the matching fmgi_shade_views_gloss call), info.hits the primary hits.
   FMGI_ERR_OOM leaves nothing allocated. */
int fmgi_view_cache_create_gloss(const fmgi_geometry *geo, const fmgi_camera *cams, int num_cams, int width,
                                 int height, int projection, int samples, int filter, fmgi_view_cache **out);
/* fmgi_view_cache_shade with the mirror bounce: rgb_dev[k] = fmgi_shade_views_gloss' rgb_out for tiles_dev[k] and
   this gloss, from one trace for every lightmap and every gloss. gloss == 0 (and fmgi_view_cache_shade on such a
   view) is the plain picture. Errors: fmgi_view_cache_shade's, then a gloss outside [0, 1] or NaN (FMGI_ERR_ARG),
   then gloss > 0 on a view without mirror records (FMGI_ERR_STATE), all before any device call. */
int fmgi_view_cache_shade_gloss(const fmgi_view_cache *vc, const void *const *tiles_dev, int num_sets,
                                const uint8_t background[3], float gloss, void *const *rgb_dev, void *coverage_dev,
                                void *stream);
/* 1 if the traced view holds mirror records, 0 if not, FMGI_ERR_ARG for a NULL handle */
int fmgi_view_cache_has_mirror(const fmgi_view_cache *vc);

/* ---- Build-defined device-resident API ---------------------------------------------------------- */
enum {
    FMGI_OK = 0,
    FMGI_ERR_NO_DEVICE = -1,
    FMGI_ERR_HIP = -2,
    FMGI_ERR_ARG = -3,
    FMGI_ERR_STATE = -4,
    FMGI_ERR_OOM = -5
};

/* Scan kernels (identical bits): EXACT = photonmap.cl's scan over every rect; FAST = conservative fp32
   filter over every rect + exact verification; GRID = FAST's filter over per-plane grid cells only;
   HYBRID = GRID's cells for the floor/ceiling planes and FAST's filter for the walls. */
enum { FMGI_KERNEL_EXACT = 0, FMGI_KERNEL_FAST = 1, FMGI_KERNEL_GRID = 2, FMGI_KERNEL_AUTO = 3, FMGI_KERNEL_HYBRID = 4 };
/* AUTO = GRID when the scene has few planes for its rect count (closed boxes), HYBRID when only the
   floor/ceiling records share few planes (apartment layouts), else FAST; a scan whose image does not
   fit LDS falls back to one that does (EXACT needs none). */
/* Deposit accumulation (both exact and order-free; results are identical):
   FX3   three int64 fixed-point atomics per deposit into the lightmap;
   STATE one u64 atomic per deposit into counts[colour state][texel] (8 KiB per texel of device memory),
         folded into the int64 lightmap at the end of every fmgi_bake_items;
   STREAM no atomics per deposit: 32-bit codes (texel << 10 | colour state) collected in each wave's LDS
         ring and written with 16-B stores (when the lightmap has at most 63 fold tiles of 2048 texels,
         sorted by tile into per-wave, per-tile 4-KB buckets; else into plain blocks that a second pass
         sorts per 8192-code slice), then summed per tile exactly in LDS (needs < 4,194,304 texels; the
         codes of a chunk of work items stay in HBM, 3.2 KB per work item at most, chunks sized to half
         of the free device memory: one 1e9-photon chunk on an MI355X);
   AUTO  STREAM when the texel count allows it, else FX3;
   NONE  PROFILING ONLY: deposits are discarded (measures the tracing work alone; wrong lightmap). */
enum { FMGI_ACCUM_AUTO = 0, FMGI_ACCUM_FX3 = 1, FMGI_ACCUM_STATE = 2, FMGI_ACCUM_NONE = 3, FMGI_ACCUM_STREAM = 4 };

/* Per-bake counters, accumulated on the device (one atomic per wave). */
typedef struct fmgi_stats {
    uint64_t photons;   /* tracePhoton calls                                     */
    uint64_t scans;     /* rectangle-list scans (photonmap.cl:194)                */
    uint64_t deposits;  /* lightmap deposits (photonmap.cl:257)                   */
    uint64_t escapes;   /* scans that hit nothing (photonmap.cl:208)              */
    uint64_t exact_rescans; /* fast kernel: scans re-done by the exact scan          */
    uint64_t tests;     /* rectangle tests actually evaluated                      */
    uint64_t rescans_tie;     /* exact_rescans caused by a runner-up within the separation band */
    uint64_t rescans_invalid; /* exact_rescans caused by a phase-1 winner that is not exactly valid */
    uint64_t stream_overflow; /* STREAM: reservations past the stream capacity (must stay 0) */
    uint64_t bucket_fallback_codes; /* STREAM, per-workgroup tile blocks: codes added to the lightmap with
                                       device atomics instead of being stored (exact; 0 unless a workgroup
                                       hits one tile much harder than a block per pool atomic, or the pool
                                       is exhausted) */
} fmgi_stats;

/* One work item of the flattened reference launch schedule (global_illumination_cl.c:246-267). */
typedef struct fmgi_launch {
    uint64_t item_begin; /* flattened index of this launch's gid 0 */
    uint32_t count;      /* workSize                               */
    int32_t rng_offset;  /* rand() value (kernel arg 4)             */
    int32_t source;      /* windows first, then lights              */
    int32_t is_window;   /* kernel arg 5                            */
} fmgi_launch;

/* One recorded bounce (debug trace mode, for per-photon parity tests). */
typedef struct fmgi_event {
    int32_t photon, depth, rect, texel;
    float rgb[3];
    uint32_t rng;
} fmgi_event;

typedef struct fmgi_context fmgi_context;

const char *fmgi_version(void);
const char *fmgi_last_error(void);
int fmgi_device_count(void);

/* Create a context on HIP device `device` (hipSetDevice is called). NULL on failure.
   device == FMGI_HOST_ONLY gives a context without a device: scene checks and fmgi_plan work, every
   device operation returns FMGI_ERR_NO_DEVICE (used by the CPU test-suite). */
#define FMGI_HOST_ONLY (-1)
fmgi_context *fmgi_create(int device);
void fmgi_destroy(fmgi_context *ctx);

/* Upload the scene: wall rectangles (the rect list scanned by every photon) and the emitters
   (windows first, then lights). The per-rectangle values photonmap.cl derives with OpenCL builtins
   (edge lengths, unit edges, sampler bases) are computed on the device by k_scene_setup with the
   builtins' gfx950 instructions, so they carry the reference kernel's bits; the scan tables (filter
   image, grid) are built on the host. */
int fmgi_set_scene(fmgi_context *ctx, const fmgi_rect *walls, int num_walls, const fmgi_rect *windows,
                   int num_windows, const fmgi_rect *lights, int num_lights, int num_texels);

/* Select the accumulation mode (FMGI_ACCUM_*); takes effect for the current and later scenes. */
int fmgi_set_accumulation(fmgi_context *ctx, int mode);
/* The mode in effect (FMGI_ACCUM_FX3, FMGI_ACCUM_STATE, FMGI_ACCUM_STREAM or FMGI_ACCUM_NONE). */
int fmgi_get_accumulation(fmgi_context *ctx);

/* Reference launch schedule for spa / wg. If rng_offsets is NULL, libc rand() is called once per
   launch in reference order; otherwise offsets are taken from rng_offsets[0..n_offsets).
   Returns the number of launches (>=0) or an error code; *total_items receives the work-item count
   (photons = 100 * items). The schedule is kept in the context for fmgi_bake_items. */
int64_t fmgi_plan(fmgi_context *ctx, int spa, int wg, const int32_t *rng_offsets, int64_t n_offsets,
                  uint64_t *total_items);
/* Copy the current schedule out (cap entries). Returns the number of launches. */
int64_t fmgi_get_plan(fmgi_context *ctx, fmgi_launch *out, int64_t cap);
/* Schedule helpers that do not call rand(). */
int64_t fmgi_plan_count(const fmgi_rect *windows, int num_windows, const fmgi_rect *lights, int num_lights,
                        int spa, int wg, uint64_t *total_items);

/* Trace flattened work items [item_begin, item_end) of the planned schedule on `stream`, adding
   exact fixed-point deposits (int64, units of 2^-25, layout [numTexels][4], .s[3] unused) into the
   device buffer lm_fx. Asynchronous; the buffer must be zeroed (or hold a previous partial sum). */
int fmgi_bake_items(fmgi_context *ctx, uint64_t item_begin, uint64_t item_end, void *lm_fx_dev,
                    int kernel, void *stream);
/* Device-side finalisation: texels_out[i].c = (float)((double)texels_in[i].c + lm_fx[i].c * 2^-25),
   .s[3] copied. Either texel pointer may alias. */
int fmgi_finalize(fmgi_context *ctx, const void *lm_fx_dev, const void *texels_in_dev, void *texels_out_dev,
                  void *stream);
/* ---- Recolouring a bake: per-state photon histograms ------------------------------ */
/* A photon's path never depends on its colour, and the colour it deposits is a pure function of its 10-bit
   colour state: bit 9 = the source kind (1: window, 0: light); below the leading 1 of bits 0-8, one bit per
   diffuse bounce, oldest first, set when that bounce was on the floor. fmgi_bake_states keeps the bake's
   deposit counts per (state, texel); fmgi_recolour folds such histograms with the tables of any palettes.
   The int64 lightmap is then what fmgi_bake_items would give had photonmap.cl's constants been the
   palette's, bit for bit; histograms of disjoint item ranges (one lamp, all windows, ...) add up to the whole
   bake, so every group of sources takes its own palette (dimmed, switched off) per scenario. */
#define FMGI_COLOUR_STATE_COUNT 1024
#define FMGI_RECOLOUR_MAX_SCENARIOS 8 /* scenarios one kernel pass carries; fmgi_recolour takes any number */
typedef struct fmgi_palette {          /* photonmap.cl:167-169, 241-249 */
    float window_rgb[3], light_rgb[3]; /* 18,18,18 / 16,16,18 */
    float floor_tint[3];               /* 1, 0.85, 0.7 */
    float albedo;                      /* 0.9 */
} fmgi_palette;
/* photonmap.cl's constants */
void fmgi_palette_reference(fmgi_palette *p);
/* Host only: the deposit of every colour state in fixed point (units of 2^-25). Per state the kernel's float
   operations in the kernel's order: start from the kind's colour; for every diffuse-bounce bit from the top,
   multiply the three channels by floor_tint if the bit is set, then by albedo; each channel is then
   (int64)ldexp(c, 25) (this truncation defines a deposit under a palette). Rows 0 and 512 (no leading 1) are
   zero. FMGI_ERR_ARG unless every component is finite, 0 <= window_rgb, light_rgb < 32, 0 <= floor_tint <= 1
   and 0 <= albedo <= 1; every value then lies in [0, 2^30). */
int fmgi_palette_table(const fmgi_palette *p, int64_t table[FMGI_COLOUR_STATE_COUNT][3]);
/* Bytes of one histogram, uint64 [FMGI_COLOUR_STATE_COUNT][num_texels]: 8 KiB per texel (0 if num_texels < 1). */
size_t fmgi_states_bytes(int num_texels);
/* fmgi_bake_items' trace of work items [item_begin, item_end), counting every deposit in the caller's device
   histogram counts_dev[state][texel] (fmgi_states_bytes(numTexels) bytes) with one 64-bit device atomic each.
   Nothing is folded or zeroed: counts add to what the buffer holds, so several ranges or calls accumulate.
   Works whatever fmgi_set_accumulation selected, and leaves that mode as it is. Asynchronous on `stream`. */
int fmgi_bake_states(fmgi_context *ctx, uint64_t item_begin, uint64_t item_end, void *counts_dev, int kernel,
                     void *stream);
/* For every scenario k and texel t:
     lm_fx[k][t][c] += sum over groups g and states s of counts[g][s][t] * table(palettes[k * num_groups + g])[s][c]
   in exact 64-bit integers (mod 2^64). counts_dev[num_groups] = device histograms of the current scene's texel
   count (read only); lm_fx_dev[num_scenarios] = distinct device lightmaps (int64 [numTexels][4]; .s[3] is not
   touched). Asynchronous on `stream`; the palettes are read before the call returns. The tables are built and
   every argument is checked on the host before any device call: FMGI_ERR_ARG for num_groups < 1,
   num_scenarios < 1, a NULL pointer or a palette fmgi_palette_table rejects, FMGI_ERR_STATE without a scene,
   then FMGI_ERR_NO_DEVICE on a host-only context. A group whose table is zero in every scenario of a pass (a
   lamp switched off) is not read. */
int fmgi_recolour(fmgi_context *ctx, const void *const *counts_dev, int num_groups, const fmgi_palette *palettes,
                  int num_scenarios, void *const *lm_fx_dev, void *stream);

/* ---- Sparse photon histograms: compact, recolour, expand, check --------------------- */
/* The sparse, blocked form of one histogram. T = numTexels, B = (T + 63) / 64 blocks of 64 consecutive texels.
   One blob of uint64 words (this layout is what files hold):
     off[B + 1]        off[0] = 0; off[b + 1] - off[b] = r_b, the largest number of non-zero states any texel of
                       block b has; rows = off[B]
     entry[64 * rows]  slot j (0 <= j < r_b) of texel t = 64 b + l is entry[(off[b] + j) * 64 + l] and holds
                       (state << 54) | count for the texel's j-th non-zero state in ascending state order, or 0
                       (padding) when the texel has fewer than j + 1 non-zero states or t >= T
   so a wave reading row off[b] + j reads 512 contiguous bytes; 8 (B + 1) + 512 rows bytes in all. Counts must be
   below 2^54. The form is canonical: a histogram has exactly one blob, bit for bit. */
#define FMGI_SPARSE_COUNT_BITS 54
typedef struct fmgi_sparse_info {
    int32_t num_texels, num_blocks;   /* num_blocks == (num_texels + 63) / 64 */
    uint64_t rows;                    /* off[num_blocks] */
    uint64_t cells;                   /* non-zero (state, texel) cells */
    uint64_t deposits;                /* sum of the counts mod 2^64 */
    uint64_t too_large;               /* cells whose count is >= 2^54 */
} fmgi_sparse_info;
/* Host only: bytes of a blob of num_texels texels and `rows` rows (0 if num_texels < 1). */
size_t fmgi_sparse_bytes(int num_texels, uint64_t rows);
/* The device calls below check their arguments on the host before any device call, in this order: FMGI_ERR_ARG
   for a NULL context or pointer (and num_groups < 1, num_scenarios < 1, a rejected palette), or an info with
   num_blocks != (num_texels + 63) / 64 or too_large != 0; FMGI_ERR_STATE without a scene; FMGI_ERR_ARG if
   info.num_texels is not the scene's texel count; FMGI_ERR_NO_DEVICE on a host-only context. Every kernel that
   reads a blob takes info.rows from the host, clamps each block's [off[b], off[b + 1]) to [0, rows] and skips a
   block whose begin exceeds its end; the state field has 10 bits. So a device blob of
   fmgi_sparse_bytes(T, info.rows) bytes cannot cause an access out of bounds, whatever it holds. */
/* One pass over the dense histogram counts_dev of the current scene's texel count: synchronises `stream` and
   fills *info. FMGI_ERR_ARG, with *info still filled, if too_large != 0. */
int fmgi_sparse_measure(fmgi_context *ctx, const void *counts_dev, fmgi_sparse_info *info, void *stream);
/* Writes the histogram's blob, fmgi_sparse_bytes(T, info->rows) bytes, to sparse_dev. Asynchronous. The offsets
   are recomputed (count, scan, fill; nothing of fmgi_sparse_measure is kept in the context) and clamped to
   info->rows, and a lane never writes outside its block's clamped rows: if the histogram changed since it was
   measured the blob is unspecified, but no byte outside the buffer is written. */
int fmgi_sparse_compact(fmgi_context *ctx, const void *counts_dev, const fmgi_sparse_info *info, void *sparse_dev,
                        void *stream);
/* counts_dev[state][t] += count for every non-padding entry, each texel's rows in order (no atomics; defined
   for duplicate entries too): expanding a compacted histogram into zeros gives the histogram. Asynchronous. */
int fmgi_sparse_expand(fmgi_context *ctx, const void *sparse_dev, const fmgi_sparse_info *info, void *counts_dev,
                       void *stream);
/* fmgi_recolour on blobs: lm_fx[k][t][c] += sum over groups g and g's entries of texel t of
   count * table(palettes[k * num_groups + g])[state][c], in exact 64-bit integers mod 2^64; .s[3] is not
   touched. sparse_dev[num_groups] with infos[num_groups]; any number of scenarios, in passes of
   FMGI_RECOLOUR_MAX_SCENARIOS; a group whose table is zero in a whole pass is not read. A wave owns its 64
   texels and adds without atomics: the groups are launches of one stream, and nothing else may add to the
   lightmaps meanwhile. Asynchronous; the palettes are read before the call returns. */
int fmgi_recolour_sparse(fmgi_context *ctx, const void *const *sparse_dev, const fmgi_sparse_info *infos,
                         int num_groups, const fmgi_palette *palettes, int num_scenarios, void *const *lm_fx_dev,
                         void *stream);
/* Host only: validates a host copy of a blob (what a loader calls before uploading) and fills *info. Checks that
   bytes covers off[], off[0] == 0, off[] does not decrease, bytes == fmgi_sparse_bytes(num_texels, off[B]); per
   texel that non-zero entries have strictly ascending state, padding comes only after them and lanes t >= T are
   all padding; and that every block has a texel that uses all its rows. FMGI_ERR_ARG otherwise, with
   fmgi_last_error naming the first violation. info->too_large is 0 (a count field cannot hold more). */
int fmgi_sparse_check(const void *sparse_host, size_t bytes, int num_texels, fmgi_sparse_info *info);

/* ---- Sparse histograms from the bake's deposit codes, and the sum of two blobs ------- */
/* A deposit code of the STREAM bake is texel << 10 | state: the key of a sparse cell. The calls below count codes
   into a sparse histogram without ever holding the dense uint64 [1024][T] form, and add two blobs cell by cell.
   Argument checks run on the host before any device call, in the order of the sparse calls above: FMGI_ERR_ARG
   (NULL context or pointer, an info with a wrong num_blocks or too_large != 0, item_begin > item_end);
   FMGI_ERR_STATE (no scene; for the bake also no plan), then for the bake a range past the plan as
   fmgi_bake_states reports it (FMGI_ERR_ARG); FMGI_ERR_ARG (an info whose
   num_texels is not the scene's); FMGI_ERR_STATE where fmgi_bake_sparse_supported is 0 (the two calls that count
   codes); FMGI_ERR_NO_DEVICE on a host-only context. fmgi_set_scene and fmgi_destroy release a held result. */
/* 1 if fmgi_bake_sparse / fmgi_sparse_from_codes can serve the current scene (its STREAM layout is the per-tile
   bucket layout: at most 63 tiles of 2048 texels, and FMGI_OPT_STREAM_LAYOUT does not force the sliced layout),
   0 if not, FMGI_ERR_ARG / FMGI_ERR_STATE for a NULL context / no scene. Host only. */
int fmgi_bake_sparse_supported(const fmgi_context *ctx);
/* fmgi_bake_items' trace of work items [item_begin, item_end) through the STREAM bucket path, whatever
   fmgi_set_accumulation selected (left as it is), with the deposit codes counted into the sparse histogram of
   exactly these items. The result is held in the context, replacing one held before; *info describes it.
   Synchronises `stream`. item_begin == item_end gives the empty histogram (rows 0). A chunk of the bake whose
   bucket fallback fired (fmgi_stats.bucket_fallback_codes moved: those deposits went to a lightmap and lost
   their state), or that holds 2^32 codes or more of one 32-texel half-block, is traced again through
   fmgi_bake_states' route into a dense scratch that lives for that chunk only (FMGI_ERR_OOM, nothing held, if it
   cannot be allocated); the result and the context's fmgi_stats are the same either way. */
int fmgi_bake_sparse(fmgi_context *ctx, uint64_t item_begin, uint64_t item_end, int kernel,
                     fmgi_sparse_info *info, void *stream);
/* Writes the held histogram's canonical blob, fmgi_sparse_bytes(T, info->rows) bytes, to sparse_dev and releases
   it. FMGI_ERR_STATE if nothing is held; FMGI_ERR_ARG if info->rows / num_texels are not the held ones. Async. */
int fmgi_bake_sparse_take(fmgi_context *ctx, const fmgi_sparse_info *info, void *sparse_dev, void *stream);
/* The histogram of n device codes (texel << 10 | state, any order) as a held result like fmgi_bake_sparse's. A code
   equal to 0xFFFFFFFF, or whose texel is >= numTexels, is skipped; *skipped (may be NULL) receives how many of the
   latter. n < 2^32. Synchronises. */
int fmgi_sparse_from_codes(fmgi_context *ctx, const void *codes_dev, uint64_t n, fmgi_sparse_info *info,
                           uint64_t *skipped, void *stream);
/* sum = a + b, cell by cell (counts add; a cell of either is a cell of the sum), in canonical form.
   _measure synchronises and fills *sum_info (FMGI_ERR_ARG with the info filled if a summed count reaches 2^54);
   fmgi_sparse_add writes fmgi_sparse_bytes(T, sum_info->rows) bytes, asynchronous, offsets recomputed and
   clamped to sum_info->rows as fmgi_sparse_compact does. sum_dev must not alias a_dev or b_dev. */
int fmgi_sparse_add_measure(fmgi_context *ctx, const void *a_dev, const fmgi_sparse_info *a_info, const void *b_dev,
                            const fmgi_sparse_info *b_info, fmgi_sparse_info *sum_info, void *stream);
int fmgi_sparse_add(fmgi_context *ctx, const void *a_dev, const fmgi_sparse_info *a_info, const void *b_dev,
                    const fmgi_sparse_info *b_info, const fmgi_sparse_info *sum_info, void *sum_dev, void *stream);
typedef struct fmgi_bake_sparse_stats {  /* of the last fmgi_bake_sparse / fmgi_sparse_from_codes of the context */
    uint64_t chunks, merges;             /* bake chunks counted; blob sums that joined them                      */
    uint64_t dense_chunks;               /* chunks that took the dense fallback (above); 0 on a healthy run      */
    uint64_t codes;                      /* codes counted from the pool (== info.deposits when dense_chunks == 0) */
    uint64_t scratch_bytes;              /* device bytes this path held at its peak, the stream pool excluded    */
} fmgi_bake_sparse_stats;
int fmgi_bake_sparse_get_stats(const fmgi_context *ctx, fmgi_bake_sparse_stats *out);

/* ---- Adaptive density filter for noisy, low-photon lightmaps ------------------------ */
/* A radiance estimate on the binned photons: per level-0 texel a square window, grown until it holds enough
   deposit energy and clipped to the texel's own wall, then the mean over that window. No reference counterpart.
   All values are unsigned 64-bit integers mod 2^64, so the result is exact and independent of any order.
   Wall w's level-0 grid is texel (x, y) = s0 + y * s1 + x, 0 <= x < s1, 0 <= y < s2 (lightmapSetup = {s0, s1,
   s2, 0}); W_r(x, y) = [max(x - r, 0), min(x + r, s1 - 1)] x [max(y - r, 0), min(y + r, s2 - 1)] holds n_r texels.
   It is a box estimate: it smooths across shadow edges inside a wall and never across walls. Level-0 ranges of
   different walls that overlap give unspecified results. */
#define FMGI_FILTER_MAX_RADIUS 16
#define FMGI_FILTER_MAX_MAPS 8   /* maps one kernel pass carries; the call takes any number */
/* deposits x the fixed-point sum of the palette's window colour (NULL: the reference's 18,18,18): the
   min_energy that stands for `deposits` first-bounce window photons. Host only. 0 (and fmgi_last_error) for a
   palette fmgi_palette_table rejects. */
uint64_t fmgi_filter_energy(const fmgi_palette *p, uint64_t deposits);
/* radii[t] = the smallest r in [0, max_radius] whose window holds S_r >= min_energy (compared unsigned), S_r the
   sum over W_r of e = g[.][0] + g[.][1] + g[.][2] of the guide lightmap g (int64 [numTexels][4]); max_radius if
   there is none; 0 for texels in no wall's level-0 grid (the mip levels). radii_dev: uint8 [numTexels]. */
int fmgi_filter_radii(fmgi_context *ctx, const void *guide_lm_fx_dev, uint64_t min_energy, int max_radius,
                      void *radii_dev /* uint8 [numTexels] */, void *stream);
/* For every map k and level-0 texel t, with r = min(radii[t], 16): out[k][t][c] = (sum of in[k][.][c] over W_r) /
   n_r (unsigned division) for c = 0..2 and out[k][t][3] = in[k][t][3]; every other texel is copied, all four
   words. A window sum below 2^64 comes out exact whatever the lightmap's total. lm_out_dev[k] may be
   lm_in_dev[k]; the maps must not overlap in any other way. radii of one guide serve any number of maps (all
   scenarios of a relight session share the radii of the reference-palette lightmap of all sources); radii all 0
   give out == in.
   Both calls take device pointers of the current scene's texel count and are asynchronous on `stream`. Arguments
   are checked on the host before any device call: FMGI_ERR_ARG for a NULL context or pointer, num_maps < 1 or
   max_radius outside 0..FMGI_FILTER_MAX_RADIUS, then FMGI_ERR_STATE without a scene, then FMGI_ERR_NO_DEVICE on a
   host-only context. The prefix sums the kernels work on live in scratch memory of the context (8 B per texel
   for the radii, 24 B per texel and map of a pass), allocated on first use; a later call's stream waits for the
   earlier call before it reuses them, without blocking the host. */
int fmgi_filter_apply(fmgi_context *ctx, const void *radii_dev, const void *const *lm_in_dev,
                      void *const *lm_out_dev, int num_maps, void *stream);

/* ---- Direct sunlight through windows: a relightable lightmap layer ------------------ */
/* The bake treats a window as a diffuse patch of sky. The sun is a direction: its light on a flat rectangle is
   colour x cosine x the fraction of each texel that sees the sun through a window, and that fraction is a count of
   sub-texel shadow rays. It needs no photons, has no noise and does not depend on the bake: one coverage map per
   sun direction serves every colour and scenario, and fmgi_sun_add drops it into the int64 lightmap that
   fmgi_recolour, fmgi_filter_apply, fmgi_finalize and the traced views pass around. No reference counterpart; the
   semantics below are the interface.

   All arithmetic is IEEE fp32 without contraction, in the order written. dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
   intersects(r, src, dir, closest) is rectangle.c:67-95 (the hit distance, or -1), on a rectangle's unit edges and
   lengths precomputed with the operations the AO, radiosity and view paths use (width * (1 / |width|), |v| =
   sqrtf((x*x + y*y) + z*z)).
     Sun vector   to_sun[3] points from the scene to the sun, any non-zero finite length:
                  l = sqrtf((x*x + y*y) + z*z), s = (x/l, y/l, z/l).
     Facing       c_w = dot(n_w, s); wall w receives sun only if c_w > 0.
     Samples      the level-0 texel (tx, ty) of wall w (lightmapSetup = {s0, s1, s2, 0}, index s0 + ty*s1 + tx) has
                  S x S samples (i, j): a = ((float)tx + (float)(2i+1) / (float)(2S)) / (float)s1, b likewise from
                  ty, j, s2; P = (pos + width*a) + height*b per component; Q = P + s*1e-5f.
     Crossing     d_v = intersects(window v, Q, s, +INFINITY), the window as the scene holds it: its normal points
                  into the room and the ray towards the sun runs against it, which is the side intersects' first
                  line lets through. dw = the smallest d_v that is not -1; a sample with no crossing is not lit.
                  Lights are not windows.
     Occlusion    the sample is blocked if any wall i of the scene gives intersects(wall_i, Q, s, dw) != -1. Any-hit:
                  the result depends neither on the order nor on which walls are skipped, as long as a skipped wall
                  could not have hit. A wall behind the window's plane fails intersects' own distance test.
     Coverage     cover[t], a uint8, is the number of lit samples of texel t, 0..S*S; 0 for every texel in no facing
                  wall's level-0 grid (the mip levels too). The call writes all numTexels bytes.
     Energy       the sun is `flux` photons per m^2 perpendicular to s, each carrying rgb in the palette's units
                  (window_rgb is 18); flux is the bake's numSamplesPerArea. For a facing wall, in doubles, multiplied
                  left to right: unit[w][c] = (int64)floor(ldexp((double)rgb[c] * (double)c_w * flux * area_t, 25)),
                  area_t = ((double)|width| * (double)|height|) / (double)(s1*s2) with the fp32 lengths above.
                  lm_fx[t][c] += (cover[t] * unit[w][c] + S*S/2) / (S*S) in integers; lm_fx[t][3] is not touched.
                  After fmgi_finalize and main.c:68-79's normalisation with the same numSamplesPerArea a fully lit
                  texel gains 0.35 * rgb[c] * c_w.
   Out of scope: a penumbra, sun entering other than through a window rectangle. The sun's bounced light is the
   next section's.

   All calls use the scene of fmgi_set_scene (walls and windows). fmgi_sun_coverage and fmgi_sun_add are
   asynchronous on `stream`; to_sun and rgb are read before the call returns. FMGI_SUN_ALL tests every wall with
   dot(n_i, s) < 0 (the others return -1 by intersects' first line); FMGI_SUN_LISTS, the product path, tests per
   window only the walls of a conservative occluder list and gives the same bytes and the same four
   counts. Arguments are checked on the host before any device call, in this order: FMGI_ERR_ARG for a NULL context
   or pointer, samples outside 1..FMGI_SUN_MAX_SAMPLES, a mode that is neither of the two, a to_sun of zero or
   non-finite length, num_maps < 1, an rgb component that is not finite or outside [0, 32), a flux that is not
   finite or <= 0; FMGI_ERR_STATE without a scene; FMGI_ERR_ARG if a unit reaches 2^55 (its product with a count
   of at most 64 then stays below 2^62); FMGI_ERR_NO_DEVICE on a host-only context. A scene without windows and a
   direction no wall faces give an all-zero map and success. The calls' tables, lists and counters live in scratch
   memory of the context; a later call's stream waits for the earlier call, the host does not. */
#define FMGI_SUN_MAX_SAMPLES 8
#define FMGI_SUN_MAX_MAPS 8            /* maps one pass of fmgi_sun_add carries; the call takes any number */
enum { FMGI_SUN_LISTS = 0, FMGI_SUN_ALL = 1 };
struct fmgi_sun_stats {                 /* of the context's last fmgi_sun_coverage; get synchronises */
    int64_t samples, facing, crossing, lit;   /* samples of all level-0 texels, of the facing walls' texels, those that
                                                 cross a window, those that are lit; order-independent */
    int64_t list_entries, tests;              /* informational: occluder-list lengths summed, intersects() run */
    double list_ms, rays_ms;                  /* device time of the list kernel and of the ray kernel */
};
int fmgi_sun_coverage(fmgi_context *ctx, const float to_sun[3], int samples, int mode,
                      void *cover_dev /* uint8 [numTexels] */, void *stream);
int fmgi_sun_get_stats(fmgi_context *ctx, struct fmgi_sun_stats *out);
/* lm_fx_dev[k] += the deposits of cover_dev (made with the same to_sun and samples) under rgb[k], in place */
int fmgi_sun_add(fmgi_context *ctx, const void *cover_dev, const float to_sun[3], int samples,
                 const float *rgb /* [num_maps][3] */, int num_maps, double flux,
                 void *const *lm_fx_dev, void *stream);
/* host only, works on FMGI_HOST_ONLY contexts: units[numWalls][3], zero rows for walls that do not face */
int fmgi_sun_units(fmgi_context *ctx, const float to_sun[3], const float rgb[3], double flux, int64_t *units);

/* ---- Bounced sunlight: coverage maps gathered through the radiosity cache ------------ */
/* fmgi_sun_add's light stops where it lands. A radiosity cache (above) holds, for every level-0 wall texel (a job),
   the texel each of its 10000 cosine-distributed rays hits, whatever the lighting. A coverage map is a byte per
   texel and a wall's cosine a constant, so the sun's radiosity on a texel is rgb x e[t] with a scalar e, and with one
   reflectance per channel bounce n is rgb[c] x refl[c]^n x g_n[t]: g_n depends on the geometry and the sun's
   direction only. fmgi_rad_cache_sun_bounce computes g_1 .. g_N per direction; fmgi_sun_add_bounced adds them under
   any colour and reflectance to the int64 lightmap. No reference counterpart; the semantics below are the interface.

   fp32 arithmetic is IEEE without contraction, in the order written; s, c_w and dot are the previous section's.
     Start table  for direction k with coverage map cover_k made with S_k samples per texel edge, and a level-0 texel
                  t of a wall w with c_w > 0: e_0[t] = ((float)cover_k[t] * c_w) / (float)(S_k*S_k). Every other entry
                  of the cache's texel table is +0: walls that do not face the sun, mip levels, the window and light
                  texels behind numTexels. A byte above S*S is used as it is (the caller's error, no memory hazard).
                  c_w comes from the cache's own wall rectangles: bit for bit fmgi_sun_units' cosine.
     Gather       for n = 1..N and job j with texel t_j: sum = +0; for ray r = 0..9999 in order, id = sids[j][r], if
                  0 <= id < numTexels then sum = sum + e_{n-1}[id]; g_n[t_j] = sum / 10000.0f. g_n is +0 at every
                  texel that is no job's, and e_n = g_n. Rays that miss (-1) and rays that hit a window or a light add
                  nothing. There is no mip step and no 0.7 / 0.3 update: a Neumann series, not the reference's
                  iteration.
     Output       per direction a device float [N][numTexels] holding rows g_1 .. g_N; the call writes all of it. A
                  direction's result depends neither on the other directions of the call nor on their number.
     Adding       for map m with rgb_m[3] and refl_m[3], a level-0 texel t of wall w (every wall, facing or not) and
                  channel c, in doubles: p_1 = (double)refl[c], p_n = p_{n-1} * (double)refl[c]; v = 0, then
                  v = v + (double)g_n[t] * p_n for n = 1..N in order;
                  q = (int64)floor(ldexp((((double)rgb[c] * v) * flux) * area_t, 25)) with the previous section's
                  area_t; lm_fx[t][c] += q. Word 3 and the mip texels are not touched; a texel whose N values are all
                  zero is not written. flux is the bake's numSamplesPerArea, as in fmgi_sun_add.

   fmgi_rad_cache_sun_bounce draws nothing from libc. It is asynchronous on `stream`, like fmgi_rad_cache_solve: the
   host arrays are read before it returns; its scratch belongs to the handle and is guarded by the handle's event (a
   later call's stream waits, the host does not, unless the scratch has to grow); more than
   FMGI_SUN_BOUNCE_MAX_DIRS directions run in further passes. Errors, found on the host before any device call:
   FMGI_ERR_ARG for a NULL handle or pointer, num_dirs < 1, bounces outside 1..FMGI_SUN_MAX_BOUNCES, a samples[k]
   outside 1..FMGI_SUN_MAX_SAMPLES, a to_sun of zero or non-finite length; then FMGI_ERR_NO_DEVICE.

   fmgi_sun_add_bounced uses the context's scene, as fmgi_sun_add does; it is asynchronous, carries up to
   FMGI_SUN_MAX_MAPS maps per pass and takes any number. Errors, in the previous section's order: FMGI_ERR_ARG for a
   NULL context or pointer, bounces out of range, num_maps < 1, an rgb component outside [0, 32) or not finite, a refl
   component outside [0, 1] or not finite, a flux not finite or <= 0; FMGI_ERR_STATE without a scene; FMGI_ERR_ARG if
   32 * bounces * 1.001 * flux * max area_t * 2^25 reaches 2^55 (g_n <= 1 up to rounding, since e_0 <= 1 and a gather
   averages: no deposit then reaches 2^55); FMGI_ERR_NO_DEVICE on a host-only context.
   Out of scope: per-wall reflectance, the floor's tint and mirror, sky or lamp light through this path. */
#define FMGI_SUN_BOUNCE_MAX_DIRS 32     /* directions one gather pass carries; the call takes any number */
#define FMGI_SUN_MAX_BOUNCES 8
int fmgi_rad_cache_sun_bounce(const fmgi_rad_cache *rc, void *const *cover_dev /* [num_dirs] uint8 [numTexels] */,
                              const float *to_sun /* [num_dirs][3] */, const int *samples /* [num_dirs] */,
                              int num_dirs, int bounces, void *const *bounce_dev /* [num_dirs] float [bounces][numTexels] */,
                              void *stream);
int fmgi_sun_add_bounced(fmgi_context *ctx, const void *bounce_dev, int bounces,
                         const float *rgb /* [num_maps][3] */, const float *refl /* [num_maps][3] */, int num_maps,
                         double flux, void *const *lm_fx_dev, void *stream);

/* The kernel FMGI_KERNEL_AUTO resolves to for the current scene. */
int fmgi_auto_kernel(const fmgi_context *ctx);
/* The profiler's name of the k_bake instance the last bake launch ran ("void (anonymous namespace)::k_bake<...>
   (BakeArgs)"; two names joined by " + " for the launch-tail pair), written NUL-terminated into buf (truncated
   to cap - 1 characters); returns its full length, 0 before the first bake. No reference counterpart: the
   measurement's handle on which instance the committed counter summaries must name. */
int fmgi_last_bake_kernel(const fmgi_context *ctx, char *buf, int cap);
/* Device-side timing of the bake's kernels (HIP events around each launch, on the bake's stream), off
   by default. fmgi_get_timing synchronises, returns the sums since the previous call and resets them. */
typedef struct {
    double bake_ms;         /* k_bake launches                                   */
    double fold_ms;         /* STREAM fold (k_bucket_count/list/fold, k_tile_runs_pre, or k_slice_sort +
                               k_tile_runs / k_tile_runs_pre over slices) */
    uint64_t bake_launches;
    uint64_t fold_launches;
} fmgi_timing;
int fmgi_set_timing(fmgi_context *ctx, int on);
int fmgi_get_timing(fmgi_context *ctx, fmgi_timing *out);
/* Counters of all bakes since the last reset (synchronises the context's device). */
int fmgi_get_stats(fmgi_context *ctx, fmgi_stats *out);
int fmgi_reset_stats(fmgi_context *ctx);
/* Debug trace: runs items [item_begin, item_end) (<= 4096 items) with the chosen kernel and returns
   every bounce in events[(item - item_begin) * 800 + k] (800 = 100 photons x 8 bounces), the number
   of events per item in counts[], and the final per-item RNG state in rng_final[]. Synchronous. */
int fmgi_trace_items(fmgi_context *ctx, uint64_t item_begin, uint64_t item_end, int kernel,
                     fmgi_event *events, int32_t *counts, uint32_t *rng_final);

/* Grid tables of FMGI_KERNEL_GRID (built by fmgi_set_scene; host-only contexts too), for tests and
   tooling. sizes[0..2] = plane pairs per axis (x, y, z), sizes[3] = cells, sizes[4] = overflow entries.
   fmgi_grid_copy fills (any pointer may be NULL):
     planes[2 * (sizes[0] + sizes[1] + sizes[2])]: per axis, pairs {plane of the +n class, plane of the
       -n class}, each {float plane, u0, v0, iu, iv, mu, mv; int32 nu, nv, cell_off; float ulo, uhi,
       vlo, vhi (the records' box, rounded outward), pad[2]} (64 B; mu = nu - 1, mv = nv - 1; NaN
       plane = padding);
     cells[sizes[3]] (32 B each): the cell's first two records as quantized bounds {uint32 qu, qv} each
       ({lo | hi << 16} of the cell's 16-bit fixed-point coordinates that the record's margin-grown
       extent can reach; {0xFFFF, 0xFFFF} when absent), then {int32 count, rect index of record 0, of
       record 1, first overflow entry};
     recs[4 * sizes[4]], idx[sizes[4]]: the overflow records (entries 3..count of every cell) and their
       rect indices. */
int fmgi_grid_sizes(const fmgi_context *ctx, int32_t sizes[5]);
/* The grid's cells per record for the next fmgi_set_scene of ctx (0, the default: the product's choice, 16,
   or the coarse LDS grids of the closed boxes); tests use it to check the grids those choices build. */
int fmgi_set_grid_cells_per_record(fmgi_context *ctx, int cells_per_record);
/* 1 in the experiment build (make experiments -> libflatmatch_gi_exp.so), whose experiment knobs
   (environment variables of measured-and-rejected paths) it reads; 0 in the product library. */
int fmgi_experiments(void);
/* Per-context handles on product paths that a given scene or launch size would not take, for tests (each
   takes effect at the next bake; FMGI_OPT_NO_AXES at the next fmgi_set_scene):
     FMGI_OPT_CHUNK_ITEMS   > 0: at most this many work items per STREAM chunk (several chunks per call)
     FMGI_OPT_POOL_LIMIT    > 0: at most this many bucket-pool blocks (the exact atomic fallback takes the rest)
     FMGI_OPT_STREAM_LAYOUT 0: the slice-sorted stream (lightmaps of more than 63 tiles); -1: by the scene
     FMGI_OPT_BUCKET_FILL   0: per-wave LDS rings, 1: lane-by-lane stores into per-wave tile blocks, 2: into
                            per-workgroup tile blocks; -1: by the tables' LDS fit
     FMGI_OPT_WIDE_TILES    0 / 1: 2048- / 4096-texel bucket tiles; -1: by the launch size
     FMGI_OPT_COOP          2, 4, 8: lanes per work item of ScanFast's small launches; 0: by the launch size
     FMGI_OPT_NO_AXES       1: closed boxes through the general grid instance (its sorted <= 4-slot phase 1)
     FMGI_OPT_PHOTON_LOCK   0 / 1: the staged and compact closed boxes through the per-lane / the wave-locked
                            photon loop; -1: by the configuration (any other value: FMGI_ERR_ARG)
     FMGI_OPT_LATTICE       0 / 1: the staged and compact closed boxes whose six planes are verified lattices of
                            rects (fmgi_lattice_copy) through their grid cells / the lattice cell of the nearest
                            plane; -1: by the configuration (any other value: FMGI_ERR_ARG). A scene without a
                            lattice runs its ordinary instance whatever the value.
     FMGI_OPT_HIST_BATCH    > 0: at most this many codes per counting batch of fmgi_bake_sparse and
                            fmgi_sparse_from_codes (several batches per chunk); 0: 64 Mi codes */
#define FMGI_OPT_CHUNK_ITEMS 1
#define FMGI_OPT_POOL_LIMIT 2
#define FMGI_OPT_STREAM_LAYOUT 3
#define FMGI_OPT_BUCKET_FILL 4
#define FMGI_OPT_WIDE_TILES 5
#define FMGI_OPT_COOP 6
#define FMGI_OPT_NO_AXES 7
#define FMGI_OPT_PHOTON_LOCK 8
#define FMGI_OPT_LATTICE 9
#define FMGI_OPT_HIST_BATCH 10
#define FMGI_OPT_COUNT 11
int fmgi_set_option(fmgi_context *ctx, int option, int64_t value);
/* Profiling builds only (make timing -> libflatmatch_gi_timing.so, -DFMGI_STAGE_TIMING): shader-clock
   cycles summed over waves per bake-loop stage {start, sample, scan phase 1, phase 2, fallback, hit,
   append}, since the last fmgi_reset_stats; all zero in the normal library. */
int fmgi_get_stage_cycles(fmgi_context *ctx, uint64_t out[16]);
int fmgi_grid_copy(const fmgi_context *ctx, void *planes, void *cells, float *recs, int32_t *idx);
/* The lattice descriptors of a closed box (built and verified by fmgi_set_scene; host-only contexts too): returns
   6 when every plane of the box is a uniform lattice of rects, else 0, and with desc != NULL copies them, per
   axis {plane of the +n class, plane of the -n class}, each {float u0, iu, mu, lo_u, v0, iv, mv, lo_v, hi_u, hi_v;
   int32 base, su, sv, nu, nv, pad} (64 B). A hit point (uh, vh) of the plane lies in lattice cell
   cu = floor(clamp((uh - u0) * iu, 0, mu)) at fraction fu = (uh - u0) * iu - cu (likewise v), all in float32;
   where lo_u <= fu <= hi_u and lo_v <= fv <= hi_v, exactly one record of the plane passes the filter test and it
   is rect base + cu * su + cv * sv. */
int fmgi_lattice_copy(const fmgi_context *ctx, void *desc);
/* FMGI_KERNEL_HYBRID's floor plan of the walls (built by fmgi_set_scene; host-only contexts too; the
   hybrid scan walks it with FMGI_PLAN=1): *bytes = its size (0: no plan for this scene); with
   blob != NULL and *bytes >= that size, copies it: {float x0, y0, 1 / cs, cs}, {int32 nx | ny << 16,
   ncells, nentries, 0}, u16 start[ncells + 1], u16 entry[nentries] (cell (ix, iy) = iy * nx + ix lists
   entry[start[i] .. start[i + 1]]: 32-B records of the filter image, record r at byte 32 r; x walls
   first, r & 1 = the class, +n = 0). */
int fmgi_plan_copy(const fmgi_context *ctx, void *blob, int32_t *bytes);
/* The filter image of FMGI_KERNEL_FAST / HYBRID (built by fmgi_set_scene; host-only contexts too): pairs[a]
   = its pairs on axis a; *bytes = its size; with img != NULL and *bytes >= that size, copies it: per axis,
   pairs[a] pairs {record of the +n class, record of the -n class}, then 16 padding records; a record is
   {float plane, cu, hwu, cv, hwv; int32 rect index (-1: padding); pad[2]} (32 B; extents grown by the
   filter margin). Pair j holds record j of each class, rect order. */
int fmgi_filter_copy(const fmgi_context *ctx, void *img, int32_t *bytes, int32_t pairs[3]);
/* FMGI_KERNEL_HYBRID's wall-pair image (built by fmgi_set_scene; host-only contexts too): for the x and then
   the y axis, groups[a] groups of two 48-B halves (the +a class, then the -a class), each half
   {float plane[2], cu[2], hwu[2], cv[2], hwv[2]; int32 rect index[2]} = records 2g and 2g + 1 of its class as
   the filter image holds them (a missing record: hwu = hwv = -1, index -1). Same size protocol. */
int fmgi_pairs_copy(const fmgi_context *ctx, void *img, int32_t *bytes, int32_t groups[2]);

/* Host helpers exported for tests (no device needed). */
void fmgi_host_sincosf(const float *x, float *s, float *c, int64_t n);
/* Device-side twin of fmgi_host_sincosf over n inputs (synchronous; for parity tests). */
int fmgi_device_sincosf(fmgi_context *ctx, const float *x, float *s, float *c, int64_t n);
/* The device library's own sinf/cosf (ROCm ocml, what photonmap.cl's sin/cos run on MI355X) over n
   inputs, for checking the restatement (synchronous; parity tests). */
int fmgi_device_sincosf_library(fmgi_context *ctx, const float *x, float *s, float *c, int64_t n);
/* Device arithmetic helpers of the bake kernel over n inputs (synchronous; for parity tests):
   op FMGI_UNIT_SQRT: out[i] = bits of the sampler's correctly rounded sqrtf(a[i]) (b unused);
   op FMGI_UNIT_TRUNC_DIV: out[i] = (int)(a[i] / b[i]), the tile index step of photonmap.cl:108-109
   (through v_rcp_f32); op FMGI_UNIT_TRUNC_DIV_INV: the same through the host-rounded 1.0f / b[i]. */
#define FMGI_UNIT_SQRT 0
#define FMGI_UNIT_TRUNC_DIV 1
#define FMGI_UNIT_TRUNC_DIV_INV 2
int fmgi_device_unit(fmgi_context *ctx, int op, const float *a, const float *b, int32_t *out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
