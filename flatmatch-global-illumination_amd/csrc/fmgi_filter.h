/* fmgi_filter.h -- the adaptive density filter's device tables and arguments (fmgi_filter.hip, fmgi_api.cpp). */
#ifndef FMGI_FILTER_H
#define FMGI_FILTER_H

#include <stdint.h>

#include <hip/hip_runtime_api.h>

constexpr int kFilterMaxRadius = 16; /* FMGI_FILTER_MAX_RADIUS */
constexpr int kFilterMaxMaps = 8;    /* FMGI_FILTER_MAX_MAPS */

/* texel -> its wall and row (wall < 0: in no wall's level-0 grid); x = texel - s0 - y * s1 */
struct FilterTex {
    int32_t wall, y;
};
/* lightmapSetup of a wall */
struct FilterWall {
    int32_t s0, s1, s2, pad;
};
/* one level-0 column of a wall */
struct FilterCol {
    int32_t wall, x;
};

struct FilterArgs {
    const FilterTex *tex;    /* [num_texels] */
    const FilterWall *walls;
    const FilterCol *cols;   /* [num_cols], the walls' columns in wall order, x ascending */
    int num_texels, num_cols;
    unsigned long long *sat; /* the context's scratch: per-wall inclusive 2-D prefix sums, [plane][num_texels] */
    /* planes: with guide, one (its energy); else 3 per map (plane 3 k + c = channel c of in[k]) */
    const unsigned long long *guide;
    const unsigned long long *in[kFilterMaxMaps];
    unsigned long long *out[kFilterMaxMaps];
    int maps;
    const uint8_t *radii_in; /* apply */
    uint8_t *radii_out;      /* radii */
    unsigned long long min_energy;
    int max_radius;
};

/* the prefix sums of `planes` planes (row scans, then column accumulation) */
hipError_t fmgi_launch_filter_sat(const FilterArgs &a, int planes, hipStream_t s);
hipError_t fmgi_launch_filter_radii(const FilterArgs &a, hipStream_t s);
hipError_t fmgi_launch_filter_apply(const FilterArgs &a, hipStream_t s);

#endif
