/* fmgi_recolour.h -- the recolour pass's device arguments (fmgi_recolour.hip, fmgi_api.cpp). */
#ifndef FMGI_RECOLOUR_H
#define FMGI_RECOLOUR_H

#include <stdint.h>

#include <hip/hip_runtime_api.h>

constexpr int kRecolourMaxK = 8;     /* FMGI_RECOLOUR_MAX_SCENARIOS */
constexpr int kRecolourStates = 1024; /* FMGI_COLOUR_STATE_COUNT */
constexpr int kRecolourWaves = 4;    /* waves per workgroup; each takes its own slice of the states */

struct RecolourArgs {
    const unsigned long long *counts; /* one group's histogram, [kRecolourStates][num_texels] */
    const uint32_t *table;            /* [kRecolourStates][k][3]: this group's deposits (< 2^30) per scenario */
    unsigned long long *lm[kRecolourMaxK]; /* the pass's lightmaps, int64 [num_texels][4] */
    int num_texels;
    int k;                            /* scenarios of this pass, 1..kRecolourMaxK */
    int slabs;                        /* gridDim.y: the states are cut into slabs x kRecolourWaves slices */
};

/* state slabs (a power of two, 1..64) for num_texels texels on num_cus compute units */
int fmgi_recolour_slabs(int num_texels, int num_cus);
hipError_t fmgi_launch_recolour(const RecolourArgs &a, hipStream_t s);

#endif
