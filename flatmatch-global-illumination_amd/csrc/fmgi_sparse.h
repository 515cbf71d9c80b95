/* fmgi_sparse.h -- the sparse, blocked photon histogram's device arguments (fmgi_sparse.hip, fmgi_api.cpp;
   DESIGN.md §14). A blob is uint64 off[B + 1] followed by uint64 entry[64 * rows]; B = blocks of 64 texels. */
#ifndef FMGI_SPARSE_H
#define FMGI_SPARSE_H

#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "fmgi_recolour.h"

constexpr int kSparseCountBits = 54; /* FMGI_SPARSE_COUNT_BITS: entry = state << 54 | count */
constexpr unsigned long long kSparseCountMask = (1ull << kSparseCountBits) - 1;

/* the four sums fmgi_sparse_measure reads back, in this order */
struct SparseSums {
    unsigned long long rows, cells, deposits, too_large;
};

struct SparseRecolourArgs {
    const unsigned long long *blob;        /* one group's blob: off[blocks + 1], entry[64 * rows] */
    const uint32_t *table;                 /* [kRecolourStates][k][3], as RecolourArgs::table */
    unsigned long long *lm[kRecolourMaxK]; /* the pass's lightmaps, int64 [num_texels][4] */
    unsigned long long rows;               /* the host's info.rows: every offset is clamped to it */
    int num_texels;
    int k;                                 /* scenarios of this pass, 1..kRecolourMaxK */
};

inline int fmgi_sparse_blocks(int num_texels) { return (int)(((int64_t)num_texels + 63) / 64); }

/* one pass over counts [kRecolourStates][num_texels]: with sums != nullptr it adds the four sums to *sums (zeroed
   by the caller), with off != nullptr it stores every block's row count r_b in off[b + 1] */
hipError_t fmgi_launch_sparse_count(const unsigned long long *counts, int num_texels, unsigned long long *off,
                                    SparseSums *sums, hipStream_t s);
/* off[1 .. blocks] (row counts) -> inclusive prefix sums in place, every value clamped to rows */
hipError_t fmgi_launch_sparse_scan(unsigned long long *off, int blocks, unsigned long long rows, hipStream_t s);
/* the entries of blob (whose off[] the scan has written) from counts; writes every slot of every block */
hipError_t fmgi_launch_sparse_fill(const unsigned long long *counts, int num_texels, unsigned long long *blob,
                                   unsigned long long rows, hipStream_t s);
/* counts[state][t] += count for every non-padding entry */
hipError_t fmgi_launch_sparse_expand(const unsigned long long *blob, int num_texels, unsigned long long rows,
                                     unsigned long long *counts, hipStream_t s);
hipError_t fmgi_launch_recolour_sparse(const SparseRecolourArgs &a, hipStream_t s);

#endif
