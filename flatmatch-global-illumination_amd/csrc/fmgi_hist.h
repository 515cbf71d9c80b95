/* fmgi_hist.h -- sparse photon histograms built from deposit codes, and the sum of two blobs (fmgi_hist.hip,
   fmgi_api.cpp). A code is texel << 10 | colour state; a half-block is 32 consecutive texels
   (code >> 15), two of them are one block of the blob (fmgi_sparse.h). */
#ifndef FMGI_HIST_H
#define FMGI_HIST_H

#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "fmgi_sparse.h"

constexpr int kHistHalfTexels = 32;   /* texels one counting workgroup holds: u32 [1024][32] = 128 KB of LDS */
constexpr int kHistHalfShift = 15;    /* code >> 15 = texel >> 5 = the half-block */
constexpr int kHistSegCodes = 1024;   /* codes per segment: a pool block (FMGI_BUCKET_BLOCK), or a slice of raw codes */
constexpr int kHistMaxHalves = 4096;  /* half-blocks the binning kernels' LDS histogram holds (63 tiles of 2048 texels: 4032) */

/* where the codes are: the bake's bucket pool (blocks of 1024 codes with a length each; segment j is block
   list[list_lo + j] of the pool's blocks listed by tile, fmgi_stream_bucket_list, or block j when list == nullptr)
   or a plain array of n codes (block_len == nullptr) */
struct HistSource {
    const uint32_t *codes;
    const uint32_t *block_len;
    const uint32_t *list;
    uint64_t list_lo;
    uint64_t nseg;  /* segments: pool blocks to read, or (n + 1023) / 1024 */
    uint64_t n;     /* plain array: its codes */
    uint64_t pool_blocks; /* pool: a listed block id at or past it is skipped */
    int num_texels; /* a code whose texel is >= num_texels is skipped */
};

/* half_count[h] += codes of half-block h (h < halves <= kHistMaxHalves); *skipped += codes that are not
   0xFFFFFFFF and whose texel is >= num_texels */
hipError_t fmgi_launch_hist_bins(const HistSource &src, uint32_t halves, unsigned long long *half_count,
                                 unsigned long long *skipped, hipStream_t s);
/* the codes of half-blocks [half_lo, half_hi) moved to scratch, each half-block's contiguous: cursor[h - half_lo]
   holds the half-block's first index in scratch (the exclusive scan of its counts) and is advanced; nothing at
   or past scratch_cap is written */
hipError_t fmgi_launch_hist_scatter(const HistSource &src, uint32_t half_lo, uint32_t half_hi, uint32_t *cursor,
                                    uint32_t *scratch, uint32_t scratch_cap, hipStream_t s);
/* one workgroup per half-block of [half_lo, half_hi): its codes scratch[start[h - half_lo], start[h - half_lo + 1])
   counted in LDS; nz[32 h + l] = the non-zero states of its texel l */
hipError_t fmgi_launch_hist_count(const uint32_t *scratch, const uint32_t *start, uint32_t scratch_cap,
                                  uint32_t half_lo, uint32_t half_hi, uint32_t *nz, hipStream_t s);
/* blocks [block_lo, block_hi): r_b = the largest nz of the block's 64 texels -> rows_local[b - block_lo + 1] and
   rows_all[b + 1]; sums->rows += r_b, sums->cells += the block's nz */
hipError_t fmgi_launch_hist_rows(const uint32_t *nz, uint32_t block_lo, uint32_t block_hi,
                                 unsigned long long *rows_local, unsigned long long *rows_all, SparseSums *sums,
                                 hipStream_t s);
/* the count again, then every slot of the blocks' rows written: piece[(off[b - block_lo] + j) * 64 + lane], off[]
   = rows_local after fmgi_launch_sparse_scan, clamped to piece_rows */
hipError_t fmgi_launch_hist_fill(const uint32_t *scratch, const uint32_t *start, uint32_t scratch_cap,
                                 uint32_t half_lo, uint32_t half_hi, const unsigned long long *off,
                                 unsigned long long piece_rows, unsigned long long *piece, hipStream_t s);

/* sum = a + b, one wave per block and one lane per texel (a two-pointer merge of two ascending lists). Both
   blobs' offsets are clamped to their rows. count: off != nullptr receives r_b in off[b + 1], sums != nullptr
   the four sums. fill: sum's off[] (scanned) is read and clamped to sum_rows; every slot is written. */
hipError_t fmgi_launch_sparse_add_count(const unsigned long long *a, unsigned long long a_rows,
                                        const unsigned long long *b, unsigned long long b_rows, int num_texels,
                                        unsigned long long *off, SparseSums *sums, hipStream_t s);
hipError_t fmgi_launch_sparse_add_fill(const unsigned long long *a, unsigned long long a_rows,
                                       const unsigned long long *b, unsigned long long b_rows, int num_texels,
                                       unsigned long long *sum, unsigned long long sum_rows, hipStream_t s);

#endif
