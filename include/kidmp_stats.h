/*
 * kidmp_stats.h -- per-level ensemble statistics on the device: moments and histograms of [ncol][nz] arrays.
 *
 * An ensemble of independent columns ends in device arrays x[col*stride + k] (the state, the column outputs of
 * kidmp_column_outputs_device, a single rate of the rate diagnostics).  kidmp_level_stats_device reduces any set of
 * them over the columns, per level and per ensemble group, without a download: count, mean, M2, min, max and, if
 * asked, a histogram per level (of dBZ: the CFAD).  KiD reports its fields as nx-means (W:248-303); this is that idea
 * at the scale of 10^5 columns.  Conventions as in kidmp.h (return codes, device binding, k fastest).
 *
 * Values and cells
 *   A cell is one (group g, field f, level k).  The MOMENTS of a cell are taken over the finite values x of level k
 *   of the columns c with group[c] == g that satisfy x > floor[f] (no floor: every finite value).  The HISTOGRAM of
 *   a cell counts every value of those columns, finite or not, and ignores the floor.
 *
 *   mom[ngroup][nfield][KIDMP_STATS_NMOM][nz], binary64, device:
 *       row 0  count, as a double                 empty cell: 0
 *       row 1  mean                                            0
 *       row 2  M2 = sum (x - mean)**2                          0      (variance = M2 / count is the caller's)
 *       row 3  min                                             +inf
 *       row 4  max                                             -inf
 *   hist[ngroup][nfield][nz][nbin+3], int64, device; not written (may be NULL) when nbin == 0:
 *       slot 0        x < edges[0]                 (-inf lands here)
 *       slot 1+b      edges[b] <= x < edges[b+1]   b = 0 .. nbin-1
 *       slot nbin+1   x >= edges[nbin]             (+inf lands here)
 *       slot nbin+2   NaN
 *     i.e. slot = the number of edges <= x (numpy.searchsorted(edges, x, side="right")).
 *
 * What is exact and what is not
 *   count, min, max and every histogram slot are exact: they do not depend on the order of the columns, on the
 *   chunking below, or on any partition of the columns into shards whose results kidmp_stats_merge joins.
 *   mean and M2 are floating-point results of Welford's updating algorithm inside a chunk and Chan's pairwise formula
 *   across chunks.  They are reproducible bit for bit for a given (ncol, nz, grouping, data) -- the chunking is a pure
 *   function of ncol, every sum runs in a fixed order, nothing is accumulated with atomics -- but they are NOT
 *   invariant under another partition: a sharded and merged result agrees with the one-call result only to rounding
 *   (mean: a few n ulp of max|x|; M2: relative n * kappa * 2**-53, kappa = sqrt(sum x**2 / M2)).
 *
 * Chunking
 *   kidmp_stats_chunks(ncol) = min(ncol, 256) for ncol >= 1, and 0 for ncol <= 0.  With C chunks and
 *   per = ceil(ncol / C), chunk j holds the columns [j*per, min((j+1)*per, ncol)); trailing chunks may be empty.  Each
 *   chunk is reduced on its own in column order, the chunks are merged in index order.
 */
#ifndef KIDMP_STATS_H
#define KIDMP_STATS_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_STATS_MAX_FIELDS 16
#define KIDMP_STATS_MAX_GROUPS 64
#define KIDMP_STATS_MAX_BINS   64
#define KIDMP_STATS_NMOM        5      /* count, mean, M2, min, max */

typedef struct kidmp_stats_request {
    int32_t nfield;                    /* 1 .. KIDMP_STATS_MAX_FIELDS */
    const void *const *field;          /* host array of nfield DEVICE pointers; element (c,k) = field[f][c*col_stride[f] + k] */
    const int64_t *col_stride;         /* host [nfield], may be NULL = nz everywhere; each >= nz */
    const double  *floor;              /* host [nfield], may be NULL = none: only values x > floor[f] enter the moments */
    const int32_t *group;              /* DEVICE [ncol], may be NULL = all columns in group 0; a value outside [0, ngroup)
                                          leaves the column out of everything */
    int32_t ngroup;                    /* 1 .. KIDMP_STATS_MAX_GROUPS */
    int32_t nbin;                      /* 0 = no histogram, else 1 .. KIDMP_STATS_MAX_BINS */
    const double  *edges;              /* DEVICE [nfield][nbin+1], ascending per field (stated, not checked; any content is
                                          memory-safe) */
} kidmp_stats_request;

/* The reduction.  The fields are binary64 arrays (kidmp_) or binary32 arrays (kidmp32_: every value is widened to
 * binary64 on load and everything after that is the same code, so on the same numbers both return the same bits).
 * col_stride lets one rate be a field: of rates[ncol][KIDMP_NRATES][nz], rate r is the pointer rates + r*nz with
 * col_stride = KIDMP_NRATES*nz.
 *   mom, hist   device, as above; they must not overlap the fields
 *   work        device workspace of at least kidmp_stats_workspace_bytes(ncol, nz, nfield, ngroup, nbin) bytes, 8-byte
 *               aligned; may be NULL where that is 0 (ncol == 0)
 * The entry never allocates and never synchronises, and enqueues only on `stream`, as one linear chain of two
 * launches (the partial pass over chunk x group x field, the combine pass); it can be captured into a hipGraph.
 * ncol == 0 returns KIDMP_OK with every cell empty.
 * Refused with KIDMP_EINVAL, nothing written: nz outside [2, KIDMP_MAX_NZ], ncol < 0 or > 2**40, nfield, ngroup or
 * nbin outside their ranges, a required NULL (the request, field, a field pointer, mom; hist and edges when nbin > 0;
 * work when ncol > 0), col_stride < nz, a workspace that is too small or misaligned, a field, group, edges, mom, hist or
 * work that is not device memory of the context's device.  A NULL context returns KIDMP_ESTATE. */
int kidmp_level_stats_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const kidmp_stats_request *req, double *mom,
                             int64_t *hist, void *work, size_t work_bytes, void *stream);
int kidmp32_level_stats_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const kidmp_stats_request *req, double *mom,
                               int64_t *hist, void *work, size_t work_bytes, void *stream);

/* No context, no GPU.  The bytes of `work`: kidmp_stats_chunks(ncol) partial results of ngroup*nfield*nz cells, each
 * KIDMP_STATS_NMOM doubles and, when nbin > 0, nbin+3 32-bit counts; rounded up to 256.  0 for bad arguments (the
 * ranges above) and for ncol == 0. */
size_t kidmp_stats_workspace_bytes(int64_t ncol, int32_t nz, int32_t nfield, int32_t ngroup, int32_t nbin);
/* No context, no GPU.  The number of column chunks, see "Chunking" above: min(ncol, 256), 0 for ncol <= 0. */
int32_t kidmp_stats_chunks(int64_t ncol);

/* Fold result b into result a, on HOST arrays laid out as mom and hist above with ncell = ngroup*nfield cells
 * (hist_a and hist_b may be NULL when nbin == 0): counts and histogram slots add, min and max combine, mean and M2 by
 * Chan's pairwise formula; an empty cell on either side leaves the other as it is, bit for bit.  For shards (multi-GPU
 * callers), batches of columns and accumulation over time steps.  KIDMP_EINVAL for a required NULL or ncell < 0, nz < 1,
 * nbin outside [0, KIDMP_STATS_MAX_BINS]. */
int kidmp_stats_merge(int64_t ncell, int32_t nz, int32_t nbin, double *mom_a, int64_t *hist_a, const double *mom_b,
                      const int64_t *hist_b);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_STATS_H */
