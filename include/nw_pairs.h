/*
 * nw_pairs.h -- C-ABI of the exact pair-distance counts in libnanowrap_hip.so (csrc/nw_pairs.hip, MI355X / gfx950): the histogram of
 * pair distances of a cloud, or between two clouds, and the same counts per localization.
 *
 * What it is for: the second-order statistics of an SMLM table -- the pair-distance histogram, Ripley's K with its L and H forms, the
 * pair correlation g(r), the local L per localization.  Upstream users take them from PYME (PairwiseDistanceHistogram, Ripleys); PYME
 * is not in the reference tree, so the definition is this project's own and is written down in csrc/nw_pairs_core.h.  This ABI gives
 * integers only; the normalisations are host arithmetic on top of them (ch_shrinkwrap_amd/pairs.py).
 *
 * Definitions:
 *   - the cloud is (n,3) float32, row-major, a host pointer or a device pointer, 1 <= n <= 2^30; a non-finite coordinate is an error;
 *   - the edges are m radii, 1 <= m <= NWQ_MAX_BINS = 64, finite, 0 <= r_0 < r_1 < ... < r_{m-1} <= 2^40; e2[b] = r_b * r_b in float64,
 *     computed once by the library, must be strictly ascending too (two radii that square to one double are refused).  r_0 = 0 is
 *     allowed: bin 0 then holds exactly coincident pairs;
 *   - d2 = (ex*ex + ey*ey) + ez*ez in float64 with e = (double)cloud point - (double)query (no fma): bit-symmetric in the two points.
 *     Squares are compared; no root is taken anywhere;
 *   - bin(d2) = #{ b : e2[b] < d2 }; a pair with bin m is not counted.  hist[b] counts e2[b-1] < d2 <= e2[b] (bin 0: d2 <= e2[0]): a pair
 *     at exactly an edge belongs to the bin the edge closes.  The cumulative count #{ d2 <= e2[b] } is the sum of hist[0 .. b];
 *   - auto mode (queries = NULL): the ordered pairs (i, j) of the cloud with j != i BY INDEX; duplicates at other indices count; every
 *     unordered pair is counted twice, once from each end, because the per-point counts need both;
 *   - cross mode: every (i of the queries, j of the cloud), nothing excluded; a query may lie anywhere, far outside the cloud's box
 *     included; 1 <= nq <= 2^30;
 *   - hist is (m) uint64; local, optional, is (nq, m) uint32 in the caller's query order (auto mode: nq = n), differential like hist;
 *     hist[b] = the sum of local[:, b], always.  With n <= 2^30 no counter can overflow;
 *   - no output depends on the cell size, on the launch geometry or on any order of arrival: there are no atomics on the results.
 *
 * How it is computed.  The cloud is binned into the query units' shared cell grid (bq::bounds<float>, bq::build_grid<float>) with this
 * unit's own cell size: h = max(0.5 r_{m-1}, widest extent / 1024), widened by a tenth at a time until the grid has at most
 * max(2 n, 65536) cells (2^26 at most, 1025 an axis).  Edges with another r_{m-1} bin again.  One lane per query -- in auto mode the
 * cloud's points in cell order -- visits every cell that can hold a point within r_{m-1} (a clamped box of cells, see the core header)
 * and keeps its m counters in a column of LDS; up to 16 bins the bin is the literal sum against uniform operands, above that a search
 * over an LDS copy of the edges.  A workgroup adds its columns into one row of partial sums, one workgroup adds the rows.
 * The cost is inherent: a query tests every cloud point of the cells its r_{m-1} reaches.
 *
 * Conventions (as include/nw_clustering.h, with its own prefix and context):
 *   - every call returns NWQ_OK (0) or a negative status; nwq_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call; without a GPU nwq_create fails with NWQ_ERR_HIP -- there is no CPU
 *     fallback;
 *   - a device pointer is read on the context's own stream with no ordering against the stream that wrote it: it must be complete
 *     before the call and unchanged until it returns;
 *   - one nwq_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_PAIRS_H_
#define NW_PAIRS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWQ_ABI_VERSION 1
#define NWQ_MAX_BINS 64

/* info[]: int64 words */
#define NWQ_INFO_WORDS 8
#define NWQ_INFO_TESTS 0            /* distance tests done */
#define NWQ_INFO_CELLS_READ 1       /* grid cells read, all queries */
#define NWQ_INFO_CELL_SIZE 2        /* the bits of a double */
#define NWQ_INFO_CELLS 3            /* cells of the grid */
#define NWQ_INFO_VARIANT 4          /* 0: up to 16 bins, the sum; 1: up to 64 bins, the search */
#define NWQ_INFO_N_QUERIES 5
#define NWQ_INFO_N_CLOUD 6
#define NWQ_INFO_BINS 7

typedef struct nwq_ctx nwq_ctx;

typedef enum nwq_status {
    NWQ_OK = 0,
    NWQ_ERR_BADARG = -1,      /* NULL pointer, size out of range, radii outside the definition */
    NWQ_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwq_last_error */
    NWQ_ERR_NONFINITE = -3,   /* a non-finite coordinate in the cloud or in the queries */
    NWQ_ERR_NOMEM = -4,
    NWQ_ERR_NOCLOUD = -5      /* nwq_count before nwq_set_cloud or before nwq_set_edges */
} nwq_status;

int nwq_abi_version(void);
int nwq_create(int device, nwq_ctx **out);
void nwq_destroy(nwq_ctx *ctx);
const char *nwq_last_error(nwq_ctx *ctx);

/* Takes a copy of the cloud into the context, where it stays for any number of counts (until the next nwq_set_cloud; a failed call
 * leaves the context without a cloud).  on_device = 0: a host pointer, checked for finiteness on the host before any HIP call; 1: a
 * device pointer, checked by the bounding-box kernel. */
int nwq_set_cloud(nwq_ctx *ctx, const float *xyz, int64_t n, int on_device);

/* The edges of the context's later counts: m radii, host pointer, checked as the definition says (NWQ_ERR_BADARG otherwise, and the
 * context keeps the edges it had).  Needs no cloud and touches no GPU. */
int nwq_set_edges(nwq_ctx *ctx, const double *radii, int64_t m);

/* One count.  queries = NULL: auto mode, nq must be 0 or the cloud's n.  Otherwise cross mode: (nq,3) float32, a host pointer
 * (on_device = 0, checked for finiteness on the host) or a device pointer (1, checked by the kernel).  The outputs are host pointers:
 * hist (m) uint64, local (n_queries, m) uint32 or NULL, info (NWQ_INFO_WORDS int64).  Bins the cloud anew if the edges ask for another
 * cell size than the grid at hand has. */
int nwq_count(nwq_ctx *ctx, const float *queries, int64_t nq, int on_device, uint64_t *hist, uint32_t *local, int64_t *info);

#ifdef __cplusplus
}
#endif

#endif
