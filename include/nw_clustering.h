/*
 * nw_clustering.h -- C-ABI of the exact DBSCAN clustering in libnanowrap_hip.so (csrc/nw_clustering.hip, MI355X / gfx950): which
 * localizations of a cloud are structure, which are background, and which structure each belongs to.
 *
 * What it is for: the step before the surface recipe.  Upstream users run PYME's DBSCANClustering ahead of it; PYME is not in the
 * reference tree, so the definition is this project's own and is written down in csrc/nw_clustering_core.h.
 *
 * Definitions:
 *   - the cloud is (n,3) float32, row-major, a host pointer or a device pointer, 1 <= n <= 2^30; a non-finite coordinate is an error;
 *   - d2(i, j) = (ex*ex + ey*ey) + ez*ez in float64 with e = (double)p_j - (double)p_i (no fma): bit-symmetric in i, j;
 *   - near(i, j) <=> d2(i, j) <= eps2, eps2 = eps * eps in float64; eps is finite, > 0 and <= 2^40.  Squares are compared, no sqrt is
 *     taken anywhere, and a pair at exactly eps2 is near;
 *   - n_eps(i) = #{ j : near(i, j) }: the point itself and its duplicates count.  count[i] = min(n_eps(i), count_cap);
 *     1 <= min_points <= count_cap <= 2^30.  count_cap = min_points is the cheap choice, count_cap >= n gives full counts;
 *   - core[i] = (n_eps(i) >= min_points);
 *   - the clusters are the connected components of the graph on the core points with near as edges, numbered 0 .. C-1 in ascending
 *     order of each component's smallest point index;
 *   - anchor[i]: a core point anchors to itself; a non-core point with a core point near it anchors to the core j that minimises
 *     (d2(i, j), j) lexicographically (the border rule: the nearest core, ties to the smallest index -- not scikit-learn's "whichever
 *     cluster reaches it first", which depends on the order of the cloud); every other point has -1;
 *   - label[i] = the cluster of anchor[i], or -1 (noise);
 *   - per cluster: size (all labelled points), n_core, first (the smallest core index), bbox (min x y z, max x y z of the members);
 *   - no output depends on the cell size, on the launch geometry or on the order in which atomics land.  Permuting the cloud permutes
 *     count, core and the partition; it changes only the numbering of the clusters and the index ties of the border rule.
 *
 * How it is computed.  The cloud is binned into the query units' shared cell grid (bq::bounds<float>, bq::build_grid<float>).  The cell
 * size is this unit's own: h = max(0.57 eps, widest extent / 1024), widened by a tenth at a time until the grid
 * has at most max(2 n, 65536) cells (2^26 at most, 1025 an axis).  A call with another eps bins again.  One lane per point, in cell order,
 * walks rings of cells around its own; ring r has nw_neighbours.h's lower bound, and the walk ends when its square exceeds eps2.
 * Core points are joined by a lock-free union-find whose roots are the components' smallest indices whatever the schedule.  Two
 * shortcuts skip distance tests and change no output; both need sqrt(3) h (1 + 2^-9) < eps (any two points of one cell are then near,
 * see the core header) and are off on a grid that was widened past that:
 *   (a) a point whose cell holds at least count_cap points has count_cap and is core;
 *   (b) the core points of one cell are joined through the cell's smallest-index core point; a cell being one component, a core point
 *       then needs one near core point of each neighbouring cell only, and leaves the rest of that cell.
 *
 * Conventions (as include/nw_neighbours.h, with its own prefix and context):
 *   - every call returns NWP_OK (0) or a negative status; nwp_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call; without a GPU nwp_create fails with NWP_ERR_HIP -- there is no CPU
 *     fallback;
 *   - a device pointer is read on the context's own stream with no ordering against the stream that wrote it: it must be complete
 *     before the call and unchanged until it returns;
 *   - one nwp_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_CLUSTERING_H_
#define NW_CLUSTERING_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWP_ABI_VERSION 1

/* info[]: int64 words */
#define NWP_INFO_WORDS 12
#define NWP_INFO_N_CORE 0
#define NWP_INFO_N_BORDER 1
#define NWP_INFO_N_NOISE 2
#define NWP_INFO_N_CLUSTERS 3
#define NWP_INFO_CELLS 4
#define NWP_INFO_CELL_SIZE 5        /* the bits of a double */
#define NWP_INFO_TESTS 6            /* distance tests done, all kernels */
#define NWP_INFO_SHORTCUT_A 7       /* points that got count_cap from their cell's population */
#define NWP_INFO_SHORTCUT_B 8       /* core points joined through their cell's smallest-index core point */
#define NWP_INFO_GUARD 9            /* 1 if the grid allowed the shortcuts and they were switched on */
#define NWP_INFO_TESTS_COUNT 10     /* of NWP_INFO_TESTS, those of the neighbour count */
#define NWP_INFO_TESTS_HOOK 11      /* and those of the unions (the rest are the border rule's) */

typedef struct nwp_ctx nwp_ctx;

typedef enum nwp_status {
    NWP_OK = 0,
    NWP_ERR_BADARG = -1,      /* NULL pointer, size out of range, eps / min_points / count_cap outside the definition */
    NWP_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwp_last_error */
    NWP_ERR_NONFINITE = -3,   /* a non-finite coordinate in the cloud */
    NWP_ERR_NOMEM = -4,
    NWP_ERR_NOCLOUD = -5      /* nwp_dbscan before nwp_set_cloud, nwp_cluster_stats before nwp_dbscan */
} nwp_status;

int nwp_abi_version(void);
int nwp_create(int device, nwp_ctx **out);
void nwp_destroy(nwp_ctx *ctx);
const char *nwp_last_error(nwp_ctx *ctx);

/* Takes a copy of the cloud into the context, where it stays for any number of queries (until the next nwp_set_cloud; a failed call
 * leaves the context without a cloud).  on_device = 0: a host pointer, checked for finiteness on the host before any HIP call; 1: a
 * device pointer, checked by the bounding-box kernel. */
int nwp_set_cloud(nwp_ctx *ctx, const float *xyz, int64_t n, int on_device);

/* Switches the two shortcuts on (the default) or off for the context's later queries.  No output but info changes with it: it is there
 * for measuring what the shortcuts save and for testing that they change nothing. */
int nwp_set_shortcuts(nwp_ctx *ctx, int on);

/* One clustering of the cloud.  The outputs are host pointers: label (n) int32, anchor (n) int32, count (n) int32, core (n) uint8 -- any
 * of these four may be NULL --, *n_clusters, and info (NWP_INFO_WORDS int64).  Bins the cloud anew if eps asks for another cell size
 * than the grid at hand has. */
int nwp_dbscan(nwp_ctx *ctx, double eps, int64_t min_points, int64_t count_cap, int32_t *label, int32_t *anchor, int32_t *count, uint8_t *core,
               int32_t *n_clusters, int64_t *info);

/* The statistics of the last nwp_dbscan's C clusters, host pointers, any may be NULL: size (C) int64, n_core (C) int64, first (C) int32,
 * bbox (C, 6) float32. */
int nwp_cluster_stats(nwp_ctx *ctx, int64_t *size, int64_t *n_core, int32_t *first, float *bbox);

#ifdef __cplusplus
}
#endif

#endif
