/*
 * nw_neighbours.h -- C-ABI of the exact k-th-nearest-neighbour distance in libnanowrap_hip.so (csrc/nw_neighbours.hip, MI355X / gfx950):
 * the distance from a position to its k-th nearest localization, for lists of queries and for the nodes of a voxel lattice.
 *
 * What it is for: a start surface whose bandwidth follows the cloud.  Upstream's recipe is pointcloud.Octree(n_points_min) ->
 * surface_fitting.DualMarchingCubes(threshold_density); both modules are PYME's and not in the reference tree.  The isosurface of the
 * k-NN density k / (4/3 pi r_k^3) at threshold_density is the level set r_k(x) = R_thr, R_thr = (3 k / (4 pi threshold_density))^(1/3):
 * with a given threshold_density that is the level set of "k localizations within R_thr".  What adapts is R_thr: it follows
 * (threshold_density, n_points_min), or -- with the threshold taken from the cloud's own k-NN density -- the cloud.  This is still NOT
 * PYME's octree: a regular grid, one resolution; the voxel size is resolution only.
 *
 * Definitions:
 *   - the cloud is (n,3) float32, row-major, a host pointer or a device pointer, 1 <= n <= 2^30;
 *   - d2(x, p) = (ex*ex + ey*ey) + ez*ez in float64 with e = (double)p - x (no fma); d = sqrt(d2);
 *   - r_k(x) is the k-th smallest d over the whole cloud as a multiset: duplicates count, and a query that is itself a cloud point
 *     counts at distance 0;
 *   - the result is min(r_k, r_cap); it is r_cap when the cloud has fewer than k points.  r_cap is a double > 0 and may be +inf;
 *   - 1 <= k <= NWK_MAX_K; anything else is NWK_ERR_BADARG;
 *   - the value depends on nothing else: not on the order of the cloud, not on ties, not on the cell size, not on the launch
 *     geometry.  Nothing but the value is returned, so a tie needs no rule.
 *
 * How the query stays exact.  The cloud is binned into the query units' shared cell grid (bq::bounds<float>, bq::build_grid<float>);
 * the cell size is this unit's own choice: r_cap / 4 when the cap is finite, about one localization per cell otherwise, widened until
 * the grid is within the unit's cell limit.  One lane per query projects the query onto the cloud's box (out2 = its squared distance
 * from the box) and walks rings of cells around the projection's cell.  Ring r has the lower bound
 * lbd = max(r - 1 - 2^-10, 0) h_cell (1 - 1e-9) (the 2^-10 of a cell covers the float32 rounding of the cells' indices, see
 * csrc/nw_neighbours_core.h); the walk ends when lbd^2 + out2 is strictly more than min(k-th best so far, r_cap)^2, the k-th best
 * being +inf until k candidates are held.  A finite cap therefore bounds the walk at ceil(r_cap / h_cell) + 2 rings.  The k best
 * candidates of a lane live in LDS ([slot][lane], no bank conflicts), with the running maximum and its slot in registers.
 *
 * Conventions (as include/nw_evaluation.h, with its own prefix and context):
 *   - every call returns NWK_OK (0) or a negative status; nwk_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call; without a GPU nwk_create fails with NWK_ERR_HIP -- there is no CPU
 *     fallback;
 *   - a device pointer is read on the context's own stream with no ordering against the stream that wrote it: it must be complete
 *     before the call and unchanged until it returns;
 *   - one nwk_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_NEIGHBOURS_H_
#define NW_NEIGHBOURS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWK_ABI_VERSION 1
#define NWK_MAX_K 32
#define NWK_FIELD_SHIFT 20        /* field = floor((r_cap - r_k) * 2^20) */

typedef struct nwk_ctx nwk_ctx;

typedef enum nwk_status {
    NWK_OK = 0,
    NWK_ERR_BADARG = -1,      /* NULL pointer, size out of range, k outside 1..NWK_MAX_K, r_cap not > 0, a grid outside its limits */
    NWK_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwk_last_error */
    NWK_ERR_NONFINITE = -3,   /* a non-finite coordinate in the cloud or in a query */
    NWK_ERR_NOMEM = -4,
    NWK_ERR_NOCLOUD = -5      /* a query while the context holds no cloud; nwk_field_ptr before nwk_node_field */
} nwk_status;

int nwk_abi_version(void);
int nwk_create(int device, nwk_ctx **out);
void nwk_destroy(nwk_ctx *ctx);
const char *nwk_last_error(nwk_ctx *ctx);

/* Takes a copy of the cloud into the context and bins it, where it stays for any number of queries (until the next nwk_set_cloud; a
 * failed call leaves the context without a cloud).  on_device = 0: a host pointer, checked for finiteness on the host before any HIP
 * call; 1: a device pointer, checked by the bounding-box kernel.  A query with a finite cap bins the cloud again if the cap asks for
 * another cell size than the grid at hand has. */
int nwk_set_cloud(nwk_ctx *ctx, const float *xyz, int64_t n, int on_device);

/* out_host[q] = min(r_k(queries[q]), r_cap) for (nq,3) float32 queries, a host pointer (queries_on_device = 0, checked on the host) or
 * a device pointer (1, checked by the kernel).  1 <= nq <= 2^30. */
int nwk_kth_distance(nwk_ctx *ctx, const float *queries, int64_t nq, int queries_on_device, int k, double r_cap, double *out_host);

/* The same for the nodes of a voxel lattice, given as nwi_density takes it: node (i, j, k) lies at
 * (double)lo[a] + ((double)index + 0.5) * (double)h along axis a, and
 *     field[(k dims[1] + j) dims[0] + i] = (uint64) floor((r_cap - min(r_k, r_cap)) * 2^20),
 * the layout nwi_extract reads (x fastest; a larger value is further inside).  r_cap must be finite and at most 2^40; the grid has
 * nwi_density's limits (3 <= dims[a] <= 2^20, at most 2^30 nodes, h > 0, everything finite).  The field stays on the device;
 * field_host (may be NULL) receives a copy. */
int nwk_node_field(nwk_ctx *ctx, const float *lo, float h, const int32_t *dims, int k, double r_cap, uint64_t *field_host);

/* The device pointer of the last nwk_node_field's field (complete: that call synchronized), NULL if there is none.  It is valid until
 * the context's next nwk_node_field or its destruction. */
const uint64_t *nwk_field_ptr(nwk_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif
