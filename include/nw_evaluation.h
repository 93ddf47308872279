/*
 * nw_evaluation.h -- C-ABI of the fit-quality metric in libnanowrap_hip.so (csrc/nw_evaluation.hip, MI355X / gfx950).
 *
 * What it stands in for: the two functions behind upstream's evaluation recipe modules (ch_shrinkwrap/evaluation_utils.py,
 * surfaced by recipe_modules/surface_feature_extraction.py:76-138), which upstream runs as a Python loop over the triangles and scipy's cKDTree:
 *   nwe_sample_mesh               -- points_from_mesh (:35-150) with p = 1: a regular grid in every triangle's own plane, the nodes inside it;
 *                                    the arrays are those of ch_shrinkwrap_amd/evaluation.py's points_from_mesh, bit for bit and in its order;
 *   nwe_nearest                   -- the exact nearest neighbour of every query point in a reference cloud, float64;
 *   nwe_average_squared_distance  -- average_squared_distance (:153-180): both directions in one call.
 *
 * Conventions (as include/nw_holepunch.h, with its own prefix and context):
 *   - every call returns NWE_OK (0) or a negative status; nwe_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked before any HIP call; without a GPU nwe_create fails with NWE_ERR_HIP -- there is no CPU fallback;
 *   - mesh arrays are HOST pointers (float32 / int32, row-major, C-contiguous);
 *   - a cloud is (n,3) float64, row-major, and may be a host pointer, a device pointer, or -- pointer NULL and n = NWE_SAMPLES -- the
 *     samples the context holds since the last nwe_sample_mesh, which never leave the device unless nwe_get_samples asks for them;
 *   - a device cloud is read on the context's own stream, with no ordering against the stream that wrote it: it must be complete
 *     (its producer synchronized) before the call, and must not change until the call returns;
 *   - outputs are host pointers;
 *   - every result is deterministic: the same bytes on every run (ties go to the smallest index; sums have a fixed reduction order);
 *   - one nwe_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_EVALUATION_H_
#define NW_EVALUATION_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWE_ABI_VERSION 1
#define NWE_SAMPLES (-1)          /* the size that, with a NULL pointer, names the samples the context holds */
#define NWE_MAX_NODES (1ll << 30) /* the most grid nodes (inside their triangle or not) one nwe_sample_mesh tests */

typedef struct nwe_ctx nwe_ctx;

typedef enum nwe_status {
    NWE_OK = 0,
    NWE_ERR_BADARG = -1,      /* NULL pointer, an empty cloud, size out of range, an index outside its array, a non-positive or non-finite dx */
    NWE_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwe_last_error */
    NWE_ERR_NONFINITE = -3,   /* a non-finite coordinate in a cloud */
    NWE_ERR_NOMEM = -4,
    NWE_ERR_NOSAMPLES = -5,   /* NWE_SAMPLES (or nwe_get_samples) while the context holds no samples */
    NWE_ERR_TOOMANY = -6      /* the faces' grids have more than NWE_MAX_NODES nodes: dx is too small for this mesh */
} nwe_status;

int nwe_abi_version(void);
int nwe_create(int device, nwe_ctx **out);
void nwe_destroy(nwe_ctx *ctx);
const char *nwe_last_error(nwe_ctx *ctx);

/* Every face f (corners pos[faces[3f+0..2]]) gets the grid of spacing dx in its own plane -- axes e0 = the first edge, e1 = normal x e0,
 * origin at the offset upstream uses -- and the nodes strictly inside it are kept.  The per-triangle set-up is float32, the nodes and
 * their positions float64, as NumPy evaluates upstream's expressions for a float32 mesh.  Faces of zero area are left out.  The samples
 * stay on the device, ordered by face and row-major within a face; *n_out = their number (0 is a valid result: the context then holds
 * no samples).  A failed call leaves the context without samples. */
int nwe_sample_mesh(nwe_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double dx, int64_t *n_out);

/* The samples the context holds: positions (n,3) float64 and the face each came from (n) int32.  Either may be NULL. */
int nwe_get_samples(nwe_ctx *ctx, double *positions_out, int32_t *face_out);

/* For every query point the nearest point of the reference cloud: dist_out[q] = sqrt((dx*dx + dy*dy) + dz*dz) in float64, idx_out[q] its
 * index (the smallest one among equally near points), *sum_sq_out = the sum of dist_out[q]^2 over the queries, reduced in a fixed order.
 * Any output may be NULL.  The reference cloud is binned into a cell grid by a counting sort; each query walks rings of cells around its
 * own until the ring's lower bound exceeds the best squared distance found, so the result is exact. */
int nwe_nearest(nwe_ctx *ctx, const double *reference, int64_t n_reference, const double *queries, int64_t n_queries,
                double *dist_out, int32_t *idx_out, double *sum_sq_out);

/* *mse01_out = the mean squared distance of points1 from their nearest neighbours in points0, *mse10_out = the same of points0 from
 * points1 (upstream's average_squared_distance returns them in this order). */
int nwe_average_squared_distance(nwe_ctx *ctx, const double *points0, int64_t n0, const double *points1, int64_t n1,
                                 double *mse01_out, double *mse10_out);

#ifdef __cplusplus
}
#endif

#endif
