/*
 * nw_distance.h -- C-ABI of the exact distance from points to a triangle mesh in libnanowrap_hip.so (csrc/nw_distance.hip, MI355X / gfx950).
 *
 * What it is for: the distance of every localization from a fitted membrane, with a sign for the side it lies on.  Upstream users get
 * this from PYME's DistanceToMesh module; PYME is not part of the reference tree, so the definitions here are this project's own:
 *   nwd_set_mesh  -- takes a mesh (and, for signs, its half-edge twin table) into the context: per-face centroids in float64, binned
 *                    into the query units' shared cell grid;
 *   nwd_query     -- for every query point the exact distance to the nearest point of the mesh's triangles, that point, the face it
 *                    lies on, which feature of the face it is (interior, edge, vertex) and the sign from the angle-weighted
 *                    pseudonormal of that feature (Baerentzen & Aanaes 2005), which is right at edges and vertices where the nearest
 *                    face's own normal is not.
 * The arithmetic is csrc/nw_distance_core.h (float64 on the float32 positions, a written-down order of operations).
 *
 * Conventions (as include/nw_evaluation.h, with its own prefix and context):
 *   - every call returns NWD_OK (0) or a negative status; nwd_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before anything is uploaded or launched; without a GPU nwd_create fails with NWD_ERR_HIP --
 *     there is no CPU fallback;
 *   - mesh arrays are HOST pointers (float32 / int32, row-major, C-contiguous); half-edge 3f+k runs faces[f][k] -> faces[f][(k+1)%3];
 *   - the queries are (n,3) float64, row-major, a host pointer or a device pointer; a device pointer is read on the context's own
 *     stream with no ordering against the stream that wrote it: it must be complete before the call and unchanged until it returns;
 *   - outputs are host pointers, in the caller's order;
 *   - every result is deterministic and a function of the input alone: ties between faces go to the smallest face id, the sum has a
 *     fixed reduction order, pseudonormals are computed inside the query (no atomics, no precomputed vertex normals);
 *   - one nwd_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 *
 * How the query stays exact.  Every face f has a centroid c_f and rho_f, the largest distance from c_f to a corner, so the whole face
 * lies within rho_f of c_f; rho_max is the largest rho_f.  A query walks rings of cells around its own (the cell of its projection
 * onto the grid's box, if it lies outside).  A centroid in ring r is at least lbd = (r - 1) h away from the projection along one axis,
 * so its face is at least sqrt(lbd^2 + out^2) - rho_max from the query (out = the query's distance from the box); the walk ends when
 * that is strictly more than the best distance found, so equally near faces are all seen.  A candidate face is skipped without the
 * exact test when |p - c_f| - rho_f is more than the best distance.
 * What one mis-shaped face costs: a face much larger than the others raises rho_max for every query, which then walks
 * ceil((rho_max + distance) / h) + 1 rings instead of two or three and reads every centroid in them (32 bytes and one square root each;
 * the exact test is still skipped by the face's own rho_f).  In the worst case -- a face spanning the mesh -- that is every cell and
 * every centroid for every query: O(cells + F) per query, slow but never inexact.  There is no list of oversize faces.
 */
#ifndef NW_DISTANCE_H_
#define NW_DISTANCE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWD_ABI_VERSION 1

/* flags of nwd_query */
#define NWD_SIGNED 1              /* dist_out carries the sign of the side: negative inside an outward-oriented closed mesh; needs a twin table */
#define NWD_RINGS 2               /* feature_out also carries, in bits 8..15, the ring at which the query's walk ended (at most 255) */

/* feature_out: bits 0..2 = 0 interior, 1..3 edge k (strictly inside it), 4..6 vertex k of the face; bit 3 = the fan walk around the
 * vertex was cut short at 256 faces (the sign is then from a partial fan) */
#define NWD_FEATURE_MASK 7
#define NWD_FEATURE_CAPPED 8

typedef struct nwd_ctx nwd_ctx;

typedef enum nwd_status {
    NWD_OK = 0,
    NWD_ERR_BADARG = -1,      /* NULL pointer, size out of range, a face index outside the vertices, a twin table that is not an involution, NWD_SIGNED without a twin table */
    NWD_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwd_last_error */
    NWD_ERR_NONFINITE = -3,   /* a non-finite vertex position or query coordinate */
    NWD_ERR_NOMEM = -4,
    NWD_ERR_NOMESH = -5       /* nwd_query while the context holds no mesh */
} nwd_status;

int nwd_abi_version(void);
int nwd_create(int device, nwd_ctx **out);
void nwd_destroy(nwd_ctx *ctx);
const char *nwd_last_error(nwd_ctx *ctx);

/* Takes the mesh into the context, where it stays for any number of queries (until the next nwd_set_mesh; a failed call leaves the
 * context without a mesh).  twin: int32[3 n_faces], twin[h] = the half-edge opposite to h or -1 on a border; or NULL for a mesh that
 * is only queried unsigned.  Checked on the host first: sizes, face indices, every twin entry -1 or in [0, 3F) with
 * twin[twin[h]] == h (NWD_ERR_BADARG); positions finite (NWD_ERR_NONFINITE). */
int nwd_set_mesh(nwd_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin);

/* For every query point: dist_out[q] = sqrt(d2) of the nearest point of the mesh (negative with NWD_SIGNED where the point lies on
 * the inner side; a distance of 0 is +0.0), closest_out[3q..] that point, face_out[q] its face (the smallest id among equally near
 * faces), feature_out[q] the feature code, *sum_sq_out = the sum of dist_out[q]^2 in a fixed reduction order.  Any output may be NULL.
 * 1 <= n <= 2^30. */
int nwd_query(nwd_ctx *ctx, const double *xyz, int64_t n, int flags, double *dist_out, double *closest_out, int32_t *face_out,
              int32_t *feature_out, double *sum_sq_out);

#ifdef __cplusplus
}
#endif

#endif
