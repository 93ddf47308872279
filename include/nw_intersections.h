/*
 * nw_intersections.h -- C-ABI of the self-intersection check of a triangle mesh in libnanowrap_hip.so (csrc/nw_intersections.hip,
 * MI355X / gfx950).
 *
 * What it is for: "closed and manifold" are statements about the face array alone; a surface can be both and still pass through
 * itself, with a wrong signed volume, wrong winding numbers and a wrong sign of its distance field.  This unit answers the third
 * question, embedded or not, at full mesh size: which pairs of faces cross.  PYME is not part of the reference tree, so the
 * definition is this project's own (csrc/nw_intersections_core.h: float64 on the float32 positions, a written-down order of
 * operations):
 *   - a crossing is PROPER: the interior of an edge of one face passes through the interior of the other face;
 *   - touching, coplanar overlap and faces that share an edge (two vertex ids) are not crossings, a flat face neither crosses nor is
 *     crossed; faces that share one vertex id are tested with the edges opposite that vertex;
 *   - vertices are the same when their ids are: positions are never compared.
 *   nwx_set_mesh  -- takes a mesh into the context: per-face centroids and radii in float64, binned into the query units' shared cell grid;
 *   nwx_find      -- for every face the number of faces it crosses, the number of crossing pairs and of crossed faces, and on request
 *                    the list of pairs;
 *   nwx_get_pairs -- copies that list out, sorted.
 *
 * Conventions (as include/nw_distance.h, with its own prefix and context):
 *   - every call returns NWX_OK (0) or a negative status; nwx_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before anything is uploaded or launched; without a GPU nwx_create fails with NWX_ERR_HIP --
 *     there is no CPU fallback;
 *   - mesh arrays and outputs are HOST pointers (float32 / int32 / int64, row-major, C-contiguous);
 *   - every result is deterministic and a function of the input alone: a pair is always evaluated with the smaller face id first, so
 *     both of its faces get the same bit whichever thread computes it; counts need no atomics; the list is sorted;
 *   - one nwx_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 *
 * How the search stays exact.  Every face f has a centroid c_f and rho_f, the largest distance from c_f to a corner (a hair enlarged),
 * so the whole face lies within rho_f of c_f; rho_max is the largest rho_f.  Faces f and g can only meet if
 * |c_f - c_g| <= rho_f + rho_g <= rho_f + rho_max, so the lane of face f visits the cells that overlap the box c_f +- (rho_f + rho_max),
 * clamped to the grid -- a bounded box, not a walk that widens -- and passes over a centroid with |c_f - c_g| (1 - slack) - rho_g > rho_f.
 * Every other face g != f gets the exact predicate.
 * What one mis-shaped face costs: a face much larger than the others raises rho_max for every lane, whose box then spans
 * (2 (rho_f + rho_max) / h + 1)^3 cells instead of a few dozen, and every centroid in them is read (32 bytes and one square root each;
 * the predicate is still skipped by the faces' own radii).  In the worst case -- a face spanning the mesh -- that is every cell and
 * every centroid for every face: O(cells + F) per face, slow but never inexact.  There is no list of oversize faces.
 */
#ifndef NW_INTERSECTIONS_H_
#define NW_INTERSECTIONS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWX_ABI_VERSION 1

/* flags of nwx_find */
#define NWX_PAIRS 1               /* the crossing pairs are listed as well (nwx_get_pairs) */
#define NWX_STATS 2               /* the candidates read and the candidates that reached the predicate are counted (nwx_get_stats) */

/* the longest list nwx_find makes */
#define NWX_MAX_PAIRS 16777216

typedef struct nwx_ctx nwx_ctx;

typedef enum nwx_status {
    NWX_OK = 0,
    NWX_ERR_BADARG = -1,      /* NULL pointer, size out of range, a face index outside the vertices, an unknown flag, a capacity below n_pairs */
    NWX_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwx_last_error */
    NWX_ERR_NONFINITE = -3,   /* a non-finite vertex position */
    NWX_ERR_NOMEM = -4,
    NWX_ERR_NOMESH = -5,      /* nwx_find while the context holds no mesh */
    NWX_ERR_TOOMANY = -6,     /* NWX_PAIRS and more than NWX_MAX_PAIRS pairs: the counts and totals are delivered, there is no list */
    NWX_ERR_NOPAIRS = -7      /* nwx_get_pairs while the context holds no list */
} nwx_status;

int nwx_abi_version(void);
int nwx_create(int device, nwx_ctx **out);
void nwx_destroy(nwx_ctx *ctx);
const char *nwx_last_error(nwx_ctx *ctx);

/* Takes the mesh into the context, where it stays for any number of calls (until the next nwx_set_mesh; a failed call leaves the
 * context without a mesh).  Checked on the host first: sizes and face indices (NWX_ERR_BADARG), positions finite (NWX_ERR_NONFINITE).
 * 3 <= n_vertices <= 2^30, 1 <= n_faces <= 2^29. */
int nwx_set_mesh(nwx_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces);

/* count_out[f] = the number of faces that face f crosses (int32[n_faces], or NULL), *n_pairs_out = the number of unordered crossing
 * pairs, *n_crossed_faces_out = the number of faces with count > 0; either may be NULL.  With NWX_PAIRS the pairs are also listed in
 * the context.  Counts and totals do not depend on the flags. */
int nwx_find(nwx_ctx *ctx, int flags, int32_t *count_out, int64_t *n_pairs_out, int64_t *n_crossed_faces_out);

/* Copies the list of the last nwx_find with NWX_PAIRS: pairs_out[2i], pairs_out[2i+1] = f < g, sorted by (f, g).  capacity: the pairs
 * that pairs_out holds; NWX_ERR_BADARG, with nothing written, if that is fewer than n_pairs. */
int nwx_get_pairs(nwx_ctx *ctx, int32_t *pairs_out, int64_t capacity);

/* out[0] = the candidates (ordered pairs f, g != f whose centroids a lane read), out[1] = those that reached the predicate, of the
 * last nwx_find with NWX_STATS (zeros otherwise). */
int nwx_get_stats(nwx_ctx *ctx, int64_t out[2]);

#ifdef __cplusplus
}
#endif

#endif
