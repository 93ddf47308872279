/*
 * nw_rays.h -- C-ABI of exact ray casting against a triangle mesh in libnanowrap_hip.so (csrc/nw_rays.hip, MI355X / gfx950).
 *
 * What it is for: how wide a fitted structure is at a place -- a tube's diameter, a sheet's thickness, the gap to the next membrane --
 * is the length of a ray along the inward normal to the first face it meets.  Every other query unit asks about a ball around a
 * point; this one follows a line through the mesh.  The parity of the faces a ray hits is also a third way to a point's side,
 * independent of the distance unit's pseudonormals and of the winding number.  PYME is not part of the reference tree, so the
 * definition is this project's own (csrc/nw_rays_core.h: float64 on the float32 positions, a written-down order of operations):
 *   - a ray is an origin, a direction of any finite length and two optional ids, a vertex and a face to pass over (-1 for none; ids
 *     are compared, never positions); a direction whose length sqrt(d.d) is zero in float64 -- the zero vector, and any shorter than
 *     about 1e-162 -- hits nothing.  No other length is special: the walk follows the direction scaled by its largest component, so
 *     it is as exact and as short at |d| = 1e-160 or 1e300 as at 1 (what the definition's own products make of such a d -- an
 *     overflowing w or t hits nothing -- is the definition, and the walk gives the same);
 *   - the edge test is INCLUSIVE, so no ray leaks through an edge or a vertex of a closed mesh; a flat face is never hit; t > 0 and
 *     t <= t_max; the hit point must lie in the ball of the face (centroid, largest corner distance a hair enlarged);
 *   - per ray: t of the nearest hit (+inf for none), its face (equal t: the smallest id; -1 for none), an info word whose bit 0 says
 *     that the ray leaves through the face's back (n.d > 0), and on request the number of faces hit.  A ray that meets an edge or a
 *     vertex in rounded arithmetic counts every face of the fan: the count is a function of the input and equals the number of
 *     crossings only off such rays.
 *   nwc_set_mesh  -- takes a mesh into the context: per-face centroids and radii in float64, binned into the query units' shared cell grid;
 *   nwc_cast      -- casts n rays against it, one lane per ray.
 *
 * Conventions (as include/nw_distance.h, with its own prefix and context):
 *   - every call returns NWC_OK (0) or a negative status; nwc_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked before any of them is uploaded (host arrays on the host; rays given as device memory by a reduction
 *     there), and a call that fails later returns only once the stream is idle; without a GPU nwc_create fails with NWC_ERR_HIP --
 *     there is no CPU fallback;
 *   - mesh arrays and outputs are HOST pointers (float32 / float64 / int32, row-major, C-contiguous); origins, directions and the two
 *     skip arrays may each be a host pointer or device memory, which is then read in place;
 *   - every result is deterministic and a function of the input alone: no atomics, one lane per ray;
 *   - one nwc_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 *
 * How the search stays exact (the argument in full: csrc/nw_rays_core.h).  Every face g has a centroid c_g and rho_g, so a hit point
 * of g lies within rho_g <= rho_max of c_g.  The ray is clipped by slabs against the centroids' box dilated by rho_max (and a slack);
 * its arc length inside is cut into pieces of one cell size; each piece visits the cells that overlap a box of half-width
 * h / 2 + rho_max around its midpoint and examines the centroids whose arc coordinate along the ray falls into that piece -- so a
 * face is examined at most once, and a face that can be hit is examined, since its centroid is within rho_g of the line and of the
 * hit's arc coordinate.  Without NWC_COUNT the walk stops before a piece that begins more than rho_max (and the slack) beyond the best
 * hit.  Every slack is relative and seven orders above the rounding it covers.
 * What one mis-shaped face costs: a face much larger than the others raises rho_max, every piece's box then covers the whole grid and
 * every ray reads every centroid once per piece: O(pieces x F) per ray, slow but never inexact.  There is no DDA and no list of
 * oversize faces.  The slack grows with the coordinates of the origin and of the mesh; a cast whose slack would exceed one cell
 * (coordinates beyond 1e9 cell sizes) is refused with NWC_ERR_BADARG rather than walked.
 */
#ifndef NW_RAYS_H_
#define NW_RAYS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWC_ABI_VERSION 1

/* flags of nwc_cast */
#define NWC_COUNT 1               /* the faces hit are counted into hits_out: the walk does not stop at the first hit */
#define NWC_STATS 2               /* pieces walked, centroids read and exact tests are summed over the rays (nwc_get_stats) */

/* the info word */
#define NWC_INFO_EXITS 1          /* the ray leaves through the back of the face it hits first (n.d > 0) */

typedef struct nwc_ctx nwc_ctx;

typedef enum nwc_status {
    NWC_OK = 0,
    NWC_ERR_BADARG = -1,      /* NULL pointer, size out of range, a face index outside the vertices, an unknown flag, t_max negative or NaN,
                                 coordinates beyond 1e9 cell sizes */
    NWC_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwc_last_error */
    NWC_ERR_NONFINITE = -3,   /* a non-finite vertex position, origin or direction */
    NWC_ERR_NOMEM = -4,
    NWC_ERR_NOMESH = -5       /* nwc_cast while the context holds no mesh */
} nwc_status;

int nwc_abi_version(void);
int nwc_create(int device, nwc_ctx **out);
void nwc_destroy(nwc_ctx *ctx);
const char *nwc_last_error(nwc_ctx *ctx);

/* Takes the mesh into the context, where it stays for any number of calls (until the next nwc_set_mesh; a failed call leaves the
 * context without a mesh).  Checked on the host first: sizes and face indices (NWC_ERR_BADARG), positions finite (NWC_ERR_NONFINITE).
 * 3 <= n_vertices <= 2^30, 1 <= n_faces <= 2^29. */
int nwc_set_mesh(nwc_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces);

/* Casts n rays (1 <= n <= 2^30): origin and dir are (n,3) float64, skip_vertex and skip_face int32[n] or NULL, t_max >= 0 (+inf
 * allowed) the same for every ray.  t_out float64[n], face_out, info_out, hits_out int32[n]; any of them may be NULL.  hits_out is
 * filled with NWC_COUNT only (NWC_ERR_BADARG without it); t, face and info do not depend on the flags. */
int nwc_cast(nwc_ctx *ctx, const double *origin, const double *dir, int64_t n, const int32_t *skip_vertex, const int32_t *skip_face,
             double t_max, int flags, double *t_out, int32_t *face_out, int32_t *info_out, int32_t *hits_out);

/* out[0] = the pieces walked, out[1] = the centroids read, out[2] = the faces that reached the exact test, summed over the rays of
 * the last nwc_cast with NWC_STATS (zeros otherwise). */
int nwc_get_stats(nwc_ctx *ctx, int64_t out[3]);

#ifdef __cplusplus
}
#endif

#endif
