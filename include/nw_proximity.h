/*
 * nw_proximity.h -- C-ABI of the exact distance between two triangle meshes in libnanowrap_hip.so (csrc/nw_proximity.hip, MI355X / gfx950).
 *
 * What it is for: contact sites between two fitted membranes (ER against mitochondria, ER against plasma membrane, two vesicles) --
 * where two surfaces come within d nm of each other, how large that patch is and what the gap is there.  nwd_query of A's vertices
 * against B answers another question: it overestimates the gap wherever the nearest approach lies inside a face or between two edges,
 * and it reports a positive distance for two surfaces that pass through each other between their vertices.  PYME is not part of the
 * reference tree and upstream has no such module, so the definitions here are this project's own:
 *   nwm_set_mesh  -- takes mesh B into the context: per-face centroids and radii in float64, binned into the query units' shared grid;
 *   nwm_query     -- for every face of mesh A the exact distance to the nearest face of B (triangle against triangle: vertex-face,
 *                    edge-edge and piercing), that face, which kind of pair it is and one closest point on each mesh, within a band.
 *
 * Definition (csrc/nw_proximity_core.h holds it as code, tests/mesh_proximity_ref.py restates it by brute force over all pairs).
 *   nwm_tri_tri(A, B), float64 on the float32 positions, nothing contracted:
 *     piercing (both faces with n.n > 0): nwx_seg_tri of A's three edges against B, then of B's three against A; at the first that holds
 *       d2 = +0.0, kind 0, both closest points the piercing point;
 *     otherwise the smallest of: nwd_point_triangle(A_k, B) (kinds 1-3), nwd_point_triangle(B_k, A) (kinds 4-6), and the edge pairs
 *       (i of A, j of B) whose closest points are interior to both (kinds 7 + 3i + j); a later candidate wins only when strictly nearer.
 *   Per face f of A, with a band d_cap (positive, +inf allowed): the minimum over all faces g of B, the smallest g among equal d2.
 *     in band (sqrt(d2) <= d_cap):  distance = sqrt(d2), partner = g, kind, closest_a, closest_b;
 *     out of band:                  distance = +inf, partner = -1, kind = -1, closest points NaN.
 *   Nothing in the result depends on the cell size, the launch geometry or the order of B's faces beyond the tie rule.  The function
 *   is not promised to be symmetric bit for bit (the edge-edge roles swap): A against B and B against A are two calls.  A mesh against
 *   itself is out of scope: every face would find itself at 0.
 *
 * Conventions (as include/nw_distance.h, with its own prefix and context):
 *   - every call returns NWM_OK (0) or a negative status; nwm_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before anything is uploaded or launched; without a GPU nwm_create fails with NWM_ERR_HIP --
 *     there is no CPU fallback;
 *   - mesh arrays are HOST pointers (float32 / int32, row-major, C-contiguous), outputs are host pointers in the order of A's faces;
 *   - the unit's own kernels (k_mm_*) use no atomics and no scratch, offsets are 64-bit, and every per-face result -- distance, partner,
 *     kind, closest points -- and every counter but one is deterministic and a function of the input alone.  The exception is
 *     NWM_INFO_TESTS: the query units' shared grid bins B's centroids with an atomic cursor per cell (nw_bq.hip), so the order of the
 *     centroids within a cell may differ from one binning to the next, and how many exact tests the bounds spare depends on that
 *     order.  Two queries on one grid give the same count;
 *   - one nwm_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 *
 * How the query stays exact.  Every face has a centroid c and rho, the largest distance from c to a corner; rho_max is the largest
 * rho of B.  Face f of A walks rings of B's centroid grid around the cell of c_f.  A centroid in ring r belongs to a face at least
 * sqrt(lbd^2 + out^2) - rho_f - rho_max away (lbd = (r - 1) h, out = c_f's distance from the grid's box); the walk ends when that is
 * strictly more than min(best, d_cap).  A far face stops after ceil((d_cap + rho_f + rho_max) / h) + 1 rings with nothing found; a
 * candidate is passed over without the exact test when |c_f - c_g| - rho_g - rho_f is more than min(best, d_cap).  The cell size is
 * this unit's own choice, max(2 m, min((d_cap + rho_max) / 2, 16 m)) with m the mean rho of B (so 16 m without a band: chosen by
 * measurement, profiles/proximity.txt), unless nwm_set_mesh names one; the centroids are binned again when the band asks for another
 * size.
 * What one mis-shaped face costs: a face much larger than the others, in either mesh, raises rho_f (for its own walk) or rho_max (for
 * every walk), which then covers ceil((rho_f + rho_max + distance) / h) + 1 rings and reads every centroid in them; the exact test is
 * still skipped by the faces' own radii.  In the worst case that is every cell and every centroid for every face: slow, never inexact.
 */
#ifndef NW_PROXIMITY_H_
#define NW_PROXIMITY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWM_ABI_VERSION 1

/* kind_out: 0 = an edge of one face pierces the other; 1-3 corner k of A's face against B's face; 4-6 corner k of B's face against A's;
 * 7 + 3i + j = the interiors of edge i of A's face and edge j of B's; -1 out of band */
#define NWM_KIND_PIERCED 0
#define NWM_KIND_EDGE_EDGE 7

/* info_out of nwm_query: NWM_INFO_WORDS int64 values */
#define NWM_INFO_WORDS 7
#define NWM_INFO_IN_BAND 0        /* the faces of A in band */
#define NWM_INFO_AT_ZERO 1        /* those of them at distance 0 */
#define NWM_INFO_RINGS 2          /* rings walked, summed over A's faces */
#define NWM_INFO_CENTROIDS 3      /* centroids of B read, summed over A's faces */
#define NWM_INFO_TESTS 4          /* exact pair tests, summed over A's faces (how many the bounds spare depends on the order of the centroids within a cell, which a new binning may change; no result does) */
#define NWM_INFO_CELLS 5          /* the cells of the centroid grid the call used */
#define NWM_INFO_CELL_SIZE 6      /* its cell size: the bits of a double */

typedef struct nwm_ctx nwm_ctx;

typedef enum nwm_status {
    NWM_OK = 0,
    NWM_ERR_BADARG = -1,      /* NULL pointer, size out of range, a face index outside the vertices, a cell size that is negative or not finite, a band that is not positive */
    NWM_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwm_last_error */
    NWM_ERR_NONFINITE = -3,   /* a non-finite vertex position */
    NWM_ERR_NOMEM = -4,
    NWM_ERR_NOMESH = -5       /* nwm_query while the context holds no mesh */
} nwm_status;

int nwm_abi_version(void);
int nwm_create(int device, nwm_ctx **out);
void nwm_destroy(nwm_ctx *ctx);
const char *nwm_last_error(nwm_ctx *ctx);

/* Takes mesh B into the context, where it stays for any number of queries (until the next nwm_set_mesh; a failed call leaves the
 * context without a mesh).  cell_size: the cell size every query's grid starts from, or 0 for the unit's choice.  Checked on the host
 * first: sizes, face indices, cell_size >= 0 and finite (NWM_ERR_BADARG); positions finite (NWM_ERR_NONFINITE). */
int nwm_set_mesh(nwm_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double cell_size);

/* Mesh A against the mesh in the context, one result per face of A: distance_out float64, partner_out int32, kind_out int32,
 * closest_a_out and closest_b_out float64 triples; info_out int64[NWM_INFO_WORDS].  Any output may be NULL.  d_cap > 0, +inf allowed.
 * The same host checks of A as nwm_set_mesh makes of B. */
int nwm_query(nwm_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double d_cap, double *distance_out,
              int32_t *partner_out, int32_t *kind_out, double *closest_a_out, double *closest_b_out, int64_t *info_out);

#ifdef __cplusplus
}
#endif

#endif
