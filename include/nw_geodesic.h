/*
 * nw_geodesic.h -- C-ABI of the distance along a mesh in libnanowrap_hip.so (csrc/nw_geodesic.hip, MI355X / gfx950): the geodesic
 * graph distance of every vertex from a set of source vertices, and which source it belongs to.
 *
 * What it is for: how far along the fitted membrane a vertex is from the nearest contact site, how a density falls off with that
 * distance, which contact site a piece of membrane belongs to.  Every other query unit measures through space; a straight line cuts
 * through the lumen and across the gap between two sheets.  Upstream answers such questions by skeletonisation, which is out of scope;
 * PYME is not in the reference tree, so the definition is this project's own and is written down in csrc/nw_geodesic_core.h.
 *
 * THIS IS A GRAPH DISTANCE WITH ONE LEVEL OF UNFOLDING, NOT AN EXACT POLYHEDRAL GEODESIC (no MMP, no heat method).  Every value is the
 * length of a real path on the surface: an upper bound of the geodesic, never below the Euclidean distance.
 *
 * Definitions (all arithmetic in float64 on the float32 positions, nothing contracted):
 *   - the mesh is (n_vertices,3) float32 positions, a host or a device pointer, and (n_faces,3) int32 faces, a host pointer;
 *     1 <= n_vertices <= 2^30, 1 <= n_faces <= 2^29; twin, optional, is (3 n_faces) int32 on the host: twin[3f+k] is the half-edge that
 *     runs the other way along the edge faces[f][k] -> faces[f][(k+1)%3], or -1 on a border; it must be mutual;
 *   - arcs: every edge {u, v} of a face, in both directions, border edges too, weight sqrt((dx dx + dy dy) + dz dz) (+0.0 for a
 *     zero-length edge).  With NWT_FLAG_DIAGONALS (needs the twin table) also, across every interior edge, the segment between the two
 *     opposite corners in the plane into which the two faces unfold, where that segment crosses the edge strictly between its ends and
 *     both faces have a height (csrc/nw_geodesic_core.h: nwt_diagonal_weight);
 *   - sources: n_sources >= 1 vertex ids, duplicates allowed, each with a start value d0 >= 0, finite (NULL: all zeros);
 *   - D is the least fixed point (from +inf) of D[v] = min(d0 of v's own sources, fl(D[u] + w) over arcs u -> v with D[u] <= d_cap):
 *     unique, independent of the order of relaxations, equal to Dijkstra's result with the same rounded additions (proof in the core
 *     header).  d_cap > 0, +inf allowed;
 *   - distance_out[v] = D[v] where D[v] <= d_cap, else +inf; a vertex no source reaches is +inf;
 *   - source_out, optional: S[v] = the smallest index i (into source_ids) from which a walk of tight arcs (fl(D[u] + w) == D[v])
 *     leads to v, starting at a source with d0_i == D[its vertex]; -1 where distance_out is +inf.  Defined by this rule, which with
 *     rounded sums need not be "the source of some shortest walk";
 *   - both outputs are functions of the positions, the oriented face set, the sources and the cap alone: not of launch geometry,
 *     batch size or the order of the faces.
 *
 * How it is computed.  nwt_set_mesh computes the weights once (k_gd_weights, one lane per half-edge).  nwt_distances seeds D (k_gd_seed,
 * 64-bit unsigned atomic min on the bit pattern, which orders as the value for non-negative doubles), then launches rounds of
 * k_gd_relax: one lane per half-edge relaxes one arc in both directions where one of its two vertices changed in the round before.
 * Rounds are launches; no workgroup ever waits on another.  The host reads the rounds' changed words once per NWT_BATCH rounds and
 * stops after a round that changed nothing; more than n_vertices + NWT_BATCH rounds is NWT_ERR_INTERNAL.  Labels, if asked for, are
 * rounds of k_gd_labels on the final D.  k_gd_finish applies the cap.  Expect it to be bound by launches and rounds, not by bandwidth.
 *
 * info[]: HALFEDGES, DIAGONALS, REACHED and IN_BAND are functions of the input.  ROUNDS, LABEL_ROUNDS, LAUNCHES, LOWERED and RELAXED
 * depend on the order in which the hardware runs workgroups: THEY ARE NOT DETERMINISTIC and belong in no bit comparison.
 *
 * Conventions (as include/nw_pairs.h, with its own prefix and context):
 *   - every call returns NWT_OK (0) or a negative status; nwt_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call, and nothing is written on refusal; without a GPU nwt_create fails with
 *     NWT_ERR_HIP -- there is no CPU fallback;
 *   - a device pointer is read on the context's own stream with no ordering against the stream that wrote it: it must be complete
 *     before the call and unchanged until it returns;
 *   - one nwt_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_GEODESIC_H_
#define NW_GEODESIC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWT_ABI_VERSION 1
#define NWT_FLAG_DIAGONALS 1

/* info[]: int64 words */
#define NWT_INFO_WORDS 10
#define NWT_INFO_HALFEDGES 0        /* 3 * n_faces */
#define NWT_INFO_DIAGONALS 1        /* diagonals that exist (0 without NWT_FLAG_DIAGONALS) */
#define NWT_INFO_REACHED 2          /* vertices with D < +inf */
#define NWT_INFO_IN_BAND 3          /* vertices with D <= d_cap */
#define NWT_INFO_ROUNDS 4           /* not deterministic: rounds of k_gd_relax */
#define NWT_INFO_LABEL_ROUNDS 5     /* not deterministic: rounds of k_gd_labels */
#define NWT_INFO_LAUNCHES 6         /* not deterministic: kernel launches of the call */
#define NWT_INFO_LOWERED 7          /* not deterministic: atomics that lowered a value */
#define NWT_INFO_RELAXED 8          /* not deterministic: arcs a lane looked at, all rounds */
#define NWT_INFO_BATCH 9            /* rounds per read of the changed words */

typedef struct nwt_ctx nwt_ctx;

typedef enum nwt_status {
    NWT_OK = 0,
    NWT_ERR_BADARG = -1,      /* NULL pointer, size or id out of range, bad d0 or d_cap, diagonals without a twin table, twins not mutual */
    NWT_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwt_last_error */
    NWT_ERR_NONFINITE = -3,   /* a non-finite position */
    NWT_ERR_NOMEM = -4,
    NWT_ERR_NOMESH = -5,      /* nwt_distances before nwt_set_mesh */
    NWT_ERR_INTERNAL = -6     /* the rounds did not end within n_vertices + NWT_BATCH: cannot happen */
} nwt_status;

int nwt_abi_version(void);
int nwt_create(int device, nwt_ctx **out);
void nwt_destroy(nwt_ctx *ctx);
const char *nwt_last_error(nwt_ctx *ctx);

/* Takes the mesh into the context and computes its weights; they stay for any number of nwt_distances calls (until the next
 * nwt_set_mesh; a failed call leaves the context without a mesh).  on_device = 0: positions is a host pointer, checked for finiteness
 * on the host before any HIP call; 1: a device pointer, checked by k_gd_weights.  faces and twin are host pointers either way. */
int nwt_set_mesh(nwt_ctx *ctx, const float *positions, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin, int on_device);

/* One distance field.  source_ids (n_sources) int32 and source_d0 (n_sources) float64 or NULL are host pointers; flags = 0 or
 * NWT_FLAG_DIAGONALS.  The outputs are host pointers: distance_out (n_vertices) float64, source_out (n_vertices) int32 or NULL,
 * info_out (NWT_INFO_WORDS int64). */
int nwt_distances(nwt_ctx *ctx, const int32_t *source_ids, const double *source_d0, int64_t n_sources, double d_cap, int flags, double *distance_out,
                  int32_t *source_out, int64_t *info_out);

#ifdef __cplusplus
}
#endif

#endif
