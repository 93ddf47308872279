/*
 * nw_surgery.h -- C-ABI of the block-boundary surgery queries in libnanowrap_hip.so (csrc/nw_surgery.hip, MI355X / gfx950).
 *
 * What it stands in for: the mesh-wide questions behind upstream's remove_necks and remove_extra_short_edges
 * (ch_shrinkwrap/_membrane_mesh.pyx:1201-1239) and behind this package's remove_inner_surfaces (PYME's is not in the reference):
 *   nws_label_faces          -- edge-connected components of a face set (union-find, atomic hooking, no rounds per diameter);
 *   nws_component_stats      -- per component: faces, area, signed volume, bounding box, border half-edges;
 *   nws_winding              -- generalized winding number of query points with respect to every component;
 *   nws_short_edge_vertices  -- upstream's short-edge selection: heads of half-edges shorter than threshold * median.
 * The surgery itself (excise, make manifold, cap, dust) is host code (ch_shrinkwrap_amd/surgery.py).
 *
 * Conventions (as include/nw_holepunch.h, with its own prefix and context):
 *   - every call returns NWS_OK (0) or a negative status; nws_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked before any HIP call; without a GPU nws_create fails with NWS_ERR_HIP -- there is no CPU fallback;
 *   - every mesh array is a HOST pointer (float32 / int32, row-major, C-contiguous); outputs are host pointers too;
 *   - half-edge 3f+k runs faces[3f+k] -> faces[3f+(k+1)%3]; twin[h] is the opposite half-edge or -1 on a border;
 *   - every result is deterministic: the same bytes on every run (union-find roots are minimum face ids; sums are 64-bit fixed point);
 *   - one nws_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_SURGERY_H_
#define NW_SURGERY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWS_ABI_VERSION 1

typedef struct nws_ctx nws_ctx;

typedef enum nws_status {
    NWS_OK = 0,
    NWS_ERR_BADARG = -1,      /* NULL pointer, size out of range, an index outside its array, a negative threshold */
    NWS_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nws_last_error */
    NWS_ERR_NOMEM = -3
} nws_status;

int nws_abi_version(void);
int nws_create(int device, nws_ctx **out);
void nws_destroy(nws_ctx *ctx);
const char *nws_last_error(nws_ctx *ctx);

/* label_out[f] = index of f's edge-connected component among the faces with mask[f] != 0 (mask NULL = every face), numbered 0..C-1 in
 * order of each component's smallest face id; -1 outside the mask.  Two faces are adjacent when twin links one of their half-edges to
 * the other.  `faces` is not read (adjacency is the twin table's); it must be non-NULL.  *n_components_out = C. */
int nws_label_faces(nws_ctx *ctx, const int32_t *faces, const int32_t *twin, const uint8_t *mask, int64_t n_faces, int32_t *label_out,
                    int32_t *n_components_out);

/* Per component c of `label` (values -1 or 0..n_components-1): face_count[c], area[c] (sum of 0.5 |(p1-p0) x (p2-p0)|), volume[c]
 * (sum of p0 . (p1 x p2) / 6: positive for a closed surface whose faces wind counter-clockwise seen from outside), bbox[6c..6c+5]
 * (min xyz, max xyz of its corners; FLT_MAX / -FLT_MAX for an empty component) and n_border[c] (its half-edges whose twin is -1 or a face
 * of another label).  Terms in float64, summed in 64-bit fixed point: identical bytes on every run.  Terms are taken relative to o, the
 * centre of pos's bounding box rounded to float32: volume[c] = sum of q0 . (q1 x q2) / 6 with q = p - o, plus o . (sum of (q1 - q0) x
 * (q2 - q0)) / 6 (which vanishes for a closed component), so that the resolution follows the mesh's extent, not its distance from the
 * origin.  The resolution of a term is 2^-k with 2^k = 2^62 / (n_faces * bound), bound = 6 M^2 for area, M^3 for the volume about o and
 * 12 M^2 for the normal sums, M = max |p - o| over pos: a component of n_c faces is within n_c 2^-k / 2 of the sum of its float64 terms
 * (for the volume, plus |o|_1 n_c 2^-k / 12 from the normal sums).  Any output may be NULL. */
int nws_component_stats(nws_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, const int32_t *twin, const int32_t *label,
                        int64_t n_faces, int32_t n_components, int64_t *face_count, double *area, double *volume, float *bbox,
                        int64_t *n_border);

/* w_out[q * n_components + c] = generalized winding number of queries[q] with respect to the faces of component c: the sum over those
 * faces of their solid angle (Van Oosterom & Strackee, float64) / 4 pi, summed in 64-bit fixed point of resolution 2^-(62 - ceil(log2(n_faces+1))).
 * Exactly 0 -- not evaluated -- for c == query_component[q] (may be -1 for none; query_component NULL = no component skipped) and for a
 * component whose bounding box (nws_component_stats) does not contain the query point. */
int nws_winding(nws_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, const int32_t *label, int64_t n_faces,
                int32_t n_components, const float *queries, const int32_t *query_component, int64_t n_queries, double *w_out);

/* flag_out[v] = 1 if v is the head of a half-edge whose length is < threshold * median, else 0 (n_vertices entries).  Lengths are float32
 * sqrt((dx*dx + dy*dy) + dz*dz), products rounded one by one, as nwr_mesh_geometry (and so TriMesh's half-edge lengths) computes them; the
 * median is numpy's of that array (the middle element, or the float32 mean of the two middle ones), selected by radix select; the
 * product is rounded to float32.  *median_out (may be NULL) = the median. */
int nws_short_edge_vertices(nws_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, float threshold,
                            uint8_t *flag_out, float *median_out);

#ifdef __cplusplus
}
#endif

#endif
