/*
 * nw_holepunch.h -- C-ABI of the hole-punch point queries in libnanowrap_hip.so (csrc/nw_holepunch.hip, MI355X / gfx950).
 *
 * What it stands in for: the three point-dependent steps of MembraneMesh.punch_holes (upstream ch_shrinkwrap/_membrane_mesh.pyx:1163-1199),
 * which upstream runs with scipy's cKDTree and a serial C loop:
 *   nwh_empty_faces  -- _holepunch_find_candidate_faces (:877-887): faces with no localization within eps of their centroid;
 *   nwh_pair_faces   -- c_holepunch_pair_candidate_faces (membrane_mesh_utils.c:1301-1376): bit-identical float32 arithmetic;
 *   nwh_prism_empty  -- the emptiness test of _holepunch_empty_prism_candidate_faces (:946-1016), one flag per pair (the greedy pass that
 *                       consumes the flags is the caller's: it is sequential and cheap).
 * The topology steps that follow (components, Euler characteristic, surgery) are host code (ch_shrinkwrap_amd/holepunch.py).
 *
 * Conventions (as include/nanowrap.h, with its own prefix and context):
 *   - every call returns NWH_OK (0) or a negative status; nwh_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked before any HIP call; without a GPU nwh_create fails with NWH_ERR_HIP -- there is no CPU fallback;
 *   - the localizations (nwh_set_points) may be a host or a device pointer; every mesh array is a HOST pointer (float32 / int32,
 *     row-major, C-contiguous): the calls gather what they need and copy it;
 *   - a face f has the corners faces[3f+0..2]; its centroid is computed from them in that order, as the reference does from
 *     prev(h), h, next(h) of the face's half-edge h (the mirror's half-edge 3f runs faces[f,0] -> faces[f,1]);
 *   - one nwh_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_HOLEPUNCH_H_
#define NW_HOLEPUNCH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWH_ABI_VERSION 1

typedef struct nwh_ctx nwh_ctx;

typedef enum nwh_status {
    NWH_OK = 0,
    NWH_ERR_BADARG = -1,      /* NULL pointer, size out of range, an index outside its array, a non-positive or non-finite eps */
    NWH_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwh_last_error */
    NWH_ERR_NONFINITE = -3,   /* a non-finite localization */
    NWH_ERR_NOMEM = -4,
    NWH_ERR_NOPOINTS = -5     /* a query before nwh_set_points */
} nwh_status;

int nwh_abi_version(void);
int nwh_create(int device, nwh_ctx **out);
void nwh_destroy(nwh_ctx *ctx);
const char *nwh_last_error(nwh_ctx *ctx);

/* The localizations ((n,3) float32, host or device) are binned into a uniform cell grid on the device (counting sort by cell); they do not
 * move during a fit, so this runs once per fit.  cell_size <= 0 picks one from the bounding box (about one localization per cell of the
 * box); the grid never has more than min(max(4 n, 65536), 2^30) cells. */
int nwh_set_points(nwh_ctx *ctx, const float *xyz, int64_t n_points, float cell_size);

/* far[f] = 1 if no localization lies within eps of face f's centroid ((p0 + p1) + p2) / 3 (the float32 mean the reference takes), else 0.
 * dist (may be NULL): the distance to the nearest localization, clipped at eps (a face with far[f] = 1 gets eps). */
int nwh_empty_faces(nwh_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, float eps,
                    uint8_t *far, float *dist);

/* pairs[i] = the j > i that the reference's serial loop picks for candidate i (the index into cands, not a face id), or -1.  face_normals is
 * (n_faces,3).  Rows are independent (the loop's `pairs[j] != -1` test never fires: row j is written after row i), so every row is searched
 * in parallel; ties go to the smallest j, as the serial loop's strict < does.  No localizations needed. */
int nwh_pair_faces(nwh_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const float *face_normals,
                   const int32_t *cands, int64_t n_cands, int32_t *pairs);

/* empty[k] = 1 if no localization within r = |c_i - c_j| + eps of c_i or of c_j lies below all six half-planes of the two faces
 * (hp . (x - p) < eps, hp = n x e / |e|), for i = k and j = pair_idx[k] (indices into cands).  Evaluated in float64. */
int nwh_prism_empty(nwh_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const float *face_normals,
                    const int32_t *cands, const int32_t *pair_idx, int64_t n, float eps, uint8_t *empty);

#ifdef __cplusplus
}
#endif

#endif
