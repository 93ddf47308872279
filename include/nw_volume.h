/*
 * nw_volume.h -- C-ABI of the banded signed-distance volume of a triangle mesh in libnanowrap_hip.so (csrc/nw_volume.hip, MI355X / gfx950).
 *
 * What it is for: a fitted membrane as a volume -- a signed distance image or an inside mask on the voxel grid of another channel, a
 * shell of given thickness, or (through nwi_set_field / nwi_extract of include/nw_isosurface.h) the surface offset by d nm from the fit.
 *   nwv_set_mesh  -- takes a mesh (and, for signs, its half-edge twin table) into the context: per-face centroids and radii in float64;
 *   nwv_volume    -- for every node of a voxel lattice the exact signed distance to the mesh's triangles, clamped to a band +-d_cap,
 *                    its face, the inside mask and the uint64 field nwi_extract reads.  The lattice's nodes are made on the device:
 *                    no list of query points exists anywhere.
 *
 * Definition (csrc/nw_volume_core.h holds it as code, tests/mesh_volume_ref.py restates it by brute force).
 *   Inputs: the mesh as nwd_set_mesh takes it; a lattice as nwi_density takes it (node (i, j, k) lies at
 *   (double)lo[a] + ((double)index + 0.5) * (double)h along axis a, x fastest, 3 <= dims[a] <= 2^20, at most 2^30 nodes, h > 0,
 *   everything finite); a band d_cap, a finite double with h <= d_cap <= 2^40.
 *   Per node: u = the exact unsigned distance to the triangles and `face` its face (nwd_point_triangle of csrc/nw_distance_core.h in
 *   float64 on the float32 positions, nothing contracted; ties go to the smallest face id).  The node is in band iff u <= d_cap.
 *     in band:      sd = +-u with the sign of the pseudonormal of the closest feature, exactly as nwd_query gives it with NWD_SIGNED
 *                   (negative inside an outward-oriented closed mesh); a distance of 0 is +0.0;
 *     out of band:  face = -1 and sd = +-d_cap with the sign of the node's predecessor on one fixed path: (i-1, j, k) if i > 0, else
 *                   (0, j-1, k) if j > 0, else (0, 0, k-1) if k > 0.  The seed (0, 0, 0) takes its sign from an exact evaluation with
 *                   no cap: the nearest face over all faces, then its pseudonormal.
 *   Why that rule is right for a closed embedded surface: if two lattice neighbours lie on different sides, the segment between them
 *   crosses the surface, so their distances add up to at most h <= d_cap and both are in band, with exact signs of their own.  An
 *   out-of-band node therefore lies on the side of its predecessor, and every path ends at the seed.  This is why d_cap < h is refused.
 *   For an open or self-crossing mesh the result is defined by the same rules and not meaningful: such a mesh has no sides, and the
 *   in-band signs are as wrong as nwd_query's.
 *   Without NWV_SIGNED: sd = min(u, d_cap), there is no sweep and no twin table is needed.
 *   Outputs: sd float64; face int32; mask uint8, 1 where sd < 0; field = (uint64) floor((d_cap - sd) * 2^NWV_FIELD_SHIFT), the layout
 *   nwi_extract reads (a larger value is further inside).  All are dims[2] x dims[1] x dims[0] arrays, x fastest.
 *   Nothing in the result depends on the cell size of the centroid grid, the launch geometry or the order of the faces beyond the tie
 *   rule.
 *
 * Conventions (as include/nw_distance.h, with its own prefix and context):
 *   - every call returns NWV_OK (0) or a negative status; nwv_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call; without a GPU nwv_create fails with NWV_ERR_HIP -- there is no CPU
 *     fallback;
 *   - mesh arrays and outputs are HOST pointers; the result arrays also stay on the device (nwv_field_ptr);
 *   - no kernel uses atomics or scratch, node indices are 64-bit, every result is a function of the input alone;
 *   - one nwv_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 *
 * How it stays exact and stops early.  A node walks rings of the centroid grid as nwd_query does, with min(best, d_cap) in place of
 * the best distance in both bounds (the ring's and the face's), both compared strictly, so a face at exactly d_cap is seen.  A far node
 * stops after ceil((d_cap + rho_max) / h_cell) + 1 rings with nothing found.  The cell size is this unit's own choice,
 * max(2 mean rho_f, (d_cap + rho_max) / 2): the centroids are binned again when the band asks for another size.
 */
#ifndef NW_VOLUME_H_
#define NW_VOLUME_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWV_ABI_VERSION 1
#define NWV_FIELD_SHIFT 20        /* field = floor((d_cap - sd) * 2^20) */

/* flags of nwv_volume */
#define NWV_SIGNED 1              /* sd carries the sign of the side and out-of-band nodes that of their predecessor; needs a twin table */

/* info_out of nwv_volume: NWV_INFO_WORDS int64 values */
#define NWV_INFO_WORDS 8
#define NWV_INFO_FLAGS 0          /* the per-call flag word: NWV_FLAG_FAN_CAPPED */
#define NWV_INFO_IN_BAND 1        /* the number of in-band nodes */
#define NWV_INFO_RINGS_NEAR 2     /* rings walked, summed over the in-band nodes */
#define NWV_INFO_CENTROIDS_NEAR 3 /* centroids read, summed over the in-band nodes */
#define NWV_INFO_RINGS_FAR 4      /* the same over the out-of-band nodes */
#define NWV_INFO_CENTROIDS_FAR 5
#define NWV_INFO_CELLS 6          /* the cells of the centroid grid the call used */
#define NWV_INFO_SEED_FACE 7      /* the nearest face of node (0, 0, 0) over all faces; -1 without NWV_SIGNED */
#define NWV_FLAG_FAN_CAPPED 1     /* a fan walk around a vertex was cut short at 256 faces (that node's sign is from a partial fan) */

typedef struct nwv_ctx nwv_ctx;

typedef enum nwv_status {
    NWV_OK = 0,
    NWV_ERR_BADARG = -1,      /* NULL pointer, size out of range, a face index outside the vertices, a twin table that is not an involution, a lattice outside its limits, d_cap outside [h, 2^40] or not finite, an unknown flag, NWV_SIGNED without a twin table */
    NWV_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwv_last_error */
    NWV_ERR_NONFINITE = -3,   /* a non-finite vertex position */
    NWV_ERR_NOMEM = -4,
    NWV_ERR_NOMESH = -5       /* nwv_volume while the context holds no mesh; nwv_get_field before nwv_volume */
} nwv_status;

int nwv_abi_version(void);
int nwv_create(int device, nwv_ctx **out);
void nwv_destroy(nwv_ctx *ctx);
const char *nwv_last_error(nwv_ctx *ctx);

/* Takes the mesh into the context, where it stays for any number of volumes (until the next nwv_set_mesh; a failed call leaves the
 * context without a mesh).  twin: int32[3 n_faces], twin[h] = the half-edge opposite to h or -1 on a border; or NULL for a mesh that is
 * only voxelized unsigned.  The same checks as nwd_set_mesh, on the host first: sizes, face indices, every twin entry -1 or in [0, 3F)
 * with twin[twin[h]] == h (NWV_ERR_BADARG); positions finite (NWV_ERR_NONFINITE). */
int nwv_set_mesh(nwv_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin);

/* The volume on the lattice (lo, h, dims) with the band d_cap.  sd_host (float64), face_host (int32), mask_host (uint8): each may be
 * NULL; info_out (int64[NWV_INFO_WORDS]) may be NULL.  The arrays stay on the device. */
int nwv_volume(nwv_ctx *ctx, const float *lo, float h, const int32_t *dims, double d_cap, int flags, double *sd_host, int32_t *face_host,
               uint8_t *mask_host, int64_t *info_out);

/* The device pointer of the last nwv_volume's uint64 field (complete: that call synchronized), NULL if there is none.  It is valid
 * until the context's next nwv_volume or its destruction. */
const uint64_t *nwv_field_ptr(nwv_ctx *ctx);

/* A copy of that field for the host: dims[2] x dims[1] x dims[0] uint64 of the last nwv_volume (NWV_ERR_NOMESH if there is none). */
int nwv_get_field(nwv_ctx *ctx, uint64_t *field_host);

#ifdef __cplusplus
}
#endif

#endif
