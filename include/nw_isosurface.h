/*
 * nw_isosurface.h -- C-ABI of the density isosurface in libnanowrap_hip.so (csrc/nw_isosurface.hip, MI355X / gfx950): the start surface of
 * a fit made from the localization cloud itself.
 *
 * What it stands in for: the first two modules of upstream's recipe (ch_shrinkwrap/test_evaluation_recipe.yaml:25-38),
 *   pointcloud.Octree -> surface_fitting.DualMarchingCubes(threshold_density, remesh) -> surface_fitting.ShrinkwrapMembrane,
 * which are PYME's and not in the reference tree.  This is NOT PYME's octree / dual marching cubes: it is a regular grid at one
 * resolution with a fixed bandwidth, defined here:
 *   nwi_density         localizations counted per voxel (uint32), then `passes` rounds of the separable binomial [1 2 1] along x, y, z in
 *                       integers WITHOUT the division: a uint64 field of plain weighted sums, zero outside the grid.  The field is exact,
 *                       independent of the order of the localizations and bit-reproducible.  A density in nm^-3 is field / (4^(3 passes) h^3).
 *   nwi_threshold_auto  thr = floor(fraction * M) (both as doubles), M = the lower median (rank (m - 1) / 2 of the m sorted values) of
 *                       the field over the voxels whose raw count is not zero.
 *   nwi_extract         sheet-aware surface nets of `field > thr` (inside) on the lattice of voxel centres (node (i,j,k) at lo + (i + 1/2) h),
 *                       closed and consistently oriented (every mesh edge used an even number of times, as often one way as the other);
 *                       manifold, every edge used twice, unless two cells that share an ambiguous face (its inside nodes on a diagonal)
 *                       each join all four crossings of that face in one sheet: the edge between their two vertices is then used four
 *                       times.  A field smoothed over more than a voxel has no such pair:
 *     - cell (i,j,k), 0 <= i < dims[0] - 1 ..., has the nodes (i + dx, j + dy, k + dz) as corners; its pattern has bit dz*4 + dy*2 + dx set
 *       for an inside corner; cube edge e = axis*4 + a + 2*b runs along `axis` at the offsets a, b along the two other axes u, v
 *       ((u, v, axis) cyclic);
 *     - one vertex per SHEET per cell, from the 256 x 12 table handed to nwi_set_sheet_table (table[cfg][e] = the sheet of the crossing
 *       on edge e: the smallest edge of its cycle, -1 if e is not crossed): two sheets through one cell never share a vertex;
 *     - vertex = lo + ((cell + 1/2) + mean of the sheet's crossings) * h per axis in float32, a crossing at t = (f0 - thr) / (f0 - f1)
 *       along its edge (integer differences, then float32), summed in ascending edge order;
 *     - one quad per lattice edge whose end nodes differ, joining the vertices of the four cells around it, normals from inside to
 *       outside, split into (0,1,2),(0,2,3) if (i + j + k) of the edge's lower node is even and (0,1,3),(1,2,3) if odd;
 *     - order: vertices by ascending key = cell_linear_index * 16 + sheet, cell_linear_index = (k (dims[1] - 1) + j)(dims[0] - 1) + i;
 *       quads by ascending (axis, linear index of the lower node), the two triangles of a quad adjacent;
 *     - an inside node on the grid's outermost layer is NWI_ERR_BORDER: the caller pads.
 *
 * Conventions (as include/nw_holepunch.h, with its own prefix and context):
 *   - every call returns NWI_OK (0) or a negative status; nwi_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked before any HIP call (host localizations included); without a GPU nwi_create fails with NWI_ERR_HIP -- there is
 *     no CPU fallback;
 *   - the field, the counts and the extracted mesh stay on the device until asked for; output arrays are HOST pointers;
 *   - one nwi_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_ISOSURFACE_H_
#define NW_ISOSURFACE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWI_ABI_VERSION 1
#define NWI_MAX_PASSES 5          /* 2^30 localizations * 4^(3*5) < 2^64 */

typedef struct nwi_ctx nwi_ctx;

typedef enum nwi_status {
    NWI_OK = 0,
    NWI_ERR_BADARG = -1,      /* NULL pointer, h <= 0 or not finite, a dimension < 3, more than 2^30 voxels or localizations, passes out of range, a malformed table */
    NWI_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwi_last_error */
    NWI_ERR_NONFINITE = -3,   /* a non-finite localization */
    NWI_ERR_NOMEM = -4,
    NWI_ERR_OUTSIDE = -5,     /* a localization outside the grid (nothing is dropped silently) */
    NWI_ERR_STATE = -6,       /* a call before the one it needs: nwi_density (or nwi_set_field), nwi_set_sheet_table, nwi_extract */
    NWI_ERR_BORDER = -7,      /* an inside node on the outermost layer of the grid: pad the grid */
    NWI_ERR_EMPTY = -8        /* no occupied voxel (nwi_threshold_auto) or no node pair across the threshold (nwi_extract) */
} nwi_status;

int nwi_abi_version(void);
int nwi_create(int device, nwi_ctx **out);
void nwi_destroy(nwi_ctx *ctx);
const char *nwi_last_error(nwi_ctx *ctx);

/* The 256 x 12 int8 sheet table (row-major, see above), checked on the host: an entry is >= 0 exactly on the edges the pattern crosses,
 * names an edge <= its own that is its own sheet, and no pattern has more than 4 sheets. */
int nwi_set_sheet_table(nwi_ctx *ctx, const int8_t *table);

/* xyz: (n,3) float32; points_on_device = 0: a host pointer, checked on the host (finite, inside the grid) before any HIP call;
 * 1: a device pointer, checked by the counting kernel.  Voxel of a coordinate = floorf((x - lo) * (1.0f / h)) in float32.
 * field_out (may be NULL): dims[2] x dims[1] x dims[0] uint64, x fastest; counts_out (may be NULL): the same shape in uint32. */
int nwi_density(nwi_ctx *ctx, const float *xyz, int64_t n_points, int points_on_device, const float *lo, float h, const int32_t *dims,
                int passes, uint64_t *field_out, uint32_t *counts_out);

/* Adopts a field made elsewhere (nwk_node_field of include/nw_neighbours.h, or a host array) by copy: dims[2] x dims[1] x dims[0] uint64,
 * x fastest, a host pointer (on_device = 0) or a device pointer (1: complete before the call, not read after it); lo, h and dims as
 * nwi_density takes them, with the same limits.  Afterwards the context is in the state nwi_extract needs; there are no counts, so
 * nwi_threshold_auto returns NWI_ERR_STATE until the next nwi_density. */
int nwi_set_field(nwi_ctx *ctx, const uint64_t *field, int on_device, const float *lo, float h, const int32_t *dims);

/* median, threshold (both field values), threshold as a density in nm^-3, number of occupied voxels; each output may be NULL but thr. */
int nwi_threshold_auto(nwi_ctx *ctx, double fraction, uint64_t *median, uint64_t *thr, double *density, int64_t *n_occupied);

int nwi_extract(nwi_ctx *ctx, uint64_t thr, int64_t *n_vertices, int64_t *n_faces);

/* vertices (n_vertices,3) float32, faces (n_faces,3) int32, keys (n_vertices) int64; each may be NULL */
int nwi_get(nwi_ctx *ctx, float *vertices, int32_t *faces, int64_t *keys);

#ifdef __cplusplus
}
#endif

#endif
