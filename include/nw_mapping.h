/*
 * nw_mapping.h -- C-ABI of mapping localizations onto a triangle mesh in libnanowrap_hip.so (csrc/nw_mapping.hip, MI355X / gfx950).
 *
 * What it is for: where on a fitted membrane the localizations are -- the surface density of the labelled protein per vertex, in
 * localizations per nm^2, and the per-vertex mean of any localization column (photons, frame, error_x, a second channel's flag, the
 * distance itself).  nwd_query gives the closest face and point per localization, 40 bytes each back to the host; it has no band to
 * drop background, no rule for splitting a localization between the corners of its face, and sums made from it in floating point
 * depend on the order of the cloud.  PYME is not part of the reference tree and upstream has no such module, so the definition here
 * is this project's own (csrc/nw_mapping_core.h holds it as code, tests/surface_mapping_ref.py restates it by brute force):
 *   nwl_set_mesh  -- takes the mesh into the context: per-face centroids and radii in float64 for the query units' shared grid, and
 *                    the per-vertex areas area3[v] = the sum over the faces at v of floor(A_f 2^20);
 *   nwl_map       -- per localization within d_cap of the mesh: the closest face (the smallest id among equals), the closest point,
 *                    the distance and three integer weights W_k >= 0 with W_0 + W_1 + W_2 = 2^20, one per corner of that face
 *                    (barycentric inside the face, linear along an edge, all on one corner at a vertex); and the accumulators
 *                      mass[v]  (uint64)  += W_k at the three corners,       count[f] (int32) += 1,
 *                      sum_lo[v, c] (uint64) += (W_k q_c) & 0xFFFFFFFF,      sum_hi[v, c] (int64) += (W_k q_c) >> 32 (arithmetic),
 *                    with q_c = (int64) rint(x_c / scale_c * 2^30) of value column c, scale_c a power of two >= max |x_c|.
 *   The caller makes n[v] = mass / 2^20, area[v] = area3 / (3 2^20), density[v] = 3 mass / area3 and
 *   mean_c[v] = (sum_hi 2^32 + sum_lo) / mass * scale_c / 2^30 from the integers.
 * Every accumulated output is an integer added with integer atomics: the result is a function of the input alone, whatever the launch
 * geometry, the order of the atomics or the order of the cloud, and a cloud mapped in chunks with NWL_ACCUMULATE gives the accumulators
 * of one call.  For at most 2^30 localizations in one set of accumulators no limb overflows (nw_mapping_core.h has the bound);
 * nwl_map refuses more.
 *
 * Conventions (as include/nw_proximity.h, with its own prefix and context):
 *   - every call returns NWL_OK (0) or a negative status; nwl_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before anything is uploaded or launched; without a GPU nwl_create fails with NWL_ERR_HIP --
 *     there is no CPU fallback;
 *   - mesh arrays are HOST pointers (float32 / int32, row-major, C-contiguous); xyz and values are host pointers or device pointers
 *     the kernels can read in place (nwd_query's contract: a device array is not copied, and its finiteness is checked on the device);
 *     scales is a host pointer; outputs are host pointers;
 *   - the kernels (k_lm_*) use no scratch, offsets are 64-bit, all stores are vector stores; the walk's counters are added per block
 *     in a fixed order;
 *   - one nwl_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 *
 * A value that is not finite, or larger than its scale, on an in-band localization ends the call with NWL_ERR_NONFINITE or
 * NWL_ERR_RANGE (the kernel raises a flag word with a plain store, the host reads it once); the context's accumulators are then
 * undefined until the next call without NWL_ACCUMULATE.  The same value on an out-of-band localization is never looked at.
 */
#ifndef NW_MAPPING_H_
#define NW_MAPPING_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWL_ABI_VERSION 1

#define NWL_MAX_VALUE_COLUMNS 8

/* flags of nwl_map */
#define NWL_ACCUMULATE 1          /* add onto the accumulators the previous call left (the same mesh, the same number of columns); without it they are zeroed first */
#define NWL_WALK_ONLY 2           /* per-localization outputs and counters only: no accumulator is touched or returned (for measuring the walk alone) */

/* info_out of nwl_map: NWL_INFO_WORDS int64 values */
#define NWL_INFO_WORDS 5
#define NWL_INFO_IN_BAND 0        /* the localizations of this call in band */
#define NWL_INFO_RINGS 1          /* rings walked, summed over the localizations */
#define NWL_INFO_CENTROIDS 2      /* centroids read, summed over the localizations */
#define NWL_INFO_CELLS 3          /* the cells of the centroid grid the call used */
#define NWL_INFO_CELL_SIZE 4      /* its cell size: the bits of a double */

typedef struct nwl_ctx nwl_ctx;

typedef enum nwl_status {
    NWL_OK = 0,
    NWL_ERR_BADARG = -1,      /* NULL pointer, size out of range, a face index outside the vertices, a face of area 2^40 or more, a band outside (0, 2^40], a scale that is no power of two, an unknown flag */
    NWL_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwl_last_error */
    NWL_ERR_NONFINITE = -3,   /* a non-finite vertex position, localization, or value of an in-band localization */
    NWL_ERR_NOMEM = -4,
    NWL_ERR_NOMESH = -5,      /* nwl_map or nwl_get_areas while the context holds no mesh */
    NWL_ERR_RANGE = -6        /* a value of an in-band localization larger than its column's scale */
} nwl_status;

int nwl_abi_version(void);
int nwl_create(int device, nwl_ctx **out);
void nwl_destroy(nwl_ctx *ctx);
const char *nwl_last_error(nwl_ctx *ctx);

/* Takes the mesh into the context, where it stays for any number of calls (until the next nwl_set_mesh; a failed call leaves the
 * context without a mesh), and zeroes nothing but the areas: the accumulators belong to nwl_map. */
int nwl_set_mesh(nwl_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces);

/* area3_out: uint64[n_vertices] of the mesh in the context */
int nwl_get_areas(nwl_ctx *ctx, uint64_t *area3_out);

/* n localizations xyz (float64 triples) against the mesh in the context.  values: float64 (n, n_columns) row-major, n_columns <=
 * NWL_MAX_VALUE_COLUMNS (NULL with 0 columns); scales: n_columns powers of two.  d_cap finite, > 0, <= 2^40.
 * Per localization: face_out int32[n], w_out int32[3n], dist_out float64[n], closest_out float64[3n].
 * Per vertex and per face, after this call: mass_out uint64[V], count_out int32[F], sum_hi_out int64[V * n_columns], sum_lo_out
 * uint64[V * n_columns].  info_out int64[NWL_INFO_WORDS].  Any output may be NULL. */
int nwl_map(nwl_ctx *ctx, const double *xyz, int64_t n, const double *values, int n_columns, const double *scales, double d_cap, int flags,
            int32_t *face_out, int32_t *w_out, double *dist_out, double *closest_out, uint64_t *mass_out, int32_t *count_out,
            int64_t *sum_hi_out, uint64_t *sum_lo_out, int64_t *info_out);

#ifdef __cplusplus
}
#endif

#endif
