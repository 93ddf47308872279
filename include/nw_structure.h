/*
 * nw_structure.h -- C-ABI of the local shape of a cloud in libnanowrap_hip.so (csrc/nw_structure.hip, MI355X / gfx950): the exact integer
 * moments of every neighbourhood of radius r, and their covariance's eigenvalues and eigenvectors by one fixed float64 procedure.
 *
 * What it is for: the neighbourhood covariance of a localization cloud (structure tensor, local PCA) -- does a localization sit on a
 * sheet, a tubule or a blob, and which way does the structure face there.  Normals for a table that has none, sheets against tubules
 * before any fit, denoising by shape, a value column to colour a fit with.  PYME is not in the reference tree and upstream has no such
 * module, so the definition is this project's own and is written down in csrc/nw_structure_core.h.
 *
 * Definitions:
 *   - the cloud is (n,3) float32, row-major, a host pointer or a device pointer, 1 <= n <= NWF_MAX_N = 2^26; a non-finite coordinate is
 *     an error;
 *   - the radius r is finite, 0 < r <= 2^40; r2 = r * r in float64, computed once by the library, must be finite and above 0;
 *   - d2 = (ex*ex + ey*ey) + ez*ez in float64 with e = (double)cloud point - (double)query (no fma);
 *     N(q) = { j : d2(p_j, q) <= r2 }, inclusive: a point at exactly r2 is in;
 *   - auto mode (queries = NULL) is cross mode with the cloud as its own queries: a point is in its own neighbourhood (d2 = 0), duplicates
 *     at other indices count, there is no special case.  Cross mode: a query may lie anywhere; 1 <= nq <= 2^26;
 *   - R = the smallest power of two >= r, s = 2^18 / R; per axis u = rint(e * s), ties to even, |u| <= 2^18;
 *   - moments (nq, 10) int64 per query: n, S1[3] = sum u, S2[6] = sum u_a u_b in the order xx xy xz yy yz zz.  |S2| <= 2^62: nothing can
 *     overflow.  They are integers, so a function of the input alone: no output depends on the order of the cloud, on the cell size, on
 *     the launch geometry or on any order of arrival;
 *   - m_a = S1_a / n, C_ab = S2_ab / n - m_a m_b in float64; NWF_SWEEPS sweeps of cyclic Jacobi rotations (0,1), (0,2), (1,2);
 *     eigenvalues (nq, 3) float64 descending, in the cloud's units squared, as computed (the small ones may be a few ulp below zero);
 *   - vectors (nq, 3, 3) float64: the rows are the axis (of the largest eigenvalue), mid and the normal (of the smallest).  Each has its
 *     component of largest magnitude positive (the first one on a tie); with a viewpoint the normal is then turned where
 *     normal . (viewpoint - q) < 0.  Orientation is local: nothing is propagated over the cloud;
 *   - flags (nq) uint8: NWF_FLAG_VALID iff n >= 3 and the largest eigenvalue > 0; NWF_FLAG_EMPTY for n = 0 (eigenvalues NaN, vectors
 *     zero); NWF_FLAG_FEW for 1 <= n < 3; NWF_FLAG_POINT for n >= 3 without extent; NWF_FLAG_TURNED where the viewpoint turned the normal.
 *     Where not valid and not empty the outputs are whatever the fixed procedure gives.
 *
 * How it is computed.  The cloud is binned into the query units' shared cell grid (bq::bounds<float>, bq::build_grid<float>) with this
 * unit's own cell size: h = max(0.5 r, widest extent / 1024), widened by a tenth at a time until the grid has at most max(2 n, 65536)
 * cells (2^26 at most, 1025 an axis).  Another r bins again.  One lane per query -- in auto mode the cloud's points in cell order --
 * visits every cell that can hold a point within r (a clamped box of cells, see the core header) and keeps its ten sums in registers;
 * a second kernel turns the sums into eigenvalues and vectors.  The cost is inherent: a query tests every cloud point of the cells its r
 * reaches.
 *
 * Conventions (as include/nw_pairs.h, with its own prefix and context):
 *   - every call returns NWF_OK (0) or a negative status; nwf_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call and before the context is used; without a GPU nwf_create fails with
 *     NWF_ERR_HIP -- there is no CPU fallback;
 *   - a device pointer is read on the context's own stream with no ordering against the stream that wrote it: it must be complete
 *     before the call and unchanged until it returns;
 *   - one nwf_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_STRUCTURE_H_
#define NW_STRUCTURE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWF_ABI_VERSION 1
#define NWF_MOMENT_WORDS 10

/* flags[]: one byte per query */
#define NWF_FLAG_VALID 1
#define NWF_FLAG_EMPTY 2
#define NWF_FLAG_FEW 4
#define NWF_FLAG_POINT 8
#define NWF_FLAG_TURNED 16

/* info[]: int64 words */
#define NWF_INFO_WORDS 8
#define NWF_INFO_TESTS 0            /* distance tests done */
#define NWF_INFO_CELLS_READ 1       /* grid cells read, all queries */
#define NWF_INFO_CELL_SIZE 2        /* the bits of a double */
#define NWF_INFO_CELLS 3            /* cells of the grid */
#define NWF_INFO_NEIGHBOURS 4       /* neighbours summed: the sum of n over the queries */
#define NWF_INFO_FEW 5              /* queries with n < 3 */
#define NWF_INFO_N_QUERIES 6
#define NWF_INFO_N_CLOUD 7

typedef struct nwf_ctx nwf_ctx;

typedef enum nwf_status {
    NWF_OK = 0,
    NWF_ERR_BADARG = -1,      /* NULL pointer, size out of range, a radius outside the definition */
    NWF_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwf_last_error */
    NWF_ERR_NONFINITE = -3,   /* a non-finite coordinate in the cloud, in the queries or in the viewpoint */
    NWF_ERR_NOMEM = -4,
    NWF_ERR_NOCLOUD = -5      /* nwf_query before nwf_set_cloud */
} nwf_status;

int nwf_abi_version(void);
int nwf_create(int device, nwf_ctx **out);
void nwf_destroy(nwf_ctx *ctx);
const char *nwf_last_error(nwf_ctx *ctx);

/* Takes a copy of the cloud into the context, where it stays for any number of queries (until the next nwf_set_cloud; a failed call
 * leaves the context without a cloud).  on_device = 0: a host pointer, checked for finiteness on the host before any HIP call; 1: a
 * device pointer, checked by the bounding-box kernel. */
int nwf_set_cloud(nwf_ctx *ctx, const float *xyz, int64_t n, int on_device);

/* One query.  queries = NULL: auto mode, nq must be 0 or the cloud's n.  Otherwise cross mode: (nq,3) float32, a host pointer
 * (on_device = 0, checked for finiteness on the host) or a device pointer (1, checked by the kernel).  viewpoint: three doubles on the
 * host, or NULL.  The outputs are host pointers, in the caller's query order, each of them optional but info: moments (nq, 10) int64,
 * eigenvalues (nq, 3) float64, vectors (nq, 9) float64, flags (nq) uint8, info (NWF_INFO_WORDS int64).  Bins the cloud anew if r asks
 * for another cell size than the grid at hand has. */
int nwf_query(nwf_ctx *ctx, const float *queries, int64_t nq, int on_device, double r, const double *viewpoint, int64_t *moments, double *eigenvalues,
              double *vectors, uint8_t *flags, int64_t *info);

#ifdef __cplusplus
}
#endif

#endif
