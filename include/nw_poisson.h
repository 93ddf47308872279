/*
 * nw_poisson.h -- C-ABI of the screened Poisson grid solver in libnanowrap_hip.so (csrc/nw_poisson.hip, MI355X / gfx950): a closed
 * surface from an oriented point cloud, the comparator of upstream's evaluation.
 *
 * What it stands in for: surface_fitting.ScreenedPoissonMesh (upstream's recipe_modules/surface_fitting.py), the second arm of
 * ch_shrinkwrap/evaluation.py (compute_spr), which wraps pymeshlab.  This is NOT pymeshlab's / Kazhdan's octree solver: it is a complete
 * cube of 2^depth nodes an axis with piecewise-linear splats and a cascadic coarse-to-fine red-black Gauss-Seidel solve, with upstream's
 * parameter names (depth, fulldepth, samplespernode, pointweight, iters, confidence) at their meaning where they have one.  The
 * definition is this project's own and is written down, with its overflow proofs, in csrc/nw_poisson_core.h; tests/screened_poisson_ref.py
 * restates it in NumPy.  In short:
 *   - samples: (n,3) float32 positions and outward normals, host or device pointers, 1 <= n <= NWO_MAX_N = 2^25; anything non-finite is
 *     an error; a normal of length 0 is skipped and counted; normals are normalised in float64 unless use_lengths (upstream's confidence),
 *     which refuses a component above 1 in magnitude; every component is quantised to rint(. 2^12);
 *   - lattice: lo[3] and h as nwi_* take them, 3 <= depth <= 9; level l has 2^l nodes an axis at lo + (i + 1/2) h 2^(depth - l); base level 2;
 *   - per level: the samples' trilinear weights (7 bits an axis) into int64 sums W and V[3] by atomics whose results are not read, the
 *     system (rhs, diag) from them, chi from zero (level 2) or prolongated from the level below, red-black sweeps, the largest residual
 *     before and after them;
 *   - the depth used: the global rule of samplespernode and fulldepth over the exact occupancy counts occ_l;
 *   - the field F = rint(chi / E 2^31) + 2^31 as uint64 at the level used and the level thr = floor(sum W F / sum W); F stays on the
 *     device and goes to nwi_set_field(on_device = 1) at (lo, h 2^(depth - used), 2^used an axis), then nwi_extract(thr).
 * What is claimed: W, V, occ and thr are exact integers; rhs, diag, chi of every level, the residuals and F are one fixed float64
 * procedure with nothing contracted: NumPy, g++ and the device give the same bits.  No claim is made that `iters` sweeps have
 * converged: the residuals say how far they got.
 *
 * Memory.  A level holds W and V[3] (int64), rhs, diag and chi (float64) of 2^(3 l) nodes each, the chi of the level below, and at the
 * level used F (uint64); the occupancy count uses one byte a node of the finest level.  Nothing is aliased, so that every array of the
 * level at hand can be read back: the peak is 8 1/4 arrays of 8 bytes a node, 8.3 GiB at depth 9 (2^27 nodes) and 1.0 GiB at depth 8,
 * besides the samples (20 bytes each) and the copy nwi_set_field takes.
 *
 * Conventions (as include/nw_isosurface.h, with its own prefix and context):
 *   - every call returns NWO_OK (0) or a negative status; nwo_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call and before the context is used (host samples included); without a GPU
 *     nwo_create fails with NWO_ERR_HIP -- there is no CPU fallback;
 *   - a device pointer is read on the context's own stream with no ordering against the stream that wrote it: it must be complete
 *     before the call and unchanged until it returns;
 *   - one nwo_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_POISSON_H_
#define NW_POISSON_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWO_ABI_VERSION 1
#define NWO_RESIDUAL_WORDS 20     /* nwo_solve's residuals: before and after the sweeps of level l at [2 l] and [2 l + 1], l <= 9 */

/* nwo_get_level's `what` */
#define NWO_GET_W 0               /* n^3 int64 */
#define NWO_GET_V 1               /* 3 n^3 int64: the planes x, y, z one after the other */
#define NWO_GET_RHS 2             /* n^3 float64 */
#define NWO_GET_DIAG 3
#define NWO_GET_CHI 4

typedef struct nwo_ctx nwo_ctx;

typedef enum nwo_status {
    NWO_OK = 0,
    NWO_ERR_BADARG = -1,      /* NULL pointer, a size, depth or level out of range, pointweight <= 0, h <= 0 or not finite, a normal component above 1 with use_lengths */
    NWO_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwo_last_error */
    NWO_ERR_NONFINITE = -3,   /* a non-finite position, normal or lattice origin */
    NWO_ERR_NOMEM = -4,
    NWO_ERR_STATE = -5,       /* a call before the one it needs: set_samples, plan, level_begin (of the level below), field */
    NWO_ERR_EMPTY = -6        /* no sample with a normal (nwo_set_samples), or a solution that is zero everywhere (nwo_field) */
} nwo_status;

int nwo_abi_version(void);
int nwo_create(int device, nwo_ctx **out);
void nwo_destroy(nwo_ctx *ctx);
const char *nwo_last_error(nwo_ctx *ctx);

/* Takes a copy of the samples and quantises the normals.  on_device = 0: host pointers, checked on the host (finite; with use_lengths no
 * component above 1 in magnitude) before any HIP call; 1: device pointers, checked by the kernel.  n_used: the samples whose normal has a
 * length above 0; n_skipped: the others.  A failed call leaves the context without samples. */
int nwo_set_samples(nwo_ctx *ctx, const float *xyz, const float *normals, int64_t n, int on_device, int use_lengths, int64_t *n_used,
                    int64_t *n_skipped);

/* The lattice and the depth used.  lo: three finite floats on the host; h > 0 and finite; 3 <= depth <= 9; fulldepth >= 0;
 * samples_per_node >= 0 and finite.  occ (may be NULL): depth + 1 int64, occ[l] = the distinct home nodes of level l for l >= 2, 0 below. */
int nwo_plan(nwo_ctx *ctx, const float *lo, float h, int depth, int fulldepth, double samples_per_node, int *depth_used, int64_t *occ);

/* Phase by phase.  nwo_level_begin: splat, system, and chi = 0 (level 2) or the prolongation of the chi at hand, which must be that of
 * level - 1; 2 <= level <= depth used.  alpha > 0 and finite. */
int nwo_level_begin(nwo_ctx *ctx, int level, double alpha);
/* sweeps >= 0 red-black sweeps of the level at hand; the largest residual before and after them (each may be NULL) */
int nwo_relax(nwo_ctx *ctx, int sweeps, double *res_before, double *res_after);
/* an array of the level at hand into host memory, x fastest */
int nwo_get_level(nwo_ctx *ctx, int what, void *host_dst);
/* replaces the chi of the level at hand by n^3 finite float64 from the host (tests craft a solution with it) */
int nwo_set_chi(nwo_ctx *ctx, const double *host_src);

/* The driver over the same phases: for l = 2 .. depth used: nwo_level_begin(l, alpha), nwo_relax(l == 2 ? coarse_iters : iters).
 * pointweight > 0 and finite, iters >= 0, coarse_iters >= 0.  alpha (may be NULL) = (pointweight occ_used) / n_used; residuals (may be
 * NULL): NWO_RESIDUAL_WORDS doubles, zero where no level ran. */
int nwo_solve(nwo_ctx *ctx, double pointweight, int iters, int coarse_iters, double *alpha, double *residuals);

/* The field of the level at hand, which must be the depth used: thr, E and sum W (each may be NULL). */
int nwo_field(nwo_ctx *ctx, uint64_t *thr, double *E, uint64_t *sum_w);
/* the device pointer of the last nwo_field's F (2^(3 used) uint64, x fastest), NULL if there is none */
const uint64_t *nwo_field_pointer(nwo_ctx *ctx);
int nwo_get_field(nwo_ctx *ctx, uint64_t *host_dst);

#ifdef __cplusplus
}
#endif

#endif
