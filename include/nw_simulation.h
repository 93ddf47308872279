/*
 * nw_simulation.h -- C-ABI of the SMLM cloud simulator in libnanowrap_hip.so (csrc/nw_simulation.hip, MI355X / gfx950).
 *
 * What it stands in for: the first stage of upstream's evaluation recipe, PointcloudFromShape (recipe_modules/simulation.py:11-61)
 * -> evaluation_utils.generate_smlm_pointcloud_from_shape (:182-263), which upstream runs in NumPy on the host:
 *   nwg_set_program / nwg_eval   -- shape.py's CSG shapes over sdf.py's primitives, as a flat postfix program evaluated in float64;
 *   nwg_normals                  -- sdf.sdf_normals (sdf.py:4-35);
 *   nwg_sample_surface           -- Shape.points' call of PYME.simulation.locify.points_from_sdf (shape.py:75-76).  PYME's sampler is not
 *                                   in the reference tree: this is the project's OWN sampler (a regular lattice with a shell test), see below;
 *   nwg_loc_error                -- util.loc_error (util.py:37-47);
 *   nwg_displace                 -- Shape.__noise (shape.py:49-55, :78-79);
 *   nwg_smlmify                  -- evaluation_utils.smlmify_points (:265-282);
 *   nwg_background               -- the background positions of evaluation_utils.py:230-243.
 *
 * Conventions (as include/nw_evaluation.h, with its own prefix and context):
 *   - every call returns NWG_OK (0) or a negative status; nwg_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked before any HIP call; without a GPU nwg_create fails with NWG_ERR_HIP -- there is no CPU fallback;
 *   - every array is a HOST pointer, row-major and C-contiguous: points, sigmas and normals (n,3) float64;
 *   - every result is deterministic: the same bytes on every run, whatever the launch geometry;
 *   - one nwg_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 *
 * Random numbers.  Counter-based Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
 * 0xBB67AE85).  No generator state lives in memory and nothing depends on the number of threads: every draw is
 *     (w0, w1, w2, w3) = philox4x32_10(counter = (item & 0xffffffff, item >> 32, stream, draw), key = (seed & 0xffffffff, seed >> 32))
 * with `item` the 64-bit index of what the draw belongs to (a lattice node's key, a point, a copy), `stream` the purpose (the caller
 * gives every purpose its own: NWG_STREAM_* below are what ch_shrinkwrap_amd/simulation.py uses) and `draw` the axis 0..2 (0 where
 * there is one draw per item).  From one block:
 *     U0 = ((((uint64)w0 << 32 | w1) >> 11) + 0.5) * 2^-53        a float64 uniform in (0, 1), never 0 or 1;  U1 likewise from (w2, w3)
 *     N  = sqrt(-2 ln U0) * cos(2 pi U1)                          Box-Muller, one normal per block
 *     K  = (uint64)w0 << 32 | w1                                  a 64-bit key
 */
#ifndef NW_SIMULATION_H_
#define NW_SIMULATION_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWG_ABI_VERSION 1
#define NWG_MAX_OPS 256            /* the longest program */
#define NWG_STACK_DEPTH 8          /* the deepest value stack a program may need (kept in registers) */
#define NWG_COORD_BITS 21          /* lattice coordinates are biased by 2^20 and must fit 21 bits: the node key is their 63-bit Morton code */
#define NWG_MAX_CELLS (1ll << 27)  /* the most cells (or candidate nodes) one refinement level may hold */
#define NWG_COPIES 10              /* smlmify_points' max_points_per_cluster */

typedef struct nwg_ctx nwg_ctx;

typedef enum nwg_status {
    NWG_OK = 0,
    NWG_ERR_BADARG = -1,      /* NULL pointer, size out of range, non-finite or non-positive parameter, a malformed program */
    NWG_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwg_last_error */
    NWG_ERR_NONFINITE = -3,   /* a non-finite coordinate or sigma */
    NWG_ERR_NOMEM = -4,
    NWG_ERR_NOPROGRAM = -5,   /* a call that evaluates the shape before nwg_set_program */
    NWG_ERR_CAPACITY = -6,    /* more detected nodes than max_points: nothing was stored */
    NWG_ERR_TOOMANY = -7,     /* a refinement level with more than NWG_MAX_CELLS cells: dx is too small for this cube */
    NWG_ERR_NOPOINTS = -8     /* nwg_get_points while the context holds none */
} nwg_status;

/* One op of the postfix program.  Primitives push the distance of the CURRENT point q; combinators pop d1, then d0, and push. */
typedef enum nwg_opcode {
    NWG_OP_FRAME = 0,         /* q = M (p - t), p the point the program was called with: a[0..8] = M row-major, a[9..11] = t.  Holds until the
                                 next NWG_OP_FRAME; the program starts with q = p.  (RotationShape.sdf, shape.py:479-480, and the `p - centroid`
                                 of Sphere / Torus / Box / Sheet, :108, :125, :240, :250; nested frames are composed by the host.) */
    NWG_OP_SPHERE = 1,        /* a[0] = R                                  sdf.sphere (sdf.py:39-46) */
    NWG_OP_TORUS = 2,         /* a[0] = r, a[1] = R of sdf.torus(p, r, R)  (sdf.py:48-58); shape.Torus passes (major, minor) */
    NWG_OP_CAPSULE = 3,       /* a[0..2] = a, a[3..5] = b, a[6] = r        sdf.capsule (sdf.py:60-77) */
    NWG_OP_ROUND_BOX = 4,     /* a[0..2] = w, a[3] = r                     sdf.round_box (sdf.py:250-269) */
    NWG_OP_SHEET = 5,         /* a[0..2] = w, a[3] = r                     sdf.sheet (sdf.py:271-292) */
    NWG_OP_UNION = 6,         /* a[0] = k                                  UnionShape.sdf (shape.py:369-376) */
    NWG_OP_DIFFERENCE = 7,    /* a[0] = k                                  DifferenceShape.sdf (shape.py:403-410): d1's shape with d0's carved out */
    NWG_OP_INTERSECTION = 8   /* a[0] = k                                  IntersectionShape.sdf (shape.py:437-444) */
} nwg_opcode;

typedef struct nwg_op {
    int32_t code;
    int32_t reserved;         /* 0 */
    double a[12];
} nwg_op;

/* what ch_shrinkwrap_amd/simulation.py passes as `stream`: one per purpose */
enum {
    NWG_STREAM_THIN = 0, NWG_STREAM_PHOTONS = 1, NWG_STREAM_DISPLACE = 2, NWG_STREAM_COPY_DISPLACE = 3, NWG_STREAM_COPY_KEY = 4,
    NWG_STREAM_COPY_PHOTONS = 5, NWG_STREAM_BG_POSITION = 6, NWG_STREAM_BG_PHOTONS = 7, NWG_STREAM_BG_COPY_DISPLACE = 8,
    NWG_STREAM_BG_COPY_KEY = 9, NWG_STREAM_BG_COPY_PHOTONS = 10
};

#define NWG_MODEL_CONSTANT 0      /* util.loc_error's `else` branch (util.py:44-45): sigma = 10.0 everywhere */
#define NWG_MODEL_EXPONENTIAL 1   /* model == 'exponential' (util.py:38-43) */

int nwg_abi_version(void);
int nwg_create(int device, nwg_ctx **out);
void nwg_destroy(nwg_ctx *ctx);
const char *nwg_last_error(nwg_ctx *ctx);

/* The shape of every later call (shape.py's classes, compiled by the host: ch_shrinkwrap_amd/simulation.py compile_shape).  Checked here:
 * 1..NWG_MAX_OPS ops, known codes, finite arguments, k >= 0, a capsule's two ends apart (|b - a|^2 > 0 in float64: sdf.capsule divides by
 * it, and upstream's result for a == b is NaN at every point), the stack never deeper than NWG_STACK_DEPTH or empty under a combinator,
 * exactly one value left at the end. */
int nwg_set_program(nwg_ctx *ctx, const nwg_op *ops, int n_ops);

/* d_out[i] = the program at xyz[i], float64, sdf.py's expressions operation for operation (no contraction). */
int nwg_eval(nwg_ctx *ctx, const double *xyz, int64_t n, double *d_out);

/* sdf.sdf_normals (sdf.py:4-35): the central difference at delta = 0.1 (each side delta / 2 away), normalised. */
int nwg_normals(nwg_ctx *ctx, const double *xyz, int64_t n, double *normals_out);

/* The project's sampler, in the place of points_from_sdf(sdf, r_max, centre, dx_min, p) (shape.py:75-76).  Lattice nodes are
 * centre + i dx, i integer per axis; the bounding cube is |i dx| <= r_max per axis.  The cube is covered by cells of 2^L nodes a side
 * (aligned to the biased integer lattice, so a cell's Morton code is its nodes' keys >> 3L); a cell is kept when
 * |sdf(cell centre)| <= lipschitz * (sqrt(3) / 2) dx 2^L + dx / 2 and split into eight, level by level (scan and compaction per level)
 * down to single nodes.  A node inside the cube is a fluorophore if -dx/2 <= sdf < dx/2 (expected number: area / dx^2, whatever the
 * surface's orientation) and detected if U0(seed, item = node key, NWG_STREAM_THIN, draw 0) < p.  Only detected nodes are stored, in
 * ascending node key, on the device; *n_out = their number (0 is a valid result).  `project` Newton steps x <- x - sdf g / |g|^2, g the
 * central difference at delta = 0.1 (sdf.grad_sdf), pull each onto the zero level set; project = 0 keeps the lattice nodes.
 * start_level: the L the refinement starts at, -1 = the smallest with at most 8 cells an axis; the result does not depend on it.
 * The start cells are listed by the host: a start_level that gives more than 2^24 of them is refused (NWG_ERR_BADARG).
 * More than max_points detected nodes: NWG_ERR_CAPACITY, and the context holds no points. */
int nwg_sample_surface(nwg_ctx *ctx, const double *centre, double r_max, double dx, double p, uint64_t seed, double lipschitz,
                       int start_level, int project, int64_t max_points, int64_t *n_out);

/* The points the context holds since the last nwg_sample_surface: node keys (n) uint64 and positions (n,3) float64.  Either may be NULL. */
int nwg_get_points(nwg_ctx *ctx, uint64_t *keys_out, double *xyz_out);

/* util.loc_error(shape = (n, 3), model, psf_width, mean_photon_count, bg_photon_count) (util.py:37-47).  NWG_MODEL_EXPONENTIAL: per
 * item i and axis a the photon number l = bg + mean * (-ln U0(seed, i, stream, a)) -- upstream draws Exp(mean), drops l <= bg and takes
 * the first n: the same distribution, as the exponential is memoryless -- and sigma = (psf_width[a] / 2.355) / sqrt(l).
 * photons_out (n,3) may be NULL.  NWG_MODEL_CONSTANT: sigma = 10.0, photons (if asked for) 0. */
int nwg_loc_error(nwg_ctx *ctx, int64_t n, uint64_t seed, uint32_t stream, int model, const double *psf_width, double mean_photon_count,
                  double bg_photon_count, double *sigma_out, double *photons_out);

/* out[i][a] = xyz[i][a] + sigma[i][a] * N(seed, i, stream, a) (Shape.__noise, shape.py:54-55, added at :78). */
int nwg_displace(nwg_ctx *ctx, const double *xyz, const double *sigma, int64_t n, uint64_t seed, uint32_t stream, double *out);

/* smlmify_points (evaluation_utils.py:265-282).  Copy j = c n + i (c < NWG_COPIES) of point i is xyz[i] + sigma[i] * N(seed, j,
 * stream_displace, axis) (:269).  sz of the NWG_COPIES n copies are chosen uniformly without replacement (:274): copy j has the key
 * K(seed, j, stream_key, 0) and the sz smallest keys are kept (equal keys: the smaller j first), found by a radix select that never
 * stores the keys; they are emitted in copy order.  Every kept copy gets a freshly drawn sigma (:277-280: not its source's, as
 * upstream): nwg_loc_error's expression with item = j and stream_photons.  copy_out (sz) int64 may be NULL: the j of every kept copy
 * (its source is j % n). */
int nwg_smlmify(nwg_ctx *ctx, const double *xyz, const double *sigma, int64_t n, int64_t sz, uint64_t seed, uint32_t stream_displace,
                uint32_t stream_key, uint32_t stream_photons, int model, const double *psf_width, double mean_photon_count,
                double bg_photon_count, double *xyz_out, double *sigma_out, int64_t *copy_out);

/* n positions uniform in the box [lo, hi] (evaluation_utils.py:242-243): out[i][a] = U0(seed, i, stream, a) * (hi[a] - lo[a]) + lo[a]. */
int nwg_background(nwg_ctx *ctx, const double *lo, const double *hi, int64_t n, uint64_t seed, uint32_t stream, double *xyz_out);

#ifdef __cplusplus
}
#endif

#endif
