/*
 * nw_skeleton.h -- C-ABI of the centreline graph of a mesh in libnanowrap_hip.so (csrc/nw_skeleton.hip, MI355X / gfx950): the level-set
 * diagram of a scalar field on the mesh, as nodes (one per connected piece of a band of the field), arcs between the nodes of
 * neighbouring bands that touch, and per node the integer sums from which its position and its cross-section's perimeter follow.
 *
 * What it is for: how many tubes a fitted network has, how long and how thick they are, how many junctions and loops, and where the
 * centreline runs.  Upstream answers with SkeletonizeMembrane (mean-curvature flow with Voronoi poles and a remesher of its own); that
 * method is iterative and not a function of its input, and is not mirrored.  The definition here is this project's own and is written
 * down in csrc/nw_skeleton_core.h; tests/mesh_skeleton_ref.py restates it in NumPy.
 *
 * THIS IS A LEVEL-SET DIAGRAM OF ONE FIELD, NOT A MEDIAL AXIS.  It depends on the field and so on the source the field was grown from.
 * A sheet becomes a chain.  A LOOP NARROWER THAN A BAND VANISHES.
 *
 * Definitions:
 *   - the mesh is (n_vertices,3) float32 positions, a host or a device pointer, (n_faces,3) int32 faces and the (3 n_faces) int32
 *     half-edge twins, host pointers: twin[3f+k] is the half-edge that runs the other way along faces[f][k] -> faces[f][(k+1)%3], -1 on
 *     a border; it must be mutual (a mesh with a non-manifold edge has no such table and is refused);
 *   - the field D is one float64 per vertex, finite or +inf, a host or a device pointer; the band width w > 0 is a float64;
 *   - b(v) = floor(D[v] / w); a vertex with D = +inf or D < 0 is dead, and so is every face with a dead corner; a nan and a band beyond
 *     2^30 are NWA_ERR_BADARG;
 *   - a live face f has the pieces (f, k), min b <= k <= max b over its corners, stored face after face, band ascending; piece_start
 *     (n_faces + 1) is the exclusive scan of the spans; more than 2^28 pieces is NWA_ERR_BADARG, and the text names the band width;
 *   - across every interior edge {u, v} of two live faces f, g the pieces (f, k) and (g, k) are joined for min(b(u), b(v)) <= k <=
 *     max(b(u), b(v)); nodes are the connected components of pieces, numbered in the order of their smallest piece;
 *   - arcs are the distinct pairs {node(f, k), node(f, k + 1)}, (smaller, larger), sorted;
 *   - a piece's contour segment joins the two points where the level (k + 1/2) w crosses the face's edges, each computed from the edge's
 *     below end; positions are quantised relative to the bounding box's lower corner with a power-of-two quantum; per node the sums of
 *     NWA_S_COLUMNS integers (csrc/nw_skeleton_core.h has the columns, the quantum and the proof that none overflows);
 *   - vertex_node[v] = the smallest node among the pieces (f, b(v)) of the faces round v, -1 if there is none.
 *   Every output but the info words named below is a function of the input alone: not of launch geometry or of the order of the atomics.
 *
 * How it is computed.  k_sk_bands (bands, spans), the shared exclusive scan, k_sk_init, k_sk_hook (one lane per half-edge h < twin[h]:
 * a lock-free union-find, the larger root hooked under the smaller with a compare-and-swap; the lane's loop runs over the edge's band
 * range), k_sk_compress, the scan over the root flags, k_sk_number, k_sk_sums (one lane per piece, 64-bit integer atomic adds),
 * k_sk_arcs (one key per piece with a band above it), k_sk_vertex (atomic min), k_sk_totals.  No workgroup waits on another.  The arc
 * keys are sorted and made distinct on the host after their download.
 *
 * info[]: HOOK_RETRIES, ATOMICS and the *_US words depend on the hardware's scheduling or on the clock: THEY ARE NOT DETERMINISTIC and
 * belong in no bit comparison.  The *_US words are filled only with NWA_FLAG_TIMING, which waits for the stream after every stage.
 *
 * Conventions (as include/nw_geodesic.h, with its own prefix and context):
 *   - every call returns NWA_OK (0) or a negative status; nwa_last_error(ctx) gives text; nothing is thrown across the ABI;
 *   - arguments are checked on the host before any HIP call, and nothing is written on refusal; without a GPU nwa_create fails with
 *     NWA_ERR_HIP -- there is no CPU fallback;
 *   - a device pointer is read on the context's own stream with no ordering against the stream that wrote it: it must be complete
 *     before the call and unchanged until it returns;
 *   - one nwa_ctx = one device + one HIP stream; a ctx is not thread-safe, distinct ctxs are independent.
 */
#ifndef NW_SKELETON_H_
#define NW_SKELETON_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWA_ABI_VERSION 1
#define NWA_FLAG_TIMING 1

/* info[]: int64 words */
#define NWA_INFO_WORDS 24
#define NWA_INFO_PIECES 0           /* P */
#define NWA_INFO_NODES 1
#define NWA_INFO_ARCS 2
#define NWA_INFO_LIVE_FACES 3
#define NWA_INFO_LIVE_VERTICES 4
#define NWA_INFO_SEGMENTS 5         /* pieces with a contour segment */
#define NWA_INFO_MAX_BAND 6         /* the largest band of a live vertex, -1 for none */
#define NWA_INFO_ARC_KEYS 7         /* pieces with a band above them: the keys before they are made distinct */
#define NWA_INFO_HOOK_RETRIES 8     /* not deterministic: compare-and-swaps of k_sk_hook that lost */
#define NWA_INFO_ATOMICS 9          /* not deterministic: compare-and-swaps issued by k_sk_hook */
#define NWA_INFO_BANDS_US 10        /* not deterministic, with NWA_FLAG_TIMING: microseconds of k_sk_bands and its totals */
#define NWA_INFO_SCAN_US 11         /*   the two scans */
#define NWA_INFO_INIT_US 12         /*   k_sk_init */
#define NWA_INFO_HOOK_US 13         /*   k_sk_hook */
#define NWA_INFO_COMPRESS_US 14     /*   k_sk_compress and k_sk_number */
#define NWA_INFO_SUMS_US 15         /*   k_sk_sums */
#define NWA_INFO_ARCS_US 16         /*   k_sk_arcs */
#define NWA_INFO_VERTEX_US 17       /*   k_sk_vertex and the last totals */
#define NWA_INFO_KEYS_DOWNLOAD_US 18 /*  the download of the arc keys */
#define NWA_INFO_DEDUP_US 19        /*   sorting them and dropping duplicates, on the host */
#define NWA_INFO_UPLOAD_US 20       /*   the field's upload or copy */

#define NWA_SUM_COLUMNS 12          /* uint64 words per node in node_sums (csrc/nw_skeleton_core.h: NWA_S_*) */

typedef struct nwa_ctx nwa_ctx;

typedef enum nwa_status {
    NWA_OK = 0,
    NWA_ERR_BADARG = -1,      /* NULL pointer, size or id out of range, twins missing or not mutual, bad width, nan or a band beyond 2^30
                                 in the field, more than 2^28 pieces */
    NWA_ERR_HIP = -2,         /* a HIP runtime call failed (also: no GPU); text in nwa_last_error */
    NWA_ERR_NONFINITE = -3,   /* a non-finite position */
    NWA_ERR_NOMEM = -4,
    NWA_ERR_NOMESH = -5,      /* nwa_skeleton before nwa_set_mesh */
    NWA_ERR_NORESULT = -6     /* nwa_fetch before a nwa_skeleton that succeeded */
} nwa_status;

int nwa_abi_version(void);
int nwa_create(int device, nwa_ctx **out);
void nwa_destroy(nwa_ctx *ctx);
const char *nwa_last_error(nwa_ctx *ctx);

/* Takes the mesh into the context; it stays for any number of nwa_skeleton calls (until the next nwa_set_mesh; a failed call leaves the
 * context without a mesh).  on_device = 0: positions is a host pointer; 1: a device pointer, of which the call takes a host copy for the
 * bounding box.  faces and twin are host pointers either way.  quantum_out, optional: 4 float64, the bounding box's lower corner and q. */
int nwa_set_mesh(nwa_ctx *ctx, const float *positions, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin, int on_device,
                 double *quantum_out);

/* The first of two calls: computes everything and leaves it in the context; info_out (NWA_INFO_WORDS int64, a host pointer) tells the
 * sizes.  field: (n_vertices) float64, a host (on_device = 0) or a device pointer (1).  flags = 0 or NWA_FLAG_TIMING. */
int nwa_skeleton(nwa_ctx *ctx, const double *field, int on_device, double band_width, int flags, int64_t *info_out);

/* The second: copies the last nwa_skeleton's result into host arrays, each of which may be NULL: piece_start (n_faces + 1) int32,
 * piece_node (P) int32, vertex_node (n_vertices) int32, node_band (N) int32, node_sums (N, NWA_SUM_COLUMNS) uint64, arcs (A, 2) int32. */
int nwa_fetch(nwa_ctx *ctx, int32_t *piece_start, int32_t *piece_node, int32_t *vertex_node, int32_t *node_band, uint64_t *node_sums, int32_t *arcs);

#ifdef __cplusplus
}
#endif

#endif
