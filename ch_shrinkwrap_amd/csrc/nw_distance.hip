// The exact distance from points to a triangle mesh on the device (MI355X, gfx950): include/nw_distance.h.
//
//   nwd_set_mesh    (bq::FaceGrid::set_faces)   the mesh query units' shared intake (nw_bq.h): k_bq_face_setup, one thread per face, the
//                                     float64 centroid and rho_f, the largest centroid-to-corner distance, a hair enlarged so that
//                                     rounding can only make a bound weaker; k_bq_rho_reduce, rho_max and the sum of rho_f, one
//                                     workgroup, a fixed order; bq::bounds, the centroids' box
//                   (bq::FaceGrid::bin)   the shared point grid in double over the centroids (bq::size_grid, bq::build_grid); a sorted
//                                     point carries its face id
//   nwd_query       (bq::bounds)      finiteness of the queries
//                   k_md_query        one thread per query: rings of cells around its own, as k_ev_nearest walks them, until
//                                     sqrt(lbd^2 + out^2) - rho_max exceeds the best distance; a centroid whose |p - c_f| - rho_f
//                                     exceeds it is passed over, every other face gets the exact test of nw_distance_core.h;
//                                     (d2, face) compared lexicographically, so the order inside a cell never shows; then the
//                                     pseudonormal of the winning feature (the fan walk through `twin`) and the sign; the block's sum
//                                     of dist^2 in a fixed order
//                   k_md_sum_final    the blocks' partial sums, one workgroup, a fixed order
//
// The scan, the point grid, the face grid, the device buffer with its staging and the context's scaffolding are the query units' shared
// ones (nw_bq.h); what is this unit's own about the grid is its starting cell size (twice the mean rho_f: a face or two per occupied
// cell).  All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <climits>
#include <string>
#include <algorithm>

#include "../../include/nw_distance.h"
#include "nw_bq.h"
#include "nw_distance_core.h"

#define NWD_EXPORT extern "C" __attribute__((visibility("default")))
#define NWD_BLOCK 256
#define NWD_SLACK BQ_FACE_RHO_SLACK   // relative slack of every bound: far above the rounding of a float64 distance, far below what matters

// ---- the query --------------------------------------------------------------------------------------------------------------------------
struct md_best {
    double d2, d;             // the best squared distance and its square root
    double c[3];              // the closest point
    int face, feature;
};

// the faces whose centroids lie in cells [c0, c1] of one row against the query
__device__ __forceinline__ void md_scan_cells(const bq::PtF64 *__restrict__ pts, const int *__restrict__ cstart, int c0, int c1, const double *q,
                                              const float *__restrict__ pos, const int *__restrict__ faces, const double *__restrict__ rho, int nf,
                                              md_best &b)
{
    const int s = cstart[c0], e = cstart[c1 + 1];
    for (int p = s; p < e; ++p) {
        const bq::PtF64 r = pts[p];
        const int f = (int)r.i;
        if (f < 0 || f >= nf) continue;                           // (cannot happen: the grid's points are numbered by face)
        const double ex = r.x - q[0], ey = r.y - q[1], ez = r.z - q[2];
        const double cd = sqrt((ex * ex + ey * ey) + ez * ez);
        if (cd * (1.0 - NWD_SLACK) - rho[f] > b.d) continue;      // the whole face is farther than the best
        const int ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
        double c[3];
        int feature;
        const double d2 = nwd_point_triangle(q, pos + 3 * (int64_t)ia, pos + 3 * (int64_t)ib, pos + 3 * (int64_t)ic, c, &feature);
        if (d2 < b.d2 || (d2 == b.d2 && f < b.face)) {
            b.d2 = d2; b.d = sqrt(d2); b.c[0] = c[0]; b.c[1] = c[1]; b.c[2] = c[2]; b.face = f; b.feature = feature;
        }
    }
}

__global__ __launch_bounds__(NWD_BLOCK) void k_md_query(const double *__restrict__ xyz, int nq, const float *__restrict__ pos, const int *__restrict__ faces,
                                                        const int *__restrict__ twin, int nf, const bq::PtF64 *__restrict__ pts,
                                                        const int *__restrict__ cstart, const double *__restrict__ rho, double rho_max, bq::Grid<double> g,
                                                        int flags, double *__restrict__ dist, double *__restrict__ closest, int *__restrict__ face_out,
                                                        int *__restrict__ feature_out, double *__restrict__ partial)
{
    __shared__ double s_w[NWD_BLOCK / 64];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double term = 0.0;
    if (i < nq) {
        const double q[3] = {xyz[3 * (int64_t)i], xyz[3 * (int64_t)i + 1], xyz[3 * (int64_t)i + 2]};
        // the query's projection onto the centroids' box: every centroid c has |c - q|^2 >= |c - q'|^2 + |q - q'|^2
        const double px = fmin(fmax(q[0], g.lo[0]), g.hi[0]), py = fmin(fmax(q[1], g.lo[1]), g.hi[1]), pz = fmin(fmax(q[2], g.lo[2]), g.hi[2]);
        const double out2 = (((q[0] - px) * (q[0] - px) + (q[1] - py) * (q[1] - py)) + (q[2] - pz) * (q[2] - pz)) * (1.0 - NWD_SLACK);
        const int cx = bq::cell_1d(px, g.lo[0], g.h, g.dims[0]), cy = bq::cell_1d(py, g.lo[1], g.h, g.dims[1]), cz = bq::cell_1d(pz, g.lo[2], g.h, g.dims[2]);
        const int rmax = max(max(max(cx, g.dims[0] - 1 - cx), max(cy, g.dims[1] - 1 - cy)), max(cz, g.dims[2] - 1 - cz));
        md_best b;
        b.d2 = INFINITY; b.d = INFINITY; b.c[0] = b.c[1] = b.c[2] = 0.0; b.face = INT_MAX; b.feature = 0;
        int r = 0;
        for (; r <= rmax; ++r) {
            // a centroid in a cell of ring r lies at least (r - 1) h from q' along one axis (a little less is assumed: cells are
            // floating-point expressions), and its face reaches at most rho_max towards the query; the walk ends when that exceeds the
            // best distance -- strictly, so that equally near faces are all seen
            const double lbd = (double)max(r - 1, 0) * g.h * (1.0 - NWD_SLACK);
            if (sqrt(lbd * lbd + out2) * (1.0 - NWD_SLACK) - rho_max > b.d) break;
            const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dims[2] - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dims[1] - 1);
            const int xa = max(cx - r, 0), xb = min(cx + r, g.dims[0] - 1);
            for (int z = z0; z <= z1; ++z) {
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * g.dims[1] + y) * g.dims[0];
                    if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
                        md_scan_cells(pts, cstart, row + xa, row + xb, q, pos, faces, rho, nf, b);         // a row of the ring's shell
                    } else {
                        if (cx - r >= 0) md_scan_cells(pts, cstart, row + cx - r, row + cx - r, q, pos, faces, rho, nf, b);
                        if (cx + r < g.dims[0]) md_scan_cells(pts, cstart, row + cx + r, row + cx + r, q, pos, faces, rho, nf, b);
                    }
                }
            }
        }
        int feature = b.feature;
        double d = b.d;
        if (b.face == INT_MAX) { b.face = -1; feature = 0; d = NAN; }        // (cannot happen: the grid holds every face)
        else if ((flags & NWD_SIGNED) && twin) {
            double N[3];
            feature |= nwd_pseudonormal(pos, faces, twin, b.face, b.feature, N);
            if (b.d2 > 0.0 && nwd_sign(q, b.c, N) < 0.0) d = -d;
        }
        if (flags & NWD_RINGS) feature |= min(r - 1, 255) << 8;              // the last ring that was walked
        if (dist) dist[i] = d;
        if (closest) { closest[3 * (int64_t)i] = b.c[0]; closest[3 * (int64_t)i + 1] = b.c[1]; closest[3 * (int64_t)i + 2] = b.c[2]; }
        if (face_out) face_out[i] = b.face;
        if (feature_out) feature_out[i] = feature;
        term = d * d;
    }
    // the block's sum: a butterfly within each wave, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(NWD_BLOCK) void k_md_sum_final(const double *__restrict__ partial, int nb, double *__restrict__ out)
{
    __shared__ double s_w[NWD_BLOCK / 64];
    double s = 0.0;
    for (int j = threadIdx.x; j < nb; j += NWD_BLOCK) s += partial[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwd_ctx : bq::Ctx {
    bq::FaceGrid m;               // the mesh of the last nwd_set_mesh and its grid (m.nf == 0: the context holds no mesh)
    bool has_twin = false;
    DevBuf mtwin;
    // nwd_query
    DevBuf up, qmm, dist, closest, face, feature, partial, sum;
};

namespace {

#define NWD_HIP(call) BQ_HIP(call, NWD_ERR_NOMEM, NWD_ERR_HIP)

const bq::FaceCodes NWD_FACE_CODES = {NWD_ERR_BADARG, NWD_ERR_NONFINITE, NWD_ERR_NOMEM, NWD_ERR_HIP};

}  // namespace

NWD_EXPORT int nwd_abi_version(void) { return NWD_ABI_VERSION; }

NWD_EXPORT int nwd_create(int device, nwd_ctx **out) { return bq::create(device, out, NWD_ERR_BADARG, NWD_ERR_HIP); }

NWD_EXPORT void nwd_destroy(nwd_ctx *ctx) { bq::destroy(ctx); }

NWD_EXPORT const char *nwd_last_error(nwd_ctx *ctx) { return bq::last_error(ctx); }

NWD_EXPORT int nwd_set_mesh(nwd_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin)
{
    if (ctx) ctx->m.nf = 0;
    bq::FaceStatus s = bq::check_faces(pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwd_set_mesh", s, NWD_FACE_CODES);
    if (twin && !bq::twin_ok(twin, n_faces)) return fail(ctx, NWD_ERR_BADARG, "nwd_set_mesh: the twin table is not -1 or an involution within [0, 3F)");
    if (!ctx) return NWD_ERR_BADARG;
    NWD_HIP(hipSetDevice(ctx->device));
    bq::FaceGrid &m = ctx->m;
    if (twin) NWD_HIP(bq::upload(ctx->stream, ctx->mtwin, twin, 3 * n_faces));
    s = m.set_faces(ctx->stream, pos, n_vertices, faces, n_faces);
    // cell size: twice the mean rho_f (a face or two per occupied cell of a surface), bq::face_cell's floor, then widened until the grid
    // is within bq::FACE_GRID_RULE
    if (s.ok()) s = m.bin(ctx->stream, bq::face_cell(2.0 * m.rho_mean, m.emax()));
    if (!s.ok()) { m.nf = 0; return bq::face_fail(ctx, "nwd_set_mesh", s, NWD_FACE_CODES); }
    ctx->has_twin = twin != nullptr;
    return NWD_OK;
}

NWD_EXPORT int nwd_query(nwd_ctx *ctx, const double *xyz, int64_t n, int flags, double *dist_out, double *closest_out, int32_t *face_out,
                         int32_t *feature_out, double *sum_sq_out)
{
    if (!xyz || n < 1 || n > (1ll << 30) || (flags & ~(NWD_SIGNED | NWD_RINGS))) return fail(ctx, NWD_ERR_BADARG, "nwd_query: a NULL cloud, a size out of range or an unknown flag");
    if (!ctx) return NWD_ERR_BADARG;
    if (ctx->m.nf < 1) return fail(ctx, NWD_ERR_NOMESH, "nwd_query: the context holds no mesh");
    if ((flags & NWD_SIGNED) && !ctx->has_twin) return fail(ctx, NWD_ERR_BADARG, "nwd_query: NWD_SIGNED needs the twin table that nwd_set_mesh was not given");
    NWD_HIP(hipSetDevice(ctx->device));
    const int nq = (int)n;
    const double *dq = xyz;
    if (!bq::on_device(xyz)) {
        if (!bq::all_finite(xyz, 3 * n)) return fail(ctx, NWD_ERR_NONFINITE, "nwd_query: a query point is not finite");
        NWD_HIP(bq::upload(ctx->stream, ctx->up, xyz, 3 * n));
        dq = ctx->up.as<double>();
    } else {
        bq::Grid<double> box;
        bool finite[2];
        NWD_HIP(bq::bounds<double>(ctx->stream, ctx->qmm, dq, nq, nullptr, 0, &box, finite));
        if (!finite[0]) return fail(ctx, NWD_ERR_NONFINITE, "nwd_query: a query point is not finite");
    }
    const int nb = nblk(nq);
    if (dist_out) NWD_HIP(ctx->dist.ensure(sizeof(double) * (size_t)nq));
    if (closest_out) NWD_HIP(ctx->closest.ensure(sizeof(double) * 3 * (size_t)nq));
    if (face_out) NWD_HIP(ctx->face.ensure(sizeof(int) * (size_t)nq));
    if (feature_out) NWD_HIP(ctx->feature.ensure(sizeof(int) * (size_t)nq));
    NWD_HIP(ctx->partial.ensure(sizeof(double) * (size_t)nb));
    NWD_HIP(ctx->sum.ensure(sizeof(double)));
    hipLaunchKernelGGL(k_md_query, dim3(nb), dim3(NWD_BLOCK), 0, ctx->stream, dq, nq, ctx->m.mpos.as<float>(), ctx->m.mfaces.as<int>(),
                       ctx->has_twin ? ctx->mtwin.as<int>() : nullptr, ctx->m.nf, ctx->m.sorted.as<bq::PtF64>(), ctx->m.cstart.as<int>(), ctx->m.rho.as<double>(),
                       ctx->m.rho_max, ctx->m.g, flags, dist_out ? ctx->dist.as<double>() : nullptr, closest_out ? ctx->closest.as<double>() : nullptr,
                       face_out ? ctx->face.as<int>() : nullptr, feature_out ? ctx->feature.as<int>() : nullptr, ctx->partial.as<double>());
    hipLaunchKernelGGL(k_md_sum_final, dim3(1), dim3(NWD_BLOCK), 0, ctx->stream, ctx->partial.as<double>(), nb, ctx->sum.as<double>());
    NWD_HIP(hipGetLastError());
    if (dist_out) NWD_HIP(hipMemcpyAsync(dist_out, ctx->dist.p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (closest_out) NWD_HIP(hipMemcpyAsync(closest_out, ctx->closest.p, sizeof(double) * 3 * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (face_out) NWD_HIP(hipMemcpyAsync(face_out, ctx->face.p, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (feature_out) NWD_HIP(hipMemcpyAsync(feature_out, ctx->feature.p, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    double sum = 0.0;
    NWD_HIP(hipMemcpyAsync(&sum, ctx->sum.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NWD_HIP(hipStreamSynchronize(ctx->stream));
    if (sum_sq_out) *sum_sq_out = sum;
    return NWD_OK;
}
