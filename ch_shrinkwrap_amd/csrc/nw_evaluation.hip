// The fit-quality metric on the device (MI355X, gfx950): include/nw_evaluation.h.
//
// Upstream's evaluation recipe (ch_shrinkwrap/evaluation_utils.py) lays a regular grid over every triangle of the fitted mesh
// (points_from_mesh, :35-150) and takes nearest-neighbour squared distances both ways between those samples and a cloud on the true
// surface (average_squared_distance, :153-180).  Here:
//
//   mesh sampling   k_ev_face_setup   one thread per face: the float32 set-up of nw_evaluation_core.h, the number of grid nodes
//                   (scan)            node offsets per face
//                   k_ev_node_test    one thread per node: its face by bisection of the offsets, the three float64 inequalities
//                   (scan)            output slots
//                   k_ev_emit         one thread per node inside its triangle: position and face id
//                   The order is the host function's by construction: nodes are numbered by face, row-major within a face.
//   nearest         (bq::bounds, bq::size_grid, bq::build_grid)   the query units' shared point grid in double: bounding box of the
//                                     reference cloud and finiteness of both, counting sort of the reference cloud by cell
//                   k_ev_nearest      one thread per query: rings of cells around its own until the ring's lower bound exceeds the best
//                                     squared distance; (d2, index) compared lexicographically, so the order inside a cell (the scatter's
//                                     atomics) never shows; the block's sum of dist^2 in a fixed order
//                   k_ev_sum_final    the blocks' partial sums, one workgroup, a fixed order
//
// The scan, the point grid, the device buffer with its staging and the context's scaffolding are the query units' shared ones (nw_bq.h);
// what is this unit's own about the grid is its starting cell size and its limits (NWE_GRID_RULE).
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <climits>
#include <string>
#include <algorithm>

#include "../../include/nw_evaluation.h"
#include "nw_bq.h"
#include "nw_evaluation_core.h"

#define NWE_EXPORT extern "C" __attribute__((visibility("default")))
#define NWE_BLOCK 256
#define NWE_FACE_NODE_CLIP (1ll << 31)          // a face's node count enters the 64-bit total clipped to this (> NWE_MAX_NODES)

typedef unsigned long long u64;

// ---- mesh sampling --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NWE_BLOCK) void k_ev_face_setup(const float *__restrict__ pos, const int *__restrict__ faces, int nf, double dx,
                                                             nwe_face_setup *__restrict__ setup, int *__restrict__ count, u64 *__restrict__ total)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    long long c = 0;
    if (f < nf) {
        const int a = faces[3 * f], b = faces[3 * f + 1], d = faces[3 * f + 2];
        nwe_face_setup s;
        nwe_setup_face(pos + 3 * (int64_t)a, pos + 3 * (int64_t)b, pos + 3 * (int64_t)d, dx, &s);
        setup[f] = s;
        c = min((long long)s.nx * (long long)s.ny, NWE_FACE_NODE_CLIP);
        count[f] = (int)min(c, (long long)INT_MAX);           // (only used when the total is within NWE_MAX_NODES: nothing was clipped then)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(total, (u64)c);
}

// the face of node i: the last f with off[f] <= i (faces without nodes share their offset with the next one)
__device__ __forceinline__ int ev_face_of(const int *__restrict__ off, int nf, int i)
{
    int lo = 0, hi = nf;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_node_test(const nwe_face_setup *__restrict__ setup, const int *__restrict__ off, int nf, int n_nodes,
                                                            double dx, int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const int f = ev_face_of(off, nf, i);
    const nwe_face_setup s = setup[f];
    double X, Y;
    flag[i] = nwe_node_inside(&s, (int64_t)(i - off[f]), dx, &X, &Y) ? 1 : 0;
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_emit(const nwe_face_setup *__restrict__ setup, const int *__restrict__ off, int nf, int n_nodes, double dx,
                                                       const int *__restrict__ flag, const int *__restrict__ slot, int n_out,
                                                       double *__restrict__ pos_out, int *__restrict__ face_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes || !flag[i]) return;
    const int o = slot[i];
    if (o < 0 || o >= n_out) return;                          // (cannot happen: slot is the scan of flag)
    const int f = ev_face_of(off, nf, i);
    const nwe_face_setup s = setup[f];
    double X, Y, p[3];
    (void)nwe_node_inside(&s, (int64_t)(i - off[f]), dx, &X, &Y);
    nwe_node_position(&s, X, Y, p);
    pos_out[3 * (int64_t)o] = p[0];
    pos_out[3 * (int64_t)o + 1] = p[1];
    pos_out[3 * (int64_t)o + 2] = p[2];
    face_out[o] = f;
}

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------------
// the points of cells [c0, c1] of one row against the query
__device__ __forceinline__ void ev_scan_cells(const bq::PtF64 *__restrict__ pts, const int *__restrict__ cstart, int c0, int c1, double qx, double qy, double qz,
                                              double &best, long long &best_i)
{
    const int s = cstart[c0], e = cstart[c1 + 1];
    for (int p = s; p < e; ++p) {
        const bq::PtF64 r = pts[p];
        const double ex = r.x - qx, ey = r.y - qy, ez = r.z - qz;
        const double d2 = (ex * ex + ey * ey) + ez * ez;
        if (d2 < best || (d2 == best && r.i < best_i)) { best = d2; best_i = r.i; }
    }
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_nearest(const double *__restrict__ q, int nq, const bq::PtF64 *__restrict__ pts, const int *__restrict__ cstart,
                                                          bq::Grid<double> g, double *__restrict__ dist, int *__restrict__ idx, double *__restrict__ partial)
{
    __shared__ double s_w[NWE_BLOCK / 64];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double term = 0.0;
    if (i < nq) {
        const double qx = q[3 * (int64_t)i], qy = q[3 * (int64_t)i + 1], qz = q[3 * (int64_t)i + 2];
        // the query's projection onto the reference cloud's box: every reference point p has |p - q|^2 >= |p - q'|^2 + |q - q'|^2
        const double px = fmin(fmax(qx, g.lo[0]), g.hi[0]), py = fmin(fmax(qy, g.lo[1]), g.hi[1]), pz = fmin(fmax(qz, g.lo[2]), g.hi[2]);
        const double out2 = (((qx - px) * (qx - px) + (qy - py) * (qy - py)) + (qz - pz) * (qz - pz)) * (1.0 - 1e-9);
        const int cx = bq::cell_1d(px, g.lo[0], g.h, g.dims[0]), cy = bq::cell_1d(py, g.lo[1], g.h, g.dims[1]), cz = bq::cell_1d(pz, g.lo[2], g.h, g.dims[2]);
        const int rmax = max(max(max(cx, g.dims[0] - 1 - cx), max(cy, g.dims[1] - 1 - cy)), max(cz, g.dims[2] - 1 - cz));
        double best = INFINITY;
        long long best_i = LLONG_MAX;
        for (int r = 0; r <= rmax; ++r) {
            // a point in a cell of ring r lies at least (r - 1) h from q' along one axis (a little less is assumed: cells are floating-point
            // expressions); the walk ends when that exceeds the best distance -- strictly, so that equally near points are all seen
            const double lbd = (double)max(r - 1, 0) * g.h * (1.0 - 1e-9);
            if (lbd * lbd + out2 > best) break;
            const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dims[2] - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dims[1] - 1);
            const int xa = max(cx - r, 0), xb = min(cx + r, g.dims[0] - 1);
            for (int z = z0; z <= z1; ++z) {
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * g.dims[1] + y) * g.dims[0];
                    if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
                        ev_scan_cells(pts, cstart, row + xa, row + xb, qx, qy, qz, best, best_i);      // a row of the ring's shell
                    } else {
                        if (cx - r >= 0) ev_scan_cells(pts, cstart, row + cx - r, row + cx - r, qx, qy, qz, best, best_i);
                        if (cx + r < g.dims[0]) ev_scan_cells(pts, cstart, row + cx + r, row + cx + r, qx, qy, qz, best, best_i);
                    }
                }
            }
        }
        const double d = sqrt(best);
        if (dist) dist[i] = d;
        if (idx) idx[i] = (int)best_i;
        term = d * d;
    }
    // the block's sum: a butterfly within each wave, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_sum_final(const double *__restrict__ partial, int nb, double *__restrict__ out)
{
    __shared__ double s_w[NWE_BLOCK / 64];
    double s = 0.0;
    for (int j = threadIdx.x; j < nb; j += NWE_BLOCK) s += partial[j];
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

struct nwe_ctx : bq::Ctx {
    // the samples of the last nwe_sample_mesh
    int64_t n_samples = 0;
    DevBuf samples, sample_face;
    // nwe_sample_mesh
    DevBuf mpos, mfaces, setup, count, off, flag, slot, total;
    // nwe_nearest
    DevBuf up0, up1, mm, cell, ccount, cstart, sorted, dist, idx, partial, sum;
    DevBuf scan_tmp;
};

namespace {

#define NWE_HIP(call) BQ_HIP(call, NWE_ERR_NOMEM, NWE_ERR_HIP)

bool cloud_args_ok(const double *p, int64_t n)
{
    return p ? (n >= 1 && n <= (1ll << 30)) : n == NWE_SAMPLES;
}

// the cloud as a device pointer: the held samples, a device pointer read in place, or a host pointer copied into `stage`
// (n fits an int: cloud_args_ok has let through at most 2^30 points, and the held samples are at most NWE_MAX_NODES = 2^30;
// a device pointer must be complete before the call: nothing orders this stream after its producer's)
int resolve(nwe_ctx *ctx, const double *p, int64_t n, DevBuf &stage, const double **dev, int *n_out)
{
    if (!p) {
        *dev = ctx->samples.as<double>();
        *n_out = (int)ctx->n_samples;
        return NWE_OK;
    }
    *n_out = (int)n;
    if (bq::on_device(p)) { *dev = p; return NWE_OK; }
    NWE_HIP(bq::upload(ctx->stream, stage, p, 3 * n));
    *dev = stage.as<double>();
    return NWE_OK;
}

// at most max(2 n, 65536) cells, up to 2^28; at most 1025 an axis; 400 widening steps
const bq::GridRule NWE_GRID_RULE = {2, 1ll << 28, 1025, 400};

// both clouds on the device already
int nearest_dev(nwe_ctx *ctx, const double *dref, int nr, const double *dq, int nq, double *dist_out, int32_t *idx_out, double *sum_out)
{
    bq::Grid<double> g;
    bool finite[2];
    NWE_HIP(bq::bounds<double>(ctx->stream, ctx->mm, dref, nr, dq, nq, &g, finite));
    if (!finite[0]) return fail(ctx, NWE_ERR_NONFINITE, "nwe_nearest: a reference point is not finite");
    if (!finite[1]) return fail(ctx, NWE_ERR_NONFINITE, "nwe_nearest: a query point is not finite");
    double ext[3], emax = 0.0;
    for (int d = 0; d < 3; ++d) { ext[d] = g.hi[d] - g.lo[d]; emax = std::max(emax, ext[d]); }
    if (!std::isfinite(emax)) return fail(ctx, NWE_ERR_BADARG, "nwe_nearest: the reference cloud's extent is not a finite double");
    // cell size: about one reference point per cell of the box (the flattest axis counts as a thousandth of the widest), at most 1025
    // cells an axis (1 for a cloud without extent); then widened until the grid is within NWE_GRID_RULE
    g.h = 1.0;
    if (emax > 0.0) {
        g.h = std::cbrt(std::max(ext[0], 1e-3 * emax) * std::max(ext[1], 1e-3 * emax) * std::max(ext[2], 1e-3 * emax) / nr);
        g.h = std::max(g.h, emax / 1024.0);
        if (!(g.h > 0.0) || !std::isfinite(g.h)) g.h = emax;
    }
    if (!bq::size_grid(NWE_GRID_RULE, nr, ext, &g.h, g.dims)) return fail(ctx, NWE_ERR_BADARG, "nwe_nearest: no cell size keeps the grid within its cap");
    int total = -1;
    NWE_HIP(bq::build_grid<double>(ctx->stream, dref, nr, g, ctx->cell, ctx->ccount, ctx->scan_tmp, ctx->cstart, ctx->sorted, &total));
    if (total != nr) return fail(ctx, NWE_ERR_HIP, "nwe_nearest: the cell counts do not add up to the reference points");
    // the queries
    const int nb = nblk(nq);
    if (dist_out) NWE_HIP(ctx->dist.ensure(sizeof(double) * (size_t)nq));
    if (idx_out) NWE_HIP(ctx->idx.ensure(sizeof(int) * (size_t)nq));
    NWE_HIP(ctx->partial.ensure(sizeof(double) * (size_t)nb));
    NWE_HIP(ctx->sum.ensure(sizeof(double)));
    hipLaunchKernelGGL(k_ev_nearest, dim3(nb), dim3(NWE_BLOCK), 0, ctx->stream, dq, nq, ctx->sorted.as<bq::PtF64>(), ctx->cstart.as<int>(), g,
                       dist_out ? ctx->dist.as<double>() : nullptr, idx_out ? ctx->idx.as<int>() : nullptr, ctx->partial.as<double>());
    hipLaunchKernelGGL(k_ev_sum_final, dim3(1), dim3(NWE_BLOCK), 0, ctx->stream, ctx->partial.as<double>(), nb, ctx->sum.as<double>());
    NWE_HIP(hipGetLastError());
    if (dist_out) NWE_HIP(hipMemcpyAsync(dist_out, ctx->dist.p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (idx_out) NWE_HIP(hipMemcpyAsync(idx_out, ctx->idx.p, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    double sum = 0.0;
    NWE_HIP(hipMemcpyAsync(&sum, ctx->sum.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NWE_HIP(hipStreamSynchronize(ctx->stream));
    if (sum_out) *sum_out = sum;
    return NWE_OK;
}

}  // namespace

NWE_EXPORT int nwe_abi_version(void) { return NWE_ABI_VERSION; }

NWE_EXPORT int nwe_create(int device, nwe_ctx **out) { return bq::create(device, out, NWE_ERR_BADARG, NWE_ERR_HIP); }

NWE_EXPORT void nwe_destroy(nwe_ctx *ctx) { bq::destroy(ctx); }

NWE_EXPORT const char *nwe_last_error(nwe_ctx *ctx) { return bq::last_error(ctx); }

NWE_EXPORT int nwe_sample_mesh(nwe_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double dx, int64_t *n_out)
{
    if (!n_out || !(dx > 0.0) || !std::isfinite(dx)) return NWE_ERR_BADARG;
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return NWE_ERR_BADARG;
    if (!ctx) return NWE_ERR_BADARG;
    *n_out = 0;
    ctx->n_samples = 0;
    NWE_HIP(hipSetDevice(ctx->device));
    const int nf = (int)n_faces;
    NWE_HIP(bq::upload(ctx->stream, ctx->mpos, pos, 3 * n_vertices));
    NWE_HIP(bq::upload(ctx->stream, ctx->mfaces, faces, 3 * n_faces));
    NWE_HIP(ctx->setup.ensure(sizeof(nwe_face_setup) * (size_t)nf));
    NWE_HIP(ctx->count.ensure(sizeof(int) * (size_t)nf));
    NWE_HIP(ctx->off.ensure(sizeof(int) * (size_t)(nf + 1)));
    NWE_HIP(ctx->total.ensure(sizeof(u64)));
    NWE_HIP(hipMemsetAsync(ctx->total.p, 0, sizeof(u64), ctx->stream));
    // pass 1: set-up and node count per face
    hipLaunchKernelGGL(k_ev_face_setup, dim3(nblk(nf)), dim3(NWE_BLOCK), 0, ctx->stream, ctx->mpos.as<float>(), ctx->mfaces.as<int>(), nf, dx,
                       ctx->setup.as<nwe_face_setup>(), ctx->count.as<int>(), ctx->total.as<u64>());
    NWE_HIP(hipGetLastError());
    u64 total = 0;
    NWE_HIP(hipMemcpyAsync(&total, ctx->total.p, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    NWE_HIP(hipStreamSynchronize(ctx->stream));
    if (total > (u64)NWE_MAX_NODES) return fail(ctx, NWE_ERR_TOOMANY, "nwe_sample_mesh: " + std::to_string(total) + " grid nodes, more than NWE_MAX_NODES");
    if (total == 0) return NWE_OK;
    const int n_nodes = (int)total;
    NWE_HIP(bq::scan_exclusive(ctx->stream, ctx->count.as<int>(), nf, ctx->off.as<int>(), ctx->scan_tmp));
    // pass 2: the nodes inside their triangle
    NWE_HIP(ctx->flag.ensure(sizeof(int) * (size_t)n_nodes));
    NWE_HIP(ctx->slot.ensure(sizeof(int) * ((size_t)n_nodes + 1)));
    hipLaunchKernelGGL(k_ev_node_test, dim3(nblk(n_nodes)), dim3(NWE_BLOCK), 0, ctx->stream, ctx->setup.as<nwe_face_setup>(), ctx->off.as<int>(), nf, n_nodes, dx,
                       ctx->flag.as<int>());
    NWE_HIP(hipGetLastError());
    int n = -1;
    NWE_HIP(bq::scan_total(ctx->stream, ctx->flag.as<int>(), n_nodes, ctx->slot.as<int>(), ctx->scan_tmp, &n));
    if (n < 0 || n > n_nodes) return fail(ctx, NWE_ERR_HIP, "nwe_sample_mesh: the output slots do not add up");
    if (n == 0) return NWE_OK;
    // pass 3: positions and face ids
    NWE_HIP(ctx->samples.ensure(sizeof(double) * 3 * (size_t)n));
    NWE_HIP(ctx->sample_face.ensure(sizeof(int) * (size_t)n));
    hipLaunchKernelGGL(k_ev_emit, dim3(nblk(n_nodes)), dim3(NWE_BLOCK), 0, ctx->stream, ctx->setup.as<nwe_face_setup>(), ctx->off.as<int>(), nf, n_nodes, dx,
                       ctx->flag.as<int>(), ctx->slot.as<int>(), n, ctx->samples.as<double>(), ctx->sample_face.as<int>());
    NWE_HIP(hipGetLastError());
    NWE_HIP(hipStreamSynchronize(ctx->stream));
    ctx->n_samples = n;
    *n_out = n;
    return NWE_OK;
}

NWE_EXPORT int nwe_get_samples(nwe_ctx *ctx, double *positions_out, int32_t *face_out)
{
    if (!ctx) return NWE_ERR_BADARG;
    if (ctx->n_samples < 1) return fail(ctx, NWE_ERR_NOSAMPLES, "nwe_get_samples: the context holds no samples");
    NWE_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->n_samples;
    if (positions_out) NWE_HIP(hipMemcpyAsync(positions_out, ctx->samples.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (face_out) NWE_HIP(hipMemcpyAsync(face_out, ctx->sample_face.p, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    NWE_HIP(hipStreamSynchronize(ctx->stream));
    return NWE_OK;
}

NWE_EXPORT int nwe_nearest(nwe_ctx *ctx, const double *reference, int64_t n_reference, const double *queries, int64_t n_queries,
                           double *dist_out, int32_t *idx_out, double *sum_sq_out)
{
    if (!cloud_args_ok(reference, n_reference) || !cloud_args_ok(queries, n_queries)) return NWE_ERR_BADARG;
    if (!ctx) return NWE_ERR_BADARG;
    if ((!reference || !queries) && ctx->n_samples < 1) return fail(ctx, NWE_ERR_NOSAMPLES, "nwe_nearest: the context holds no samples");
    NWE_HIP(hipSetDevice(ctx->device));
    const double *dref, *dq;
    int nr, nq;
    int r = resolve(ctx, reference, n_reference, ctx->up0, &dref, &nr);
    if (r != NWE_OK) return r;
    r = resolve(ctx, queries, n_queries, ctx->up1, &dq, &nq);
    if (r != NWE_OK) return r;
    return nearest_dev(ctx, dref, nr, dq, nq, dist_out, idx_out, sum_sq_out);
}

NWE_EXPORT int nwe_average_squared_distance(nwe_ctx *ctx, const double *points0, int64_t n0, const double *points1, int64_t n1,
                                            double *mse01_out, double *mse10_out)
{
    if (!cloud_args_ok(points0, n0) || !cloud_args_ok(points1, n1) || !mse01_out || !mse10_out) return NWE_ERR_BADARG;
    if (!ctx) return NWE_ERR_BADARG;
    if ((!points0 || !points1) && ctx->n_samples < 1) return fail(ctx, NWE_ERR_NOSAMPLES, "nwe_average_squared_distance: the context holds no samples");
    NWE_HIP(hipSetDevice(ctx->device));
    const double *d0, *d1;
    int m0, m1;
    int r = resolve(ctx, points0, n0, ctx->up0, &d0, &m0);
    if (r != NWE_OK) return r;
    r = resolve(ctx, points1, n1, ctx->up1, &d1, &m1);
    if (r != NWE_OK) return r;
    double s01 = 0.0, s10 = 0.0;
    r = nearest_dev(ctx, d0, m0, d1, m1, nullptr, nullptr, &s01);
    if (r != NWE_OK) return r;
    r = nearest_dev(ctx, d1, m1, d0, m0, nullptr, nullptr, &s10);
    if (r != NWE_OK) return r;
    *mse01_out = s01 / (double)m1;
    *mse10_out = s10 / (double)m0;
    return NWE_OK;
}
