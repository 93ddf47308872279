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
//   nearest         k_ev_bbox         bounding box (ordered 64-bit keys, atomicMin / atomicMax) and finiteness of a cloud
//                   k_ev_cell_count, (scan), k_ev_scatter   counting sort of the reference cloud by cell
//                   k_ev_nearest      one thread per query: rings of cells around its own until the ring's lower bound exceeds the best
//                                     squared distance; (d2, index) compared lexicographically, so the order inside a cell (the scatter's
//                                     atomics) never shows; the block's sum of dist^2 in a fixed order
//                   k_ev_sum_final    the blocks' partial sums, one workgroup, a fixed order
//
// The scan, the device buffer and the context's scaffolding are the block-boundary units' shared ones (nw_bq.h).
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

struct nwe_grid {
    double lo[3], hi[3];           // the reference cloud's bounding box
    double h;
    int dims[3];
};

struct ev_pt {                     // a reference point in cell order, with its index in the caller's array
    double x, y, z;
    long long i;
};

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
// monotone double <-> u64 map (atomicMin / atomicMax on doubles)
__device__ __host__ __forceinline__ u64 ev_enc(double d)
{
    const u64 u = __builtin_bit_cast(u64, d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __host__ __forceinline__ double ev_dec(u64 e)
{
    return __builtin_bit_cast(double, (e >> 63) ? (e ^ 0x8000000000000000ull) : ~e);
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_bbox(const double *__restrict__ xyz, int n, u64 *__restrict__ mm /* [7]: min xyz, max xyz, nonfinite */)
{
    u64 lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    int bad = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double x = xyz[3 * (int64_t)i + d];
            if (!isfinite(x)) { bad = 1; continue; }
            lo[d] = min(lo[d], ev_enc(x));
            hi[d] = max(hi[d], ev_enc(x));
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[d] = min(lo[d], __shfl_xor(lo[d], o, 64)); hi[d] = max(hi[d], __shfl_xor(hi[d], o, 64)); }
    }
    bad = __ballot(bad) != 0;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { atomicMin(&mm[d], lo[d]); atomicMax(&mm[3 + d], hi[d]); }
        if (bad) atomicOr(&mm[6], 1ull);
    }
}

// cell index: the same double expression for binning and for every query
__device__ __forceinline__ int ev_cell_1d(double x, double lo, double h, int dim)
{
    const double t = floor((x - lo) / h);
    return (int)fmin(fmax(t, 0.0), (double)(dim - 1));
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_cell_count(const double *__restrict__ xyz, int n, nwe_grid g, int *__restrict__ cell, int *__restrict__ count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = xyz[3 * (int64_t)i], y = xyz[3 * (int64_t)i + 1], z = xyz[3 * (int64_t)i + 2];
    const int c = (ev_cell_1d(z, g.lo[2], g.h, g.dims[2]) * g.dims[1] + ev_cell_1d(y, g.lo[1], g.h, g.dims[1])) * g.dims[0] + ev_cell_1d(x, g.lo[0], g.h, g.dims[0]);
    cell[i] = c;
    atomicAdd(&count[c], 1);
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_scatter(const double *__restrict__ xyz, int n, const int *__restrict__ cell, int *__restrict__ cursor,
                                                          ev_pt *__restrict__ sorted)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = atomicAdd(&cursor[cell[i]], 1);          // (order inside a cell is arbitrary: the query compares (d2, index))
    if (slot < 0 || slot >= n) return;                        // (cannot happen: the cursors start at the scan of the counts)
    ev_pt p;
    p.x = xyz[3 * (int64_t)i]; p.y = xyz[3 * (int64_t)i + 1]; p.z = xyz[3 * (int64_t)i + 2]; p.i = i;
    sorted[slot] = p;
}

// the points of cells [c0, c1] of one row against the query
__device__ __forceinline__ void ev_scan_cells(const ev_pt *__restrict__ pts, const int *__restrict__ cstart, int c0, int c1, double qx, double qy, double qz,
                                              double &best, long long &best_i)
{
    const int s = cstart[c0], e = cstart[c1 + 1];
    for (int p = s; p < e; ++p) {
        const ev_pt r = pts[p];
        const double ex = r.x - qx, ey = r.y - qy, ez = r.z - qz;
        const double d2 = (ex * ex + ey * ey) + ez * ez;
        if (d2 < best || (d2 == best && r.i < best_i)) { best = d2; best_i = r.i; }
    }
}

__global__ __launch_bounds__(NWE_BLOCK) void k_ev_nearest(const double *__restrict__ q, int nq, const ev_pt *__restrict__ pts, const int *__restrict__ cstart,
                                                          nwe_grid g, double *__restrict__ dist, int *__restrict__ idx, double *__restrict__ partial)
{
    __shared__ double s_w[NWE_BLOCK / 64];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double term = 0.0;
    if (i < nq) {
        const double qx = q[3 * (int64_t)i], qy = q[3 * (int64_t)i + 1], qz = q[3 * (int64_t)i + 2];
        // the query's projection onto the reference cloud's box: every reference point p has |p - q|^2 >= |p - q'|^2 + |q - q'|^2
        const double px = fmin(fmax(qx, g.lo[0]), g.hi[0]), py = fmin(fmax(qy, g.lo[1]), g.hi[1]), pz = fmin(fmax(qz, g.lo[2]), g.hi[2]);
        const double out2 = (((qx - px) * (qx - px) + (qy - py) * (qy - py)) + (qz - pz) * (qz - pz)) * (1.0 - 1e-9);
        const int cx = ev_cell_1d(px, g.lo[0], g.h, g.dims[0]), cy = ev_cell_1d(py, g.lo[1], g.h, g.dims[1]), cz = ev_cell_1d(pz, g.lo[2], g.h, g.dims[2]);
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
    hipPointerAttribute_t attr;
    const bool on_device = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();                                  // (a host pointer leaves an error behind on some runtimes)
    *n_out = (int)n;
    if (on_device) { *dev = p; return NWE_OK; }
    NWE_HIP(stage.ensure(sizeof(double) * 3 * (size_t)n));
    NWE_HIP(hipMemcpyAsync(stage.p, p, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    *dev = stage.as<double>();
    return NWE_OK;
}

// cell size: about one reference point per cell of the box (the flattest axis counts as a thousandth of the widest), at most 1025 cells
// an axis, then widened until the grid has at most max(2 n, 65536) cells
int make_grid(nwe_ctx *ctx, const u64 *mm, int n, nwe_grid *g)
{
    double ext[3], emax = 0.0;
    for (int d = 0; d < 3; ++d) { g->lo[d] = ev_dec(mm[d]); g->hi[d] = ev_dec(mm[3 + d]); ext[d] = g->hi[d] - g->lo[d]; emax = std::max(emax, ext[d]); }
    if (!std::isfinite(emax)) return fail(ctx, NWE_ERR_BADARG, "nwe_nearest: the reference cloud's extent is not a finite double");
    double h = 1.0;
    if (emax > 0.0) {
        h = std::cbrt(std::max(ext[0], 1e-3 * emax) * std::max(ext[1], 1e-3 * emax) * std::max(ext[2], 1e-3 * emax) / n);
        h = std::max(h, emax / 1024.0);
        if (!(h > 0.0) || !std::isfinite(h)) h = emax;
    }
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(2ll * n, 65536), 1ll << 28);      // (cell ids and the scan are int)
    for (int it = 0; it < 400; ++it) {
        int64_t cells = 1;
        for (int d = 0; d < 3; ++d) { g->dims[d] = (int)std::min(1025.0, std::floor(ext[d] / h) + 1.0); cells *= g->dims[d]; }
        if (cells <= cap) break;
        h *= 1.1;
    }
    g->h = h;
    if ((int64_t)g->dims[0] * g->dims[1] * g->dims[2] > cap) return fail(ctx, NWE_ERR_BADARG, "nwe_nearest: no cell size keeps the grid within its cap");
    return NWE_OK;
}

// both clouds on the device already
int nearest_dev(nwe_ctx *ctx, const double *dref, int nr, const double *dq, int nq, double *dist_out, int32_t *idx_out, double *sum_out)
{
    // bounding box of the reference cloud, finiteness of both
    NWE_HIP(ctx->mm.ensure(sizeof(u64) * 14));
    const u64 mm0[14] = {~0ull, ~0ull, ~0ull, 0, 0, 0, 0, ~0ull, ~0ull, ~0ull, 0, 0, 0, 0};
    NWE_HIP(hipMemcpyAsync(ctx->mm.p, mm0, sizeof(mm0), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_ev_bbox, dim3(std::min(nblk(nr), 1024)), dim3(NWE_BLOCK), 0, ctx->stream, dref, nr, ctx->mm.as<u64>());
    hipLaunchKernelGGL(k_ev_bbox, dim3(std::min(nblk(nq), 1024)), dim3(NWE_BLOCK), 0, ctx->stream, dq, nq, ctx->mm.as<u64>() + 7);
    NWE_HIP(hipGetLastError());
    u64 mm[14];
    NWE_HIP(hipMemcpyAsync(mm, ctx->mm.p, sizeof(mm), hipMemcpyDeviceToHost, ctx->stream));
    NWE_HIP(hipStreamSynchronize(ctx->stream));
    if (mm[6]) return fail(ctx, NWE_ERR_NONFINITE, "nwe_nearest: a reference point is not finite");
    if (mm[13]) return fail(ctx, NWE_ERR_NONFINITE, "nwe_nearest: a query point is not finite");
    nwe_grid g;
    const int r = make_grid(ctx, mm, nr, &g);
    if (r != NWE_OK) return r;
    const int64_t ncell = (int64_t)g.dims[0] * g.dims[1] * g.dims[2];
    // counting sort of the reference cloud by cell
    NWE_HIP(ctx->cell.ensure(sizeof(int) * (size_t)nr));
    NWE_HIP(ctx->ccount.ensure(sizeof(int) * (size_t)(ncell + 1)));            // counts, then the cursors
    NWE_HIP(ctx->cstart.ensure(sizeof(int) * (size_t)(ncell + 1)));
    NWE_HIP(ctx->sorted.ensure(sizeof(ev_pt) * (size_t)nr));
    NWE_HIP(hipMemsetAsync(ctx->ccount.p, 0, sizeof(int) * (size_t)(ncell + 1), ctx->stream));
    hipLaunchKernelGGL(k_ev_cell_count, dim3(nblk(nr)), dim3(NWE_BLOCK), 0, ctx->stream, dref, nr, g, ctx->cell.as<int>(), ctx->ccount.as<int>());
    NWE_HIP(hipGetLastError());
    NWE_HIP(bq::scan_exclusive(ctx->stream, ctx->ccount.as<int>(), (int)ncell, ctx->cstart.as<int>(), ctx->scan_tmp));
    NWE_HIP(hipMemcpyAsync(ctx->ccount.p, ctx->cstart.p, sizeof(int) * (size_t)ncell, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_ev_scatter, dim3(nblk(nr)), dim3(NWE_BLOCK), 0, ctx->stream, dref, nr, ctx->cell.as<int>(), ctx->ccount.as<int>(), ctx->sorted.as<ev_pt>());
    NWE_HIP(hipGetLastError());
    int total = -1;
    NWE_HIP(hipMemcpyAsync(&total, ctx->cstart.as<int>() + ncell, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NWE_HIP(hipStreamSynchronize(ctx->stream));
    if (total != nr) return fail(ctx, NWE_ERR_HIP, "nwe_nearest: the cell counts do not add up to the reference points");
    // the queries
    const int nb = nblk(nq);
    if (dist_out) NWE_HIP(ctx->dist.ensure(sizeof(double) * (size_t)nq));
    if (idx_out) NWE_HIP(ctx->idx.ensure(sizeof(int) * (size_t)nq));
    NWE_HIP(ctx->partial.ensure(sizeof(double) * (size_t)nb));
    NWE_HIP(ctx->sum.ensure(sizeof(double)));
    hipLaunchKernelGGL(k_ev_nearest, dim3(nb), dim3(NWE_BLOCK), 0, ctx->stream, dq, nq, ctx->sorted.as<ev_pt>(), ctx->cstart.as<int>(), g,
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
    const size_t bpos = sizeof(float) * 3 * (size_t)n_vertices, bfac = sizeof(int) * 3 * (size_t)nf;
    NWE_HIP(ctx->mpos.ensure(bpos));
    NWE_HIP(ctx->mfaces.ensure(bfac));
    NWE_HIP(ctx->setup.ensure(sizeof(nwe_face_setup) * (size_t)nf));
    NWE_HIP(ctx->count.ensure(sizeof(int) * (size_t)nf));
    NWE_HIP(ctx->off.ensure(sizeof(int) * (size_t)(nf + 1)));
    NWE_HIP(ctx->total.ensure(sizeof(u64)));
    NWE_HIP(hipMemcpyAsync(ctx->mpos.p, pos, bpos, hipMemcpyHostToDevice, ctx->stream));
    NWE_HIP(hipMemcpyAsync(ctx->mfaces.p, faces, bfac, hipMemcpyHostToDevice, ctx->stream));
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
    NWE_HIP(bq::scan_exclusive(ctx->stream, ctx->flag.as<int>(), n_nodes, ctx->slot.as<int>(), ctx->scan_tmp));
    int n = -1;
    NWE_HIP(hipMemcpyAsync(&n, ctx->slot.as<int>() + n_nodes, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NWE_HIP(hipStreamSynchronize(ctx->stream));
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
