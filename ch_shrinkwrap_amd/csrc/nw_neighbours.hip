// The exact k-th-nearest-neighbour distance on the device (MI355X, gfx950): include/nw_neighbours.h.
//
//   (bq::CloudGrid: set_cloud, bin)   the cloud query units' shared cloud grid in float (nw_bq.h): bounding box and finiteness of the
//                                     cloud, counting sort of the cloud by cell (the walks read a sorted point's coordinates as a
//                                     float4 and leave its fourth word, the index, alone)
//   k_kn_queries     one lane per query of a list: the ring walk of kn_walk, the result as a double
//   k_kn_nodes       one lane per node of a voxel lattice, lanes along x: the same walk, the result quantised into the uint64 field
//
// kn_walk is shaped like k_ev_nearest's: the query projected onto the cloud's box, rings of cells around the projection's cell, an end
// as soon as the ring's lower bound exceeds what could still matter.  What differs is what a lane keeps: not one best pair but the k
// smallest squared distances, in a column of LDS ([slot][lane]: a wave's 64 lanes hit 64 different pairs of banks whatever their slots
// are), with the running maximum and its slot in registers (nwk_list, csrc/nw_neighbours_core.h).  128 lanes x 32 slots x 8 bytes =
// 32 KB a workgroup.  A list indexed at run time in registers would go to scratch; LDS takes the index as an address.
//
// The device buffer with its staging, the cloud grid and the context's scaffolding are the query units' shared ones (nw_bq.h); what is
// this unit's own about the grid is its starting cell size, and that the cloud is binned as soon as it is set.
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <string>
#include <algorithm>

#include "../../include/nw_neighbours.h"
#include "nw_bq.h"
#include "nw_neighbours_core.h"

#define NWK_EXPORT extern "C" __attribute__((visibility("default")))
#define NWK_BLOCK 128
#define NWK_MAX_DIM (1 << 20)       // per axis of a node lattice, as nwi_density's
#define NWK_MAX_CAP 1099511627776.0 // 2^40: (r_cap - r) * 2^20 fits the field with room to spare

static_assert(NWK_MAX_K == NWK_CORE_MAX_K, "the core header's list is sized for NWK_MAX_K");

typedef unsigned long long u64;

// the cell of a coordinate inside the box, along one axis, in double (the cloud's own cells are float expressions: NWK_CELL_SLACK)
__device__ __forceinline__ int kn_cell_1d(double x, double lo, double h, int dim)
{
    const double t = floor((x - lo) / h);
    return (int)fmin(fmax(t, 0.0), (double)(dim - 1));
}

// the points of cells [c0, c1] of one row against the query
__device__ __forceinline__ void kn_scan_cells(const float4 *__restrict__ pts, const int *__restrict__ cstart, int c0, int c1, double qx, double qy, double qz,
                                              double *s, int k, nwk_list *L)
{
    const int b = cstart[c0], e = cstart[c1 + 1];
    for (int p = b; p < e; ++p) {
        const float4 r = pts[p];
        nwk_list_insert(s, NWK_BLOCK, k, L, nwk_dist2(r.x, r.y, r.z, qx, qy, qz));
    }
}

// the k-th smallest squared distance from (qx, qy, qz) to the cloud, or anything above cap2 if it is above cap2 (+inf if fewer than k
// points were met); s = this lane's column of LDS
__device__ __forceinline__ double kn_walk(double qx, double qy, double qz, const float4 *__restrict__ pts, const int *__restrict__ cstart,
                                          const bq::Grid<float> &g, int k, double cap2, double *s)
{
    const double h = (double)g.h;
    const double lox = (double)g.lo[0], loy = (double)g.lo[1], loz = (double)g.lo[2];
    // the query's projection onto the cloud's box: every point p of the cloud has |p - q|^2 >= |p - q'|^2 + |q - q'|^2
    const double px = fmin(fmax(qx, lox), (double)g.hi[0]), py = fmin(fmax(qy, loy), (double)g.hi[1]), pz = fmin(fmax(qz, loz), (double)g.hi[2]);
    const double out2 = (((qx - px) * (qx - px) + (qy - py) * (qy - py)) + (qz - pz) * (qz - pz)) * (1.0 - 1e-9);
    const int cx = kn_cell_1d(px, lox, h, g.dims[0]), cy = kn_cell_1d(py, loy, h, g.dims[1]), cz = kn_cell_1d(pz, loz, h, g.dims[2]);
    const int rmax = max(max(max(cx, g.dims[0] - 1 - cx), max(cy, g.dims[1] - 1 - cy)), max(cz, g.dims[2] - 1 - cz));
    nwk_list L;
    nwk_list_init(&L);
    for (int r = 0; r <= rmax; ++r) {
        if (nwk_walk_ends(r, h, out2, &L, k, cap2)) break;
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dims[2] - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dims[1] - 1);
        const int xa = max(cx - r, 0), xb = min(cx + r, g.dims[0] - 1);
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * g.dims[1] + y) * g.dims[0];
                if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
                    kn_scan_cells(pts, cstart, row + xa, row + xb, qx, qy, qz, s, k, &L);               // a row of the ring's shell
                } else {
                    if (cx - r >= 0) kn_scan_cells(pts, cstart, row + cx - r, row + cx - r, qx, qy, qz, s, k, &L);
                    if (cx + r < g.dims[0]) kn_scan_cells(pts, cstart, row + cx + r, row + cx + r, qx, qy, qz, s, k, &L);
                }
            }
        }
    }
    return nwk_list_kth(&L, k);
}

__global__ __launch_bounds__(NWK_BLOCK) void k_kn_queries(const float *__restrict__ q, int nq, const float4 *__restrict__ pts, const int *__restrict__ cstart,
                                                          bq::Grid<float> g, int k, double r_cap, double cap2, double *__restrict__ out,
                                                          int *__restrict__ bad /* bit 0: a non-finite query */)
{
    __shared__ double s_best[NWK_MAX_K * NWK_BLOCK];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float fx = q[3 * (int64_t)i], fy = q[3 * (int64_t)i + 1], fz = q[3 * (int64_t)i + 2];
    if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) {
        atomicOr(bad, 1);
        out[i] = r_cap;
        return;
    }
    const double kth2 = kn_walk((double)fx, (double)fy, (double)fz, pts, cstart, g, k, cap2, s_best + threadIdx.x);
    out[i] = nwk_result(kth2, r_cap);
}

__global__ __launch_bounds__(NWK_BLOCK) void k_kn_nodes(float lo0, float lo1, float lo2, float hv, int nx, int ny, int nz, const float4 *__restrict__ pts,
                                                        const int *__restrict__ cstart, bq::Grid<float> g, int k, double r_cap, double cap2,
                                                        u64 *__restrict__ field)
{
    __shared__ double s_best[NWK_MAX_K * NWK_BLOCK];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nx * ny * nz) return;
    const int i = idx % nx, j = (idx / nx) % ny, kz = idx / (nx * ny);
    const double kth2 = kn_walk(nwk_node_coord(lo0, hv, i), nwk_node_coord(lo1, hv, j), nwk_node_coord(lo2, hv, kz), pts, cstart, g, k, cap2,
                                s_best + threadIdx.x);
    field[idx] = nwk_quantise(nwk_result(kth2, r_cap), r_cap);
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwk_ctx : bq::Ctx {
    bq::CloudGrid grid;                 // the cloud (nwk_set_cloud), its box and its cells
    // the queries
    DevBuf q, dist, flag;
    // the node field
    DevBuf field;
    int64_t n_field = 0;
};

namespace {

#define NWK_HIP(call) BQ_HIP(call, NWK_ERR_NOMEM, NWK_ERR_HIP)

const bq::CloudCodes NWK_CODES = {NWK_ERR_BADARG, NWK_ERR_NONFINITE, NWK_ERR_NOMEM, NWK_ERR_HIP};

bool k_and_cap_ok(int k, double r_cap) { return k >= 1 && k <= NWK_MAX_K && r_cap > 0.0; }             // (a nan cap fails the comparison)

// the cell size a query starts from: a quarter of a finite cap, else about one point per cell of the box (the flattest axis counts as
// a thousandth of the widest); never below 1/1024 of the widest axis, 1 for a cloud without extent
double starting_cell(const nwk_ctx *ctx, double r_cap)
{
    double ext[3], emax = 0.0;
    for (int d = 0; d < 3; ++d) { ext[d] = (double)ctx->grid.g.hi[d] - (double)ctx->grid.g.lo[d]; emax = std::max(emax, ext[d]); }
    if (!(emax > 0.0)) return 1.0;
    double h = std::isfinite(r_cap) ? r_cap / 4.0
                                    : std::cbrt(std::max(ext[0], 1e-3 * emax) * std::max(ext[1], 1e-3 * emax) * std::max(ext[2], 1e-3 * emax) / ctx->grid.n);
    h = std::max(h, emax / 1024.0);
    if (!(h > 0.0) || !std::isfinite(h)) h = emax;
    return h;
}

// the grid for a query with this cap: the one at hand if it was sized from the same starting cell, else the cloud binned anew
int ensure_grid(nwk_ctx *ctx, double r_cap)
{
    const bq::CloudStatus s = ctx->grid.bin(ctx->stream, starting_cell(ctx, r_cap));
    return s.ok() ? NWK_OK : bq::cloud_fail(ctx, "nwk", s, NWK_CODES);
}

}  // namespace

NWK_EXPORT int nwk_abi_version(void) { return NWK_ABI_VERSION; }

NWK_EXPORT int nwk_create(int device, nwk_ctx **out) { return bq::create(device, out, NWK_ERR_BADARG, NWK_ERR_HIP); }

NWK_EXPORT void nwk_destroy(nwk_ctx *ctx) { bq::destroy(ctx); }

NWK_EXPORT const char *nwk_last_error(nwk_ctx *ctx) { return bq::last_error(ctx); }

NWK_EXPORT int nwk_set_cloud(nwk_ctx *ctx, const float *xyz, int64_t n, int on_device)
{
    if (!xyz || n < 1 || n > (1ll << 30) || (on_device != 0 && on_device != 1)) return NWK_ERR_BADARG;
    if (!on_device && !bq::all_finite(xyz, 3 * n)) return fail(ctx, NWK_ERR_NONFINITE, "nwk_set_cloud: a localization is not finite");
    if (!ctx) return NWK_ERR_BADARG;
    NWK_HIP(hipSetDevice(ctx->device));
    const bq::CloudStatus s = ctx->grid.set_cloud(ctx->stream, xyz, n, on_device != 0);
    if (!s.ok()) return bq::cloud_fail(ctx, "nwk_set_cloud", s, NWK_CODES);
    const int r = ensure_grid(ctx, INFINITY);
    if (r != NWK_OK) ctx->grid.n = 0;
    return r;
}

NWK_EXPORT int nwk_kth_distance(nwk_ctx *ctx, const float *queries, int64_t nq, int queries_on_device, int k, double r_cap, double *out_host)
{
    if (!queries || !out_host || nq < 1 || nq > (1ll << 30) || (queries_on_device != 0 && queries_on_device != 1)) return NWK_ERR_BADARG;
    if (!k_and_cap_ok(k, r_cap)) return NWK_ERR_BADARG;
    if (!queries_on_device && !bq::all_finite(queries, 3 * nq)) return fail(ctx, NWK_ERR_NONFINITE, "nwk_kth_distance: a query is not finite");
    if (!ctx) return NWK_ERR_BADARG;
    if (ctx->grid.n < 1) return fail(ctx, NWK_ERR_NOCLOUD, "nwk_kth_distance: nwk_set_cloud first");
    NWK_HIP(hipSetDevice(ctx->device));
    const int r = ensure_grid(ctx, r_cap);
    if (r != NWK_OK) return r;
    const float *dq = queries;
    if (!queries_on_device) {
        NWK_HIP(bq::upload(ctx->stream, ctx->q, queries, 3 * nq));
        dq = ctx->q.as<float>();
    }
    NWK_HIP(ctx->dist.ensure(sizeof(double) * (size_t)nq));
    NWK_HIP(ctx->flag.ensure(sizeof(int)));
    NWK_HIP(hipMemsetAsync(ctx->flag.p, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_kn_queries, dim3(nblk(nq, NWK_BLOCK)), dim3(NWK_BLOCK), 0, ctx->stream, dq, (int)nq, ctx->grid.sorted.as<float4>(), ctx->grid.cstart.as<int>(),
                       ctx->grid.g, k, r_cap, r_cap * r_cap, ctx->dist.as<double>(), ctx->flag.as<int>());
    NWK_HIP(hipGetLastError());
    int bad = 0;
    NWK_HIP(hipMemcpyAsync(&bad, ctx->flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NWK_HIP(hipMemcpyAsync(out_host, ctx->dist.p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    NWK_HIP(hipStreamSynchronize(ctx->stream));
    if (bad) return fail(ctx, NWK_ERR_NONFINITE, "nwk_kth_distance: a query is not finite");
    return NWK_OK;
}

NWK_EXPORT int nwk_node_field(nwk_ctx *ctx, const float *lo, float h, const int32_t *dims, int k, double r_cap, uint64_t *field_host)
{
    if (!lo || !dims || !(h > 0.0f) || !std::isfinite(h)) return NWK_ERR_BADARG;
    if (!k_and_cap_ok(k, r_cap) || !(r_cap <= NWK_MAX_CAP)) return NWK_ERR_BADARG;
    int64_t nvox = 1;
    for (int d = 0; d < 3; ++d) {
        if (!std::isfinite(lo[d]) || dims[d] < 3 || dims[d] > NWK_MAX_DIM) return NWK_ERR_BADARG;
        nvox *= dims[d];
    }
    if (nvox > (1ll << 30)) return NWK_ERR_BADARG;
    if (!ctx) return NWK_ERR_BADARG;
    if (ctx->grid.n < 1) return fail(ctx, NWK_ERR_NOCLOUD, "nwk_node_field: nwk_set_cloud first");
    NWK_HIP(hipSetDevice(ctx->device));
    ctx->n_field = 0;
    const int r = ensure_grid(ctx, r_cap);
    if (r != NWK_OK) return r;
    NWK_HIP(ctx->field.ensure(sizeof(u64) * (size_t)nvox));
    hipLaunchKernelGGL(k_kn_nodes, dim3(nblk(nvox, NWK_BLOCK)), dim3(NWK_BLOCK), 0, ctx->stream, lo[0], lo[1], lo[2], h, dims[0], dims[1], dims[2],
                       ctx->grid.sorted.as<float4>(), ctx->grid.cstart.as<int>(), ctx->grid.g, k, r_cap, r_cap * r_cap, ctx->field.as<u64>());
    NWK_HIP(hipGetLastError());
    if (field_host) NWK_HIP(hipMemcpyAsync(field_host, ctx->field.p, sizeof(u64) * (size_t)nvox, hipMemcpyDeviceToHost, ctx->stream));
    NWK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->n_field = nvox;
    return NWK_OK;
}

NWK_EXPORT const uint64_t *nwk_field_ptr(nwk_ctx *ctx) { return (ctx && ctx->n_field > 0) ? ctx->field.as<uint64_t>() : nullptr; }
