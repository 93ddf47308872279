// The local shape of a localization cloud on the device (MI355X, gfx950): include/nw_structure.h.
//
//   (bq::CloudGrid: set_cloud, bin)   the cloud query units' shared cloud grid in float (nw_bq.h): bounding box and finiteness of the
//                                     cloud, the cloud in cell order with every point's index in the caller's array, the cells' starts
//   k_st_moments     one lane per query (auto mode: the cloud's points in cell order, so a wave's boxes overlap and its lanes read the same
//                    cells; cross mode: the caller's order): the walk of nwf_walk, every visited point's inclusive test, a neighbour's
//                    three quantised offsets and their six products into ten 64-bit sums held in registers -- no LDS column, no atomics on
//                    any result.  At the end a lane stores its ten words, and the workgroup its four counters
//   k_st_eigen       one lane per query in the caller's order: moments -> covariance -> Jacobi -> order -> signs -> flags (nwf_shape).  A
//                    kernel of its own, so that the walk's occupancy does not pay for its eighteen live doubles
//   k_st_totals      the workgroups' counters, one workgroup; integer sums in a fixed order
//
// The definition -- the neighbourhood, the quantisation, the moments, the float64 procedure, the walk with its proof -- is
// csrc/nw_structure_core.h, which the tests also compile for the CPU.  The device buffer, the cloud grid and the context's scaffolding are
// the query units' shared ones (nw_bq.h).  All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <string>
#include <algorithm>

#include "../../include/nw_structure.h"
#include "nw_bq.h"
#include "nw_structure_core.h"

#define NWF_EXPORT extern "C" __attribute__((visibility("default")))
#define NWF_BLOCK 256               // k_st_eigen, k_st_totals
#define NWF_LANES 128               // k_st_moments
// a workgroup's counters
#define NWF_COUNTERS 4
#define NWF_C_TESTS 0
#define NWF_C_CELLS 1
#define NWF_C_NEIGHBOURS 2
#define NWF_C_FEW 3

typedef unsigned long long u64;

// what a lane does with a visited point: the test, and a neighbour's terms into the lane's ten sums
struct st_visit {
    double x, y, z, r2, s;
    nwf_sums m;
    unsigned tests;
    __device__ __forceinline__ void operator()(const nwf_pt &p)
    {
        ++tests;
        nwf_visit(&m, p.x, p.y, p.z, x, y, z, r2, s);
    }
};

// queries = nullptr: auto mode, lane p is the cloud's p-th point in cell order and its row is the point's index
__global__ __launch_bounds__(NWF_LANES) void k_st_moments(const float *__restrict__ queries, int nq, const nwf_pt *__restrict__ pts,
                                                          const int *__restrict__ cstart, nwf_grid G, double r, double r2, double s,
                                                          long long *__restrict__ moments, u64 *__restrict__ part,
                                                          int *__restrict__ bad /* bit 0: a non-finite query */)
{
    constexpr int WAVES = NWF_LANES / 64;
    __shared__ u64 s_w[WAVES * NWF_COUNTERS];
    const int lane = threadIdx.x;
    const int p = blockIdx.x * NWF_LANES + lane;
    u64 tests = 0, cells = 0, neighbours = 0, few = 0;
    if (p < nq) {
        st_visit v;
        nwf_sums_init(&v.m);
        v.tests = 0u;
        bool ok = true;
        int row;                                              // (below 2^26; widened where it is used)
        if (queries) {
            const float fx = queries[3 * (int64_t)p], fy = queries[3 * (int64_t)p + 1], fz = queries[3 * (int64_t)p + 2];
            ok = isfinite(fx) && isfinite(fy) && isfinite(fz);
            if (!ok) atomicOr(bad, 1);
            v.x = (double)fx; v.y = (double)fy; v.z = (double)fz;
            row = p;
        } else {
            const nwf_pt pt = pts[p];
            v.x = (double)pt.x; v.y = (double)pt.y; v.z = (double)pt.z;
            row = pt.i;
        }
        if (ok) {
            v.r2 = r2; v.s = s;
            int read = 0;
            nwf_walk(pts, cstart, G, v.x, v.y, v.z, r, r2, v, &read);
            tests = v.tests;
            cells = (u64)read;
            neighbours = (u64)v.m.n;
            few = v.m.n < 3 ? 1 : 0;
        }
        // (a refused query leaves a row of zeros: the call fails, and nothing reads memory that was never written)
        long long *out = moments + (int64_t)row * NWF_MOMENT_WORDS;
        out[0] = v.m.n;
        out[1] = v.m.sx; out[2] = v.m.sy; out[3] = v.m.sz;
        out[4] = v.m.xx; out[5] = v.m.xy; out[6] = v.m.xz;
        out[7] = v.m.yy; out[8] = v.m.yz; out[9] = v.m.zz;
    }
    // the four counters: a butterfly within each wave, then the waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tests += __shfl_xor(tests, o, 64); cells += __shfl_xor(cells, o, 64);
        neighbours += __shfl_xor(neighbours, o, 64); few += __shfl_xor(few, o, 64);
    }
    if ((lane & 63) == 0) {
        u64 *w = s_w + (lane >> 6) * NWF_COUNTERS;
        w[NWF_C_TESTS] = tests; w[NWF_C_CELLS] = cells; w[NWF_C_NEIGHBOURS] = neighbours; w[NWF_C_FEW] = few;
    }
    __syncthreads();
    if (lane < NWF_COUNTERS) {
        u64 t = 0;
        for (int w = 0; w < WAVES; ++w) t += s_w[w * NWF_COUNTERS + lane];
        part[(int64_t)blockIdx.x * NWF_COUNTERS + lane] = t;
    }
}

// where[3 q ..]: the queries' positions in the caller's order (cross mode: the queries; auto mode: the cloud)
__global__ __launch_bounds__(NWF_BLOCK) void k_st_eigen(const long long *__restrict__ moments, const float *__restrict__ where, int nq, double step,
                                                        int has_view, double vx, double vy, double vz, double *__restrict__ eigenvalues,
                                                        double *__restrict__ vectors, unsigned char *__restrict__ flags)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const long long *in = moments + (int64_t)q * NWF_MOMENT_WORDS;
    nwf_sums m;
    m.n = in[0];
    m.sx = in[1]; m.sy = in[2]; m.sz = in[3];
    m.xx = in[4]; m.xy = in[5]; m.xz = in[6];
    m.yy = in[7]; m.yz = in[8]; m.zz = in[9];
    double wx = 0.0, wy = 0.0, wz = 0.0;
    if (has_view) {
        wx = vx - (double)where[3 * (int64_t)q]; wy = vy - (double)where[3 * (int64_t)q + 1]; wz = vz - (double)where[3 * (int64_t)q + 2];
    }
    double lam[3], vec[9];
    const unsigned char flag = nwf_shape(m, step, has_view != 0, wx, wy, wz, lam, vec);
    double *l = eigenvalues + (int64_t)q * 3, *v = vectors + (int64_t)q * 9;
    l[0] = lam[0]; l[1] = lam[1]; l[2] = lam[2];
    v[0] = vec[0]; v[1] = vec[1]; v[2] = vec[2];
    v[3] = vec[3]; v[4] = vec[4]; v[5] = vec[5];
    v[6] = vec[6]; v[7] = vec[7]; v[8] = vec[8];
    flags[q] = flag;
}

// totals[c] = the sum of column c of part[nb][NWF_COUNTERS]: a thread adds every 64th row of its column, then the column's threads are
// added in order
__global__ __launch_bounds__(NWF_BLOCK) void k_st_totals(const u64 *__restrict__ part, int64_t nb, u64 *__restrict__ totals)
{
    __shared__ u64 s_acc[NWF_BLOCK];
    constexpr int SLICES = NWF_BLOCK / NWF_COUNTERS;
    const int c = threadIdx.x & (NWF_COUNTERS - 1), s = threadIdx.x / NWF_COUNTERS;
    u64 acc = 0;
    for (int64_t b = s; b < nb; b += SLICES) acc += part[b * NWF_COUNTERS + c];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < NWF_COUNTERS) {
        u64 t = 0;
        for (int k = 0; k < SLICES; ++k) t += s_acc[k * NWF_COUNTERS + threadIdx.x];
        totals[threadIdx.x] = t;
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;

struct nwf_ctx : bq::Ctx {
    bq::CloudGrid grid;                 // the cloud (nwf_set_cloud), its box and its cells
    // one query
    DevBuf q, moments, eigenvalues, vectors, flags, part, totals, flag;
};

namespace {

#define NWF_HIP(call) BQ_HIP(call, NWF_ERR_NOMEM, NWF_ERR_HIP)

const bq::CloudCodes NWF_CODES = {NWF_ERR_BADARG, NWF_ERR_NONFINITE, NWF_ERR_NOMEM, NWF_ERR_HIP};

// the cell size a query starts from: NWF_CELL_OF_R of the radius (bq::cloud_cell)
double starting_cell(const nwf_ctx *ctx, double r) { return bq::cloud_cell(NWF_CELL_OF_R * r, ctx->grid.emax()); }

}  // namespace

NWF_EXPORT int nwf_abi_version(void) { return NWF_ABI_VERSION; }

NWF_EXPORT int nwf_create(int device, nwf_ctx **out) { return bq::create(device, out, NWF_ERR_BADARG, NWF_ERR_HIP); }

NWF_EXPORT void nwf_destroy(nwf_ctx *ctx) { bq::destroy(ctx); }

NWF_EXPORT const char *nwf_last_error(nwf_ctx *ctx) { return bq::last_error(ctx); }

NWF_EXPORT int nwf_set_cloud(nwf_ctx *ctx, const float *xyz, int64_t n, int on_device)
{
    if (!xyz || n < 1 || n > NWF_MAX_N || (on_device != 0 && on_device != 1)) return NWF_ERR_BADARG;
    if (!on_device && !bq::all_finite(xyz, 3 * n)) {
        if (ctx) ctx->grid.forget();                              // (a failed call leaves no cloud, whichever check failed)
        return fail(ctx, NWF_ERR_NONFINITE, "nwf_set_cloud: a localization is not finite");
    }
    if (!ctx) return NWF_ERR_BADARG;
    NWF_HIP(hipSetDevice(ctx->device));
    const bq::CloudStatus s = ctx->grid.set_cloud(ctx->stream, xyz, n, on_device != 0);
    return s.ok() ? NWF_OK : bq::cloud_fail(ctx, "nwf_set_cloud", s, NWF_CODES);
}

NWF_EXPORT int nwf_query(nwf_ctx *ctx, const float *queries, int64_t nq, int on_device, double r, const double *viewpoint, int64_t *moments,
                         double *eigenvalues, double *vectors, uint8_t *flags, int64_t *info)
{
    if (!info || (on_device != 0 && on_device != 1)) return NWF_ERR_BADARG;
    if (queries ? (nq < 1 || nq > NWF_MAX_N) : nq < 0) return NWF_ERR_BADARG;
    double r2 = 0.0;
    if (!nwf_radius(r, &r2)) return fail(ctx, NWF_ERR_BADARG, "nwf_query: the radius is finite, above 0 and at most 2^40, and so is its square");
    if (viewpoint && !bq::all_finite(viewpoint, 3)) return fail(ctx, NWF_ERR_NONFINITE, "nwf_query: the viewpoint is not finite");
    if (queries && !on_device && !bq::all_finite(queries, 3 * nq)) return fail(ctx, NWF_ERR_NONFINITE, "nwf_query: a query is not finite");
    if (!ctx) return NWF_ERR_BADARG;
    if (ctx->grid.n < 1) return fail(ctx, NWF_ERR_NOCLOUD, "nwf_query: nwf_set_cloud first");
    if (!queries && nq != 0 && nq != ctx->grid.n) return fail(ctx, NWF_ERR_BADARG, "nwf_query: without queries nq is 0 or the cloud's n");
    NWF_HIP(hipSetDevice(ctx->device));
    const bq::CloudStatus binned = ctx->grid.bin(ctx->stream, starting_cell(ctx, r));
    if (!binned.ok()) return bq::cloud_fail(ctx, "nwf", binned, NWF_CODES);
    const bq::Grid<float> &g = ctx->grid.g;
    hipStream_t st = ctx->stream;
    const int n_queries = queries ? (int)nq : ctx->grid.n;
    const int nb = bq::nblk(n_queries, NWF_LANES);
    double s = 0.0, step = 0.0;
    nwf_scale(r, &s, &step);

    const float *dq = nullptr;
    if (queries) {
        dq = queries;
        if (!on_device) {
            NWF_HIP(bq::upload(st, ctx->q, queries, 3 * nq));
            dq = ctx->q.as<float>();
        }
    }
    const bool shape = eigenvalues || vectors || flags;
    NWF_HIP(ctx->moments.ensure(sizeof(long long) * NWF_MOMENT_WORDS * (size_t)n_queries));
    NWF_HIP(ctx->part.ensure(sizeof(u64) * NWF_COUNTERS * (size_t)nb));
    NWF_HIP(ctx->totals.ensure(sizeof(u64) * NWF_COUNTERS));
    NWF_HIP(ctx->flag.ensure(sizeof(int)));
    NWF_HIP(hipMemsetAsync(ctx->flag.p, 0, sizeof(int), st));
    if (shape) {
        NWF_HIP(ctx->eigenvalues.ensure(sizeof(double) * 3 * (size_t)n_queries));
        NWF_HIP(ctx->vectors.ensure(sizeof(double) * 9 * (size_t)n_queries));
        NWF_HIP(ctx->flags.ensure((size_t)n_queries));
    }

    nwf_grid G;
    for (int d = 0; d < 3; ++d) { G.lo[d] = (double)g.lo[d]; G.hi[d] = (double)g.hi[d]; G.dims[d] = g.dims[d]; }
    G.h = (double)g.h;
    hipLaunchKernelGGL(k_st_moments, dim3(nb), dim3(NWF_LANES), 0, st, dq, n_queries, ctx->grid.sorted.as<nwf_pt>(), ctx->grid.cstart.as<int>(), G, r, r2, s,
                       ctx->moments.as<long long>(), ctx->part.as<u64>(), ctx->flag.as<int>());
    hipLaunchKernelGGL(k_st_totals, dim3(1), dim3(NWF_BLOCK), 0, st, ctx->part.as<u64>(), (int64_t)nb, ctx->totals.as<u64>());
    if (shape)
        hipLaunchKernelGGL(k_st_eigen, dim3(bq::nblk(n_queries, NWF_BLOCK)), dim3(NWF_BLOCK), 0, st, ctx->moments.as<long long>(),
                           dq ? dq : ctx->grid.cloud.as<float>(), n_queries, step, viewpoint ? 1 : 0, viewpoint ? viewpoint[0] : 0.0, viewpoint ? viewpoint[1] : 0.0,
                           viewpoint ? viewpoint[2] : 0.0, ctx->eigenvalues.as<double>(), ctx->vectors.as<double>(), ctx->flags.as<unsigned char>());
    NWF_HIP(hipGetLastError());

    u64 tot[NWF_COUNTERS];
    int bad = 0;
    NWF_HIP(hipMemcpyAsync(tot, ctx->totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    NWF_HIP(hipMemcpyAsync(&bad, ctx->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    NWF_HIP(hipStreamSynchronize(st));
    if (bad) return fail(ctx, NWF_ERR_NONFINITE, "nwf_query: a query is not finite");
    const size_t nqs = (size_t)n_queries;
    if (moments) NWF_HIP(hipMemcpyAsync(moments, ctx->moments.p, sizeof(long long) * NWF_MOMENT_WORDS * nqs, hipMemcpyDeviceToHost, st));
    if (eigenvalues) NWF_HIP(hipMemcpyAsync(eigenvalues, ctx->eigenvalues.p, sizeof(double) * 3 * nqs, hipMemcpyDeviceToHost, st));
    if (vectors) NWF_HIP(hipMemcpyAsync(vectors, ctx->vectors.p, sizeof(double) * 9 * nqs, hipMemcpyDeviceToHost, st));
    if (flags) NWF_HIP(hipMemcpyAsync(flags, ctx->flags.p, nqs, hipMemcpyDeviceToHost, st));
    NWF_HIP(hipStreamSynchronize(st));
    info[NWF_INFO_TESTS] = (int64_t)tot[NWF_C_TESTS];
    info[NWF_INFO_CELLS_READ] = (int64_t)tot[NWF_C_CELLS];
    info[NWF_INFO_CELL_SIZE] = __builtin_bit_cast(int64_t, G.h);
    info[NWF_INFO_CELLS] = g.cells();
    info[NWF_INFO_NEIGHBOURS] = (int64_t)tot[NWF_C_NEIGHBOURS];
    info[NWF_INFO_FEW] = (int64_t)tot[NWF_C_FEW];
    info[NWF_INFO_N_QUERIES] = n_queries;
    info[NWF_INFO_N_CLOUD] = ctx->grid.n;
    return NWF_OK;
}
