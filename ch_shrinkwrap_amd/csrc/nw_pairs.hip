// Exact pair-distance counts of a localization cloud on the device (MI355X, gfx950): include/nw_pairs.h.
//
//   (bq::CloudGrid: set_cloud, bin)   the cloud query units' shared cloud grid in float (nw_bq.h): bounding box and finiteness of the
//                                     cloud, the cloud in cell order with every point's index in the caller's array, the cells' starts
//   k_pq_pairs<W>    one lane per query (auto mode: the cloud's points in cell order; cross mode: the caller's order): the walk of
//                    nwq_walk, every visited point's bin, the lane's m counters in a column of LDS ([bin][lane], uint32: the column
//                    stride is the workgroup's size, so a wave's increments never share a bank whatever their bins are, and nothing
//                    is indexed at run time in registers); no atomics.  At the end the column goes to `local` if asked, and the
//                    workgroup's columns are added per bin into one row of 64-bit partial sums
//   k_pq_totals      the partial rows, one workgroup; integer sums: any order gives the same bits
//
// Two instantiations of one template.  <false>, up to 16 bins: 128 lanes, 16 x 128 x 4 bytes = 8 KB of LDS; the edges are kernel
// arguments, padded with +inf to 16, and the bin is the definition itself -- a sum of 16 comparisons against scalar operands, without a
// branch.  <true>, up to 64 bins: the bin is nwq_bin_search over an LDS copy of the padded edges.  64 bins x 128 lanes x 4 bytes are
// 32 KB on their own and would leave no room for that copy, so this variant runs 64 lanes a workgroup: 16 KB of columns and 512 bytes of
// edges.  With either size the LDS lets the same number of waves onto a CU.
//
// The definition -- the edges, the bin, the walk with its proof -- is csrc/nw_pairs_core.h, which the tests also compile for the CPU.
// The device buffer, the cloud grid and the context's scaffolding are the query units' shared ones (nw_bq.h).
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <string>
#include <algorithm>

#include "../../include/nw_pairs.h"
#include "nw_bq.h"
#include "nw_pairs_core.h"

#define NWQ_EXPORT extern "C" __attribute__((visibility("default")))
#define NWQ_BLOCK 256               // k_pq_totals
#define NWQ_LANES_NARROW 128
#define NWQ_LANES_WIDE 64
// a workgroup's two counters beside its row of bins
#define NWQ_COUNTERS 2
#define NWQ_C_TESTS 0
#define NWQ_C_CELLS 1

typedef unsigned long long u64;
typedef unsigned int u32;

// the edges of the narrow variant: kernel arguments, so uniform operands
struct pq_edges {
    double e2[NWQ_NARROW_BINS];
};

// what a lane does with a visited point: its bin, one increment in the lane's column
template <bool WIDE> struct pq_visit {
    double x, y, z;
    int self;                           // the index that is not a pair with the query (-1: none)
    int m;
    const double *e2;                   // WIDE: the LDS copy of the padded edges
    pq_edges E;                         // else: the padded edges as uniform operands
    u32 *col;                           // the lane's column: bin b at col[b * lanes]
    u32 tests;
    __device__ __forceinline__ void operator()(const nwq_pt &p)
    {
        if (p.i == self) return;
        ++tests;
        const double d2 = nwq_dist2(p, x, y, z);
        int bin;
        if (WIDE) {
            bin = nwq_bin_search(e2, d2);
        } else {
            bin = 0;
#pragma unroll
            for (int b = 0; b < NWQ_NARROW_BINS; ++b) bin += E.e2[b] < d2 ? 1 : 0;
        }
        if (bin < m) col[bin * (WIDE ? NWQ_LANES_WIDE : NWQ_LANES_NARROW)] += 1u;
    }
};

// queries = nullptr: auto mode, lane p is the cloud's p-th point in cell order and leaves itself out by index
template <bool WIDE>
__global__ __launch_bounds__(WIDE ? NWQ_LANES_WIDE : NWQ_LANES_NARROW) void k_pq_pairs(const float *__restrict__ queries, int nq, const nwq_pt *__restrict__ pts,
                                                                                      const int *__restrict__ cstart, nwq_grid G, pq_edges E,
                                                                                      const double *__restrict__ e2_all, int m, double r_max, double r_max2,
                                                                                      u32 *__restrict__ local, u64 *__restrict__ part_hist,
                                                                                      u64 *__restrict__ part_cnt, int *__restrict__ bad /* bit 0: a non-finite query */)
{
    constexpr int LANES = WIDE ? NWQ_LANES_WIDE : NWQ_LANES_NARROW;
    constexpr int BINS = WIDE ? NWQ_MAX_BINS : NWQ_NARROW_BINS;
    constexpr int WAVES = LANES / 64;
    // the columns, and behind them the wide variant's copy of the edges (64 doubles)
    __shared__ alignas(16) u32 s_col[BINS * LANES + (WIDE ? 2 * NWQ_MAX_BINS : 0)];
    double *s_e2 = (double *)(s_col + BINS * LANES);
    const int lane = threadIdx.x;
    const int p = blockIdx.x * LANES + lane;
    if (WIDE && lane < NWQ_MAX_BINS) s_e2[lane] = e2_all[lane];
#pragma unroll
    for (int b = 0; b < BINS; ++b) s_col[b * LANES + lane] = 0u;
    __syncthreads();

    u64 tests = 0, cells = 0;
    int64_t row = -1;                                         // where the lane's counts go in `local`
    if (p < nq) {
        pq_visit<WIDE> v;
        bool ok = true;
        if (queries) {
            const float fx = queries[3 * (int64_t)p], fy = queries[3 * (int64_t)p + 1], fz = queries[3 * (int64_t)p + 2];
            ok = isfinite(fx) && isfinite(fy) && isfinite(fz);
            if (!ok) atomicOr(bad, 1);
            v.x = (double)fx; v.y = (double)fy; v.z = (double)fz;
            v.self = -1;
            row = p;
        } else {
            const nwq_pt pt = pts[p];
            v.x = (double)pt.x; v.y = (double)pt.y; v.z = (double)pt.z;
            v.self = pt.i;
            row = pt.i;
        }
        if (ok) {
            v.m = m;
            v.e2 = s_e2;
            v.E = E;
            v.col = s_col + lane;
            v.tests = 0u;
            long long read = 0;
            nwq_walk(pts, cstart, G, v.x, v.y, v.z, r_max, r_max2, v, &read);
            tests = v.tests;
            cells = (u64)read;
        }
    }
    if (local && row >= 0) {
        for (int b = 0; b < m; ++b) local[row * m + b] = s_col[b * LANES + lane];
    }
    __syncthreads();
    // thread b adds row b over the lanes, starting b lanes in: the threads of a wave read different banks
    u64 sum = 0;
    if (lane < m) {
        for (int j = 0; j < LANES; ++j) sum += s_col[lane * LANES + ((j + lane) & (LANES - 1))];
    }
    if (lane < BINS) part_hist[(int64_t)blockIdx.x * BINS + lane] = sum;
    // the two counters: a butterfly within each wave, then the waves through the columns' memory
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { tests += __shfl_xor(tests, o, 64); cells += __shfl_xor(cells, o, 64); }
    __syncthreads();                                          // (the columns have been read)
    u64 *s_w = (u64 *)s_col;
    if ((lane & 63) == 0) { s_w[(lane >> 6) * NWQ_COUNTERS + NWQ_C_TESTS] = tests; s_w[(lane >> 6) * NWQ_COUNTERS + NWQ_C_CELLS] = cells; }
    __syncthreads();
    if (lane < NWQ_COUNTERS) {
        u64 s = 0;
        for (int w = 0; w < WAVES; ++w) s += s_w[w * NWQ_COUNTERS + lane];
        part_cnt[(int64_t)blockIdx.x * NWQ_COUNTERS + lane] = s;
    }
}

// out[c] = the sum of column c of rows[nb][width], width a power of two up to NWQ_BLOCK: a thread adds every (NWQ_BLOCK / width)-th row
// of its column, then the column's threads are added in order
__device__ __forceinline__ void pq_column_sums(const u64 *__restrict__ rows, int64_t nb, int width, u64 *__restrict__ out, u64 *s_acc)
{
    const int c = threadIdx.x & (width - 1), s = threadIdx.x / width, slices = NWQ_BLOCK / width;
    u64 acc = 0;
    for (int64_t b = s; b < nb; b += slices) acc += rows[b * width + c];
    __syncthreads();
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < width) {
        u64 t = 0;
        for (int k = 0; k < slices; ++k) t += s_acc[k * width + threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// totals[0 .. bins) = hist (the rows' padding adds zeros), totals[NWQ_MAX_BINS ..] = the two counters
__global__ __launch_bounds__(NWQ_BLOCK) void k_pq_totals(const u64 *__restrict__ part_hist, const u64 *__restrict__ part_cnt, int64_t nb, int bins,
                                                         u64 *__restrict__ totals)
{
    __shared__ u64 s_acc[NWQ_BLOCK];
    pq_column_sums(part_hist, nb, bins, totals, s_acc);
    pq_column_sums(part_cnt, nb, NWQ_COUNTERS, totals + NWQ_MAX_BINS, s_acc);
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;

struct nwq_ctx : bq::Ctx {
    bq::CloudGrid grid;                 // the cloud (nwq_set_cloud), its box and its cells
    // the edges (nwq_set_edges): m = 0 until then
    int m = 0;
    double radii[NWQ_MAX_BINS], e2[NWQ_MAX_BINS];
    bool edges_on_device = false;
    DevBuf e2_dev;
    double cell_of_rmax = NWQ_CELL_OF_RMAX;
    // one count
    DevBuf q, local, part_hist, part_cnt, totals, flag;
};

namespace {

#define NWQ_HIP(call) BQ_HIP(call, NWQ_ERR_NOMEM, NWQ_ERR_HIP)

const bq::CloudCodes NWQ_CODES = {NWQ_ERR_BADARG, NWQ_ERR_NONFINITE, NWQ_ERR_NOMEM, NWQ_ERR_HIP};

// the cell size a count starts from: NWQ_CELL_OF_RMAX of the largest radius (bq::cloud_cell); a cloud without extent and a zero radius
// get one cell of side 1
double starting_cell(const nwq_ctx *ctx, double r_max) { return bq::cloud_cell(ctx->cell_of_rmax * r_max, ctx->grid.emax()); }

}  // namespace

NWQ_EXPORT int nwq_abi_version(void) { return NWQ_ABI_VERSION; }

NWQ_EXPORT int nwq_create(int device, nwq_ctx **out)
{
    const int r = bq::create(device, out, NWQ_ERR_BADARG, NWQ_ERR_HIP);
    if (r != 0) return r;
    // (developer knob for profiles/pairs.txt's sweep of the starting cell; no output depends on it)
    const char *s = std::getenv("NW_PAIRS_CELL_OF_RMAX");
    const double v = s ? std::atof(s) : 0.0;
    if (v >= 0.01 && v <= 100.0) (*out)->cell_of_rmax = v;
    return NWQ_OK;
}

NWQ_EXPORT void nwq_destroy(nwq_ctx *ctx) { bq::destroy(ctx); }

NWQ_EXPORT const char *nwq_last_error(nwq_ctx *ctx) { return bq::last_error(ctx); }

NWQ_EXPORT int nwq_set_cloud(nwq_ctx *ctx, const float *xyz, int64_t n, int on_device)
{
    if (!xyz || n < 1 || n > NWQ_MAX_N || (on_device != 0 && on_device != 1)) return NWQ_ERR_BADARG;
    if (!on_device && !bq::all_finite(xyz, 3 * n)) {
        if (ctx) ctx->grid.forget();                              // (a failed call leaves no cloud, whichever check failed)
        return fail(ctx, NWQ_ERR_NONFINITE, "nwq_set_cloud: a localization is not finite");
    }
    if (!ctx) return NWQ_ERR_BADARG;
    NWQ_HIP(hipSetDevice(ctx->device));
    const bq::CloudStatus s = ctx->grid.set_cloud(ctx->stream, xyz, n, on_device != 0);
    return s.ok() ? NWQ_OK : bq::cloud_fail(ctx, "nwq_set_cloud", s, NWQ_CODES);
}

NWQ_EXPORT int nwq_set_edges(nwq_ctx *ctx, const double *radii, int64_t m)
{
    double e2[NWQ_MAX_BINS];
    if (!nwq_edges(radii, m, e2)) return fail(ctx, NWQ_ERR_BADARG, "nwq_set_edges: 1 to 64 finite radii, 0 <= r_0 < r_1 < ... <= 2^40, with ascending squares");
    if (!ctx) return NWQ_ERR_BADARG;
    ctx->m = (int)m;
    for (int b = 0; b < NWQ_MAX_BINS; ++b) { ctx->e2[b] = e2[b]; ctx->radii[b] = b < m ? radii[b] : 0.0; }
    ctx->edges_on_device = false;
    return NWQ_OK;
}

NWQ_EXPORT int nwq_count(nwq_ctx *ctx, const float *queries, int64_t nq, int on_device, uint64_t *hist, uint32_t *local, int64_t *info)
{
    if (!hist || !info || (on_device != 0 && on_device != 1)) return NWQ_ERR_BADARG;
    if (queries ? (nq < 1 || nq > NWQ_MAX_N) : nq < 0) return NWQ_ERR_BADARG;
    if (queries && !on_device && !bq::all_finite(queries, 3 * nq)) return fail(ctx, NWQ_ERR_NONFINITE, "nwq_count: a query is not finite");
    if (!ctx) return NWQ_ERR_BADARG;
    if (ctx->grid.n < 1) return fail(ctx, NWQ_ERR_NOCLOUD, "nwq_count: nwq_set_cloud first");
    if (ctx->m < 1) return fail(ctx, NWQ_ERR_NOCLOUD, "nwq_count: nwq_set_edges first");
    if (!queries && nq != 0 && nq != ctx->grid.n) return fail(ctx, NWQ_ERR_BADARG, "nwq_count: without queries nq is 0 or the cloud's n");
    NWQ_HIP(hipSetDevice(ctx->device));
    const int m = ctx->m;
    const double r_max = ctx->radii[m - 1], r_max2 = ctx->e2[m - 1];
    const bq::CloudStatus binned = ctx->grid.bin(ctx->stream, starting_cell(ctx, r_max));
    if (!binned.ok()) return bq::cloud_fail(ctx, "nwq", binned, NWQ_CODES);
    const bq::Grid<float> &g = ctx->grid.g;
    hipStream_t st = ctx->stream;
    const int n_queries = queries ? (int)nq : ctx->grid.n;
    const bool wide = m > NWQ_NARROW_BINS;
    const int lanes = wide ? NWQ_LANES_WIDE : NWQ_LANES_NARROW, bins = wide ? NWQ_MAX_BINS : NWQ_NARROW_BINS;
    const int nb = bq::nblk(n_queries, lanes);

    const float *dq = nullptr;
    if (queries) {
        dq = queries;
        if (!on_device) {
            NWQ_HIP(bq::upload(st, ctx->q, queries, 3 * nq));
            dq = ctx->q.as<float>();
        }
    }
    if (!ctx->edges_on_device) {
        NWQ_HIP(bq::upload(st, ctx->e2_dev, ctx->e2, NWQ_MAX_BINS));
        NWQ_HIP(hipStreamSynchronize(st));
        ctx->edges_on_device = true;
    }
    const size_t local_words = (size_t)n_queries * (size_t)m;
    if (local)
        NWQ_HIP(ctx->local.ensure(sizeof(u32) * local_words));
    NWQ_HIP(ctx->part_hist.ensure(sizeof(u64) * (size_t)bins * (size_t)nb));
    NWQ_HIP(ctx->part_cnt.ensure(sizeof(u64) * NWQ_COUNTERS * (size_t)nb));
    NWQ_HIP(ctx->totals.ensure(sizeof(u64) * (NWQ_MAX_BINS + NWQ_COUNTERS)));
    NWQ_HIP(ctx->flag.ensure(sizeof(int)));
    NWQ_HIP(hipMemsetAsync(ctx->flag.p, 0, sizeof(int), st));

    nwq_grid G;
    for (int d = 0; d < 3; ++d) { G.lo[d] = (double)g.lo[d]; G.hi[d] = (double)g.hi[d]; G.dims[d] = g.dims[d]; }
    G.h = (double)g.h;
    pq_edges E;
    for (int b = 0; b < NWQ_NARROW_BINS; ++b) E.e2[b] = ctx->e2[b];
    u32 *dlocal = local ? ctx->local.as<u32>() : nullptr;
    if (wide)
        hipLaunchKernelGGL(k_pq_pairs<true>, dim3(nb), dim3(lanes), 0, st, dq, n_queries, ctx->grid.sorted.as<nwq_pt>(), ctx->grid.cstart.as<int>(), G, E, ctx->e2_dev.as<double>(),
                           m, r_max, r_max2, dlocal, ctx->part_hist.as<u64>(), ctx->part_cnt.as<u64>(), ctx->flag.as<int>());
    else
        hipLaunchKernelGGL(k_pq_pairs<false>, dim3(nb), dim3(lanes), 0, st, dq, n_queries, ctx->grid.sorted.as<nwq_pt>(), ctx->grid.cstart.as<int>(), G, E, ctx->e2_dev.as<double>(),
                           m, r_max, r_max2, dlocal, ctx->part_hist.as<u64>(), ctx->part_cnt.as<u64>(), ctx->flag.as<int>());
    hipLaunchKernelGGL(k_pq_totals, dim3(1), dim3(NWQ_BLOCK), 0, st, ctx->part_hist.as<u64>(), ctx->part_cnt.as<u64>(), (int64_t)nb, bins, ctx->totals.as<u64>());
    NWQ_HIP(hipGetLastError());

    u64 tot[NWQ_MAX_BINS + NWQ_COUNTERS];
    int bad = 0;
    NWQ_HIP(hipMemcpyAsync(tot, ctx->totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    NWQ_HIP(hipMemcpyAsync(&bad, ctx->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    NWQ_HIP(hipStreamSynchronize(st));
    if (bad) return fail(ctx, NWQ_ERR_NONFINITE, "nwq_count: a query is not finite");
    if (local) {
        NWQ_HIP(hipMemcpyAsync(local, ctx->local.p, sizeof(u32) * local_words, hipMemcpyDeviceToHost, st));
        NWQ_HIP(hipStreamSynchronize(st));
    }
    for (int b = 0; b < m; ++b) hist[b] = tot[b];
    info[NWQ_INFO_TESTS] = (int64_t)tot[NWQ_MAX_BINS + NWQ_C_TESTS];
    info[NWQ_INFO_CELLS_READ] = (int64_t)tot[NWQ_MAX_BINS + NWQ_C_CELLS];
    info[NWQ_INFO_CELL_SIZE] = __builtin_bit_cast(int64_t, G.h);
    info[NWQ_INFO_CELLS] = g.cells();
    info[NWQ_INFO_VARIANT] = wide ? 1 : 0;
    info[NWQ_INFO_N_QUERIES] = n_queries;
    info[NWQ_INFO_N_CLOUD] = ctx->grid.n;
    info[NWQ_INFO_BINS] = m;
    return NWQ_OK;
}
