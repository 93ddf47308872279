// Exact DBSCAN clustering of a localization cloud on the device (MI355X, gfx950): include/nw_clustering.h.
//
//   (bq::CloudGrid: set_cloud, bin)   the cloud query units' shared cloud grid in float (nw_bq.h): bounding box and finiteness of the
//                                     cloud, the cloud in cell order with every point's index in the caller's array, the cells' starts
//   k_pc_count       one lane per point, in cell order: the ring walk up to count_cap -> count, core; shortcut (a)
//   k_pc_hook        one lane per core point: union with every core point near it that has a smaller index, as k_ws_hook does it (find
//                    both roots, CAS the larger onto the smaller, climb from what is found on failure); shortcut (b): a cell's core
//                    points go through its smallest-index one, and one near pair then joins two cells
//   k_pc_compress    root of every core point, the root flags
//   bq::scan_total + k_pc_number      roots are flagged, scanned (the query units' shared scan) and every core point gets its root's rank
//   k_pc_border      one lane per non-core point: the same walk, the (d2, index) minimum over the core points near it
//   k_pc_stats       size, n_core (integer adds), first and the box (ordered-key min / max) per cluster; results of atomics are not read
//   k_pc_totals      the blocks' counters, one workgroup, a fixed order
//
// The definition -- near, the walk, the guard of the shortcuts, the three visitors -- is csrc/nw_clustering_core.h, which the tests also
// compile for the CPU.  The device buffer, the cloud grid and the context's scaffolding are the query units' shared ones (nw_bq.h).
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <climits>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/nw_clustering.h"
#include "nw_bq.h"
#include "nw_clustering_core.h"

#define NWP_EXPORT extern "C" __attribute__((visibility("default")))
#define NWP_BLOCK 256
#define NWP_WAVES (NWP_BLOCK / 64)
// the blocks' counters
#define NWP_PARTIALS 8
#define NWP_P_TESTS_COUNT 0
#define NWP_P_SHORTCUT_A 1
#define NWP_P_TESTS_HOOK 2
#define NWP_P_SHORTCUT_B 3
#define NWP_P_TESTS_BORDER 4
#define NWP_P_N_CORE 5
#define NWP_P_N_BORDER 6
#define NWP_P_N_NOISE 7

typedef long long i64;
typedef unsigned long long u64;

// what the kernels need of the grid besides the cells' starts
struct pc_grid {
    bq::Grid<float> g;
    double h;                           // (double)g.h
};

__device__ __forceinline__ int pc_cell_of(const nwp_pt &p, const bq::Grid<float> &g, int *cx, int *cy, int *cz)
{
    *cx = bq::cell_1d(p.x, g.lo[0], g.h, g.dims[0]);
    *cy = bq::cell_1d(p.y, g.lo[1], g.h, g.dims[1]);
    *cz = bq::cell_1d(p.z, g.lo[2], g.h, g.dims[2]);
    return (*cz * g.dims[1] + *cy) * g.dims[0] + *cx;
}

// two counters of a block into its row of the partials (col_b < 0: one counter): a butterfly within each wave, then the waves in order
__device__ __forceinline__ void pc_block_counters(i64 a, i64 b, int col_a, int col_b, i64 *__restrict__ partial)
{
    __shared__ i64 s_w[NWP_WAVES][2];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_w[threadIdx.x >> 6][0] = a; s_w[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < (col_b < 0 ? 1 : 2)) {
        i64 s = 0;
        for (int w = 0; w < NWP_WAVES; ++w) s += s_w[w][threadIdx.x];
        partial[(int64_t)blockIdx.x * NWP_PARTIALS + (threadIdx.x == 0 ? col_a : col_b)] = s;
    }
}

// cell_min[c] = the smallest index among the core points of cell c (read by k_pc_hook, shortcut (b)); parent[i] = i
__global__ __launch_bounds__(NWP_BLOCK) void k_pc_count(const nwp_pt *__restrict__ pts, const int *__restrict__ cstart, pc_grid G, int n, double eps2,
                                                        int min_points, int cap, int shortcuts, int *__restrict__ count, unsigned char *__restrict__ core,
                                                        unsigned char *__restrict__ core_sorted, int *__restrict__ parent, int *__restrict__ cell_min,
                                                        i64 *__restrict__ partial)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    i64 tests = 0, by_a = 0;
    if (p < n) {
        const nwp_pt pt = pts[p];
        int cx, cy, cz;
        const int c = pc_cell_of(pt, G.g, &cx, &cy, &cz);
        int cnt;
        if (shortcuts && cstart[c + 1] - cstart[c] >= cap) {
            cnt = cap;                                        // (a): every point of the cell is near
            by_a = 1;
        } else {
            nwp_count_visit v = {(double)pt.x, (double)pt.y, (double)pt.z, eps2, 0, cap, 0};
            nwp_walk(pts, cstart, G.g.dims, G.h, cx, cy, cz, eps2, 0, v);
            cnt = v.cnt;
            tests = v.tests;
        }
        const bool is_core = cnt >= min_points;               // (below the cap the walk was complete: cnt = n_eps)
        count[pt.i] = cnt;
        core[pt.i] = is_core ? 1 : 0;
        core_sorted[p] = is_core ? 1 : 0;
        parent[pt.i] = pt.i;
        if (shortcuts && is_core) atomicMin(&cell_min[c], pt.i);
    }
    pc_block_counters(tests, by_a, NWP_P_TESTS_COUNT, NWP_P_SHORTCUT_A, partial);
}

// ---- union-find, as nw_surgery.hip's (ECL-CC) ---------------------------------------------------------------------------------------
__device__ __forceinline__ int pc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of v with path halving; parent[x] <= x always (hooking only ever lowers it), so the walk ends at the smallest index of the tree
__device__ int pc_find(int *parent, int v)
{
    int p = pc_load(&parent[v]);
    while (true) {
        const int gp = pc_load(&parent[p]);
        if (gp == p) return p;
        __hip_atomic_store(&parent[v], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (any ancestor is a valid parent)
        v = p;
        p = gp;
    }
}

struct pc_union {
    int *parent;
    __device__ void unite(int f, int g)
    {
        int a = pc_find(parent, f), b = pc_find(parent, g);
        while (a != b) {
            if (a > b) { const int s = a; a = b; b = s; }
            // hook root b onto a; if b is no longer a root, climb from what it points to now
            const int old = atomicCAS(&parent[b], b, a);
            if (old == b) break;
            b = pc_find(parent, old);
        }
    }
};

__global__ __launch_bounds__(NWP_BLOCK) void k_pc_hook(const nwp_pt *__restrict__ pts, const int *__restrict__ cstart, pc_grid G, int n, double eps2,
                                                       int shortcuts, const unsigned char *__restrict__ core_sorted, const int *__restrict__ cell_min,
                                                       int *parent, i64 *__restrict__ partial)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    i64 tests = 0, by_b = 0;
    if (p < n && core_sorted[p]) {
        const nwp_pt pt = pts[p];
        int cx, cy, cz;
        const int c = pc_cell_of(pt, G.g, &cx, &cy, &cz);
        pc_union u = {parent};
        if (shortcuts) {
            const int m = cell_min[c];                        // (b): the cell's core points are all near each other
            if (m < pt.i) { u.unite(pt.i, m); by_b = 1; }
        }
        nwp_hook_visit<pc_union> v = {(double)pt.x, (double)pt.y, (double)pt.z, eps2, pt.i, shortcuts != 0, core_sorted, &u, 0};
        nwp_walk(pts, cstart, G.g.dims, G.h, cx, cy, cz, eps2, shortcuts ? 1 : 0, v);
        tests = v.tests;
    }
    pc_block_counters(tests, by_b, NWP_P_TESTS_HOOK, NWP_P_SHORTCUT_B, partial);
}

// root[i] = the root of core point i, -1 for the others (a separate array: concurrent path halving may still rewrite parent[])
__global__ __launch_bounds__(NWP_BLOCK) void k_pc_compress(int n, const unsigned char *__restrict__ core, int *parent, int *__restrict__ root,
                                                           int *__restrict__ is_root)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!core[i]) { root[i] = -1; is_root[i] = 0; return; }
    const int r = pc_find(parent, i);
    root[i] = r;
    is_root[i] = (r == i) ? 1 : 0;
}

// a core point: the rank of its root among the roots, and itself as its anchor; -1 for the others until k_pc_border
__global__ __launch_bounds__(NWP_BLOCK) void k_pc_number(int n, const int *__restrict__ root, const int *__restrict__ rank, int *__restrict__ label,
                                                         int *__restrict__ anchor)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    label[i] = r < 0 ? -1 : rank[r];
    anchor[i] = r < 0 ? -1 : i;
}

__global__ __launch_bounds__(NWP_BLOCK) void k_pc_border(const nwp_pt *__restrict__ pts, const int *__restrict__ cstart, pc_grid G, int n, double eps2,
                                                         const unsigned char *__restrict__ core_sorted, const int *__restrict__ root,
                                                         const int *__restrict__ rank, int *__restrict__ label, int *__restrict__ anchor,
                                                         i64 *__restrict__ partial)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    i64 tests = 0;
    if (p < n && !core_sorted[p]) {
        const nwp_pt pt = pts[p];
        int cx, cy, cz;
        pc_cell_of(pt, G.g, &cx, &cy, &cz);
        nwp_border_visit v = {(double)pt.x, (double)pt.y, (double)pt.z, eps2, core_sorted, 0.0, -1, 0};
        nwp_walk(pts, cstart, G.g.dims, G.h, cx, cy, cz, eps2, 0, v);
        tests = v.tests;
        if (v.best_i >= 0) {                                  // (only core points' entries of label are read elsewhere: none is written here)
            anchor[pt.i] = v.best_i;
            label[pt.i] = rank[root[v.best_i]];
        }
    }
    pc_block_counters(tests, 0, NWP_P_TESTS_BORDER, -1, partial);
}

// ---- per-cluster statistics ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ i64 pc_wave_sum(i64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int pc_wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int pc_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// the label every lane of the wave holds (lanes with -1 aside), or -2 if they differ; -1 if no lane holds one
__device__ __forceinline__ int pc_wave_label(int lab)
{
    const u64 live = __ballot(lab >= 0);
    if (live == 0ull) return -1;
    const int first = __shfl(lab, __ffsll((unsigned long long)live) - 1, 64);
    return __ballot(lab >= 0 && lab != first) == 0ull ? first : -2;
}

struct pc_acc {
    u64 *size, *n_core;                 // C each
    int *first;                         // C, starts at INT_MAX
    int *lo, *hi;                       // 3C ordered keys each, start at INT_MAX / INT_MIN
};

__global__ __launch_bounds__(NWP_BLOCK) void k_pc_stats(const float *__restrict__ xyz, const int *__restrict__ label, const unsigned char *__restrict__ core,
                                                        int n, pc_acc acc, i64 *__restrict__ partial)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lab = i < n ? label[i] : -1;
    const bool is_core = i < n && core[i];
    i64 n_core = is_core ? 1 : 0, n_border = (lab >= 0 && !is_core) ? 1 : 0, n_noise = (i < n && lab < 0) ? 1 : 0;
    i64 cs = lab >= 0 ? 1 : 0, cc = n_core;
    int first = is_core ? i : INT_MAX;
    int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = INT_MIN, hi1 = INT_MIN, hi2 = INT_MIN;
    if (lab >= 0) {
        lo0 = hi0 = bq::enc_ord(xyz[3 * (int64_t)i]);
        lo1 = hi1 = bq::enc_ord(xyz[3 * (int64_t)i + 1]);
        lo2 = hi2 = bq::enc_ord(xyz[3 * (int64_t)i + 2]);
    }
    // one set of atomics per wave when every labelled lane of the wave holds the same cluster
    const int wl = pc_wave_label(lab);
    bool emit = lab >= 0;
    int c = lab;
    if (wl >= 0) {
        cs = pc_wave_sum(cs); cc = pc_wave_sum(cc);
        first = pc_wave_min(first);
        lo0 = pc_wave_min(lo0); lo1 = pc_wave_min(lo1); lo2 = pc_wave_min(lo2);
        hi0 = pc_wave_max(hi0); hi1 = pc_wave_max(hi1); hi2 = pc_wave_max(hi2);
        emit = (threadIdx.x & 63) == 0;
        c = wl;
    }
    if (emit) {
        atomicAdd(&acc.size[c], (u64)cs);
        if (cc) atomicAdd(&acc.n_core[c], (u64)cc);
        if (first != INT_MAX) atomicMin(&acc.first[c], first);
        atomicMin(&acc.lo[3 * (int64_t)c], lo0); atomicMin(&acc.lo[3 * (int64_t)c + 1], lo1); atomicMin(&acc.lo[3 * (int64_t)c + 2], lo2);
        atomicMax(&acc.hi[3 * (int64_t)c], hi0); atomicMax(&acc.hi[3 * (int64_t)c + 1], hi1); atomicMax(&acc.hi[3 * (int64_t)c + 2], hi2);
    }
    // the block's three counters
    __shared__ i64 s_w[NWP_WAVES][3];
    n_core = pc_wave_sum(n_core); n_border = pc_wave_sum(n_border); n_noise = pc_wave_sum(n_noise);
    if ((threadIdx.x & 63) == 0) { s_w[threadIdx.x >> 6][0] = n_core; s_w[threadIdx.x >> 6][1] = n_border; s_w[threadIdx.x >> 6][2] = n_noise; }
    __syncthreads();
    if (threadIdx.x < 3) {
        i64 s = 0;
        for (int w = 0; w < NWP_WAVES; ++w) s += s_w[w][threadIdx.x];
        partial[(int64_t)blockIdx.x * NWP_PARTIALS + NWP_P_N_CORE + threadIdx.x] = s;
    }
}

// out[c] = the blocks' counters in a fixed order
__global__ __launch_bounds__(NWP_BLOCK) void k_pc_totals(const i64 *__restrict__ partial, int64_t nb, i64 *__restrict__ out)
{
    __shared__ i64 s_w[NWP_WAVES][NWP_PARTIALS];
    i64 v[NWP_PARTIALS];
#pragma unroll
    for (int c = 0; c < NWP_PARTIALS; ++c) v[c] = 0;
    for (int64_t b = threadIdx.x; b < nb; b += NWP_BLOCK) {
#pragma unroll
        for (int c = 0; c < NWP_PARTIALS; ++c) v[c] += partial[b * NWP_PARTIALS + c];
    }
#pragma unroll
    for (int c = 0; c < NWP_PARTIALS; ++c) v[c] = pc_wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NWP_PARTIALS; ++c) s_w[threadIdx.x >> 6][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < NWP_PARTIALS) {
        i64 s = 0;
        for (int w = 0; w < NWP_WAVES; ++w) s += s_w[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;

struct nwp_ctx : bq::Ctx {
    bq::CloudGrid grid;                 // the cloud (nwp_set_cloud), its box and its cells
    bool shortcuts = true;
    // one query
    DevBuf count, core, core_sorted, parent, cell_min, root, is_root, rank, label, anchor, partial, totals;
    // the last query's clusters (-1: none)
    int n_clusters = -1;
    DevBuf size, n_core, first, lo, hi;
};

namespace {

#define NWP_HIP(call) BQ_HIP(call, NWP_ERR_NOMEM, NWP_ERR_HIP)

const bq::CloudCodes NWP_CODES = {NWP_ERR_BADARG, NWP_ERR_NONFINITE, NWP_ERR_NOMEM, NWP_ERR_HIP};

inline int nblk(int64_t n) { return bq::nblk(n, NWP_BLOCK); }

// the cell size a query starts from: NWP_CELL_OF_EPS of eps (bq::cloud_cell)
double starting_cell(const nwp_ctx *ctx, double eps) { return bq::cloud_cell(NWP_CELL_OF_EPS * eps, ctx->grid.emax()); }

}  // namespace

NWP_EXPORT int nwp_abi_version(void) { return NWP_ABI_VERSION; }

NWP_EXPORT int nwp_create(int device, nwp_ctx **out) { return bq::create(device, out, NWP_ERR_BADARG, NWP_ERR_HIP); }

NWP_EXPORT void nwp_destroy(nwp_ctx *ctx) { bq::destroy(ctx); }

NWP_EXPORT const char *nwp_last_error(nwp_ctx *ctx) { return bq::last_error(ctx); }

NWP_EXPORT int nwp_set_cloud(nwp_ctx *ctx, const float *xyz, int64_t n, int on_device)
{
    if (!xyz || n < 1 || n > NWP_MAX_N || (on_device != 0 && on_device != 1)) return NWP_ERR_BADARG;
    if (!on_device && !bq::all_finite(xyz, 3 * n)) return fail(ctx, NWP_ERR_NONFINITE, "nwp_set_cloud: a localization is not finite");
    if (!ctx) return NWP_ERR_BADARG;
    NWP_HIP(hipSetDevice(ctx->device));
    ctx->n_clusters = -1;
    const bq::CloudStatus s = ctx->grid.set_cloud(ctx->stream, xyz, n, on_device != 0);
    return s.ok() ? NWP_OK : bq::cloud_fail(ctx, "nwp_set_cloud", s, NWP_CODES);
}

NWP_EXPORT int nwp_set_shortcuts(nwp_ctx *ctx, int on)
{
    if (!ctx || (on != 0 && on != 1)) return NWP_ERR_BADARG;
    ctx->shortcuts = on != 0;
    return NWP_OK;
}

NWP_EXPORT int nwp_dbscan(nwp_ctx *ctx, double eps, int64_t min_points, int64_t count_cap, int32_t *label, int32_t *anchor, int32_t *count, uint8_t *core,
                          int32_t *n_clusters, int64_t *info)
{
    if (!n_clusters || !info || !nwp_args_ok(eps, min_points, count_cap)) return NWP_ERR_BADARG;
    if (!ctx) return NWP_ERR_BADARG;
    if (ctx->grid.n < 1) return fail(ctx, NWP_ERR_NOCLOUD, "nwp_dbscan: nwp_set_cloud first");
    NWP_HIP(hipSetDevice(ctx->device));
    ctx->n_clusters = -1;
    const bq::CloudStatus binned = ctx->grid.bin(ctx->stream, starting_cell(ctx, eps));
    if (!binned.ok()) return bq::cloud_fail(ctx, "nwp", binned, NWP_CODES);
    const int n = ctx->grid.n, nb = nblk(n);
    const int64_t ncell = ctx->grid.g.cells();
    pc_grid G;
    G.g = ctx->grid.g;
    G.h = (double)ctx->grid.g.h;
    const double eps2 = eps * eps;
    const int shortcuts = (ctx->shortcuts && nwp_shortcuts_ok(G.h, eps)) ? 1 : 0;
    hipStream_t st = ctx->stream;

    NWP_HIP(ctx->count.ensure(sizeof(int) * (size_t)n));
    NWP_HIP(ctx->core.ensure((size_t)n));
    NWP_HIP(ctx->core_sorted.ensure((size_t)n));
    NWP_HIP(ctx->parent.ensure(sizeof(int) * (size_t)n));
    NWP_HIP(ctx->cell_min.ensure(sizeof(int) * (size_t)ncell));
    NWP_HIP(ctx->root.ensure(sizeof(int) * (size_t)n));
    NWP_HIP(ctx->is_root.ensure(sizeof(int) * (size_t)n));
    NWP_HIP(ctx->rank.ensure(sizeof(int) * ((size_t)n + 1)));
    NWP_HIP(ctx->label.ensure(sizeof(int) * (size_t)n));
    NWP_HIP(ctx->anchor.ensure(sizeof(int) * (size_t)n));
    NWP_HIP(ctx->partial.ensure(sizeof(i64) * NWP_PARTIALS * (size_t)nb));
    NWP_HIP(ctx->totals.ensure(sizeof(i64) * NWP_PARTIALS));
    NWP_HIP(hipMemsetAsync(ctx->partial.p, 0, sizeof(i64) * NWP_PARTIALS * (size_t)nb, st));
    if (shortcuts) NWP_HIP(hipMemsetD32Async((hipDeviceptr_t)ctx->cell_min.p, INT_MAX, (size_t)ncell, st));

    const nwp_pt *pts = ctx->grid.sorted.as<nwp_pt>();
    const int *cstart = ctx->grid.cstart.as<int>();
    hipLaunchKernelGGL(k_pc_count, dim3(nb), dim3(NWP_BLOCK), 0, st, pts, cstart, G, n, eps2, (int)min_points, (int)count_cap, shortcuts, ctx->count.as<int>(),
                       ctx->core.as<unsigned char>(), ctx->core_sorted.as<unsigned char>(), ctx->parent.as<int>(), ctx->cell_min.as<int>(), ctx->partial.as<i64>());
    hipLaunchKernelGGL(k_pc_hook, dim3(nb), dim3(NWP_BLOCK), 0, st, pts, cstart, G, n, eps2, shortcuts, ctx->core_sorted.as<unsigned char>(),
                       ctx->cell_min.as<int>(), ctx->parent.as<int>(), ctx->partial.as<i64>());
    hipLaunchKernelGGL(k_pc_compress, dim3(nb), dim3(NWP_BLOCK), 0, st, n, ctx->core.as<unsigned char>(), ctx->parent.as<int>(), ctx->root.as<int>(),
                       ctx->is_root.as<int>());
    NWP_HIP(hipGetLastError());
    int C = -1;
    NWP_HIP(bq::scan_total(st, ctx->is_root.as<int>(), n, ctx->rank.as<int>(), ctx->grid.scan_tmp, &C));
    if (C < 0 || C > n) return fail(ctx, NWP_ERR_HIP, "nwp_dbscan: the roots do not add up");
    hipLaunchKernelGGL(k_pc_number, dim3(nb), dim3(NWP_BLOCK), 0, st, n, ctx->root.as<int>(), ctx->rank.as<int>(), ctx->label.as<int>(), ctx->anchor.as<int>());
    hipLaunchKernelGGL(k_pc_border, dim3(nb), dim3(NWP_BLOCK), 0, st, pts, cstart, G, n, eps2, ctx->core_sorted.as<unsigned char>(), ctx->root.as<int>(),
                       ctx->rank.as<int>(), ctx->label.as<int>(), ctx->anchor.as<int>(), ctx->partial.as<i64>());
    NWP_HIP(hipGetLastError());

    const size_t Cb = (size_t)std::max(C, 1);
    NWP_HIP(ctx->size.ensure(sizeof(u64) * Cb));
    NWP_HIP(ctx->n_core.ensure(sizeof(u64) * Cb));
    NWP_HIP(ctx->first.ensure(sizeof(int) * Cb));
    NWP_HIP(ctx->lo.ensure(sizeof(int) * 3 * Cb));
    NWP_HIP(ctx->hi.ensure(sizeof(int) * 3 * Cb));
    NWP_HIP(hipMemsetAsync(ctx->size.p, 0, sizeof(u64) * Cb, st));
    NWP_HIP(hipMemsetAsync(ctx->n_core.p, 0, sizeof(u64) * Cb, st));
    NWP_HIP(hipMemsetD32Async((hipDeviceptr_t)ctx->first.p, INT_MAX, Cb, st));
    NWP_HIP(hipMemsetD32Async((hipDeviceptr_t)ctx->lo.p, INT_MAX, 3 * Cb, st));
    NWP_HIP(hipMemsetD32Async((hipDeviceptr_t)ctx->hi.p, INT_MIN, 3 * Cb, st));
    pc_acc acc = {ctx->size.as<u64>(), ctx->n_core.as<u64>(), ctx->first.as<int>(), ctx->lo.as<int>(), ctx->hi.as<int>()};
    hipLaunchKernelGGL(k_pc_stats, dim3(nb), dim3(NWP_BLOCK), 0, st, ctx->grid.cloud.as<float>(), ctx->label.as<int>(), ctx->core.as<unsigned char>(), n, acc,
                       ctx->partial.as<i64>());
    hipLaunchKernelGGL(k_pc_totals, dim3(1), dim3(NWP_BLOCK), 0, st, ctx->partial.as<i64>(), (int64_t)nb, ctx->totals.as<i64>());
    NWP_HIP(hipGetLastError());

    i64 tot[NWP_PARTIALS];
    NWP_HIP(hipMemcpyAsync(tot, ctx->totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    if (label) NWP_HIP(hipMemcpyAsync(label, ctx->label.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (anchor) NWP_HIP(hipMemcpyAsync(anchor, ctx->anchor.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (count) NWP_HIP(hipMemcpyAsync(count, ctx->count.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (core) NWP_HIP(hipMemcpyAsync(core, ctx->core.p, (size_t)n, hipMemcpyDeviceToHost, st));
    NWP_HIP(hipStreamSynchronize(st));

    *n_clusters = C;
    info[NWP_INFO_N_CORE] = tot[NWP_P_N_CORE];
    info[NWP_INFO_N_BORDER] = tot[NWP_P_N_BORDER];
    info[NWP_INFO_N_NOISE] = tot[NWP_P_N_NOISE];
    info[NWP_INFO_N_CLUSTERS] = C;
    info[NWP_INFO_CELLS] = ncell;
    info[NWP_INFO_CELL_SIZE] = __builtin_bit_cast(int64_t, G.h);
    info[NWP_INFO_TESTS] = (tot[NWP_P_TESTS_COUNT] + tot[NWP_P_TESTS_HOOK]) + tot[NWP_P_TESTS_BORDER];
    info[NWP_INFO_SHORTCUT_A] = tot[NWP_P_SHORTCUT_A];
    info[NWP_INFO_SHORTCUT_B] = tot[NWP_P_SHORTCUT_B];
    info[NWP_INFO_GUARD] = shortcuts;
    info[NWP_INFO_TESTS_COUNT] = tot[NWP_P_TESTS_COUNT];
    info[NWP_INFO_TESTS_HOOK] = tot[NWP_P_TESTS_HOOK];
    ctx->n_clusters = C;
    return NWP_OK;
}

NWP_EXPORT int nwp_cluster_stats(nwp_ctx *ctx, int64_t *size, int64_t *n_core, int32_t *first, float *bbox)
{
    if (!ctx) return NWP_ERR_BADARG;
    if (ctx->n_clusters < 0) return fail(ctx, NWP_ERR_NOCLOUD, "nwp_cluster_stats: nwp_dbscan first");
    const size_t C = (size_t)ctx->n_clusters;
    if (C == 0) return NWP_OK;
    NWP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<int> lo, hi;
    if (size) NWP_HIP(hipMemcpyAsync(size, ctx->size.p, sizeof(u64) * C, hipMemcpyDeviceToHost, st));
    if (n_core) NWP_HIP(hipMemcpyAsync(n_core, ctx->n_core.p, sizeof(u64) * C, hipMemcpyDeviceToHost, st));
    if (first) NWP_HIP(hipMemcpyAsync(first, ctx->first.p, sizeof(int) * C, hipMemcpyDeviceToHost, st));
    if (bbox) {
        lo.resize(3 * C);
        hi.resize(3 * C);
        NWP_HIP(hipMemcpyAsync(lo.data(), ctx->lo.p, sizeof(int) * 3 * C, hipMemcpyDeviceToHost, st));
        NWP_HIP(hipMemcpyAsync(hi.data(), ctx->hi.p, sizeof(int) * 3 * C, hipMemcpyDeviceToHost, st));
    }
    NWP_HIP(hipStreamSynchronize(st));
    if (bbox)
        for (size_t c = 0; c < C; ++c)
            for (int d = 0; d < 3; ++d) { bbox[6 * c + d] = bq::dec_ord(lo[3 * c + d]); bbox[6 * c + 3 + d] = bq::dec_ord(hi[3 * c + d]); }
    return NWP_OK;
}
