// The self-intersection check of a triangle mesh on the device (MI355X, gfx950): include/nw_intersections.h.
//
//   nwx_set_mesh    (bq::FaceGrid::set_faces)   the mesh query units' shared intake (nw_bq.h): k_bq_face_setup, one thread per face, the
//                                     float64 centroid and rho_f, the largest centroid-to-corner distance, a hair enlarged so that
//                                     rounding can only make a bound weaker; k_bq_rho_reduce, rho_max and the sum of rho_f, one
//                                     workgroup, a fixed order; bq::bounds, the centroids' box
//                   (bq::FaceGrid::bin)   the shared point grid in double over the centroids (bq::size_grid, bq::build_grid); a sorted
//                                     point carries its face id
//   nwx_find        k_mx_count        one thread per face f: the cells that overlap the box c_f +- (rho_f + rho_max), row by row; a
//                                     centroid with |c_f - c_g| (1 - slack) - rho_g > rho_f is passed over, every other face g != f gets
//                                     the pair predicate of nw_intersections_core.h with the smaller id first; count[f] = the faces
//                                     that f crosses, up[f] = those of them with g > f.  Both directions are computed: no atomics.
//                   k_mx_totals       the sums of two int arrays and how many entries of the second are > 0 (the pairs = the sum of
//                                     up[], the crossed faces = the entries of count[] above 0), one workgroup, integers
//                   (bq::scan_total)  with NWX_PAIRS: where each face's pairs start in the list
//                   k_mx_emit         with NWX_PAIRS: the same walk for the faces with up[f] > 0 (the others leave at once; crossed
//                                     faces are rare), over the partners g > f; pair k of the face goes to slot start[f] + k, and only
//                                     if k < up[f] -- were the two passes ever to disagree, nothing would be written out of range
//                   k_mx_stats        with NWX_STATS: the same walk once more, into arrays of its own: per face the candidates whose
//                                     centroids it read and those that reached the predicate (then k_mx_totals)
//   nwx_get_pairs   the list, sorted by (f, g) on the host
//
// The scan, the point grid, the face grid, the device buffer with its staging and the context's scaffolding are the query units' shared
// ones (nw_bq.h); the starting cell size is the distance unit's (twice the mean rho_f: a face or two per occupied cell).
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <array>
#include <algorithm>

#include "../../include/nw_intersections.h"
#include "nw_bq.h"
#include "nw_intersections_core.h"

#define NWX_EXPORT extern "C" __attribute__((visibility("default")))
#define NWX_BLOCK 256
#define NWX_SLACK BQ_FACE_RHO_SLACK   // relative slack of every bound: far above the rounding of a float64 distance, far below what matters
#define NWX_CELL_SLACK 1e-6       // of a cell, added to the box in cell units: far above the rounding of (x - lo) / h below 1025

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
// the cells [lo, hi] along one axis that a box of half-width w cells around the coordinate x can overlap
__device__ __forceinline__ void mx_cell_range(double x, double lo, double h, int dim, double w, int &c0, int &c1)
{
    const double t = (x - lo) / h;
    c0 = (int)fmin(fmax(floor(t - w - NWX_CELL_SLACK), 0.0), (double)(dim - 1));
    c1 = (int)fmin(fmax(floor(t + w + NWX_CELL_SLACK), 0.0), (double)(dim - 1));
}

// The walk of face f, three times over.  MX_COUNT: a = count[f], b = up[f] out.  MX_EMIT: b = up[f], start[f] in, pairs out.
// MX_STATS: a = the candidates read, b = those that reached the predicate, out.
enum { MX_COUNT = 0, MX_EMIT = 1, MX_STATS = 2 };

struct mx_mesh {
    const float *pos;
    const int *faces;
    int nf;
    const bq::PtF64 *pts;        // the centroids in cell order, each with its face id
    const int *cstart;
    const double *rho;
    double rho_max, lo0, lo1, lo2, h;
    int d0, d1, d2;
};

template <int MODE>
__device__ __forceinline__ void mx_walk(const mx_mesh &m, int f, int *__restrict__ a, int *__restrict__ b, const int *__restrict__ start,
                                        int *__restrict__ pairs)
{
    const int slots = MODE == MX_EMIT ? b[f] : 0;
    if (MODE == MX_EMIT && slots <= 0) return;
    const nwx_tri F = nwx_load(m.pos, m.faces, f);
    nwx_v3 c;
    (void)nwx_face_centroid(F, &c);                                  // (the centroid k_bq_face_setup stored, bit for bit: bq::face_centroid both times)
    const double rho_f = m.rho[f];
    const double w = (rho_f + m.rho_max) / m.h;
    int x0, x1, y0, y1, z0, z1;
    mx_cell_range(c.x, m.lo0, m.h, m.d0, w, x0, x1);
    mx_cell_range(c.y, m.lo1, m.h, m.d1, w, y0, y1);
    mx_cell_range(c.z, m.lo2, m.h, m.d2, w, z0, z1);
    const int64_t slot0 = MODE == MX_EMIT ? (int64_t)start[f] : 0;
    int n_a = 0, n_b = 0;
    for (int z = z0; z <= z1; ++z) {
        for (int y = y0; y <= y1; ++y) {
            const int row = (z * m.d1 + y) * m.d0;
            const int s = m.cstart[row + x0], e = m.cstart[row + x1 + 1];
            for (int p = s; p < e; ++p) {
                const bq::PtF64 r = m.pts[p];
                const int h = (int)r.i;
                if (h == f || h < 0 || h >= m.nf) continue;             // (out of range cannot happen: the grid's points are numbered by face)
                if (MODE == MX_EMIT && h < f) continue;
                if (MODE == MX_STATS) ++n_a;
                const double ex = r.x - c.x, ey = r.y - c.y, ez = r.z - c.z;
                const double cd = sqrt((ex * ex + ey * ey) + ez * ez);
                if (cd * (1.0 - NWX_SLACK) - m.rho[h] > rho_f) continue;  // the two faces are too far apart to meet
                if (MODE == MX_STATS) { ++n_b; continue; }
                const nwx_tri G = nwx_load(m.pos, m.faces, h);
                const bool first = f < h;
                nwx_tri A, B;
                A.i0 = first ? F.i0 : G.i0; A.i1 = first ? F.i1 : G.i1; A.i2 = first ? F.i2 : G.i2;
                B.i0 = first ? G.i0 : F.i0; B.i1 = first ? G.i1 : F.i1; B.i2 = first ? G.i2 : F.i2;
                A.a = first ? F.a : G.a; A.b = first ? F.b : G.b; A.c = first ? F.c : G.c;
                B.a = first ? G.a : F.a; B.b = first ? G.b : F.b; B.c = first ? G.c : F.c;
                if (!nwx_pair(A, B)) continue;
                if (MODE == MX_EMIT) {
                    if (n_b < slots) { pairs[2 * (slot0 + n_b)] = f; pairs[2 * (slot0 + n_b) + 1] = h; }
                    ++n_b;
                } else {
                    ++n_a;
                    if (h > f) ++n_b;
                }
            }
        }
    }
    if (MODE != MX_EMIT) { a[f] = n_a; b[f] = n_b; }
}

__global__ __launch_bounds__(NWX_BLOCK) void k_mx_count(mx_mesh m, int *__restrict__ count, int *__restrict__ up)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nf) mx_walk<MX_COUNT>(m, f, count, up, nullptr, nullptr);
}

__global__ __launch_bounds__(NWX_BLOCK) void k_mx_emit(mx_mesh m, int *__restrict__ up, const int *__restrict__ start, int *__restrict__ pairs)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nf) mx_walk<MX_EMIT>(m, f, nullptr, up, start, pairs);
}

__global__ __launch_bounds__(NWX_BLOCK) void k_mx_stats(mx_mesh m, int *__restrict__ n_read, int *__restrict__ n_tested)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nf) mx_walk<MX_STATS>(m, f, n_read, n_tested, nullptr, nullptr);
}

// out[0] = the sum of a[], out[1] = the sum of b[], out[2] = the number of entries of b[] above 0
__global__ __launch_bounds__(NWX_BLOCK) void k_mx_totals(const int *__restrict__ a, const int *__restrict__ b, int nf, long long *__restrict__ out)
{
    __shared__ long long s_a[NWX_BLOCK / 64], s_b[NWX_BLOCK / 64], s_n[NWX_BLOCK / 64];
    long long ta = 0, tb = 0, tn = 0;
    for (int j = threadIdx.x; j < nf; j += NWX_BLOCK) { ta += a[j]; tb += b[j]; tn += b[j] > 0 ? 1 : 0; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ta += __shfl_xor(ta, o, 64); tb += __shfl_xor(tb, o, 64); tn += __shfl_xor(tn, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = ta; s_b[threadIdx.x >> 6] = tb; s_n[threadIdx.x >> 6] = tn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3];
        out[1] = ((s_b[0] + s_b[1]) + s_b[2]) + s_b[3];
        out[2] = ((s_n[0] + s_n[1]) + s_n[2]) + s_n[3];
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwx_ctx : bq::Ctx {
    bq::FaceGrid m;               // the mesh of the last nwx_set_mesh and its grid (m.nf == 0: the context holds no mesh)
    // nwx_find
    bool has_pairs = false;       // the list of the last nwx_find with NWX_PAIRS is in `pairs`
    int64_t n_pairs = 0;
    int64_t stats[2] = {0, 0};
    DevBuf count, up, start, pairs, tot, n_read, n_tested;
};

namespace {

#define NWX_HIP(call) BQ_HIP(call, NWX_ERR_NOMEM, NWX_ERR_HIP)

const bq::FaceCodes NWX_FACE_CODES = {NWX_ERR_BADARG, NWX_ERR_NONFINITE, NWX_ERR_NOMEM, NWX_ERR_HIP};

}  // namespace

NWX_EXPORT int nwx_abi_version(void) { return NWX_ABI_VERSION; }

NWX_EXPORT int nwx_create(int device, nwx_ctx **out) { return bq::create(device, out, NWX_ERR_BADARG, NWX_ERR_HIP); }

NWX_EXPORT void nwx_destroy(nwx_ctx *ctx) { bq::destroy(ctx); }

NWX_EXPORT const char *nwx_last_error(nwx_ctx *ctx) { return bq::last_error(ctx); }

NWX_EXPORT int nwx_set_mesh(nwx_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces)
{
    if (ctx) { ctx->m.nf = 0; ctx->has_pairs = false; ctx->n_pairs = 0; ctx->stats[0] = ctx->stats[1] = 0; }
    bq::FaceStatus s = bq::check_faces(pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwx_set_mesh", s, NWX_FACE_CODES);
    if (!ctx) return NWX_ERR_BADARG;
    NWX_HIP(hipSetDevice(ctx->device));
    bq::FaceGrid &m = ctx->m;
    s = m.set_faces(ctx->stream, pos, n_vertices, faces, n_faces);
    // cell size: the distance unit's, twice the mean rho_f with bq::face_cell's floor
    if (s.ok()) s = m.bin(ctx->stream, bq::face_cell(2.0 * m.rho_mean, m.emax()));
    if (!s.ok()) { m.nf = 0; return bq::face_fail(ctx, "nwx_set_mesh", s, NWX_FACE_CODES); }
    return NWX_OK;
}

NWX_EXPORT int nwx_find(nwx_ctx *ctx, int flags, int32_t *count_out, int64_t *n_pairs_out, int64_t *n_crossed_faces_out)
{
    if (flags & ~(NWX_PAIRS | NWX_STATS)) return fail(ctx, NWX_ERR_BADARG, "nwx_find: an unknown flag");
    if (!ctx) return NWX_ERR_BADARG;
    ctx->has_pairs = false;
    ctx->n_pairs = 0;
    ctx->stats[0] = ctx->stats[1] = 0;
    if (ctx->m.nf < 1) return fail(ctx, NWX_ERR_NOMESH, "nwx_find: the context holds no mesh");
    NWX_HIP(hipSetDevice(ctx->device));
    const int nf = ctx->m.nf, nb = nblk(nf);
    NWX_HIP(ctx->count.ensure(sizeof(int) * (size_t)nf));
    NWX_HIP(ctx->up.ensure(sizeof(int) * (size_t)nf));
    NWX_HIP(ctx->tot.ensure(sizeof(long long) * 3));
    const bq::FaceGrid &fg = ctx->m;
    mx_mesh m;
    m.pos = fg.mpos.as<float>(); m.faces = fg.mfaces.as<int>(); m.nf = nf;
    m.pts = fg.sorted.as<bq::PtF64>(); m.cstart = fg.cstart.as<int>(); m.rho = fg.rho.as<double>();
    m.rho_max = fg.rho_max; m.lo0 = fg.g.lo[0]; m.lo1 = fg.g.lo[1]; m.lo2 = fg.g.lo[2]; m.h = fg.g.h;
    m.d0 = fg.g.dims[0]; m.d1 = fg.g.dims[1]; m.d2 = fg.g.dims[2];
    long long tot[3] = {0, 0, 0};                                 // pairs, (the sum of count[]), crossed faces
    if (flags & NWX_STATS) {
        long long st[3] = {0, 0, 0};                              // candidates read, candidates tested
        NWX_HIP(ctx->n_read.ensure(sizeof(int) * (size_t)nf));
        NWX_HIP(ctx->n_tested.ensure(sizeof(int) * (size_t)nf));
        hipLaunchKernelGGL(k_mx_stats, dim3(nb), dim3(NWX_BLOCK), 0, ctx->stream, m, ctx->n_read.as<int>(), ctx->n_tested.as<int>());
        hipLaunchKernelGGL(k_mx_totals, dim3(1), dim3(NWX_BLOCK), 0, ctx->stream, ctx->n_read.as<int>(), ctx->n_tested.as<int>(), nf, ctx->tot.as<long long>());
        NWX_HIP(hipGetLastError());
        NWX_HIP(hipMemcpyAsync(st, ctx->tot.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
        NWX_HIP(hipStreamSynchronize(ctx->stream));
        ctx->stats[0] = st[0];
        ctx->stats[1] = st[1];
    }
    hipLaunchKernelGGL(k_mx_count, dim3(nb), dim3(NWX_BLOCK), 0, ctx->stream, m, ctx->count.as<int>(), ctx->up.as<int>());
    hipLaunchKernelGGL(k_mx_totals, dim3(1), dim3(NWX_BLOCK), 0, ctx->stream, ctx->up.as<int>(), ctx->count.as<int>(), nf, ctx->tot.as<long long>());
    NWX_HIP(hipGetLastError());
    NWX_HIP(hipMemcpyAsync(tot, ctx->tot.p, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
    if (count_out) NWX_HIP(hipMemcpyAsync(count_out, ctx->count.p, sizeof(int) * (size_t)nf, hipMemcpyDeviceToHost, ctx->stream));
    NWX_HIP(hipStreamSynchronize(ctx->stream));
    if (tot[0] < 0 || tot[2] < 0 || tot[2] > nf || tot[1] != 2 * tot[0]) return fail(ctx, NWX_ERR_HIP, "nwx_find: the totals are out of range");
    ctx->n_pairs = tot[0];
    if (n_pairs_out) *n_pairs_out = tot[0];
    if (n_crossed_faces_out) *n_crossed_faces_out = tot[2];
    if (!(flags & NWX_PAIRS)) return NWX_OK;
    if (tot[0] > NWX_MAX_PAIRS) return fail(ctx, NWX_ERR_TOOMANY, "nwx_find: more pairs than NWX_MAX_PAIRS; the counts are delivered, the list is not made");
    if (tot[0] > 0) {
        int total = -1;
        NWX_HIP(ctx->start.ensure(sizeof(int) * ((size_t)nf + 1)));
        NWX_HIP(bq::scan_total(ctx->stream, ctx->up.as<int>(), nf, ctx->start.as<int>(), ctx->m.scan_tmp, &total));
        if (total != tot[0]) return fail(ctx, NWX_ERR_HIP, "nwx_find: the scan of the pair counts does not add up");
        NWX_HIP(ctx->pairs.ensure(sizeof(int) * 2 * (size_t)total));
        hipLaunchKernelGGL(k_mx_emit, dim3(nb), dim3(NWX_BLOCK), 0, ctx->stream, m, ctx->up.as<int>(), (const int *)ctx->start.as<int>(), ctx->pairs.as<int>());
        NWX_HIP(hipGetLastError());
        NWX_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->has_pairs = true;
    return NWX_OK;
}

NWX_EXPORT int nwx_get_pairs(nwx_ctx *ctx, int32_t *pairs_out, int64_t capacity)
{
    if (!ctx) return NWX_ERR_BADARG;
    if (!ctx->has_pairs) return fail(ctx, NWX_ERR_NOPAIRS, "nwx_get_pairs: the context holds no list (nwx_find with NWX_PAIRS makes one)");
    if (capacity < ctx->n_pairs || (ctx->n_pairs > 0 && !pairs_out)) return fail(ctx, NWX_ERR_BADARG, "nwx_get_pairs: the capacity is below the number of pairs");
    if (ctx->n_pairs == 0) return NWX_OK;
    NWX_HIP(hipSetDevice(ctx->device));
    std::vector<std::array<int32_t, 2>> list((size_t)ctx->n_pairs);
    NWX_HIP(hipMemcpyAsync(list.data(), ctx->pairs.p, sizeof(int32_t) * 2 * list.size(), hipMemcpyDeviceToHost, ctx->stream));
    NWX_HIP(hipStreamSynchronize(ctx->stream));
    std::sort(list.begin(), list.end());                          // (within a face the walk lists its partners in cell order)
    std::memcpy(pairs_out, list.data(), sizeof(int32_t) * 2 * list.size());
    return NWX_OK;
}

NWX_EXPORT int nwx_get_stats(nwx_ctx *ctx, int64_t out[2])
{
    if (!ctx || !out) return fail(ctx, NWX_ERR_BADARG, "nwx_get_stats: a NULL argument");
    out[0] = ctx->stats[0];
    out[1] = ctx->stats[1];
    return NWX_OK;
}
