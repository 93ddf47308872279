// The exact distance between two triangle meshes on the device (MI355X, gfx950): include/nw_proximity.h.
//
//   nwm_set_mesh    k_mm_face_setup   one thread per face of B: the float64 centroid and rho (nw_distance_core.h), a hair enlarged
//                   k_mm_rho_reduce   rho_max and the sum of rho, one workgroup, a fixed order
//                   (bq::bounds)      the centroids' box
//   nwm_query       (bq::size_grid, bq::build_grid)   B's centroids binned at the cell size the band asks for, if the grid at hand has another
//                   k_mm_face_setup   the same for A's faces
//                   k_mm_query        one lane per face of A: the capped ring walk of nw_proximity_core.h over B's centroid grid, the exact
//                                     triangle-triangle test on every face it cannot rule out, (d2, face) compared lexicographically so
//                                     that the order inside a cell never shows; d2, the partner and the block's counters
//                   k_mm_finish       one lane per face of A: the winning pair once more for its kind and closest points (the pair
//                                     function is pure: the same bits), or the out-of-band values
//                   k_mm_totals       the blocks' counters, one workgroup, a fixed order
//
// The scan, the point grid, the device buffer with its staging and the context's scaffolding are the query units' shared ones (nw_bq.h).
// No kernel of this file uses atomics or scratch (build.py's KERNEL_BUDGETS checks the latter); all stores are vector stores; offsets
// are 64-bit.  The shared grid's counting sort does use an atomic cursor per cell, so the order of the centroids within a cell is not
// fixed from one binning to the next: no result depends on it, the count of exact tests does (include/nw_proximity.h).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <climits>
#include <cstring>
#include <string>
#include <algorithm>

#include "../../include/nw_proximity.h"
#include "nw_bq.h"
#include "nw_proximity_core.h"

#define NWM_EXPORT extern "C" __attribute__((visibility("default")))
#define NWM_BLOCK 256
#define NWM_PARTIALS 5            // per block: faces in band, faces at 0, rings, centroids read, exact tests

static_assert(sizeof(nwm_pt) == sizeof(bq::PtF64), "the walk reads the shared grid's sorted points in place");

// ---- set-up ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NWM_BLOCK) void k_mm_face_setup(const float *__restrict__ pos, const int *__restrict__ faces, int nf,
                                                             double *__restrict__ cen, double *__restrict__ rho)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
    double m[3];
    const double r = nwd_face_centroid(pos + 3 * (int64_t)a, pos + 3 * (int64_t)b, pos + 3 * (int64_t)c, m);
    cen[3 * (int64_t)f] = m[0];
    cen[3 * (int64_t)f + 1] = m[1];
    cen[3 * (int64_t)f + 2] = m[2];
    rho[f] = r * (1.0 + NWM_CORE_SLACK);
}

// out[0] = the largest rho, out[1] = their sum
__global__ __launch_bounds__(NWM_BLOCK) void k_mm_rho_reduce(const double *__restrict__ rho, int nf, double *__restrict__ out)
{
    __shared__ double s_m[NWM_BLOCK / 64], s_s[NWM_BLOCK / 64];
    double m = 0.0, s = 0.0;
    for (int j = threadIdx.x; j < nf; j += NWM_BLOCK) { m = fmax(m, rho[j]); s += rho[j]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmax(m, __shfl_xor(m, o, 64)); s += __shfl_xor(s, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_s[threadIdx.x >> 6] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
        out[1] = ((s_s[0] + s_s[1]) + s_s[2]) + s_s[3];
    }
}

// ---- the query --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NWM_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 8))) void k_mm_query(const float *__restrict__ apos, const int *__restrict__ afaces, int nfa, const double *__restrict__ acen,
                                                        const double *__restrict__ arho, const float *__restrict__ bpos, const int *__restrict__ bfaces,
                                                        int nfb, const nwm_pt *__restrict__ pts, const int *__restrict__ cstart,
                                                        const double *__restrict__ rho, double rho_max, nwm_grid g, double d_cap,
                                                        double *__restrict__ d2_out, int *__restrict__ partner_out, long long *__restrict__ partial)
{
    __shared__ long long s_w[NWM_BLOCK / 64][NWM_PARTIALS];
    const int f = blockIdx.x * NWM_BLOCK + threadIdx.x;
    long long in_band = 0, at_zero = 0, rings = 0, cens = 0, tests = 0;
    if (f < nfa) {
        const int ia = afaces[3 * (int64_t)f], ib = afaces[3 * (int64_t)f + 1], ic = afaces[3 * (int64_t)f + 2];
        const double cf[3] = {acen[3 * (int64_t)f], acen[3 * (int64_t)f + 1], acen[3 * (int64_t)f + 2]};
        nwm_best b;
        int n_cen = 0, n_tests = 0;
        rings = nwm_walk(cf, arho[f], apos + 3 * (int64_t)ia, apos + 3 * (int64_t)ib, apos + 3 * (int64_t)ic, bpos, bfaces, nfb, pts, cstart, rho,
                         rho_max, g, d_cap, b, n_cen, n_tests);
        const int partner = nwm_partner(b, d_cap);
        d2_out[f] = b.d2;
        partner_out[f] = partner;
        cens = n_cen; tests = n_tests;
        if (partner >= 0) { in_band = 1; at_zero = b.d2 == 0.0 ? 1 : 0; }
    }
    // the block's counters: a butterfly within each wave, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        in_band += __shfl_xor(in_band, o, 64);
        at_zero += __shfl_xor(at_zero, o, 64);
        rings += __shfl_xor(rings, o, 64);
        cens += __shfl_xor(cens, o, 64);
        tests += __shfl_xor(tests, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        long long *w = s_w[threadIdx.x >> 6];
        w[0] = in_band; w[1] = at_zero; w[2] = rings; w[3] = cens; w[4] = tests;
    }
    __syncthreads();
    if (threadIdx.x < NWM_PARTIALS) {
        const int c = threadIdx.x;
        partial[(int64_t)blockIdx.x * NWM_PARTIALS + c] = ((s_w[0][c] + s_w[1][c]) + s_w[2][c]) + s_w[3][c];
    }
}

__global__ __launch_bounds__(NWM_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 8))) void k_mm_finish(const float *__restrict__ apos, const int *__restrict__ afaces, int nfa, const float *__restrict__ bpos,
                                                         const int *__restrict__ bfaces, const int *__restrict__ partner, double *__restrict__ distance,
                                                         int *__restrict__ kind_out, double *__restrict__ closest_a, double *__restrict__ closest_b)
{
    const int f = blockIdx.x * NWM_BLOCK + threadIdx.x;
    if (f >= nfa) return;
    const int ia = afaces[3 * (int64_t)f], ib = afaces[3 * (int64_t)f + 1], ic = afaces[3 * (int64_t)f + 2];
    double d, ca[3], cb[3];
    int kind;
    nwm_finish(apos + 3 * (int64_t)ia, apos + 3 * (int64_t)ib, apos + 3 * (int64_t)ic, bpos, bfaces, partner[f], &d, &kind, ca, cb);
    distance[f] = d;
    kind_out[f] = kind;
    closest_a[3 * (int64_t)f] = ca[0]; closest_a[3 * (int64_t)f + 1] = ca[1]; closest_a[3 * (int64_t)f + 2] = ca[2];
    closest_b[3 * (int64_t)f] = cb[0]; closest_b[3 * (int64_t)f + 1] = cb[1]; closest_b[3 * (int64_t)f + 2] = cb[2];
}

// out[c] = the blocks' counters in a fixed order
__global__ __launch_bounds__(NWM_BLOCK) void k_mm_totals(const long long *__restrict__ partial, int64_t nb, long long *__restrict__ out)
{
    __shared__ long long s_w[NWM_BLOCK / 64][NWM_PARTIALS];
    long long v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0;
    for (int64_t b = threadIdx.x; b < nb; b += NWM_BLOCK) {
        v0 += partial[b * NWM_PARTIALS];
        v1 += partial[b * NWM_PARTIALS + 1];
        v2 += partial[b * NWM_PARTIALS + 2];
        v3 += partial[b * NWM_PARTIALS + 3];
        v4 += partial[b * NWM_PARTIALS + 4];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v0 += __shfl_xor(v0, o, 64);
        v1 += __shfl_xor(v1, o, 64);
        v2 += __shfl_xor(v2, o, 64);
        v3 += __shfl_xor(v3, o, 64);
        v4 += __shfl_xor(v4, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        long long *w = s_w[threadIdx.x >> 6];
        w[0] = v0; w[1] = v1; w[2] = v2; w[3] = v3; w[4] = v4;
    }
    __syncthreads();
    if (threadIdx.x < NWM_PARTIALS) {
        const int c = threadIdx.x;
        out[c] = ((s_w[0][c] + s_w[1][c]) + s_w[2][c]) + s_w[3][c];
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwm_ctx : bq::Ctx {
    // mesh B of the last nwm_set_mesh
    int nf = 0;                   // 0: the context holds no mesh
    double rho_max = 0.0, rho_mean = 0.0, cell_size = 0.0;
    bq::Grid<double> g{};         // lo, hi: the centroids' box; h, dims: the grid at hand
    double h_start = 0.0;         // the cell size the grid at hand was sized from (0: none)
    DevBuf mpos, mfaces, cen, rho, red, mm, cell, ccount, cstart, sorted, scan_tmp;
    // nwm_query: mesh A and its results
    DevBuf apos, afaces, acen, arho, d2, partner, dist, kind, ca, cb, partial, totals;
};

namespace {

#define NWM_HIP(call) BQ_HIP(call, NWM_ERR_NOMEM, NWM_ERR_HIP)

// at most max(16 F, 65536) cells, up to 2^26; at most 1025 an axis; 400 widening steps (nwd_'s rule)
const bq::GridRule NWM_GRID_RULE = {16, 1ll << 26, 1025, 400};

// the host checks of a mesh, A or B -> NWM_OK or the status, with its text
int check_mesh(nwm_ctx *ctx, const char *who, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces)
{
    if (!pos || !faces || n_vertices < 3 || n_faces < 1 || n_vertices > (1ll << 30) || n_faces > (1ll << 29)) return fail(ctx, NWM_ERR_BADARG, std::string(who) + ": a NULL array or a size out of range");
    if (!bq::all_finite(pos, 3 * n_vertices)) return fail(ctx, NWM_ERR_NONFINITE, std::string(who) + ": a vertex position is not finite");
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return fail(ctx, NWM_ERR_BADARG, std::string(who) + ": a face index outside the vertices");
    return NWM_OK;
}

// the cell size a band starts from: the one nwm_set_mesh was given, else max(2 m, min((d_cap + rho_max) / 2, 16 m)) with m the mean rho
// of B, and at least a 1024th of the widest axis; 1 for a mesh without extent.  2 m is a face or two per occupied cell of a surface;
// half of d_cap + rho_max ends a far face's walk after three or four rings; 16 m is where a walk without a band was fastest when it
// was measured (profiles/proximity.txt: its rings cost more than the centroids a larger cell makes it read), and it keeps a wide band
// from turning the grid into a few cells that hold every centroid
double starting_cell(const nwm_ctx *ctx, double d_cap)
{
    if (ctx->cell_size > 0.0) return ctx->cell_size;
    double emax = 0.0;
    for (int d = 0; d < 3; ++d) emax = std::max(emax, ctx->g.hi[d] - ctx->g.lo[d]);
    if (!(emax > 0.0)) return 1.0;
    double h = std::max(2.0 * ctx->rho_mean, std::min((d_cap + ctx->rho_max) / 2.0, 16.0 * ctx->rho_mean));
    h = std::max(h, emax / 1024.0);
    if (!(h > 0.0) || !std::isfinite(h)) h = emax;
    return h;
}

// the grid for this band: the one at hand if it was sized from the same starting cell, else the centroids binned anew
int ensure_grid(nwm_ctx *ctx, double d_cap)
{
    const double h0 = starting_cell(ctx, d_cap);
    if (ctx->h_start == h0) return NWM_OK;
    ctx->h_start = 0.0;
    double ext[3];
    for (int d = 0; d < 3; ++d) ext[d] = ctx->g.hi[d] - ctx->g.lo[d];
    ctx->g.h = h0;
    if (!bq::size_grid(NWM_GRID_RULE, ctx->nf, ext, &ctx->g.h, ctx->g.dims)) return fail(ctx, NWM_ERR_BADARG, "nwm_query: no cell size keeps the grid within its cap");
    int total = -1;
    NWM_HIP(bq::build_grid<double>(ctx->stream, ctx->cen.as<double>(), ctx->nf, ctx->g, ctx->cell, ctx->ccount, ctx->scan_tmp, ctx->cstart, ctx->sorted, &total));
    if (total != ctx->nf) return fail(ctx, NWM_ERR_HIP, "nwm_query: the cell counts do not add up to the faces");
    ctx->h_start = h0;
    return NWM_OK;
}

}  // namespace

NWM_EXPORT int nwm_abi_version(void) { return NWM_ABI_VERSION; }

NWM_EXPORT int nwm_create(int device, nwm_ctx **out) { return bq::create(device, out, NWM_ERR_BADARG, NWM_ERR_HIP); }

NWM_EXPORT void nwm_destroy(nwm_ctx *ctx) { bq::destroy(ctx); }

NWM_EXPORT const char *nwm_last_error(nwm_ctx *ctx) { return bq::last_error(ctx); }

NWM_EXPORT int nwm_set_mesh(nwm_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double cell_size)
{
    if (ctx) { ctx->nf = 0; ctx->h_start = 0.0; }
    const int ok = check_mesh(ctx, "nwm_set_mesh", pos, n_vertices, faces, n_faces);
    if (ok != NWM_OK) return ok;
    if (!(cell_size >= 0.0) || !std::isfinite(cell_size)) return fail(ctx, NWM_ERR_BADARG, "nwm_set_mesh: the cell size must be 0 or a positive finite double");
    if (!ctx) return NWM_ERR_BADARG;
    NWM_HIP(hipSetDevice(ctx->device));
    const int nf = (int)n_faces;
    NWM_HIP(bq::upload(ctx->stream, ctx->mpos, pos, 3 * n_vertices));
    NWM_HIP(bq::upload(ctx->stream, ctx->mfaces, faces, 3 * n_faces));
    NWM_HIP(ctx->cen.ensure(sizeof(double) * 3 * (size_t)nf));
    NWM_HIP(ctx->rho.ensure(sizeof(double) * (size_t)nf));
    NWM_HIP(ctx->red.ensure(sizeof(double) * 2));
    hipLaunchKernelGGL(k_mm_face_setup, dim3(nblk(nf)), dim3(NWM_BLOCK), 0, ctx->stream, ctx->mpos.as<float>(), ctx->mfaces.as<int>(), nf,
                       ctx->cen.as<double>(), ctx->rho.as<double>());
    hipLaunchKernelGGL(k_mm_rho_reduce, dim3(1), dim3(NWM_BLOCK), 0, ctx->stream, ctx->rho.as<double>(), nf, ctx->red.as<double>());
    NWM_HIP(hipGetLastError());
    double red[2] = {0.0, 0.0};
    NWM_HIP(hipMemcpyAsync(red, ctx->red.p, sizeof(red), hipMemcpyDeviceToHost, ctx->stream));
    NWM_HIP(hipStreamSynchronize(ctx->stream));                   // (red is a stack array, and the uploads' sources are the caller's)
    bool finite[2];
    NWM_HIP(bq::bounds<double>(ctx->stream, ctx->mm, ctx->cen.as<double>(), nf, nullptr, 0, &ctx->g, finite));
    if (!finite[0] || !std::isfinite(red[0]) || !std::isfinite(red[1])) return fail(ctx, NWM_ERR_NONFINITE, "nwm_set_mesh: a face's centroid or radius is not a finite double");
    double emax = 0.0;
    for (int d = 0; d < 3; ++d) emax = std::max(emax, ctx->g.hi[d] - ctx->g.lo[d]);
    if (!std::isfinite(emax)) return fail(ctx, NWM_ERR_BADARG, "nwm_set_mesh: the mesh's extent is not a finite double");
    ctx->rho_max = red[0];
    ctx->rho_mean = red[1] / (double)nf;
    ctx->cell_size = cell_size;
    ctx->nf = nf;
    return NWM_OK;
}

NWM_EXPORT int nwm_query(nwm_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double d_cap, double *distance_out,
                         int32_t *partner_out, int32_t *kind_out, double *closest_a_out, double *closest_b_out, int64_t *info_out)
{
    const int ok = check_mesh(ctx, "nwm_query", pos, n_vertices, faces, n_faces);
    if (ok != NWM_OK) return ok;
    if (!(d_cap > 0.0)) return fail(ctx, NWM_ERR_BADARG, "nwm_query: the band must be positive (+inf for none)");
    if (!ctx) return NWM_ERR_BADARG;
    if (ctx->nf < 1) return fail(ctx, NWM_ERR_NOMESH, "nwm_query: the context holds no mesh");
    NWM_HIP(hipSetDevice(ctx->device));
    const int r = ensure_grid(ctx, d_cap);
    if (r != NWM_OK) return r;
    const int nfa = (int)n_faces;
    const int nb = nblk(nfa, NWM_BLOCK);
    NWM_HIP(bq::upload(ctx->stream, ctx->apos, pos, 3 * n_vertices));
    NWM_HIP(bq::upload(ctx->stream, ctx->afaces, faces, 3 * n_faces));
    NWM_HIP(ctx->acen.ensure(sizeof(double) * 3 * (size_t)nfa));
    NWM_HIP(ctx->arho.ensure(sizeof(double) * (size_t)nfa));
    NWM_HIP(ctx->d2.ensure(sizeof(double) * (size_t)nfa));
    NWM_HIP(ctx->partner.ensure(sizeof(int) * (size_t)nfa));
    NWM_HIP(ctx->dist.ensure(sizeof(double) * (size_t)nfa));
    NWM_HIP(ctx->kind.ensure(sizeof(int) * (size_t)nfa));
    NWM_HIP(ctx->ca.ensure(sizeof(double) * 3 * (size_t)nfa));
    NWM_HIP(ctx->cb.ensure(sizeof(double) * 3 * (size_t)nfa));
    NWM_HIP(ctx->partial.ensure(sizeof(long long) * NWM_PARTIALS * (size_t)nb));
    NWM_HIP(ctx->totals.ensure(sizeof(long long) * NWM_PARTIALS));
    nwm_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = ctx->g.lo[d]; g.hi[d] = ctx->g.hi[d]; g.dims[d] = ctx->g.dims[d]; }
    g.h = ctx->g.h;
    hipLaunchKernelGGL(k_mm_face_setup, dim3(nb), dim3(NWM_BLOCK), 0, ctx->stream, ctx->apos.as<float>(), ctx->afaces.as<int>(), nfa,
                       ctx->acen.as<double>(), ctx->arho.as<double>());
    hipLaunchKernelGGL(k_mm_query, dim3(nb), dim3(NWM_BLOCK), 0, ctx->stream, ctx->apos.as<float>(), ctx->afaces.as<int>(), nfa, ctx->acen.as<double>(),
                       ctx->arho.as<double>(), ctx->mpos.as<float>(), ctx->mfaces.as<int>(), ctx->nf, ctx->sorted.as<nwm_pt>(), ctx->cstart.as<int>(),
                       ctx->rho.as<double>(), ctx->rho_max, g, d_cap, ctx->d2.as<double>(), ctx->partner.as<int>(), ctx->partial.as<long long>());
    hipLaunchKernelGGL(k_mm_finish, dim3(nb), dim3(NWM_BLOCK), 0, ctx->stream, ctx->apos.as<float>(), ctx->afaces.as<int>(), nfa, ctx->mpos.as<float>(),
                       ctx->mfaces.as<int>(), ctx->partner.as<int>(), ctx->dist.as<double>(), ctx->kind.as<int>(), ctx->ca.as<double>(), ctx->cb.as<double>());
    hipLaunchKernelGGL(k_mm_totals, dim3(1), dim3(NWM_BLOCK), 0, ctx->stream, ctx->partial.as<long long>(), (int64_t)nb, ctx->totals.as<long long>());
    NWM_HIP(hipGetLastError());
    long long tot[NWM_PARTIALS] = {0, 0, 0, 0, 0};
    NWM_HIP(hipMemcpyAsync(tot, ctx->totals.p, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
    if (distance_out) NWM_HIP(hipMemcpyAsync(distance_out, ctx->dist.p, sizeof(double) * (size_t)nfa, hipMemcpyDeviceToHost, ctx->stream));
    if (partner_out) NWM_HIP(hipMemcpyAsync(partner_out, ctx->partner.p, sizeof(int) * (size_t)nfa, hipMemcpyDeviceToHost, ctx->stream));
    if (kind_out) NWM_HIP(hipMemcpyAsync(kind_out, ctx->kind.p, sizeof(int) * (size_t)nfa, hipMemcpyDeviceToHost, ctx->stream));
    if (closest_a_out) NWM_HIP(hipMemcpyAsync(closest_a_out, ctx->ca.p, sizeof(double) * 3 * (size_t)nfa, hipMemcpyDeviceToHost, ctx->stream));
    if (closest_b_out) NWM_HIP(hipMemcpyAsync(closest_b_out, ctx->cb.p, sizeof(double) * 3 * (size_t)nfa, hipMemcpyDeviceToHost, ctx->stream));
    NWM_HIP(hipStreamSynchronize(ctx->stream));                   // (tot is a stack array, and the uploads' sources are the caller's)
    if (info_out) {
        for (int c = 0; c < NWM_PARTIALS; ++c) info_out[c] = tot[c];
        info_out[NWM_INFO_CELLS] = ctx->g.cells();
        int64_t bits;
        std::memcpy(&bits, &ctx->g.h, sizeof(bits));
        info_out[NWM_INFO_CELL_SIZE] = bits;
    }
    return NWM_OK;
}
