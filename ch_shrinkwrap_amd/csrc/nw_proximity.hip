// The exact distance between two triangle meshes on the device (MI355X, gfx950): include/nw_proximity.h.
//
//   nwm_set_mesh    (bq::FaceGrid::set_faces)   the mesh query units' shared intake (nw_bq.h) for B: k_bq_face_setup, one thread per face,
//                                     the float64 centroid and rho, a hair enlarged; k_bq_rho_reduce, rho_max and the sum of rho, one
//                                     workgroup, a fixed order; bq::bounds, the centroids' box
//   nwm_query       (bq::FaceGrid::bin)   B's centroids binned at the cell size the band asks for, if the grid at hand has another
//                   (bq::face_setup)  k_bq_face_setup for A's faces
//                   k_mm_query        one lane per face of A: the capped ring walk of nw_proximity_core.h over B's centroid grid, the exact
//                                     triangle-triangle test on every face it cannot rule out, (d2, face) compared lexicographically so
//                                     that the order inside a cell never shows; d2, the partner and the block's counters
//                   k_mm_finish       one lane per face of A: the winning pair once more for its kind and closest points (the pair
//                                     function is pure: the same bits), or the out-of-band values
//                   k_mm_totals       the blocks' counters, one workgroup, a fixed order
//
// The scan, the point grid, the face grid, the device buffer with its staging and the context's scaffolding are the query units' shared
// ones (nw_bq.h).
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
    bq::FaceGrid m;               // mesh B of the last nwm_set_mesh and the grid at hand (m.nf == 0: the context holds no mesh)
    double cell_size = 0.0;       // the cell size nwm_set_mesh was given (0: the band's)
    // nwm_query: mesh A and its results
    DevBuf apos, afaces, acen, arho, d2, partner, dist, kind, ca, cb, partial, totals;
};

namespace {

#define NWM_HIP(call) BQ_HIP(call, NWM_ERR_NOMEM, NWM_ERR_HIP)

const bq::FaceCodes NWM_FACE_CODES = {NWM_ERR_BADARG, NWM_ERR_NONFINITE, NWM_ERR_NOMEM, NWM_ERR_HIP};

}  // namespace

NWM_EXPORT int nwm_abi_version(void) { return NWM_ABI_VERSION; }

NWM_EXPORT int nwm_create(int device, nwm_ctx **out) { return bq::create(device, out, NWM_ERR_BADARG, NWM_ERR_HIP); }

NWM_EXPORT void nwm_destroy(nwm_ctx *ctx) { bq::destroy(ctx); }

NWM_EXPORT const char *nwm_last_error(nwm_ctx *ctx) { return bq::last_error(ctx); }

NWM_EXPORT int nwm_set_mesh(nwm_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double cell_size)
{
    if (ctx) ctx->m.nf = 0;
    bq::FaceStatus s = bq::check_faces(pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwm_set_mesh", s, NWM_FACE_CODES);
    if (!(cell_size >= 0.0) || !std::isfinite(cell_size)) return fail(ctx, NWM_ERR_BADARG, "nwm_set_mesh: the cell size must be 0 or a positive finite double");
    if (!ctx) return NWM_ERR_BADARG;
    NWM_HIP(hipSetDevice(ctx->device));
    s = ctx->m.set_faces(ctx->stream, pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwm_set_mesh", s, NWM_FACE_CODES);
    ctx->cell_size = cell_size;
    return NWM_OK;
}

NWM_EXPORT int nwm_query(nwm_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, double d_cap, double *distance_out,
                         int32_t *partner_out, int32_t *kind_out, double *closest_a_out, double *closest_b_out, int64_t *info_out)
{
    bq::FaceStatus s = bq::check_faces(pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwm_query", s, NWM_FACE_CODES);
    if (!(d_cap > 0.0)) return fail(ctx, NWM_ERR_BADARG, "nwm_query: the band must be positive (+inf for none)");
    if (!ctx) return NWM_ERR_BADARG;
    if (ctx->m.nf < 1) return fail(ctx, NWM_ERR_NOMESH, "nwm_query: the context holds no mesh");
    NWM_HIP(hipSetDevice(ctx->device));
    bq::FaceGrid &m = ctx->m;
    // the grid for this band: at the cell size nwm_set_mesh was given, else from nwm_band_cell and bq::face_cell
    s = m.bin(ctx->stream, ctx->cell_size > 0.0 ? ctx->cell_size : bq::face_cell(nwm_band_cell(m.rho_mean, m.rho_max, d_cap), m.emax()));
    if (!s.ok()) return bq::face_fail(ctx, "nwm_query", s, NWM_FACE_CODES);
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
    for (int d = 0; d < 3; ++d) { g.lo[d] = m.g.lo[d]; g.hi[d] = m.g.hi[d]; g.dims[d] = m.g.dims[d]; }
    g.h = m.g.h;
    NWM_HIP(bq::face_setup(ctx->stream, ctx->apos.as<float>(), ctx->afaces.as<int>(), nfa, ctx->acen.as<double>(), ctx->arho.as<double>()));
    hipLaunchKernelGGL(k_mm_query, dim3(nb), dim3(NWM_BLOCK), 0, ctx->stream, ctx->apos.as<float>(), ctx->afaces.as<int>(), nfa, ctx->acen.as<double>(),
                       ctx->arho.as<double>(), m.mpos.as<float>(), m.mfaces.as<int>(), m.nf, m.sorted.as<nwm_pt>(), m.cstart.as<int>(),
                       m.rho.as<double>(), m.rho_max, g, d_cap, ctx->d2.as<double>(), ctx->partner.as<int>(), ctx->partial.as<long long>());
    hipLaunchKernelGGL(k_mm_finish, dim3(nb), dim3(NWM_BLOCK), 0, ctx->stream, ctx->apos.as<float>(), ctx->afaces.as<int>(), nfa, m.mpos.as<float>(),
                       m.mfaces.as<int>(), ctx->partner.as<int>(), ctx->dist.as<double>(), ctx->kind.as<int>(), ctx->ca.as<double>(), ctx->cb.as<double>());
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
        info_out[NWM_INFO_CELLS] = m.g.cells();
        int64_t bits;
        std::memcpy(&bits, &m.g.h, sizeof(bits));
        info_out[NWM_INFO_CELL_SIZE] = bits;
    }
    return NWM_OK;
}
