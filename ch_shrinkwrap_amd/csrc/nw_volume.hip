// The banded exact signed-distance volume of a triangle mesh on the device (MI355X, gfx950): include/nw_volume.h.
//
//   nwv_set_mesh    (bq::FaceGrid::set_faces)   the mesh query units' shared intake (nw_bq.h): k_bq_face_setup, one thread per face, the
//                                     float64 centroid and rho_f, a hair enlarged; k_bq_rho_reduce, rho_max and the sum of rho_f, one
//                                     workgroup, a fixed order; bq::bounds, the centroids' box
//   nwv_volume      (bq::FaceGrid::bin)   the centroids binned at the cell size the band asks for, if the grid at hand has another
//                   k_vx_nodes        one lane per node: its own position from (lo, h, index), the capped ring walk of nw_volume_core.h,
//                                     the band rule and, in band, the pseudonormal's sign; sd, face, and the block's counters
//                   k_vx_seed         one workgroup over all faces for node (0, 0, 0): the (d2, face) lexicographic minimum, its
//                                     pseudonormal, and the seed's sign if the seed is out of band
//                   k_vx_sweep        the sign sweep, launched three times: the z-line of (0, 0, .), the y-lines of (0, ., k), the
//                                     x-rows.  One wave per line, 64 nodes at a time: an out-of-band node takes the sign of the nearest
//                                     in-band node before it in the chunk (two ballots), or the sign carried in from the chunk before
//                   k_vx_finish       field and mask from sd
//                   k_vx_totals       the blocks' counters, one workgroup, a fixed order
//
// No kernel uses atomics or scratch (build.py's KERNEL_BUDGETS checks the latter); all stores are vector stores; node indices are 64-bit.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <climits>
#include <string>
#include <algorithm>

#include "../../include/nw_volume.h"
#include "nw_bq.h"
#include "nw_volume_core.h"

#define NWV_EXPORT extern "C" __attribute__((visibility("default")))
#define NWV_BLOCK 256
#define NWV_PARTIALS 6            // per block: flag word, in-band nodes, rings near, centroids near, rings far, centroids far

static_assert(sizeof(nwv_pt) == sizeof(bq::PtF64), "the walk reads the shared grid's sorted points in place");

// ---- the nodes ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NWV_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_vx_nodes(float lo0, float lo1, float lo2, float hv, int nx, int ny, int64_t nvox,
                                                        const float *__restrict__ pos, const int *__restrict__ faces, const int *__restrict__ twin, int nf,
                                                        const nwv_pt *__restrict__ pts, const int *__restrict__ cstart, const double *__restrict__ rho,
                                                        double rho_max, nwv_grid g, double d_cap, double *__restrict__ sd, int *__restrict__ face_out,
                                                        long long *__restrict__ partial)
{
    __shared__ long long s_w[NWV_BLOCK / 64][NWV_PARTIALS];
    const int64_t idx = (int64_t)blockIdx.x * NWV_BLOCK + threadIdx.x;
    long long flag = 0, in_band = 0, rings_near = 0, cen_near = 0, rings_far = 0, cen_far = 0;
    if (idx < nvox) {
        const int64_t i = idx % nx, j = (idx / nx) % ny, k = idx / ((int64_t)nx * ny);
        const double q[3] = {nwv_node_coord(lo0, hv, i), nwv_node_coord(lo1, hv, j), nwv_node_coord(lo2, hv, k)};
        nwv_best b;
        int n_cen = 0, capped = 0, face;
        const int rings = nwv_walk(q, pos, faces, nf, pts, cstart, rho, rho_max, g, d_cap, b, n_cen);
        sd[idx] = nwv_node_value(q, b, d_cap, pos, faces, twin, &face, &capped);
        face_out[idx] = face;
        flag = capped ? NWV_FLAG_FAN_CAPPED : 0;
        if (face >= 0) { in_band = 1; rings_near = rings; cen_near = n_cen; }
        else { rings_far = rings; cen_far = n_cen; }
    }
    // the block's counters: a butterfly within each wave, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        flag |= __shfl_xor(flag, o, 64);
        in_band += __shfl_xor(in_band, o, 64);
        rings_near += __shfl_xor(rings_near, o, 64);
        cen_near += __shfl_xor(cen_near, o, 64);
        rings_far += __shfl_xor(rings_far, o, 64);
        cen_far += __shfl_xor(cen_far, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        long long *w = s_w[threadIdx.x >> 6];
        w[0] = flag; w[1] = in_band; w[2] = rings_near; w[3] = cen_near; w[4] = rings_far; w[5] = cen_far;
    }
    __syncthreads();
    if (threadIdx.x < NWV_PARTIALS) {
        const int c = threadIdx.x;
        partial[(int64_t)blockIdx.x * NWV_PARTIALS + c] = c == 0 ? (s_w[0][0] | s_w[1][0] | s_w[2][0] | s_w[3][0])
                                                                 : ((s_w[0][c] + s_w[1][c]) + s_w[2][c]) + s_w[3][c];
    }
}

// the seed (0, 0, 0) against all faces, no cap: seed_out[0] = its face; if the seed is out of band, sd[0] takes the exact sign
__global__ __launch_bounds__(NWV_BLOCK) void k_vx_seed(float lo0, float lo1, float lo2, float hv, const float *__restrict__ pos, const int *__restrict__ faces,
                                                       const int *__restrict__ twin, int nf, double d_cap, double *__restrict__ sd,
                                                       const int *__restrict__ face_out, long long *__restrict__ seed_out)
{
    __shared__ double s_d2[NWV_BLOCK / 64];
    __shared__ int s_f[NWV_BLOCK / 64];
    const double q[3] = {nwv_node_coord(lo0, hv, 0), nwv_node_coord(lo1, hv, 0), nwv_node_coord(lo2, hv, 0)};
    double best = INFINITY;
    int bf = INT_MAX;
    for (int f = threadIdx.x; f < nf; f += NWV_BLOCK) {
        const int ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
        double c[3];
        int feature;
        const double d2 = nwd_point_triangle(q, pos + 3 * (int64_t)ia, pos + 3 * (int64_t)ib, pos + 3 * (int64_t)ic, c, &feature);
        if (d2 < best) { best = d2; bf = f; }                      // (a lane's faces come in ascending order: the first of equals stays)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(best, o, 64);
        const int of = __shfl_xor(bf, o, 64);
        if (od < best || (od == best && of < bf)) { best = od; bf = of; }
    }
    if ((threadIdx.x & 63) == 0) { s_d2[threadIdx.x >> 6] = best; s_f[threadIdx.x >> 6] = bf; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < NWV_BLOCK / 64; ++w)
        if (s_d2[w] < best || (s_d2[w] == best && s_f[w] < bf)) { best = s_d2[w]; bf = s_f[w]; }
    seed_out[0] = bf == INT_MAX ? -1 : bf;
    if (bf == INT_MAX || face_out[0] != -1) return;                // in band: the node's own walk has given it its sign
    const int ia = faces[3 * (int64_t)bf], ib = faces[3 * (int64_t)bf + 1], ic = faces[3 * (int64_t)bf + 2];
    double c[3], N[3];
    int feature;
    const double d2 = nwd_point_triangle(q, pos + 3 * (int64_t)ia, pos + 3 * (int64_t)ib, pos + 3 * (int64_t)ic, c, &feature);
    nwd_pseudonormal(pos, faces, twin, bf, feature, N);
    sd[0] = nwv_out_of_band(d_cap, (d2 > 0.0 && nwd_sign(q, c, N) < 0.0) ? -1.0 : 1.0);
}

// One stage of the sign sweep: n_lines lines of n nodes, line L = the nodes L * pitch + t * stride, t = 0 .. n-1, whose node 0 is
// resolved.  Along a line the predecessor of node t is node t - 1 (nwv_predecessor; nwv_sweep_stage names the lines).  One wave per line.
__global__ __launch_bounds__(NWV_BLOCK) void k_vx_sweep(int64_t n_lines, int64_t pitch, int64_t n, int64_t stride, double d_cap,
                                                        double *__restrict__ sd, const int *__restrict__ face)
{
    const int lane = threadIdx.x & 63;
    const int64_t line = ((int64_t)blockIdx.x * NWV_BLOCK + threadIdx.x) >> 6;
    if (line >= n_lines) return;                                   // (a whole wave)
    const int64_t base = line * pitch;
    bool carry_neg = sd[base] < 0.0;
    for (int64_t t0 = 1; t0 < n; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool valid = t < n;
        const int64_t idx = base + (valid ? t : 0) * stride;
        const bool in_band = valid && face[idx] != -1;
        const bool neg = in_band && sd[idx] < 0.0;
        const unsigned long long m = __ballot(in_band), s = __ballot(neg);
        if (valid && !in_band) {
            const unsigned long long below = m & ((1ull << lane) - 1ull);
            const bool mine = below ? ((s >> (63 - __clzll((long long)below))) & 1ull) != 0ull : carry_neg;
            sd[idx] = nwv_out_of_band(d_cap, mine ? -1.0 : 1.0);
        }
        if (m) carry_neg = ((s >> (63 - __clzll((long long)m))) & 1ull) != 0ull;       // the sign of the chunk's last node
    }
}

__global__ __launch_bounds__(NWV_BLOCK) void k_vx_finish(const double *__restrict__ sd, int64_t nvox, double d_cap, unsigned long long *__restrict__ field,
                                                         unsigned char *__restrict__ mask)
{
    const int64_t idx = (int64_t)blockIdx.x * NWV_BLOCK + threadIdx.x;
    if (idx >= nvox) return;
    const double v = sd[idx];
    field[idx] = nwv_quantise(v, d_cap);
    mask[idx] = v < 0.0 ? 1 : 0;
}

// out[c] = the blocks' counters in a fixed order (c = 0: or-ed)
__global__ __launch_bounds__(NWV_BLOCK) void k_vx_totals(const long long *__restrict__ partial, int64_t nb, long long *__restrict__ out)
{
    __shared__ long long s_w[NWV_BLOCK / 64][NWV_PARTIALS];
    long long v[NWV_PARTIALS] = {0, 0, 0, 0, 0, 0};
    for (int64_t b = threadIdx.x; b < nb; b += NWV_BLOCK) {
        v[0] |= partial[b * NWV_PARTIALS];
#pragma unroll
        for (int c = 1; c < NWV_PARTIALS; ++c) v[c] += partial[b * NWV_PARTIALS + c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v[0] |= __shfl_xor(v[0], o, 64);
#pragma unroll
        for (int c = 1; c < NWV_PARTIALS; ++c) v[c] += __shfl_xor(v[c], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NWV_PARTIALS; ++c) s_w[threadIdx.x >> 6][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < NWV_PARTIALS) {
        const int c = threadIdx.x;
        out[c] = c == 0 ? (s_w[0][0] | s_w[1][0] | s_w[2][0] | s_w[3][0]) : ((s_w[0][c] + s_w[1][c]) + s_w[2][c]) + s_w[3][c];
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwv_ctx : bq::Ctx {
    bq::FaceGrid m;               // the mesh of the last nwv_set_mesh and the grid at hand (m.nf == 0: the context holds no mesh)
    bool has_twin = false;
    DevBuf mtwin;
    // nwv_volume
    DevBuf sd, face, field, mask, partial, totals;
    int64_t n_field = 0;
};

namespace {

#define NWV_HIP(call) BQ_HIP(call, NWV_ERR_NOMEM, NWV_ERR_HIP)

const bq::FaceCodes NWV_FACE_CODES = {NWV_ERR_BADARG, NWV_ERR_NONFINITE, NWV_ERR_NOMEM, NWV_ERR_HIP};
const int NWV_MAX_DIM = 1 << 20;
const double NWV_MAX_CAP = 1099511627776.0;           // 2^40

}  // namespace

NWV_EXPORT int nwv_abi_version(void) { return NWV_ABI_VERSION; }

NWV_EXPORT int nwv_create(int device, nwv_ctx **out) { return bq::create(device, out, NWV_ERR_BADARG, NWV_ERR_HIP); }

NWV_EXPORT void nwv_destroy(nwv_ctx *ctx) { bq::destroy(ctx); }

NWV_EXPORT const char *nwv_last_error(nwv_ctx *ctx) { return bq::last_error(ctx); }

NWV_EXPORT int nwv_set_mesh(nwv_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin)
{
    if (ctx) { ctx->m.nf = 0; ctx->n_field = 0; }
    bq::FaceStatus s = bq::check_faces(pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwv_set_mesh", s, NWV_FACE_CODES);
    if (twin && !bq::twin_ok(twin, n_faces)) return fail(ctx, NWV_ERR_BADARG, "nwv_set_mesh: the twin table is not -1 or an involution within [0, 3F)");
    if (!ctx) return NWV_ERR_BADARG;
    NWV_HIP(hipSetDevice(ctx->device));
    if (twin) NWV_HIP(bq::upload(ctx->stream, ctx->mtwin, twin, 3 * n_faces));
    s = ctx->m.set_faces(ctx->stream, pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwv_set_mesh", s, NWV_FACE_CODES);
    ctx->has_twin = twin != nullptr;
    return NWV_OK;
}

NWV_EXPORT int nwv_volume(nwv_ctx *ctx, const float *lo, float h, const int32_t *dims, double d_cap, int flags, double *sd_host, int32_t *face_host,
                          uint8_t *mask_host, int64_t *info_out)
{
    if (ctx) ctx->n_field = 0;
    if (!lo || !dims || !(h > 0.0f) || !std::isfinite(h) || (flags & ~NWV_SIGNED)) return fail(ctx, NWV_ERR_BADARG, "nwv_volume: a NULL lattice, a voxel size that is not positive and finite, or an unknown flag");
    if (!std::isfinite(d_cap) || !(d_cap >= (double)h) || !(d_cap <= NWV_MAX_CAP)) return fail(ctx, NWV_ERR_BADARG, "nwv_volume: the band must be finite and within [h, 2^40]");
    int64_t nvox = 1;
    for (int d = 0; d < 3; ++d) {
        if (!std::isfinite(lo[d]) || dims[d] < 3 || dims[d] > NWV_MAX_DIM) return fail(ctx, NWV_ERR_BADARG, "nwv_volume: a lattice origin that is not finite or a dimension outside [3, 2^20]");
        nvox *= dims[d];
    }
    if (nvox > (1ll << 30)) return fail(ctx, NWV_ERR_BADARG, "nwv_volume: more than 2^30 nodes");
    if (!ctx) return NWV_ERR_BADARG;
    if (ctx->m.nf < 1) return fail(ctx, NWV_ERR_NOMESH, "nwv_volume: the context holds no mesh");
    const bool is_signed = (flags & NWV_SIGNED) != 0;
    if (is_signed && !ctx->has_twin) return fail(ctx, NWV_ERR_BADARG, "nwv_volume: NWV_SIGNED needs the twin table that nwv_set_mesh was not given");
    NWV_HIP(hipSetDevice(ctx->device));
    bq::FaceGrid &m = ctx->m;
    // the grid for this band, from the cell size bq::band_cell and bq::face_cell give
    const bq::FaceStatus s = m.bin(ctx->stream, bq::face_cell(bq::band_cell(m.rho_mean, m.rho_max, d_cap), m.emax()));
    if (!s.ok()) return bq::face_fail(ctx, "nwv_volume", s, NWV_FACE_CODES);
    const int nb = nblk(nvox, NWV_BLOCK);
    const int nx = dims[0], ny = dims[1], nz = dims[2];
    NWV_HIP(ctx->sd.ensure(sizeof(double) * (size_t)nvox));
    NWV_HIP(ctx->face.ensure(sizeof(int) * (size_t)nvox));
    NWV_HIP(ctx->field.ensure(sizeof(uint64_t) * (size_t)nvox));
    NWV_HIP(ctx->mask.ensure((size_t)nvox));
    NWV_HIP(ctx->partial.ensure(sizeof(long long) * NWV_PARTIALS * (size_t)nb));
    NWV_HIP(ctx->totals.ensure(sizeof(long long) * (NWV_PARTIALS + 1)));
    nwv_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = m.g.lo[d]; g.hi[d] = m.g.hi[d]; g.dims[d] = m.g.dims[d]; }
    g.h = m.g.h;
    const int *twin = is_signed ? ctx->mtwin.as<int>() : nullptr;
    double *sd = ctx->sd.as<double>();
    int *face = ctx->face.as<int>();
    long long *totals = ctx->totals.as<long long>();
    hipLaunchKernelGGL(k_vx_nodes, dim3(nb), dim3(NWV_BLOCK), 0, ctx->stream, lo[0], lo[1], lo[2], h, nx, ny, nvox, m.mpos.as<float>(), m.mfaces.as<int>(),
                       twin, m.nf, m.sorted.as<nwv_pt>(), m.cstart.as<int>(), m.rho.as<double>(), m.rho_max, g, d_cap, sd, face,
                       ctx->partial.as<long long>());
    if (is_signed) {
        hipLaunchKernelGGL(k_vx_seed, dim3(1), dim3(NWV_BLOCK), 0, ctx->stream, lo[0], lo[1], lo[2], h, m.mpos.as<float>(), m.mfaces.as<int>(), twin,
                           m.nf, d_cap, sd, face, totals + NWV_PARTIALS);
        for (int stage = 0; stage < 3; ++stage) {
            int64_t n_lines, pitch, n, stride;
            nwv_sweep_stage(stage, nx, ny, nz, &n_lines, &pitch, &n, &stride);
            hipLaunchKernelGGL(k_vx_sweep, dim3(nblk(64 * n_lines, NWV_BLOCK)), dim3(NWV_BLOCK), 0, ctx->stream, n_lines, pitch, n, stride, d_cap, sd, face);
        }
    }
    hipLaunchKernelGGL(k_vx_finish, dim3(nb), dim3(NWV_BLOCK), 0, ctx->stream, sd, nvox, d_cap, ctx->field.as<unsigned long long>(), ctx->mask.as<unsigned char>());
    hipLaunchKernelGGL(k_vx_totals, dim3(1), dim3(NWV_BLOCK), 0, ctx->stream, ctx->partial.as<long long>(), (int64_t)nb, totals);
    NWV_HIP(hipGetLastError());
    long long tot[NWV_PARTIALS + 1] = {0, 0, 0, 0, 0, 0, -1};
    NWV_HIP(hipMemcpyAsync(tot, totals, sizeof(long long) * (is_signed ? NWV_PARTIALS + 1 : NWV_PARTIALS), hipMemcpyDeviceToHost, ctx->stream));
    if (sd_host) NWV_HIP(hipMemcpyAsync(sd_host, sd, sizeof(double) * (size_t)nvox, hipMemcpyDeviceToHost, ctx->stream));
    if (face_host) NWV_HIP(hipMemcpyAsync(face_host, face, sizeof(int) * (size_t)nvox, hipMemcpyDeviceToHost, ctx->stream));
    if (mask_host) NWV_HIP(hipMemcpyAsync(mask_host, ctx->mask.p, (size_t)nvox, hipMemcpyDeviceToHost, ctx->stream));
    NWV_HIP(hipStreamSynchronize(ctx->stream));
    if (info_out) {
        for (int c = 0; c < NWV_PARTIALS; ++c) info_out[c] = tot[c];
        info_out[NWV_INFO_CELLS] = m.g.cells();
        info_out[NWV_INFO_SEED_FACE] = tot[NWV_PARTIALS];
    }
    ctx->n_field = nvox;
    return NWV_OK;
}

NWV_EXPORT const uint64_t *nwv_field_ptr(nwv_ctx *ctx) { return (ctx && ctx->n_field > 0) ? ctx->field.as<uint64_t>() : nullptr; }

NWV_EXPORT int nwv_get_field(nwv_ctx *ctx, uint64_t *field_host)
{
    if (!field_host) return fail(ctx, NWV_ERR_BADARG, "nwv_get_field: a NULL array");
    if (!ctx) return NWV_ERR_BADARG;
    if (ctx->n_field < 1) return fail(ctx, NWV_ERR_NOMESH, "nwv_get_field: nwv_volume first");
    NWV_HIP(hipSetDevice(ctx->device));
    NWV_HIP(hipMemcpyAsync(field_host, ctx->field.p, sizeof(uint64_t) * (size_t)ctx->n_field, hipMemcpyDeviceToHost, ctx->stream));
    NWV_HIP(hipStreamSynchronize(ctx->stream));
    return NWV_OK;
}
