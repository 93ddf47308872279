// Localizations mapped onto a triangle mesh on the device (MI355X, gfx950): include/nw_mapping.h.
//
//   nwl_set_mesh    (bq::FaceGrid::set_faces)   the mesh query units' shared intake (nw_bq.h), with this unit's kernel in place of
//                                     k_bq_face_setup:
//                   k_lm_face_setup   one thread per face: the float64 centroid and rho_f (bq::face_centroid), a hair enlarged, and
//                                     floor(A_f 2^20) added to area3 of its three corners (64-bit integer atomics)
//                   (k_bq_rho_reduce, bq::bounds)   rho_max and the sum of rho_f, one workgroup, a fixed order; the centroids' box
//   nwl_map         (bq::FaceGrid::bin)   the centroids binned at the cell size the band asks for, if the grid at hand has another
//                   k_lm_map          one lane per localization: the capped ring walk of nw_volume_core.h, the band rule and the weights
//                                     of nw_mapping_core.h; face, weights, distance, closest point; in band the integer atomics on
//                                     mass, count and the two limbs of every value column; the block's counters
//                   k_lm_totals       the blocks' counters, one workgroup, a fixed order
//
// Every accumulator is an integer and every add an integer atomic whose result is not read: the sums do not depend on the order the
// adds arrive in.  No kernel uses scratch (build.py's KERNEL_BUDGETS checks it); all stores are vector stores; offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <climits>
#include <string>
#include <algorithm>

#include "../../include/nw_mapping.h"
#include "nw_bq.h"
#include "nw_mapping_core.h"

#define NWL_EXPORT extern "C" __attribute__((visibility("default")))
#define NWL_BLOCK 256
#define NWL_PARTIALS 3            // per block: in-band localizations, rings, centroids
#define NWL_FLAG_WORDS 3          // raised by plain stores: a face beyond the area limit, a non-finite value, a value beyond its scale

static_assert(sizeof(nwv_pt) == sizeof(bq::PtF64), "the walk reads the shared grid's sorted points in place");
static_assert(NWL_MAX_COLUMNS == NWL_MAX_VALUE_COLUMNS, "the header's and the core's column limits");

typedef unsigned long long u64;

// ---- set-up ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NWL_BLOCK) void k_lm_face_setup(const float *__restrict__ pos, const int *__restrict__ faces, int nf,
                                                             double *__restrict__ cen, double *__restrict__ rho, u64 *__restrict__ area3,
                                                             int *__restrict__ flag)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
    const float *pa = pos + 3 * (int64_t)a, *pb = pos + 3 * (int64_t)b, *pc = pos + 3 * (int64_t)c;
    double m[3];
    const double r = nwd_face_centroid(pa, pb, pc, m);             // (bq::face_centroid, the face grid's)
    cen[3 * (int64_t)f] = m[0];
    cen[3 * (int64_t)f + 1] = m[1];
    cen[3 * (int64_t)f + 2] = m[2];
    rho[f] = r * (1.0 + BQ_FACE_RHO_SLACK);
    uint64_t aq;
    if (!nwl_face_area(pa, pb, pc, &aq)) { flag[0] = 1; return; }
    if (aq) {
        atomicAdd(area3 + a, (u64)aq);
        atomicAdd(area3 + b, (u64)aq);
        atomicAdd(area3 + c, (u64)aq);
    }
}

// ---- the localizations ------------------------------------------------------------------------------------------------------------------
// mass == nullptr: no accumulator is touched (NWL_WALK_ONLY)
__global__ __launch_bounds__(NWL_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_lm_map(
    const double *__restrict__ xyz, int64_t n, const double *__restrict__ values, int n_col, const double *__restrict__ scales,
    const float *__restrict__ pos, const int *__restrict__ faces, int nf, const nwv_pt *__restrict__ pts, const int *__restrict__ cstart,
    const double *__restrict__ rho, double rho_max, nwv_grid g, double d_cap, int *__restrict__ face_out, int *__restrict__ w_out,
    double *__restrict__ dist_out, double *__restrict__ closest_out, u64 *__restrict__ mass, int *__restrict__ count, u64 *__restrict__ sum_hi,
    u64 *__restrict__ sum_lo, int *__restrict__ flag, long long *__restrict__ partial)
{
    __shared__ long long s_w[NWL_BLOCK / 64][NWL_PARTIALS];
    const int64_t i = (int64_t)blockIdx.x * NWL_BLOCK + threadIdx.x;
    long long in_band = 0, rings = 0, n_cen = 0;
    if (i < n) {
        const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        nwl_hit h;
        int cen = 0;
        rings = nwl_locate(p, pos, faces, nf, pts, cstart, rho, rho_max, g, d_cap, h, cen);
        n_cen = cen;
        if (face_out) face_out[i] = h.face;
        if (w_out) { w_out[3 * i] = h.w[0]; w_out[3 * i + 1] = h.w[1]; w_out[3 * i + 2] = h.w[2]; }
        if (dist_out) dist_out[i] = h.d;
        if (closest_out) { closest_out[3 * i] = h.c[0]; closest_out[3 * i + 1] = h.c[1]; closest_out[3 * i + 2] = h.c[2]; }
        if (h.face >= 0) {
            in_band = 1;
            if (mass) {
                const int64_t va = faces[3 * (int64_t)h.face], vb = faces[3 * (int64_t)h.face + 1], vc = faces[3 * (int64_t)h.face + 2];
                // (a weight of 0 adds nothing anywhere: its atomics are left out)
                if (h.w[0]) atomicAdd(mass + va, (u64)h.w[0]);
                if (h.w[1]) atomicAdd(mass + vb, (u64)h.w[1]);
                if (h.w[2]) atomicAdd(mass + vc, (u64)h.w[2]);
                atomicAdd(count + h.face, 1);
                for (int c = 0; c < n_col; ++c) {
                    int64_t q;
                    const int bad = nwl_quantise(values[i * n_col + c], scales[c], &q);
                    if (bad) { flag[bad] = 1; continue; }
                    if (q == 0) continue;
                    uint64_t lo;
                    int64_t hi;
                    if (h.w[0]) {
                        nwl_limbs((int64_t)h.w[0] * q, &lo, &hi);
                        if (lo) atomicAdd(sum_lo + va * n_col + c, (u64)lo);
                        if (hi) atomicAdd(sum_hi + va * n_col + c, (u64)hi);
                    }
                    if (h.w[1]) {
                        nwl_limbs((int64_t)h.w[1] * q, &lo, &hi);
                        if (lo) atomicAdd(sum_lo + vb * n_col + c, (u64)lo);
                        if (hi) atomicAdd(sum_hi + vb * n_col + c, (u64)hi);
                    }
                    if (h.w[2]) {
                        nwl_limbs((int64_t)h.w[2] * q, &lo, &hi);
                        if (lo) atomicAdd(sum_lo + vc * n_col + c, (u64)lo);
                        if (hi) atomicAdd(sum_hi + vc * n_col + c, (u64)hi);
                    }
                }
            }
        }
    }
    // the block's counters: a butterfly within each wave, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        in_band += __shfl_xor(in_band, o, 64);
        rings += __shfl_xor(rings, o, 64);
        n_cen += __shfl_xor(n_cen, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        long long *w = s_w[threadIdx.x >> 6];
        w[0] = in_band; w[1] = rings; w[2] = n_cen;
    }
    __syncthreads();
    if (threadIdx.x < NWL_PARTIALS) {
        const int c = threadIdx.x;
        partial[(int64_t)blockIdx.x * NWL_PARTIALS + c] = ((s_w[0][c] + s_w[1][c]) + s_w[2][c]) + s_w[3][c];
    }
}

// out[c] = the blocks' counters in a fixed order
__global__ __launch_bounds__(NWL_BLOCK) void k_lm_totals(const long long *__restrict__ partial, int64_t nb, long long *__restrict__ out)
{
    __shared__ long long s_w[NWL_BLOCK / 64][NWL_PARTIALS];
    long long v[NWL_PARTIALS] = {0, 0, 0};
    for (int64_t b = threadIdx.x; b < nb; b += NWL_BLOCK) {
#pragma unroll
        for (int c = 0; c < NWL_PARTIALS; ++c) v[c] += partial[b * NWL_PARTIALS + c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < NWL_PARTIALS; ++c) v[c] += __shfl_xor(v[c], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NWL_PARTIALS; ++c) s_w[threadIdx.x >> 6][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < NWL_PARTIALS) {
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

struct nwl_ctx : bq::Ctx {
    bq::FaceGrid m;               // the mesh of the last nwl_set_mesh and the grid at hand (m.nf == 0: the context holds no mesh)
    DevBuf area3, flag;
    int flag_h[NWL_FLAG_WORDS] = {0, 0, 0};      // (in the context: nwl_set_mesh's copy into it is queued inside bq::FaceGrid::set_faces)
    // nwl_map
    DevBuf up, upv, scales, qmm, face, w, dist, closest, mass, count, sum_hi, sum_lo, partial, totals;
    int acc_columns = -1;         // the columns of the accumulators at hand (-1: none to add onto)
    int64_t acc_n = 0;            // the localizations they have seen
};

namespace {

#define NWL_HIP(call) BQ_HIP(call, NWL_ERR_NOMEM, NWL_ERR_HIP)

const bq::FaceCodes NWL_FACE_CODES = {NWL_ERR_BADARG, NWL_ERR_NONFINITE, NWL_ERR_NOMEM, NWL_ERR_HIP};
const double NWL_MAX_CAP = 1099511627776.0;           // 2^40
const int64_t NWL_MAX_N = 1ll << 30;

// bq::FaceGrid::set_faces' set-up step: the vertex areas and the flag words cleared, k_lm_face_setup, and the flag words on their way
// back; set_faces synchronises the stream before it returns
hipError_t face_setup_with_areas(void *user, hipStream_t stream, const float *pos, int64_t n_vertices, const int *faces, int nf, double *cen, double *rho)
{
    nwl_ctx *ctx = (nwl_ctx *)user;
    const size_t nv = (size_t)n_vertices;
    BQ_TRY(ctx->area3.ensure(sizeof(uint64_t) * nv));
    BQ_TRY(ctx->flag.ensure(sizeof(int) * NWL_FLAG_WORDS));
    BQ_TRY(hipMemsetAsync(ctx->area3.p, 0, sizeof(uint64_t) * nv, stream));
    BQ_TRY(hipMemsetAsync(ctx->flag.p, 0, sizeof(int) * NWL_FLAG_WORDS, stream));
    hipLaunchKernelGGL(k_lm_face_setup, dim3(nblk(nf)), dim3(NWL_BLOCK), 0, stream, pos, faces, nf, cen, rho, ctx->area3.as<u64>(), ctx->flag.as<int>());
    BQ_TRY(hipGetLastError());
    return hipMemcpyAsync(ctx->flag_h, ctx->flag.p, sizeof(ctx->flag_h), hipMemcpyDeviceToHost, stream);
}

bool power_of_two(double s)
{
    int e;
    return std::isfinite(s) && s > 0.0 && std::frexp(s, &e) == 0.5 && e > -900 && e < 900;
}

}  // namespace

NWL_EXPORT int nwl_abi_version(void) { return NWL_ABI_VERSION; }

NWL_EXPORT int nwl_create(int device, nwl_ctx **out) { return bq::create(device, out, NWL_ERR_BADARG, NWL_ERR_HIP); }

NWL_EXPORT void nwl_destroy(nwl_ctx *ctx) { bq::destroy(ctx); }

NWL_EXPORT const char *nwl_last_error(nwl_ctx *ctx) { return bq::last_error(ctx); }

NWL_EXPORT int nwl_set_mesh(nwl_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces)
{
    if (ctx) { ctx->m.nf = 0; ctx->acc_columns = -1; ctx->acc_n = 0; }
    bq::FaceStatus s = bq::check_faces(pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwl_set_mesh", s, NWL_FACE_CODES);
    if (!ctx) return NWL_ERR_BADARG;
    NWL_HIP(hipSetDevice(ctx->device));
    s = ctx->m.set_faces(ctx->stream, pos, n_vertices, faces, n_faces, face_setup_with_areas, ctx);
    if (!s.ok()) return bq::face_fail(ctx, "nwl_set_mesh", s, NWL_FACE_CODES);
    // (after set_faces' own checks, of which only the non-finite centroid can fail: the extent of finite centroids of float32 corners is finite)
    if (ctx->flag_h[0]) { ctx->m.nf = 0; return fail(ctx, NWL_ERR_BADARG, "nwl_set_mesh: a face of area 2^40 or more"); }
    return NWL_OK;
}

NWL_EXPORT int nwl_get_areas(nwl_ctx *ctx, uint64_t *area3_out)
{
    if (!area3_out) return fail(ctx, NWL_ERR_BADARG, "nwl_get_areas: a NULL array");
    if (!ctx) return NWL_ERR_BADARG;
    if (ctx->m.nf < 1) return fail(ctx, NWL_ERR_NOMESH, "nwl_get_areas: the context holds no mesh");
    NWL_HIP(hipSetDevice(ctx->device));
    NWL_HIP(hipMemcpyAsync(area3_out, ctx->area3.p, sizeof(uint64_t) * (size_t)ctx->m.nv, hipMemcpyDeviceToHost, ctx->stream));
    NWL_HIP(hipStreamSynchronize(ctx->stream));
    return NWL_OK;
}

NWL_EXPORT int nwl_map(nwl_ctx *ctx, const double *xyz, int64_t n, const double *values, int n_columns, const double *scales, double d_cap, int flags,
                       int32_t *face_out, int32_t *w_out, double *dist_out, double *closest_out, uint64_t *mass_out, int32_t *count_out,
                       int64_t *sum_hi_out, uint64_t *sum_lo_out, int64_t *info_out)
{
    const bool accumulate = (flags & NWL_ACCUMULATE) != 0, walk_only = (flags & NWL_WALK_ONLY) != 0;
    const int keep_columns = ctx ? ctx->acc_columns : -1;
    const int64_t keep_n = ctx ? ctx->acc_n : 0;
    if (ctx && !walk_only) { ctx->acc_columns = -1; ctx->acc_n = 0; }            // (whatever fails below leaves nothing to add onto)
    if (!xyz || n < 1 || n > NWL_MAX_N || (flags & ~(NWL_ACCUMULATE | NWL_WALK_ONLY)) || (accumulate && walk_only)) return fail(ctx, NWL_ERR_BADARG, "nwl_map: a NULL cloud, a size out of range or an unknown flag");
    if (n_columns < 0 || n_columns > NWL_MAX_VALUE_COLUMNS || (n_columns > 0 && (!values || !scales))) return fail(ctx, NWL_ERR_BADARG, "nwl_map: more than 8 value columns, or columns without values or scales");
    for (int c = 0; c < n_columns; ++c)
        if (!power_of_two(scales[c])) return fail(ctx, NWL_ERR_BADARG, "nwl_map: a scale that is not a power of two within [2^-900, 2^899]");
    if (!std::isfinite(d_cap) || !(d_cap > 0.0) || !(d_cap <= NWL_MAX_CAP)) return fail(ctx, NWL_ERR_BADARG, "nwl_map: the band must be finite and within (0, 2^40]");
    if (!ctx) return NWL_ERR_BADARG;
    if (ctx->m.nf < 1) return fail(ctx, NWL_ERR_NOMESH, "nwl_map: the context holds no mesh");
    if (accumulate && keep_columns != n_columns) return fail(ctx, NWL_ERR_BADARG, "nwl_map: NWL_ACCUMULATE needs the accumulators of a call with the same mesh and the same number of columns");
    if (accumulate && keep_n + n > NWL_MAX_N) return fail(ctx, NWL_ERR_BADARG, "nwl_map: more than 2^30 localizations in one set of accumulators");
    NWL_HIP(hipSetDevice(ctx->device));
    const double *dq = xyz;
    if (!bq::on_device(xyz)) {
        if (!bq::all_finite(xyz, 3 * n)) return fail(ctx, NWL_ERR_NONFINITE, "nwl_map: a localization is not finite");
        NWL_HIP(bq::upload(ctx->stream, ctx->up, xyz, 3 * n));
        dq = ctx->up.as<double>();
    } else {
        bq::Grid<double> box;
        bool finite[2];
        NWL_HIP(bq::bounds<double>(ctx->stream, ctx->qmm, dq, (int)n, nullptr, 0, &box, finite));
        if (!finite[0]) return fail(ctx, NWL_ERR_NONFINITE, "nwl_map: a localization is not finite");
    }
    const double *dv = nullptr;
    if (n_columns > 0 && !walk_only) {
        dv = values;
        if (!bq::on_device(values)) {
            NWL_HIP(bq::upload(ctx->stream, ctx->upv, values, n * n_columns));
            dv = ctx->upv.as<double>();
        }
        NWL_HIP(bq::upload(ctx->stream, ctx->scales, scales, n_columns));
    }
    bq::FaceGrid &m = ctx->m;
    // the grid for this band, the volume unit's rule: from the cell size bq::band_cell and bq::face_cell give
    const bq::FaceStatus s = m.bin(ctx->stream, bq::face_cell(bq::band_cell(m.rho_mean, m.rho_max, d_cap), m.emax()));
    if (!s.ok()) return bq::face_fail(ctx, "nwl_map", s, NWL_FACE_CODES);
    const int nb = nblk(n, NWL_BLOCK);
    const size_t nv = (size_t)m.nv, nf = (size_t)m.nf, nvc = std::max<size_t>(nv * (size_t)n_columns, 1);
    if (face_out) NWL_HIP(ctx->face.ensure(sizeof(int) * (size_t)n));
    if (w_out) NWL_HIP(ctx->w.ensure(sizeof(int) * 3 * (size_t)n));
    if (dist_out) NWL_HIP(ctx->dist.ensure(sizeof(double) * (size_t)n));
    if (closest_out) NWL_HIP(ctx->closest.ensure(sizeof(double) * 3 * (size_t)n));
    NWL_HIP(ctx->partial.ensure(sizeof(long long) * NWL_PARTIALS * (size_t)nb));
    NWL_HIP(ctx->totals.ensure(sizeof(long long) * NWL_PARTIALS));
    NWL_HIP(ctx->flag.ensure(sizeof(int) * NWL_FLAG_WORDS));
    NWL_HIP(hipMemsetAsync(ctx->flag.p, 0, sizeof(int) * NWL_FLAG_WORDS, ctx->stream));
    if (!walk_only) {
        // (a buffer that has to grow loses its contents: only without NWL_ACCUMULATE can that happen, the sizes being the mesh's)
        const bool fresh = !accumulate || ctx->mass.bytes < sizeof(uint64_t) * nv || ctx->count.bytes < sizeof(int) * nf || ctx->sum_hi.bytes < sizeof(int64_t) * nvc ||
                           ctx->sum_lo.bytes < sizeof(uint64_t) * nvc;
        if (accumulate && fresh) return fail(ctx, NWL_ERR_BADARG, "nwl_map: NWL_ACCUMULATE without accumulators at hand");
        NWL_HIP(ctx->mass.ensure(sizeof(uint64_t) * nv));
        NWL_HIP(ctx->count.ensure(sizeof(int) * nf));
        NWL_HIP(ctx->sum_hi.ensure(sizeof(int64_t) * nvc));
        NWL_HIP(ctx->sum_lo.ensure(sizeof(uint64_t) * nvc));
        if (fresh) {
            NWL_HIP(hipMemsetAsync(ctx->mass.p, 0, sizeof(uint64_t) * nv, ctx->stream));
            NWL_HIP(hipMemsetAsync(ctx->count.p, 0, sizeof(int) * nf, ctx->stream));
            NWL_HIP(hipMemsetAsync(ctx->sum_hi.p, 0, sizeof(int64_t) * nvc, ctx->stream));
            NWL_HIP(hipMemsetAsync(ctx->sum_lo.p, 0, sizeof(uint64_t) * nvc, ctx->stream));
        }
    }
    nwv_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = m.g.lo[d]; g.hi[d] = m.g.hi[d]; g.dims[d] = m.g.dims[d]; }
    g.h = m.g.h;
    hipLaunchKernelGGL(k_lm_map, dim3(nb), dim3(NWL_BLOCK), 0, ctx->stream, dq, n, dv, walk_only ? 0 : n_columns, ctx->scales.as<double>(),
                       m.mpos.as<float>(), m.mfaces.as<int>(), m.nf, m.sorted.as<nwv_pt>(), m.cstart.as<int>(), m.rho.as<double>(),
                       m.rho_max, g, d_cap, face_out ? ctx->face.as<int>() : nullptr, w_out ? ctx->w.as<int>() : nullptr,
                       dist_out ? ctx->dist.as<double>() : nullptr, closest_out ? ctx->closest.as<double>() : nullptr,
                       walk_only ? nullptr : ctx->mass.as<u64>(), ctx->count.as<int>(), ctx->sum_hi.as<u64>(), ctx->sum_lo.as<u64>(), ctx->flag.as<int>(),
                       ctx->partial.as<long long>());
    hipLaunchKernelGGL(k_lm_totals, dim3(1), dim3(NWL_BLOCK), 0, ctx->stream, ctx->partial.as<long long>(), (int64_t)nb, ctx->totals.as<long long>());
    NWL_HIP(hipGetLastError());
    long long tot[NWL_PARTIALS] = {0, 0, 0};
    int flag[NWL_FLAG_WORDS] = {0, 0, 0};
    NWL_HIP(hipMemcpyAsync(tot, ctx->totals.p, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
    NWL_HIP(hipMemcpyAsync(flag, ctx->flag.p, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
    NWL_HIP(hipStreamSynchronize(ctx->stream));                   // (the flag words are read once, before anything is handed out)
    if (flag[NWL_Q_NONFINITE]) return fail(ctx, NWL_ERR_NONFINITE, "nwl_map: a value of an in-band localization is not finite");
    if (flag[NWL_Q_RANGE]) return fail(ctx, NWL_ERR_RANGE, "nwl_map: a value of an in-band localization is larger than its column's scale");
    if (face_out) NWL_HIP(hipMemcpyAsync(face_out, ctx->face.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (w_out) NWL_HIP(hipMemcpyAsync(w_out, ctx->w.p, sizeof(int) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out) NWL_HIP(hipMemcpyAsync(dist_out, ctx->dist.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (closest_out) NWL_HIP(hipMemcpyAsync(closest_out, ctx->closest.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (!walk_only) {
        if (mass_out) NWL_HIP(hipMemcpyAsync(mass_out, ctx->mass.p, sizeof(uint64_t) * nv, hipMemcpyDeviceToHost, ctx->stream));
        if (count_out) NWL_HIP(hipMemcpyAsync(count_out, ctx->count.p, sizeof(int) * nf, hipMemcpyDeviceToHost, ctx->stream));
        if (sum_hi_out && n_columns) NWL_HIP(hipMemcpyAsync(sum_hi_out, ctx->sum_hi.p, sizeof(int64_t) * nv * (size_t)n_columns, hipMemcpyDeviceToHost, ctx->stream));
        if (sum_lo_out && n_columns) NWL_HIP(hipMemcpyAsync(sum_lo_out, ctx->sum_lo.p, sizeof(uint64_t) * nv * (size_t)n_columns, hipMemcpyDeviceToHost, ctx->stream));
    }
    NWL_HIP(hipStreamSynchronize(ctx->stream));
    if (info_out) {
        info_out[NWL_INFO_IN_BAND] = tot[0];
        info_out[NWL_INFO_RINGS] = tot[1];
        info_out[NWL_INFO_CENTROIDS] = tot[2];
        info_out[NWL_INFO_CELLS] = m.g.cells();
        info_out[NWL_INFO_CELL_SIZE] = __builtin_bit_cast(int64_t, m.g.h);
    }
    if (walk_only) return NWL_OK;                                 // (the accumulators at hand are as they were)
    ctx->acc_columns = n_columns;
    ctx->acc_n = (accumulate ? keep_n : 0) + n;
    return NWL_OK;
}
